"""The ranking family (k_rank_*, k_rank_*_x, k_topk_*, k_pool_*; docs/DESIGN.md
§2) on the loop and launch paths that the shapes of test_rank.py,
test_rank_cross.py, test_rank_topk.py and test_rank_pool.py never take:

  A  k_pool_score's request loop on its second and third trip
  B  the template widths 2 and 16 of every kernel of the family
  C  contexts and pool rows whose lane shares cross a probe chunk (more than
     512 keys at 8 occurrences in flight, more than 256 at 4), and a crossed
     context whose operands lie in its tenth chunk of 64
  D  up to 64 requests inside one tile, runs of empty requests on tile edges
  E  pool_topk with a request's rows across the 4096-row top-k tile edge

A score is a function of its own context and candidate alone, bit for bit, so
the new paths are compared exactly with small calls that the neighbouring
files hold to ref64, and with ref64 itself (err <= e_p on every compared
element) where the rows are few.  No tolerance of this file's own.

Worst error/bound ratios on an MI355X (every case prints its own): A 0.25
(fm8-reference; 0.17 LR), B 0.13 ranked, 0.008 crossed, 0.33 pooled (fm2-
reference), C 0.0075 ranked (the long rows hold mostly zero weights: few
roundings against a bound sized for the row's length), 0.05 crossed, 0.0013
pooled, D 0.27, and 0.43 with the pair cross.  The file takes 8.5 s there, CPU
twins included; no case more than 0.4 s."""
import functools

import numpy as np
import pytest
import torch

import test_rank as tr
import test_rank_cross as tx
import test_rank_pool as tp
from test_rank import CAND_COUNTS, CONFIGS, CPU, F32, _bits, _engine, _keys, _rank
from test_rank_pool import _lexsort_topk, _vecs

from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Engine

DEVS = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="hip", marks=pytest.mark.gpu)]


def _dev(request, name):
    return request.getfixturevalue("gpu_device") if name == "cuda" else CPU


def _hold(what, p, ref, first=None):
    """err <= e_p on every element of p against ref's rows (its `first` rows);
    prints the worst ratio like the neighbours."""
    rp, re = ref.p[:first], ref.e_p[:first]
    err = np.abs(np.asarray(p, dtype=np.float64).reshape(-1) - rp)
    print("%s: worst error/bound %.3g" % (what, float((err / re).max())))
    assert err.shape == re.shape and (err <= re).all(), what


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- A: the request loop of k_pool_score ---------------------------------------------
# kernels_pool.hip: kPoolTileN = 128 candidates per workgroup, kPoolTileM = 32
# requests per block, kPoolTargetGrid = 2048; gx = ceil(N / 128), blocks =
# ceil(R / 32), gy = min(blocks, 65535, max(1, 2048 / gx)) and workgroup y takes
# the blocks y, y + gy, ..
#   N = 128 * 2049 + 5: gx = 2050 > 2048, gy = 1, one workgroup walks all 2 or 3
#     blocks; the last one holds 1 row (R = 33, 65) or 32 (R = 96)
#   R = 32 * 2048 + 33: blocks = 2050, gy = 2048 (N = 1) or 1024 (N = 129); only
#     some y take another trip, the block of 1 row (65568) is nobody's first
POOL_MODELS = {"lr": (CONFIGS[0], 0), "fm16-standard": (("fm", 16, "standard"), 1),  # KP 2, 18
               "fm32-standard": (CONFIGS[10], 10), "fm8-reference": (CONFIGS[5], 5)}  # KP 34, 4
BIG_N, BIG_R = 128 * 2049 + 5, 32 * 2048 + 33
TRIPS = [(33, BIG_N), (65, BIG_N), (96, BIG_N), (BIG_R, 1), (BIG_R, 129)]
SAMPLE = 256  # random pairs held to ref64, besides the named ones


def _launch(R, N):
    gx, blocks = -(-N // 128), -(-R // 32)
    return blocks, min(blocks, 65535, max(1, 2048 // gx))


@functools.lru_cache(maxsize=None)
def _small(dev, name):
    """31 contexts x 127 candidates, real vectors, scored in one trip: the shape
    class test_rank_pool.py holds to ref64.  Computed once, never changed."""
    c, i = POOL_MODELS[name]
    e = _engine(c, i, dev)
    rng = np.random.default_rng(17)
    ctx = [_keys(rng, n) if n >= 0 else np.arange(-n, -n + 4, dtype=np.uint64)
           for n in tp.CTX_LENS + [(7 * q) % 40 for q in range(8, 31)]]
    cands = [_keys(rng, tp.ROW_LENS[r % 5]) for r in range(127)]
    cv, pv = _vecs(e, ctx), _vecs(e, cands)
    assert _launch(len(ctx), len(cands)) == (1, 1)
    return e, ctx, cands, cv, pv, e.pool_score(cv, pv)


def _deal(rng, n, size):
    """size indices below n, permutation after permutation: every index occurs
    and no period lines up with a tile."""
    return np.concatenate([rng.permutation(n) for _ in range(-(-size // n))])[:size]


@pytest.mark.parametrize("R,N", TRIPS, ids=["%dx%d" % t for t in TRIPS])
@pytest.mark.parametrize("name", POOL_MODELS)
@pytest.mark.parametrize("dev", DEVS)
def test_pool_score_on_later_trips_of_the_request_loop(request, dev, name, R, N):
    """Every bit of the big product against the one-trip product of the rows it
    was gathered from, then a fixed sample of it (the corners of the last
    block, the first row of every trip, 256 seeded pairs) against ref64.
    Worst error/bound ratio on an MI355X: the printed line of each case."""
    dev = _dev(request, dev)
    e, ctx, cands, cv, pv, small = _small(dev, name)
    blocks, gy = _launch(R, N)
    assert blocks > gy  # (a workgroup takes a second trip)
    rng = np.random.default_rng(R + N)
    ir, in_ = _deal(rng, len(ctx), R), _deal(rng, len(cands), N)
    tr_, tn = torch.from_numpy(ir).to(dev), torch.from_numpy(in_).to(dev)
    big = e.pool_score(cv[tr_].contiguous(), pv[tn].contiguous())
    want = small[tr_][:, tn]
    assert big.shape == (R, N)
    assert torch.equal(big.view(torch.int32), want.contiguous().view(torch.int32))
    rows = {0, 32 * (blocks - 1), R - 1} | {32 * t * gy for t in range(-(-blocks // gy))}
    cols = {0, 128 * ((N - 1) // 128), N - 1}
    pairs = {(r, n) for r in rows for n in cols}
    pairs |= set(zip(rng.integers(0, R, SAMPLE).tolist(), rng.integers(0, N, SAMPLE).tolist()))
    pr, pn = (np.array(x, dtype=np.int64) for x in zip(*sorted(pairs)))
    got = big[torch.from_numpy(pr).to(dev), torch.from_numpy(pn).to(dev)].cpu().numpy()
    full = [np.concatenate([ctx[ir[r]], cands[in_[n]]]) for r, n in zip(pr, pn)]
    _hold("%s %dx%d" % (name, R, N), got, tx._ref(e, POOL_MODELS[name][0], full))


# ---- B: widths 2 and 16 ----------------------------------------------------------------
WIDE = [("fm", d, m) for d in (2, 16) for m in ("reference", "standard")]
WIDE_IDS = ["%s%d-%s" % c for c in WIDE]


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(WIDE)), ids=WIDE_IDS)
def test_rank_widths_2_and_16(gpu_device, i):
    """test_rank's geometry.  Worst error/bound ratio on an MI355X: the printed
    line of each case."""
    c, layout = WIDE[i], ("csr", "rm", "fm")[i % 3]
    e = _engine(c, i, gpu_device, serve_fused=False)
    assert e.ranks and e.frozen
    ctx, cands = tr._requests(layout)
    p = _rank(e, ctx, cands, CAND_COUNTS, layout)
    req = np.repeat(np.arange(len(ctx)), CAND_COUNTS)
    full = [np.concatenate([ctx[q], cands[r]]) for r, q in enumerate(req)]
    _hold("%s %s" % (c, layout), p, tx._ref(e, c, full))
    assert _same(p, _rank(e, ctx, cands, CAND_COUNTS, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(WIDE)), ids=WIDE_IDS)
def test_crossed_rank_widths_2_and_16(gpu_device, i):
    """test_rank_cross's geometry under its full spec (16 crosses of arity 4)."""
    c, layout, X = WIDE[i], ("csr", "rm", "fm")[(i + 1) % 3], tx.SPECS["full"]
    req = tx._requests(layout)
    rows, _ = tx._expand(*req, CAND_COUNTS, X)
    e = tx._engine(c, i, gpu_device, rows, len(X), serve_fused=False)
    p = tx._rank(e, *req, CAND_COUNTS, X, layout)
    _hold("%s %s full" % (c, layout), p, tx._ref(e, c, rows))
    assert _same(p, tx._rank(e, *req, CAND_COUNTS, X, layout))


@pytest.mark.parametrize("i", range(len(WIDE)), ids=WIDE_IDS)
@pytest.mark.parametrize("dev", DEVS)
def test_pool_widths_2_and_16(request, dev, i):
    """test_rank_pool._within_bound's check (it takes an index into CONFIGS, not
    a config) over the pools 1 and 129 and 1 and 33 requests.  Standard math at
    v_dim 2 is Dk = 2 inside KP = 4: an operand without a zero column."""
    dev, c = _dev(request, dev), WIDE[i]
    e = _engine(c, i, dev)
    assert e.pools and e.pool_width == ((1 + (c[1] if c[2] == "standard" else 1) + 3) & ~3)
    rng = np.random.default_rng(5)
    ctx = [_keys(rng, n) if n >= 0 else np.arange(-n, -n + 4, dtype=np.uint64)
           for n in tp.CTX_LENS + [q % 5 for q in range(8, 33)]]
    cv = _vecs(e, ctx)
    for j, N in enumerate((1, 129)):
        layout = ("csr", "rm", "fm")[(i + j) % 3]
        lens = ([tp.ROW_LENS[r % 5] for r in range(N)] if layout == "csr"
                else [9 if layout == "rm" else 17] * N)
        cands = [_keys(rng, n) for n in lens]
        pv = _vecs(e, cands, layout)
        ref = tx._ref(e, c, [np.concatenate([x, y]) for x in ctx for y in cands])
        ry = ref.y.reshape(len(ctx), N)
        for R in (1, 33):
            p = e.pool_score(cv[:R], pv).cpu().numpy()
            assert p.shape == (R, N)
            _hold("%s %s %dx%d" % (c, layout, R, N), p, ref, first=R * N)
            if R > 7:
                assert (ry[1] > 31).all() and (p[1] == 1.0).all()         # the upper clamp
                assert (ry[7] < -31).all() and (p[7] == F32(1e-6)).all()  # the lower clamp


# ---- C: lane shares across a probe chunk -------------------------------------------------
# a lane's share of n keys is ceil((n - lane) / 64): 4 | 5 at 256 | 257 (the
# wide rows' 4 occurrences in flight), 8 | 9 at 512 | 513, 9 | 10 at 576 | 577
LONG = [256, 257, 512, 513, 576, 577]
LONG_MODELS = [0, 6, 9]  # LR, fm8-standard (8 in flight), fm32-reference (4 in flight)
LONG_IDS = ["lr", "fm8-standard", "fm32-reference"]
# ref64's bound grows with a row's sum of |weights| (reference FM's with its
# square): 577 ordinary keys put a logit of width 32 in the hundreds and the
# bound above 1, where neither it nor a clamped score's bits could show a wrong
# occurrence.  So a long row holds keys of weight zero, and planted keys at
# the first and last occurrence of the lanes' probe chunks: a dropped, doubled
# or misplaced occurrence there moves the score by far more than the bound.
EDGES = [0, 63, 64, 255, 256, 257, 319, 320, 511, 512, 513, 575, 576]
ZERO = np.arange(20000, 20640, dtype=np.uint64)


def _long_engine(i, dev):
    e = _engine(CONFIGS[i], i, dev)
    e.import_weights(ZERO, np.zeros((len(ZERO), e.params_per_key), F32))
    assert not e.pull(ZERO).any() and e.pull(np.arange(100, 4100, dtype=np.uint64))[:, 0].all()
    return e


def _long_row(rng, n):
    k = rng.permutation(ZERO)[:n]
    at = [j for j in EDGES if j < n]
    k[at] = rng.integers(100, 4100, len(at))
    return k


def _squeeze(k):
    """k without its chunks of 64 that hold weights of zero alone.  Every other
    occurrence keeps its lane and its place in the lane's order, and adding
    +0.0f changes no sum: the row's sums keep every bit, over fewer chunks."""
    parts = [k[a:a + 64] for a in range(0, len(k), 64)]
    out = np.concatenate([x for x in parts if (x < ZERO[0]).any()])
    assert len(out) <= len(k) - 64
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("i", LONG_MODELS, ids=LONG_IDS)
def test_rank_long_contexts(gpu_device, i):
    c = CONFIGS[i]
    e = _long_engine(i, gpu_device)
    rng = np.random.default_rng(23)
    ctx = [_long_row(rng, n) for n in LONG]
    cands = [_keys(rng, n) for _ in LONG for n in (0, 8, 17)]
    p = _rank(e, ctx, cands, [3] * len(LONG))
    full = [np.concatenate([ctx[r // 3], y]) for r, y in enumerate(cands)]
    _hold("%s long contexts" % (c,), p, tx._ref(e, c, full))
    for q in range(len(LONG)):  # alone, and after the other requests of the tile
        assert _same(p[3 * q:3 * q + 3], _rank(e, [ctx[q]], cands[3 * q:3 * q + 3], [3])), q
    assert _same(p, _rank(e, [_squeeze(k) for k in ctx], cands, [3] * len(LONG)))


@pytest.mark.parametrize("i", LONG_MODELS, ids=LONG_IDS)
@pytest.mark.parametrize("dev", DEVS)
def test_pool_long_rows(request, dev, i):
    dev, c = _dev(request, dev), CONFIGS[i]
    e = _long_engine(i, dev)
    rng = np.random.default_rng(29)
    ctx, cands = [_long_row(rng, n) for n in LONG], [_long_row(rng, n) for n in LONG]
    short = _keys(rng, 5)
    cv, pv = _vecs(e, [short] + ctx)[1:], _vecs(e, [short] + cands)[1:]
    for q in range(len(LONG)):  # row q + 1 is wave (q + 1) % 4 of its workgroup, alone wave 0
        assert _same(cv[q:q + 1].cpu(), _vecs(e, [ctx[q]]).cpu()), q
        assert _same(pv[q:q + 1].cpu(), _vecs(e, [cands[q]]).cpu()), q
    assert _same(pv.cpu(), _vecs(e, cands).cpu())
    assert _same(cv.cpu(), _vecs(e, [_squeeze(k) for k in ctx]).cpu())
    p = e.pool_score(cv.contiguous(), pv.contiguous()).cpu().numpy()
    full = [np.concatenate([x, y]) for x in ctx for y in cands]
    _hold("%s long rows" % (c,), p, tx._ref(e, c, full))


# operand fields of the long crossed context: LATE only at index 576, the lone
# entry of the tenth chunk; TWICE at 0 and again at 300 with another key; CAND
# in candidates only; NOWHERE in neither
LATE, TWICE, CAND, NOWHERE = 11, 5, 23, 40
LONG_SPEC = [(TWICE, LATE), (TWICE, CAND), (LATE, NOWHERE)]  # complete by 576; mixed; never


def _long_crossed():
    rng = np.random.default_rng(37)
    # (keys below 40000: a sixth planted, so the logit stays off the sigmoid's flat ends)
    ctx = [tx._keys(rng, 7), rng.integers(100, 40000, size=577).astype(np.uint64)]
    cf = [np.array([200, TWICE, 201, 3, 202, 203, 204], np.int32),
          (200 + np.arange(577) % 50).astype(np.int32)]
    cf[1][[0, 300, 576]] = TWICE, TWICE, LATE
    assert ctx[1][0] != ctx[1][300]
    counts = [5, 70]
    lens = [tr.ROW_LENS[r % 5] for r in range(sum(counts))]
    cands = [tx._keys(rng, n) for n in lens]
    df = [rng.choice([CAND, LATE, TWICE, 200, 201], n).astype(np.int32) for n in lens]
    return ctx, cf, cands, df, counts


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 4], ids=["lr", "fm8-standard"])
def test_crossed_rank_finds_operands_in_a_late_chunk(gpu_device, i):
    c = tx.CONFIGS[i]
    req = _long_crossed()
    rows, plain = tx._expand(*req, LONG_SPEC)
    e = tx._engine(c, i, gpu_device, rows, len(LONG_SPEC))
    p = tx._rank(e, *req, LONG_SPEC)
    ref = tx._ref(e, c, rows)
    _hold("%s long crossed context" % (c,), p, ref)
    if c[0] == "lr":  # the crosses matter: without their keys most rows miss the bound
        bare = tx._ref(e, c, plain)
        assert (np.abs(p.astype(np.float64) - bare.p) > bare.e_p)[5:].mean() > 0.5
    assert _same(p[5:], tx._rank(e, *(x[1:] for x in req[:2]), req[2][5:], req[3][5:], [70],
                                 LONG_SPEC))


# ---- D: many requests per tile -------------------------------------------------------------
# 200 requests.  (A run of 64 one-row requests that fills a tile and a request
# that fills another and takes a row of each neighbour cannot share 3 tiles:
# these are 6.)
MANY = ([0] * 3 + [63, 66]      # leading empties; rows 0 .. 62; 63 .. 128: a tile and a row each side
        + [1] * 38 + [0] * 5 + [2] * 5 + [3] * 5  # rows 129 .. 191; empties inside a tile
        + [0] * 5               # a run of empties that ends on the edge 192
        + [1] * 64              # rows 192 .. 255: a lane each, aligned to the tile
        + [0] * 5 + [1]         # a run of empties that starts on the edge 256; row 256
        + [1] * 64              # rows 257 .. 320: the same run shifted by 1
        + [0] * 3)              # trailing empties
SOLO = [0, 63, 128, 191, 192, 256, 257, 320]  # rows also ranked in a call of their own


def _many(rng):
    rp = np.concatenate([[0], np.cumsum(MANY)])
    assert len(MANY) == 200 and rp[-1] == 321 and rp[5] == 129
    assert (rp[58:64] == 192).all() and (rp[127:133] == 256).all() and rp[133] == 257
    ctx = [_keys(rng, q % 10) for q in range(len(MANY))]
    cands = [_keys(rng, tr.ROW_LENS[r % 5]) for r in range(int(rp[-1]))]
    return ctx, cands, np.repeat(np.arange(len(MANY)), MANY)


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 6], ids=["lr", "fm8-standard"])
def test_rank_many_requests_per_tile(gpu_device, i):
    c = CONFIGS[i]
    e = _engine(c, i, gpu_device)
    ctx, cands, req = _many(np.random.default_rng(41))
    p = _rank(e, ctx, cands, MANY)
    full = [np.concatenate([ctx[q], cands[r]]) for r, q in enumerate(req)]
    _hold("%s 200 requests" % (c,), p, tx._ref(e, c, full))
    # every pair as a request of its own: 64 contexts per tile in every tile
    assert _same(p, _rank(e, [ctx[q] for q in req], cands, [1] * len(cands)))
    for r in SOLO:
        assert _same(p[r:r + 1], _rank(e, [ctx[req[r]]], [cands[r]], [1])), r


@pytest.mark.gpu
def test_crossed_rank_many_requests_per_tile(gpu_device):
    c, X = tx.CONFIGS[0], tx.SPECS["pair"]
    rng = np.random.default_rng(43)
    ctx, cands, req = _many(rng)
    cf = [rng.choice([3, 7, 200, 201], len(k)).astype(np.int32) for k in ctx]
    df = [rng.choice([3, 7, 200, 201], len(k)).astype(np.int32) for k in cands]
    rows, _ = tx._expand(ctx, cf, cands, df, MANY, X)
    e = tx._engine(c, 0, gpu_device, rows, len(X))
    p = tx._rank(e, ctx, cf, cands, df, MANY, X)
    _hold("%s 200 requests, pair" % (c,), p, tx._ref(e, c, rows))
    assert _same(p, tx._rank(e, [ctx[q] for q in req], [cf[q] for q in req], cands, df,
                             [1] * len(cands), X))
    for r in SOLO:
        q = req[r]
        assert _same(p[r:r + 1], tx._rank(e, [ctx[q]], [cf[q]], [cands[r]], [df[r]], [1], X)), r


# ---- E: pool_topk across the top-k tile edge ---------------------------------------------
@pytest.mark.parametrize("N", [4095, 4097])
@pytest.mark.parametrize("kind", ["lr", "fm8-standard"])
@pytest.mark.parametrize("dev", DEVS)
def test_pool_topk_across_a_tile_edge(request, dev, kind, N):
    """3 requests of N scores in one array: their rows cross the 4096-row tile
    edges of k_topk_tile at 1 | 2 (N = 4095) and at 4096 | 4095 | 4094 rows."""
    dev = _dev(request, dev)
    model = ModelConfig(kind="lr") if kind == "lr" else ModelConfig(kind="fm", v_dim=8,
                                                                    fm_math="standard")
    e = Engine(model, OptimConfig(kind="frozen", frozen_from="ftrl"),
               EngineConfig(table_log2_cap=13, max_rows=512, max_nnz=512 * 16), device=dev)
    rng = np.random.default_rng(3)
    keys = np.arange(100, 4100).astype(np.uint64)
    W = rng.normal(0, 0.05, (len(keys), e.params_per_key)).astype(F32)
    W[:, 0] = np.round(rng.normal(0, 0.3, len(keys)), 1)  # (coarse weights: equal scores occur)
    e.import_weights(keys, W)
    ctx = [rng.integers(100, 5000, 9).astype(np.uint64) for _ in range(3)]
    # one or two of 40 keys: every score many times, on both sides of an edge
    cands = [rng.integers(100, 140, 1 + r % 2).astype(np.uint64) for r in range(N)]
    cv, pv = _vecs(e, ctx), _vecs(e, cands)
    p = e.pool_score(cv, pv).cpu().numpy()
    assert all(len(np.unique(_bits(x))) < N // 2 for x in p)
    for k in (1, 7, 1024):
        idx, score = (t.cpu().numpy() for t in e.pool_topk(cv, pv, k))
        assert idx.shape == (3, k) and idx.dtype == np.int32
        for q in range(3):
            wi, ws = _lexsort_topk(p[q], k)
            assert np.array_equal(idx[q], wi) and _same(score[q], ws), (q, k)
