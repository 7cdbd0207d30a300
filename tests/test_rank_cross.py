"""Candidate ranking of models with feature crosses (k_rank_lr_x / k_rank_fm_x,
docs/DESIGN.md §2): rank_step(..., crosses=...) scores a candidate as the model
scores the row context ++ candidate ++ the spec's cross keys of that row, so it
is held to ref64's bound on those rows; the context's share is a function of
the context alone, so tiling and chunking may not change a bit."""
import numpy as np
import pytest
import torch

import test_rank as tr
from xflow_amd import checkpoint
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Batch, Engine, cross_keys
from xflow_amd.serve import Predictor
from xflow_amd.testing import ref64

F32 = np.float32
NONE = np.uint64(2**64 - 1)
LOG2 = 14  # 8028 planted keys in 16384 slots: load 0.49, chains leave the home slot
CONFIGS = [("lr", 0, "reference")] + [("fm", d, m) for d in (1, 8, 10, 32)
                                      for m in ("reference", "standard")]
# every operand slot in use, 64 distinct fields: cross c takes fields 4c .. 4c + 3
SPECS = {"pair": [(3, 7)], "full": [tuple(range(4 * c, 4 * c + 4)) for c in range(16)]}
# test_rank's geometry: request boundaries inside a tile (60), on a tile edge
# (64), across two tiles; a request without candidates; an empty context
CTX_LENS = [63, 4, 64, 7, 130, 0, 65, 1, 4]
# crosses of the full spec a context completes (it holds fields 0 .. 4j - 1;
# the context of 130 entries its last eight):
# 16, 9, 8, 1 and 0 incomplete ones are the probe-chunk edges; tile 0 holds 15
# and 0, tile 2 holds 16 and 8, tile 4 holds 8, 0, 7 and 0
COMPLETE = [15, 0, 16, 0, 8, 0, 7, 0, 0]
CAND_COUNTS = tr.CAND_COUNTS


def _keys(rng, n):
    return rng.integers(100, 9100, size=n).astype(np.uint64)  # planted below 6400: 30 % absent


def _requests(layout, seed=5):
    """Contexts and candidates with their field ids.  Operand fields are 0..63,
    fields from 200 belong to no cross."""
    rng = np.random.default_rng(seed)
    ctx, cf = [], []
    for n, j in zip(CTX_LENS, COMPLETE):
        extra = rng.choice([4 * j + 1, 4 * j + 2, 3, 200, 201], size=n - 4 * j)
        cf.append(rng.permutation(np.concatenate([np.arange(4 * j), extra])).astype(np.int32))
        ctx.append(_keys(rng, n))
    # 130 entries that complete crosses 8 .. 15; field 7 first at index 100 and
    # again at 120, field 3 left to the candidates
    cf[4] = np.concatenate([np.arange(32, 64), np.arange(200, 330)])[:130].astype(np.int32)
    cf[4][[100, 120]] = 7
    # the first occurrence of field 3 holds the raw key ~0, a real key follows
    cf[1][:], ctx[1][0] = [3, 3, 1, 2], NONE
    rows = sum(CAND_COUNTS)
    lens = (np.array([tr.ROW_LENS[r % 5] for r in range(rows)]) if layout == "csr"
            else np.full(rows, 9 if layout == "rm" else 17))
    cands = [_keys(rng, n) for n in lens]
    # a quarter of the entries in fields 3 and 7 (both sides hold them with
    # different keys, a candidate holds them twice), most in 0..63, some in none
    df = [np.where(rng.random(n) < 0.25, rng.choice([3, 7], n),
                   np.where(rng.random(n) < 0.8, rng.integers(0, 64, n), 200)).astype(np.int32)
          for n in lens]
    for r in (1, 61):  # (request 0's context has field 7, request 1's has not)
        df[r][:2], cands[r][0] = 7, NONE
    return ctx, cf, cands, df


def _expand(ctx, cf, cands, df, counts, spec):
    """The rows the model scores, context ++ candidate ++ cross keys (operand =
    the raw key at the field's first index, else 2^64 - 1), and the same rows
    without the cross keys."""
    rows, plain = [], []
    for r, q in enumerate(np.repeat(np.arange(len(ctx)), counts)):
        k, f = np.concatenate([ctx[q], cands[r]]), np.concatenate([cf[q], df[r]]).tolist()
        x = [cross_keys(c, [[k[f.index(g)] if g in f else NONE for g in c]])[0] for c in spec]
        plain.append(np.where(k == NONE, NONE - np.uint64(1), k))  # (sanitize_key)
        rows.append(np.concatenate([plain[-1], np.array(x, np.uint64)]))
    return rows, plain


def _engine(c, i, dev, rows, C, **kw):
    """test_rank's table, and 70 % of the rows' cross keys with weights like
    the base keys'; keys no row holds fill it to load 0.49."""
    kind, D, math = c
    model = ModelConfig(kind=kind, **({"v_dim": D, "fm_math": math} if kind == "fm" else {}))
    e = Engine(model, OptimConfig(kind="frozen", frozen_from=("ftrl", "sgd")[i % 2], sgd_v_init=0.003),
               EngineConfig(table_log2_cap=LOG2, max_rows=512, max_nnz=512 * 64, **kw), device=dev)
    rng = np.random.default_rng(31 + D)
    xk = np.unique(np.concatenate([r[len(r) - C:] for r in rows]))
    xk = xk[rng.random(len(xk)) < 0.7]
    keys = np.concatenate([np.arange(100, 6400, dtype=np.uint64), xk])
    keys = np.concatenate([keys, (1 << 40) + np.arange(8028 - len(keys), dtype=np.uint64)])
    W = rng.normal(0, 0.05, (len(keys), 1 + D)).astype(F32)
    W[:, 0] = rng.normal(0, 0.3, len(keys))
    e.import_weights(keys, W)
    return e


def _batch(cands, df, layout, dev):
    b = tr._batch(cands, layout, dev)
    b.fgid = tr._batch([f.astype(np.uint64) for f in df], layout, dev).keys.to(torch.int32)
    return b


def _rank(e, ctx, cf, cands, df, counts, spec, layout="csr"):
    dev, cat = e.device, lambda p, dt: np.concatenate(p + [np.zeros(0, dt)])
    return e.rank_step(tr._t(cat(ctx, np.uint64).view(np.int64), np.int64, dev),
                       tr._t(tr._ptr(ctx), np.int32, dev),
                       tr._t(np.concatenate([[0], np.cumsum(counts)]), np.int32, dev),
                       _batch(cands, df, layout, dev), ctx_fgid=tr._t(cat(cf, np.int32), np.int32, dev),
                       crosses=spec).cpu().numpy()


def _ref(e, c, rows):
    keys = np.concatenate(rows)
    uk = np.unique(keys)
    return ref64.reference(c[0], c[1], uk, e.pull(uk), keys, tr._ptr(rows), fm_math=c[2])


@pytest.mark.gpu
@pytest.mark.parametrize("spec", sorted(SPECS))
@pytest.mark.parametrize("i", range(len(CONFIGS)), ids=["%s%d-%s" % c for c in CONFIGS])
def test_crossed_rank_within_the_float64_bound(gpu_device, i, spec):
    """ref64 on the expanded rows with its own chain length N = n + m + C: a
    context of n entries and j complete crosses and a candidate of m entries
    pass at most ceil(n / 64) + 6 + m + C - j additions that round.  LR, whose
    bound is the tightest against one key's weight (reference FM's grows with
    the square of the row's latent sum), shows once per spec that the same
    reference without the cross keys is off by more than the bound on most
    rows: a wrong or missing cross key cannot hide inside the tolerance."""
    c, layout, X = CONFIGS[i], ("csr", "rm", "fm")[i % 3], SPECS[spec]
    req = _requests(layout)
    rows, plain = _expand(*req, CAND_COUNTS, X)
    e = _engine(c, i, gpu_device, rows, len(X), serve_fused=False)
    p = _rank(e, *req, CAND_COUNTS, X, layout)
    ref = _ref(e, c, rows)
    err = np.abs(p.astype(np.float64) - ref.p)
    print("%s %s %s: worst error/bound %.3g" % (c, layout, spec, float((err / ref.e_p).max())))
    assert (err <= ref.e_p).all()
    if c[0] == "lr":
        bare = _ref(e, c, plain)
        assert (np.abs(p.astype(np.float64) - bare.p) > bare.e_p).mean() > 0.5
    assert np.array_equal(tr._bits(p), tr._bits(_rank(e, *req, CAND_COUNTS, X, layout)))


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 4], ids=["lr", "fm8-standard"])
def test_tiling_chunking_and_the_switch(gpu_device, i, tmp_path):
    c = CONFIGS[i]
    X = [(3, 7), (3, 30), (5, 28, 31), (40, 2)]  # context-only, both sides, a field nowhere
    rng = np.random.default_rng(11)
    cf, df = np.arange(26, dtype=np.int32), np.arange(26, 39, dtype=np.int32)
    ctx, cands = _keys(rng, 26), [_keys(rng, 13) for _ in range(70)]
    other, before = _keys(rng, 26), [_keys(rng, 13) for _ in range(37)]
    one = ([ctx], [cf], cands, [df] * 70, [70])
    two = ([other, ctx], [cf, cf], before + cands, [df] * 107, [37, 70])
    rows = _expand(*two, X)[0]
    e = _engine(c, i, gpu_device, rows, len(X))
    alone = _rank(e, *one, X)
    ref = _ref(e, c, rows[37:])
    assert (np.abs(alone.astype(np.float64) - ref.p) <= ref.e_p).all()
    assert np.array_equal(tr._bits(alone), tr._bits(_rank(e, *one, X)))
    assert np.array_equal(tr._bits(alone), tr._bits(_rank(e, *two, X)[37:]))
    assert np.array_equal(tr._bits(alone), tr._bits(_rank(e, [ctx], [cf], cands[::-1], [df] * 70, [70], X)[::-1]))
    checkpoint.save_serving(e, str(tmp_path / "s"), 0, 1, meta=checkpoint.cross_meta(X, 64),
                            barrier=lambda: None)
    ls = lambda parts: [k.tolist() for k in parts]
    args = ([other.tolist(), ctx.tolist()], [ls(before), ls(cands)],
            [cf.tolist()] * 2, [[df.tolist()] * 37, [df.tolist()] * 70])
    key = np.where(alone > 0, alone, 0).astype(F32).view(np.uint32).astype(np.int64)
    best = np.lexsort((np.arange(70), -key))[:10]
    for max_rows in (64, 4096):
        pred = Predictor(str(tmp_path / "s"), device=gpu_device, max_rows=max_rows)
        assert pred.engine.ranks and pred.crosses == X
        got = pred.rank_keys(*args)
        assert np.array_equal(tr._bits(alone), tr._bits(got[1])) and got[0].shape == (37,)
        idx, sc = pred.rank_keys(*args, top_k=10)[1]
        assert np.array_equal(idx, best) and np.array_equal(tr._bits(sc), tr._bits(alone[best]))
    with pytest.raises(ValueError):  # a crossed model looks its operands up by field id
        pred.rank_keys(*args[:2])
    off = Predictor(str(tmp_path / "s"), device=gpu_device, max_rows=4096, rank_cross=False)
    with pytest.raises(RuntimeError):
        _rank(off.engine, *one, X)
    got = off.rank_keys(*args)[1]  # (rows expanded on the host, cross_batch, eval_step)
    assert (np.abs(got.astype(np.float64) - ref.p) <= ref.e_p).all()
