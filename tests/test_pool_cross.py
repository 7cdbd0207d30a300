"""Pool subsets of models with feature crosses (kernels_pool_cross.hip,
docs/DESIGN.md §2): pool_rows(..., crosses=) keeps operand rows next to the
vectors and pool_subset(..., crosses=) hashes and probes every pair's cross
keys inside the kernel.  An entry is an fp32 evaluation of the model on the row
context ++ candidate ++ cross keys, so it is held to ref64's bound on that row;
it depends on its own two rows and the table alone, so no bit may depend on the
rest of the call."""
import numpy as np
import pytest
import torch

import test_rank as tr
import test_rank_cross as tx
from test_rank import CPU, F32, _bits

from xflow_amd import checkpoint
from xflow_amd.serve import Predictor, make_app

BOTH = pytest.mark.parametrize("dev", [pytest.param("gpu", marks=pytest.mark.gpu), "cpu"])
IDS = ["%s%d-%s" % c for c in tx.CONFIGS]
X4 = [(3, 7), (3, 30), (5, 28, 31), (40, 2)]  # context-only, both sides, a field nowhere


def _dev(dev, request):
    return request.getfixturevalue("gpu_device") if dev == "gpu" else CPU


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)


def _rows(e, keys, fgid, X, layout="csr", fold=False):
    return e.pool_rows(tx._batch(keys, fgid, layout, e.device), crosses=X, fold=fold)


def _subset(e, cx, px, index, ptr, X):
    """cx / px: (vectors, operand rows) of the contexts and of the pool."""
    return e.pool_subset(cx[0], px[0], _i32(index, e.device), _i32(ptr, e.device), crosses=X,
                         ctx_ops=cx[1], pool_ops=px[1]).cpu().numpy()


@BOTH
@pytest.mark.parametrize("spec", sorted(tx.SPECS))
@pytest.mark.parametrize("i", range(len(tx.CONFIGS)), ids=IDS)
def test_crossed_subset_within_the_float64_bound(dev, i, spec, request):
    """Every request of test_rank_cross against the pool indices of its own
    candidates: ref64's own bound on the expanded rows.  For LR under the pair
    cross the same call without crosses misses it on most rows."""
    c, layout, X = tx.CONFIGS[i], ("csr", "rm", "fm")[i % 3], tx.SPECS[spec]
    ctx, cf, cands, df = req = tx._requests(layout)
    rows, _ = tx._expand(*req, tx.CAND_COUNTS, X)
    e = tx._engine(c, i, _dev(dev, request), rows, len(X))
    index, ptr = np.arange(len(cands)), np.concatenate([[0], np.cumsum(tx.CAND_COUNTS)])
    p = _subset(e, _rows(e, ctx, cf, X, fold=True), _rows(e, cands, df, X, layout), index, ptr, X)
    ref = tx._ref(e, c, rows)
    err = np.abs(p.astype(np.float64) - ref.p)
    print("%s %s %s: worst error/bound %.3g" % (c, layout, spec, float((err / ref.e_p).max())))
    assert (err <= ref.e_p).all()
    if c[0] == "lr" and spec == "pair":
        bare = e.pool_subset(e.pool_rows(tx._batch(ctx, cf, "csr", e.device)),
                             e.pool_rows(tx._batch(cands, df, layout, e.device)),
                             _i32(index, e.device), _i32(ptr, e.device)).cpu().numpy()
        assert (np.abs(bare.astype(np.float64) - ref.p) > ref.e_p).mean() > 0.5


@BOTH
@pytest.mark.parametrize("i", [0, 4, 8], ids=["lr", "fm8-standard", "fm32-standard"])
def test_no_bit_depends_on_the_company(dev, i, request):
    dev, c = _dev(dev, request), tx.CONFIGS[i]
    rng = np.random.default_rng(11)
    # contexts that hold fields 0 .. 25 (complete (3, 7)), none, and only field 3
    cf = [np.arange(26, dtype=np.int32), np.arange(200, 226, dtype=np.int32),
          np.full(26, 3, np.int32), np.arange(26, dtype=np.int32)[::-1].copy()]
    ctx = [tx._keys(rng, 26) for _ in cf]
    df = [np.arange(26, 39, dtype=np.int32)] * 200
    cands = [tx._keys(rng, 13) for _ in df]
    rows = tx._expand(ctx, cf, cands * 4, df * 4, [200] * 4, X4)[0]
    e = tx._engine(c, i, dev, rows, len(X4), pool_subset_stage=True)
    cx, px = _rows(e, ctx, cf, X4, fold=True), _rows(e, cands, df, X4, "rm")
    ref = tx._ref(e, c, rows)
    full = _subset(e, cx, px, np.tile(np.arange(200), 4), np.arange(5) * 200, X4)  # [q][n]
    assert (np.abs(full.astype(np.float64) - ref.p) <= ref.e_p).all()
    want = _bits(full).reshape(4, 200)
    one = lambda q: tuple(t[q:q + 1] for t in cx)
    index = rng.integers(0, 200, 70)
    for q in range(4):  # alone, reversed, split over two calls
        assert np.array_equal(_bits(_subset(e, one(q), px, index, [0, 70], X4)), want[q, index])
        assert np.array_equal(_bits(_subset(e, one(q), px, index[::-1], [0, 70], X4)), want[q, index[::-1]])
        assert np.array_equal(_bits(_subset(e, one(q), px, index[:33], [0, 33], X4)), want[q, index[:33]])
    # 513 entries: empty requests at the start, in the middle and at the end,
    # lists across a wave and a workgroup edge, a slice of a larger pool
    qmap, ptr = np.array([0, 1, 2, 3, 0, 1, 2]), np.cumsum([0, 0, 200, 0, 100, 1, 212, 0])
    index = rng.integers(0, 100, 513)
    q = qmap[np.searchsorted(ptr, np.arange(513), side="right") - 1]
    sub = (px[0][50:150].contiguous(), px[1][50:150].contiguous())
    mixed = lambda eng: _bits(_subset(eng, tuple(t[torch.from_numpy(qmap).to(dev)] for t in cx), sub,
                                      index, ptr, X4))
    assert np.array_equal(mixed(e), want[q, index + 50])
    d = tx._engine(c, i, dev, rows, len(X4), pool_subset_stage=False)
    assert np.array_equal(mixed(d), want[q, index + 50])


@BOTH
@pytest.mark.parametrize("i", [0, 4], ids=["lr", "fm8-standard"])
def test_folded_contexts(dev, i, request):
    """Contexts 1 and 0 of test_rank_cross complete none and 15 of the full
    spec's crosses: folding changes the second vector alone; unfolded vectors
    are the uncrossed ones."""
    X = tx.SPECS["full"]
    ctx, cf, _, _ = req = tx._requests("csr")
    e = tx._engine(tx.CONFIGS[i], i, _dev(dev, request), tx._expand(*req, tx.CAND_COUNTS, X)[0], len(X))
    folded, ops = _rows(e, ctx[:2], cf[:2], X, fold=True)
    plain, ops2 = _rows(e, ctx[:2], cf[:2], X)
    assert torch.equal(ops, ops2)
    f, p = _bits(folded.cpu().numpy()), _bits(plain.cpu().numpy())
    assert np.array_equal(f[1], p[1]) and not np.array_equal(f[0], p[0])
    bare = e.pool_rows(tx._batch(ctx[:2], cf[:2], "csr", e.device))
    assert np.array_equal(p, _bits(bare.cpu().numpy()))


@BOTH
def test_operand_rows(dev, request):
    """A field twice, only past the 64th entry, absent, and first with key ~0."""
    X = [(3, 7), (5, 9, 3)]  # distinct fields in slot order: 3, 7, 5, 9
    rng = np.random.default_rng(2)
    f = [np.array([3, 3, 7]), np.arange(200, 270), np.array([7, 1, 7]), np.zeros(0, int), np.arange(130) % 10]
    f[1][66], f[1][69] = 5, 5
    keys = [tx._keys(rng, len(x)) for x in f]
    keys[2][0] = tx.NONE
    e = tx._engine(tx.CONFIGS[0], 0, _dev(dev, request), [np.zeros(2, np.uint64)], 2)
    got = _rows(e, keys, [x.astype(np.int32) for x in f], X)[1].cpu().numpy().view(np.uint64)
    want = np.full((len(f), 5), tx.NONE)
    for r, (k, x) in enumerate(zip(keys, f)):
        at = [np.flatnonzero(x == u) for u in (3, 7, 5, 9)]
        want[r, 0] = sum(1 << u for u, a in enumerate(at) if len(a))
        for u, a in enumerate(at):
            if len(a):
                want[r, 1 + u] = k[a[0]]
    assert np.array_equal(got, want) and e.pool_ops_width(X) == 5


def _snapshot(dev, tmp_path):
    rng = np.random.default_rng(3)
    cf, df = list(range(26)), list(range(26, 39))
    ctx = [tx._keys(rng, 26) for _ in range(3)]
    cands = [tx._keys(rng, 13) for _ in range(300)]
    rows = tx._expand(ctx, [np.array(cf)] * 3, cands * 3, [np.array(df)] * 900, [300] * 3, X4)[0]
    checkpoint.save_serving(tx._engine(tx.CONFIGS[0], 0, dev, rows, len(X4)), str(tmp_path / "s"), 0, 1,
                            meta=checkpoint.cross_meta(X4, 64), barrier=lambda: None)
    ls = lambda parts: [k.tolist() for k in parts]
    return ls(ctx), [cf] * 3, ls(cands), [df] * 300, [rng.integers(0, 300, n).tolist() for n in (0, 200, 131)]


@BOTH
def test_rank_pool_of_a_crossed_model(dev, tmp_path, request):
    dev = _dev(dev, request)
    ctx, cf, cands, df, subsets = _snapshot(dev, tmp_path)
    want = None
    for max_scores in (1 << 26, 210):  # one chunk; chunks of [0, 200] and [131] entries
        pred = Predictor(str(tmp_path / "s"), device=dev, max_rows=256, pool_max_scores=max_scores)
        pool = pred.build_pool(cands, fields=df)  # (two chunks of rows)
        p = pred.rank_pool(ctx, pool, subsets=subsets, context_fields=cf)
        if want is None:
            e, A = pred.engine, lambda parts, dt: [np.array(x, dt) for x in parts]
            cx = _rows(e, A(ctx, np.uint64), A(cf, np.int32), X4, fold=True)
            ptr = tr._ptr(subsets)
            want = np.split(_subset(e, cx, (pool.vecs, pool.ops), np.concatenate(subsets), ptr, X4), ptr[1:-1])
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(p, want))
    whole = pred.rank_pool(ctx, pool, context_fields=cf)
    again = pred.rank_pool(ctx, pool, subsets=[list(range(300))] * 3, context_fields=cf)
    assert all(np.array_equal(_bits(a), _bits(b)) and a.shape == (300,) for a, b in zip(whole, again))
    for q, (idx, sc) in enumerate(pred.rank_pool(ctx, pool, top_k=10, context_fields=cf)):
        key = np.where(whole[q] > 0, whole[q], 0).astype(F32).view(np.uint32).astype(np.int64)
        best = np.lexsort((np.arange(300), -key))[:10]
        assert np.array_equal(idx, best) and np.array_equal(_bits(sc), _bits(whole[q][best]))
    with pytest.raises(ValueError):
        pred.rank_pool(ctx, pool, subsets=subsets)
    with pytest.raises(ValueError, match="rank_keys"):
        pred.build_pool(cands)


def test_routes_take_fields(tmp_path):
    pytest.importorskip("fastapi")
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    ctx, cf, cands, df, _ = _snapshot(CPU, tmp_path)
    pred = Predictor(str(tmp_path / "s"), device=CPU)
    c = TestClient(make_app(pred))
    assert c.post("/pool", json={"name": "a", "candidates": cands[:9], "fields": df[:9]}).status_code == 200
    want = pred.rank_pool(ctx[:2], pred.build_pool(cands[:9], fields=df[:9]), subsets=[[8, 0, 8], [3]],
                          context_fields=cf[:2])
    r = c.post("/rank", json={"pool": "a", "context": ctx[0], "pool_index": [8, 0, 8],
                              "context_fields": cf[0]})
    assert r.status_code == 200 and np.array_equal(F32(r.json()["pctr"]), want[0])
    r = c.post("/rank", json={"pool": "a", "contexts": ctx[:2], "pool_index": [[8, 0, 8], [3]],
                              "context_fields": cf[:2]})
    assert [np.array_equal(F32(x), w) for x, w in zip(r.json()["pctr"], want)] == [True, True]
    assert c.post("/rank", json={"pool": "a", "context": ctx[0], "pool_index": [3]}).status_code == 400
    assert c.post("/pool", json={"name": "b", "candidates": cands[:9]}).status_code == 400
