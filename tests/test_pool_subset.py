"""Pool subsets (kernels_pool_subset.hip, docs/DESIGN.md §2): every request
scored against its own list of candidates of a resident pool.  An entry is an
fp32 evaluation of the model on the row (context keys, then candidate keys), so
it is held to ref64's bound on that row; it depends on its own two vectors
alone, so no bit may depend on what else a call holds, where the entry stands
or how the kernel gathers the rows."""
import numpy as np
import pytest
import torch

from test_rank import CONFIGS, CPU, F32, _batch, _bits, _engine, _keys, _ptr
from test_rank_pool import CTX_LENS, IDS, ROW_LENS, _lexsort_topk

from xflow_amd import checkpoint
from xflow_amd.serve import Predictor, make_app
from xflow_amd.testing import ref64

N, R = 129, 33
BOTH = pytest.mark.parametrize("dev", [pytest.param("gpu", marks=pytest.mark.gpu), "cpu"])


def _dev(dev, request):
    return request.getfixturevalue("gpu_device") if dev == "gpu" else CPU


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)


def _subset(e, cv, pv, index, ptr):
    return e.pool_subset(cv, pv, _t(index, e.device), _t(ptr, e.device)).cpu().numpy()


def _cases(rng):
    """(context of every request, req_ptr, index): flat lists of every length
    around the wave (64) and the workgroup (256)."""
    for M in (0, 1, 63, 64, 65, 255, 256, 257, 513):
        index = rng.integers(0, N, M)
        index[1:2] = index[:1]  # a repeated index
        # one request owns everything, between requests without candidates
        yield [0, (1, 7, 4)[M % 3], 2], [0, 0, M, M], index
        if M == 64:  # a wave of one-entry requests
            yield np.arange(64) % R, np.arange(65), index
        if M == 257:  # every context, the two clamps among them
            yield np.arange(R), np.concatenate([[0], np.sort(rng.integers(0, M + 1, R - 1)), [M]]), index
        if M == 513:  # empty at the start, in the middle, at the end; [200, 300) crosses a tile
            yield [0, 1, 2, 7, 4, 5, 6], np.cumsum([0, 0, 200, 0, 100, 1, 212, 0]), index


def _within_bound(dev, i):
    c = CONFIGS[i]
    e = _engine(c, i, dev)
    rng = np.random.default_rng(5)
    ctx = [_keys(rng, n) if n >= 0 else np.arange(-n, -n + 4, dtype=np.uint64)
           for n in CTX_LENS + [q % 5 for q in range(8, R)]]
    cands = [_keys(rng, ROW_LENS[r % 5]) for r in range(N)]
    cv, pv = e.pool_rows(_batch(ctx, "csr", dev)), e.pool_rows(_batch(cands, "csr", dev))
    full = [np.concatenate([x, y]) for x in ctx for y in cands]
    keys = np.concatenate(full)
    uk = np.unique(keys)
    ref = ref64.reference(c[0], c[1], uk, e.pull(uk), keys, _ptr(full), fm_math=c[2])
    rp, re, ry = (a.reshape(R, N) for a in (ref.p, ref.e_p, ref.y))
    assert (ry[1] > 31).all() and (ry[7] < -31).all()
    worst = 0.0
    for qmap, ptr, index in _cases(rng):
        qmap, ptr = np.asarray(qmap), np.asarray(ptr)
        p = _subset(e, cv[torch.from_numpy(qmap).to(dev)], pv, index, ptr)
        q = qmap[np.searchsorted(ptr, np.arange(len(index)), side="right") - 1]
        err = np.abs(p.astype(np.float64) - rp[q, index])
        worst = max([worst] + list(err / re[q, index]))
        assert p.shape == index.shape and (err <= re[q, index]).all(), (len(index), worst)
        assert (p[q == 1] == 1.0).all() and (p[q == 7] == F32(1e-6)).all()  # the clamps
    print("%s: worst error/bound %.3g" % (c, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CONFIGS)), ids=IDS)
def test_subset_scores_within_the_float64_bound(gpu_device, i):
    """Worst error/bound ratio on an MI355X: the printed line of each case."""
    _within_bound(gpu_device, i)


@pytest.mark.parametrize("i", range(len(CONFIGS)), ids=IDS)
def test_subset_scores_within_the_float64_bound_cpu(i):
    _within_bound(CPU, i)


def _vectors(e, seed, n_ctx=5, n_rows=500):
    rng = np.random.default_rng(seed)
    cv = e.pool_rows(_batch([_keys(rng, 26) for _ in range(n_ctx)], "csr", e.device))
    return cv, e.pool_rows(_batch([_keys(rng, 13) for _ in range(n_rows)], "rm", e.device)), rng


@BOTH
@pytest.mark.parametrize("i", [0, 6], ids=["lr", "fm8-standard"])
def test_a_bad_index_scores_zero_and_reads_nothing(dev, i, request):
    e = _engine(CONFIGS[i], i, _dev(dev, request))
    cv, pv, rng = _vectors(e, 7, n_rows=N)
    index, ptr = rng.integers(0, N, 300), [0, 70, 70, 130, 299, 300]
    bad = index.copy()
    at = [0, 1, 63, 64, 69, 70, 255, 256, 299]
    bad[at] = [-1, N, 2 ** 31 - 1] * 3
    want, got = _bits(_subset(e, cv, pv, index, ptr)), _bits(_subset(e, cv, pv, bad, ptr))
    assert (got[at] == 0).all() and (want[at] != 0).all()
    got[at] = want[at]
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 4, 6, 10], ids=["lr", "fm3-standard", "fm8-standard", "fm32-standard"])
def test_no_bit_depends_on_the_company(gpu_device, i):
    e = _engine(CONFIGS[i], i, gpu_device, pool_subset_stage=True)
    cv, big, rng = _vectors(e, 11)
    pv = big[150:350].contiguous()
    alone = _bits(_subset(e, cv[2:3], pv, [77], [0, 1]))[0]
    index = rng.integers(0, 200, 300)
    index[[0, 63, 64, 256]] = 77
    among = _bits(_subset(e, cv[2:3], pv, index, [0, 300]))
    assert (among[[0, 63, 64, 256]] == alone).all()
    # another request numbering, a slice of a larger pool
    ptr = [0, 10, 10, 290, 300, 300]
    renumbered = _bits(_subset(e, cv[[4, 0, 2, 1, 3]], pv, index, ptr))
    assert np.array_equal(renumbered[10:290], among[10:290])
    assert np.array_equal(_bits(_subset(e, cv[2:3], big, index + 150, [0, 300])), among)
    if e.pool_width > 4:  # the staged gather against every lane's own loads
        d = _engine(CONFIGS[i], i, gpu_device, pool_subset_stage=False)
        assert np.array_equal(_bits(_subset(d, cv[[4, 0, 2, 1, 3]], pv, index, ptr)), renumbered)
        assert np.array_equal(_bits(_subset(d, cv[2:3], big, index + 150, [0, 300])), among)


def _snapshot(i, dev, tmp_path):
    checkpoint.save_serving(_engine(CONFIGS[i], i, dev), str(tmp_path / "s"), 0, 1,
                            barrier=lambda: None)
    rng = np.random.default_rng(3)
    return ([_keys(rng, 26).tolist() for _ in range(5)], [_keys(rng, 13).tolist() for _ in range(1500)],
            [rng.integers(0, 1500, n).tolist() for n in (0, 1, 700, 1500, 3)])


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 6], ids=["lr", "fm8-standard"])
def test_rank_pool_subsets_chunked_and_not(gpu_device, i, tmp_path):
    ctx, rows, subsets = _snapshot(i, gpu_device, tmp_path)
    want = None
    for max_scores in (1 << 26, 1503):  # one chunk; chunks of [0, 1, 700] and [1500, 3] entries
        pred = Predictor(str(tmp_path / "s"), device=gpu_device, max_rows=1024,
                         pool_max_scores=max_scores)
        pool = pred.build_pool(rows)  # (two chunks of rows)
        p = pred.rank_pool(ctx, pool, subsets=subsets)
        assert [x.shape for x in p] == [(len(s),) for s in subsets] and all(x.dtype == F32 for x in p)
        if want is None:
            e = pred.engine
            cv = e.pool_rows(_batch([np.array(c, np.uint64) for c in ctx], "csr", gpu_device))
            want = np.split(_subset(e, cv, pool.vecs, np.concatenate(subsets), _ptr(subsets)),
                            _ptr(subsets)[1:-1])
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(p, want))
        for k in (1, 10, 1024):
            for q, (idx, sc) in enumerate(pred.rank_pool(ctx, pool, top_k=k, subsets=subsets)):
                wi, ws = _lexsort_topk(p[q], k)
                assert len(idx) == min(k, len(subsets[q])) and idx.dtype == np.int32
                assert np.array_equal(idx, np.array(subsets[q], np.int32)[wi])
                assert np.array_equal(_bits(sc), _bits(ws))
    with pytest.raises(ValueError):
        pred.rank_pool(ctx[:1], pool, subsets=[[1500]])


def test_rank_route_takes_pool_index(tmp_path):
    pytest.importorskip("fastapi")
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    ctx, rows, _ = _snapshot(0, CPU, tmp_path)
    pred = Predictor(str(tmp_path / "s"), device=CPU)
    c = TestClient(make_app(pred))
    assert c.post("/pool", json={"name": "a", "candidates": rows[:9]}).status_code == 200
    want = pred.rank_pool(ctx[:2], pred.build_pool(rows[:9]), subsets=[[8, 0, 8], [3]])
    r = c.post("/rank", json={"pool": "a", "context": ctx[0], "pool_index": [8, 0, 8]})
    assert r.status_code == 200 and np.array_equal(F32(r.json()["pctr"]), want[0])
    r = c.post("/rank", json={"pool": "a", "contexts": ctx[:2], "pool_index": [[8, 0, 8], [3]],
                              "top_k": 2})
    first = np.array([8, 0, 8])[_lexsort_topk(want[0], 2)[0]].tolist()
    assert [x["index"] for x in r.json()["results"]] == [first, [3]]
    assert c.post("/rank", json={"pool": "a", "context": ctx[0], "pool_index": [9]}).status_code == 400
