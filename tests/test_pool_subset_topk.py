"""Pool subset top-k (kernels_pool_subset_topk.hip, docs/DESIGN.md §2): every
request's best k entries of its own list, scored and selected in one kernel.
The fused scores have pool_subset's bits by construction and pool_subset is held
to ref64 (test_pool_subset.py), so the reference is a numpy lexsort of
Engine.pool_subset's scores by (sort key descending, position ascending), cut at
k and mapped through index; a score of sort key 0 compares as +0.0."""
import numpy as np
import pytest
import torch

from test_pool_subset import BOTH, _dev, _t
from test_rank import CONFIGS, CPU, F32, _batch, _bits, _engine, _keys
from test_rank_pool import _lexsort_topk

from xflow_amd import checkpoint
from xflow_amd.serve import Predictor

N, C = 300, 7  # pool candidates (100 .. 149 are one row: 50 equal scores), contexts
# CONFIGS index, pool_subset_stage: LR (W = 4), reference FM-8 (KP = 4), standard
# FM-8 (W = 12, direct), standard FM-32 (W = 36) staged and forced direct
MODELS = [(0, None), (5, None), (6, None), (10, True), (10, False)]
IDS = ["lr", "fm8-reference", "fm8-standard", "fm32-staged", "fm32-direct"]


def _setup(i, dev, **kw):
    e = _engine(CONFIGS[i], i, dev, **kw)
    rng = np.random.default_rng(9)
    ctx = [_keys(rng, 26) for _ in range(C - 1)] + [np.arange(1, 5, dtype=np.uint64)]  # (clamped: all tie)
    cands = [_keys(rng, 13) for _ in range(N)]
    cands[100:150] = [cands[100]] * 50
    return e, e.pool_rows(_batch(ctx, "csr", dev)), e.pool_rows(_batch(cands, "rm", dev))


def _lists():
    """(req_ptr, index): one request around the wave and the tile, one over
    three tiles (two merge rounds at k = 1024), 40 requests with empty ones and
    one across entry 4096, 256 requests of 16."""
    rng = np.random.default_rng(4)
    many = rng.integers(1, 301, 40)
    many[[0, 7, 8, 39]] = 0
    for lens in [[n] for n in (1, 63, 64, 65, 4095, 4096, 4097, 9000)] + [many, [16] * 256]:
        ptr = np.concatenate([[0], np.cumsum(lens)])
        index = rng.integers(0, N, ptr[-1])
        if ptr[-1] > 64:
            index[5:55] = rng.permutation(np.arange(100, 150))  # equal scores, by position
            index[[3, 60]] = -1, N                              # out of range: +0.0, last
        yield ptr, index
    assert ptr[-1] == 4096 and 4096 not in np.cumsum(many) and many.sum() > 4096


def _want(p, index, ptr, k):
    idx, sc = np.full((len(ptr) - 1, k), -1, np.int32), np.zeros((len(ptr) - 1, k), F32)
    for q, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        o, s = _lexsort_topk(p[a:b], k)
        idx[q, :len(o)], sc[q, :len(o)] = index[a:b][o], np.where(s > 0, s, 0)
    return idx, _bits(sc)


def _got(e, cv, pv, it, pt, k):
    idx, sc = (t.cpu().numpy() for t in e.pool_subset_topk(cv, pv, it, pt, k))
    assert idx.dtype == np.int32 and sc.dtype == F32 and idx.shape == sc.shape == (len(pt) - 1, k)
    return idx, _bits(np.where(sc > 0, sc, 0))


def _check(dev, i, stage):
    kw = {"pool_subset_topk_fused_max": 0}  # (the kernel at every size)
    if stage is not None:
        kw["pool_subset_stage"] = stage
    e, cv, pv = _setup(i, dev, **kw)
    gpu = dev.type != "cpu"
    assert e.pool_subset_topk_fused == gpu
    if gpu:  # the composed path of the same build, and the CPU backend
        d = _setup(i, dev, pool_subset_topk_fused=False, **kw)[0]
        c, ccv, cpv = _setup(i, CPU)
        assert not d.pool_subset_topk_fused
    for ptr, index in _lists():
        it, pt = _t(index, dev), _t(ptr, dev)
        qv = cv[torch.arange(len(ptr) - 1, device=dev) % C]
        p = e.pool_subset(qv, pv, it, pt).cpu().numpy()
        for k in (1, 10, 1024):
            want = _want(p, index, ptr, k)
            got = _got(e, qv, pv, it, pt, k)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (len(index), k)
            if gpu:
                ab = _got(d, qv, pv, it, pt, k)
                assert np.array_equal(ab[0], want[0]) and np.array_equal(ab[1], want[1])
                cpu = _got(c, ccv[torch.arange(len(ptr) - 1) % C], cpv, _t(index, CPU), _t(ptr, CPU), k)
                assert np.array_equal(cpu[0], want[0]), (len(index), k)


@pytest.mark.gpu
@pytest.mark.parametrize("i,stage", MODELS, ids=IDS)
def test_fused_equals_the_sorted_subset_scores(gpu_device, i, stage):
    _check(gpu_device, i, stage)


@pytest.mark.parametrize("i,stage", MODELS[:3], ids=IDS[:3])
def test_cpu_backend_equals_the_sorted_subset_scores(i, stage):
    _check(CPU, i, stage)


@BOTH
def test_ties_keep_their_position_and_bad_indices_rank_last(dev, request):
    dev = _dev(dev, request)
    e, cv, pv = _setup(6, dev)
    tied = np.random.default_rng(1).permutation(np.arange(100, 150))
    idx, sc = e.pool_subset_topk(cv[:1], pv, _t(tied, dev), _t([0, 50], dev), 60)
    assert np.array_equal(idx.cpu().numpy()[0], np.concatenate([tied, [-1] * 10]))
    assert len(set(_bits(sc.cpu())[0, :50])) == 1 and (_bits(sc.cpu())[0, 50:] == 0).all()
    idx, sc = e.pool_subset_topk(cv[:2], pv, _t([N, 5, -1, 7, -1], dev), _t([0, 4, 5], dev), 4)
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    assert sorted(idx[0, :2]) == [5, 7] and list(idx[0, 2:]) == [N, -1] and list(idx[1]) == [-1] * 4
    assert (sc[0, :2] > 0).all() and (_bits(sc)[0, 2:] == 0).all() and (_bits(sc)[1] == 0).all()
    with pytest.raises(ValueError):
        e.pool_subset_topk(cv[:1], pv, _t(tied, dev), _t([0, 50], dev), 1025)


@BOTH
def test_rank_pool_top_k_equals_the_selection_from_all_scores(dev, request, tmp_path):
    dev = _dev(dev, request)
    checkpoint.save_serving(_engine(CONFIGS[6], 6, dev), str(tmp_path / "s"), 0, 1, barrier=lambda: None)
    rng = np.random.default_rng(3)
    ctx = [_keys(rng, 26).tolist() for _ in range(3)]
    subsets = [rng.integers(0, N, n).tolist() for n in (700, 0, 3)]
    pred = Predictor(str(tmp_path / "s"), device=dev, max_rows=1024)
    pool = pred.build_pool([_keys(rng, 13).tolist() for _ in range(N)])
    p = pred.rank_pool(ctx, pool, subsets=subsets)
    for q, (idx, sc) in enumerate(pred.rank_pool(ctx, pool, subsets=subsets, top_k=5)):
        wi, ws = _lexsort_topk(p[q], 5)
        assert idx.dtype == np.int32 and np.array_equal(idx, np.array(subsets[q], np.int32)[wi])
        assert np.array_equal(_bits(sc), _bits(ws))
