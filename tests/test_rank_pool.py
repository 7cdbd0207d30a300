"""Candidate pools (kernels_pool.hip, docs/DESIGN.md §2): R contexts scored
against a resident pool of N candidates as one matrix product of their pool
vectors.  A score is an fp32 evaluation of the model on the row (context keys,
then candidate keys) in a regrouped association, so it is held to ref64's bound
on those rows; a vector depends on its row alone and a score on its two
vectors alone, so no bit may depend on what else a call holds."""
import numpy as np
import pytest
import torch

from test_rank import CONFIGS, CPU, F32, _batch, _bits, _engine, _keys, _ptr
from test_serving_refresh import _trainer, _ver

from xflow_amd import checkpoint
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Batch, Engine
from xflow_amd.serve import Predictor
from xflow_amd.testing import ref64

# the wave edges of a context's lanes; -1 / -5: keys 1..4 / 5..8, the clamps
CTX_LENS = [63, -1, 64, 0, 130, 65, 1, -5]
ROW_LENS = [0, 7, 8, 9, 17]  # the probe chunk edges
POOLS = [1, 127, 128, 129]   # the workgroup tile of 128 candidates
REQS = [1, 31, 32, 33]       # the matrix instruction's 32 requests
IDS = ["%s%d-%s" % c for c in CONFIGS]


def _vecs(e, rows, layout="csr"):
    return e.pool_rows(_batch(rows, layout, e.device))


def _within_bound(dev, i):
    """Every (context, candidate) pair of every R x N shape against ref64 on
    the concatenated row.  ref.e_p holds for any fp32 evaluation order of y:
    the regrouped form's absolute-value expression A_r + A_i + sum |vs_r| |vs_i|
    is the row's own A, and its longest rounding chain -- a lane's share of a
    part, 6 butterfly steps, the finish, Dk + 2 accumulations -- is below the
    row's N."""
    c = CONFIGS[i]
    e = _engine(c, i, dev)
    assert e.pools and e.pool_width % 4 == 0
    rng = np.random.default_rng(5)
    ctx = [_keys(rng, n) if n >= 0 else np.arange(-n, -n + 4, dtype=np.uint64)
           for n in CTX_LENS + [q % 5 for q in range(8, max(REQS))]]  # (the rest: short, for R)
    cv = _vecs(e, ctx)
    worst = 0.0
    for j, N in enumerate(POOLS):
        layout = ("csr", "rm", "fm")[(i + j) % 3]
        lens = [ROW_LENS[r % 5] for r in range(N)] if layout == "csr" else [9 if layout == "rm" else 17] * N
        cands = [_keys(rng, n) for n in lens]
        pv = _vecs(e, cands, layout)
        full = [np.concatenate([x, y]) for x in ctx for y in cands]
        keys = np.concatenate(full)
        uk = np.unique(keys)
        ref = ref64.reference(c[0], c[1], uk, e.pull(uk), keys, _ptr(full), fm_math=c[2])
        rp, re, ry = (a.reshape(len(ctx), N) for a in (ref.p, ref.e_p, ref.y))
        for R in REQS:
            p = e.pool_score(cv[:R], pv).cpu().numpy()
            err = np.abs(p.astype(np.float64) - rp[:R])
            worst = max(worst, float((err / re[:R]).max()))
            assert p.shape == (R, N) and (err <= re[:R]).all(), (R, N, worst)
            if R > 7:
                assert (ry[1] > 31).all() and (p[1] == 1.0).all()         # the upper clamp
                assert (ry[7] < -31).all() and (p[7] == F32(1e-6)).all()  # the lower clamp
    print("%s: worst error/bound %.3g" % (c, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CONFIGS)), ids=IDS)
def test_pool_scores_within_the_float64_bound(gpu_device, i):
    """Worst error/bound ratio on an MI355X: the printed line of each case."""
    _within_bound(gpu_device, i)


@pytest.mark.parametrize("i", range(len(CONFIGS)), ids=IDS)
def test_pool_scores_within_the_float64_bound_cpu(i):
    _within_bound(CPU, i)


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 6], ids=["lr", "fm8-standard"])
def test_no_bit_depends_on_the_company(gpu_device, i):
    e = _engine(CONFIGS[i], i, gpu_device)
    rng = np.random.default_rng(11)
    ctx, others = _keys(rng, 26), [_keys(rng, 30) for _ in range(40)]
    rows = [_keys(rng, 13) for _ in range(500)]
    pv, big = _vecs(e, rows[150:350]), _vecs(e, rows, "rm")
    assert np.array_equal(_bits(pv.cpu()), _bits(big[150:350].cpu()))
    assert np.array_equal(_bits(big.cpu()), _bits(_vecs(e, rows, "fm").cpu()))
    cv = _vecs(e, [ctx])
    assert np.array_equal(_bits(cv.cpu()), _bits(_vecs(e, others[:17] + [ctx] + others[17:])[17:18].cpu()))
    alone = _bits(e.pool_score(cv, pv).cpu())
    among = e.pool_score(_vecs(e, others[:17] + [ctx] + others[17:]), pv)
    assert np.array_equal(alone[0], _bits(among.cpu())[17])
    assert np.array_equal(alone, _bits(e.pool_score(cv, big)[:, 150:350].cpu()))
    assert np.array_equal(alone, _bits(e.pool_score(cv, pv.flip(0).contiguous()).flip(1).cpu()))


def _lexsort_topk(p, k):
    key = np.where(p > 0, p, 0).astype(np.float32).view(np.uint32).astype(np.int64)
    o = np.lexsort((np.arange(len(p)), -key))[:k]
    return o.astype(np.int32), p[o]


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 6], ids=["lr", "fm8-standard"])
def test_rank_pool_topk_chunked_and_not(gpu_device, i, tmp_path):
    checkpoint.save_serving(_engine(CONFIGS[i], i, gpu_device), str(tmp_path / "s"), 0, 1,
                            barrier=lambda: None)
    rng = np.random.default_rng(3)
    ctx = [_keys(rng, 26).tolist() for _ in range(5)]
    rows = [_keys(rng, 13).tolist() for _ in range(1500)]
    want = None
    for max_scores in (1 << 26, 2 * 1500):  # one chunk; chunks of two requests
        pred = Predictor(str(tmp_path / "s"), device=gpu_device, max_rows=1024,
                         pool_max_scores=max_scores)
        pool = pred.build_pool(rows)  # (two chunks of rows)
        p = pred.rank_pool(ctx, pool)
        assert len(p) == 5 and all(x.shape == (1500,) and x.dtype == F32 for x in p)
        want = p if want is None else want
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(p, want))
        for k in (1, 10, 1024):
            for q, (idx, sc) in enumerate(pred.rank_pool(ctx, pool, top_k=k)):
                wi, ws = _lexsort_topk(p[q], k)
                assert np.array_equal(idx, wi) and np.array_equal(_bits(sc), _bits(ws))


@pytest.mark.gpu
def test_a_pool_follows_refresh(gpu_device, tmp_path):
    sroot = tmp_path / "serving"
    t = _trainer(tmp_path, sroot, full_every=8)
    try:
        t.train_epochs(2)
    finally:
        t.close()
    checkpoint.publish_serving(str(sroot), 1, keep=99)
    pred = Predictor(str(sroot), device=gpu_device, max_rows=64)
    uk = pred.engine.export_table()[0]
    rng = np.random.default_rng(2)
    rows = [rng.choice(uk, 13).tolist() for _ in range(150)]
    ctx = [rng.choice(uk, 26).tolist() for _ in range(3)]
    pool = pred.build_pool(rows)
    old = np.stack(pred.rank_pool(ctx, pool))
    checkpoint.publish_serving(str(sroot), 2, keep=99)
    assert pred.refresh()["mode"] == "delta"
    got = np.stack(pred.rank_pool(ctx, pool))
    fresh = Predictor(_ver(sroot, 2), device=gpu_device, max_rows=64)
    assert np.array_equal(_bits(got), _bits(np.stack(fresh.rank_pool(ctx, fresh.build_pool(rows)))))
    assert np.array_equal(_bits(got), _bits(np.stack(pred.rank_pool(ctx, pred.build_pool(rows)))))
    assert not np.array_equal(_bits(got), _bits(old))


# ---- CPU -----------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["mvm-snapshot", "crossed-lr", "full-lr"])
def test_build_pool_refuses_what_does_not_decompose(tmp_path, what):
    model = ModelConfig(kind="mvm", v_dim=3) if what == "mvm-snapshot" else ModelConfig(kind="lr")
    src = Engine(model, OptimConfig(kind="sgd"),
                 EngineConfig(table_log2_cap=10, max_rows=16, max_nnz=64), device=CPU)
    src.train_step(Batch(keys=torch.arange(1, 33, dtype=torch.int64), labels=torch.ones(8),
                         fgid=torch.arange(32, dtype=torch.int32) % 4, nnz_per_row=4))
    if what == "full-lr":
        checkpoint.save(src, str(tmp_path), 0, 1, barrier=lambda: None)
    else:
        meta = checkpoint.cross_meta([(0, 3)], 5) if what == "crossed-lr" else None
        checkpoint.save_serving(src, str(tmp_path), 0, 1, meta=meta, barrier=lambda: None)
    with pytest.raises(ValueError, match="rank_keys" if what == "crossed-lr" else "snapshot"):
        Predictor(str(tmp_path), device=CPU, max_rows=4).build_pool([[1, 2], [3]])


def test_engine_refusals():
    cfg = EngineConfig(table_log2_cap=10, max_rows=16, max_nnz=64)
    live = Engine(ModelConfig(kind="lr"), OptimConfig(kind="ftrl"), cfg, device=CPU)
    rows = [np.arange(100, 104, dtype=np.uint64)]
    assert not live.pools
    with pytest.raises(RuntimeError):
        _vecs(live, rows)
    e = _engine(CONFIGS[6], 6, CPU)
    v = _vecs(e, rows)
    assert v.shape == (1, e.pool_width) and e.pool_width == 12
    for bad in (v[:, :8].contiguous(), torch.zeros(1, 16)):
        with pytest.raises(ValueError):
            e.pool_score(bad, v)
        with pytest.raises(ValueError):
            e.pool_score(v, bad)
