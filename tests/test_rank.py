"""Candidate ranking (k_rank_lr / k_rank_fm, docs/DESIGN.md §2): one context
scored against many candidate rows.  The kernel's result for a candidate is an
fp32 evaluation of the model on the row (context keys, then candidate keys), so
it is held to ref64's bound on those rows; its context sums are a function of
the context alone, so tiling and chunking may not change a bit."""
import numpy as np
import pytest
import torch

from xflow_amd import checkpoint
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Batch, Engine
from xflow_amd.serve import Predictor
from xflow_amd.testing import ref64

F32 = np.float32
CPU = torch.device("cpu")
LOG2 = 13  # 4008 planted keys in 8192 slots: load 0.49, chains leave the home slot
CONFIGS = [("lr", 0, "reference")] + [("fm", d, m) for d in (1, 3, 8, 10, 32)
                                      for m in ("reference", "standard")]
# request boundaries inside a tile (60), on a tile edge (64), across two tiles
# (134 .. 263 over 192 and 256); the request without candidates keeps a context
CTX_LENS = [63, -1, 64, 7, 130, 0, 65, 1, -5]  # (-1 / -5: keys 1..4 / 5..8, the clamps)
CAND_COUNTS = [60, 4, 70, 0, 129, 1, 5, 6, 3]
ROW_LENS = [0, 7, 8, 9, 17]  # the probe chunk edges for N = 8 and N = 4


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _engine(c, i, dev, **kw):
    kind, D, math = c
    model = ModelConfig(kind=kind, **({"v_dim": D, "fm_math": math} if kind == "fm" else {}))
    e = Engine(model, OptimConfig(kind="frozen", frozen_from=("ftrl", "sgd")[i % 2], sgd_v_init=0.003),
               EngineConfig(table_log2_cap=LOG2, max_rows=512, max_nnz=512 * 64, **kw), device=dev)
    rng = np.random.default_rng(31 + D)
    keys = np.concatenate([np.arange(1, 9), np.arange(100, 4100)]).astype(np.uint64)
    W = rng.normal(0, 0.05, (len(keys), 1 + D)).astype(F32)
    W[:, 0] = rng.normal(0, 0.3, len(keys))
    W[:4, 0], W[4:8, 0] = 12.0, -12.0
    e.import_weights(keys, W)
    return e


def _keys(rng, n):
    k = rng.integers(100, 5700, size=n).astype(np.uint64)  # about 30 % absent (>= 5100)
    k[k >= 4100] += 1000
    return k


def _requests(layout, seed=5):
    rng = np.random.default_rng(seed)
    ctx = [_keys(rng, abs(n)) if n >= 0 else np.arange(-n, -n + 4, dtype=np.uint64) for n in CTX_LENS]
    rows = sum(CAND_COUNTS)
    lens = (np.array([ROW_LENS[r % 5] for r in range(rows)]) if layout == "csr"
            else np.full(rows, 9 if layout == "rm" else 17))
    return ctx, [_keys(rng, n) for n in lens]


def _t(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)


def _ptr(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)


def _batch(cands, layout, dev):
    rows = len(cands)
    flat = np.concatenate(cands + [np.zeros(0, np.uint64)]).view(np.int64)
    lab = torch.zeros(rows, device=dev)
    if layout == "csr":
        return Batch(keys=_t(flat, np.int64, dev), labels=lab, row_ptr=_t(_ptr(cands), np.int32, dev))
    F = len(cands[0])
    flat = flat.reshape(rows, F)
    return Batch(keys=_t((flat.T if layout == "fm" else flat).reshape(-1), np.int64, dev), labels=lab,
                 nnz_per_row=F, field_major=layout == "fm")


def _rank(e, ctx, cands, counts, layout="csr"):
    dev = e.device
    ck = np.concatenate(ctx + [np.zeros(0, np.uint64)]).view(np.int64)
    return e.rank_step(_t(ck, np.int64, dev), _t(_ptr(ctx), np.int32, dev),
                       _t(np.concatenate([[0], np.cumsum(counts)]), np.int32, dev),
                       _batch(cands, layout, dev)).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CONFIGS)), ids=["%s%d-%s" % c for c in CONFIGS])
def test_rank_within_the_float64_bound(gpu_device, i):
    """ref64 on the rows (context, then candidate) with its own chain length
    N: the kernel adds no rounding beyond it.  A sum of n context and m
    candidate terms passes at most ceil(n / 64) - 1 additions in its lane, 6
    butterfly steps and m candidate additions that round, and the addition of
    an empty lane's or subtree's +0.0f is exact (n <= 64: at most ceil(log2 n)
    butterfly steps round) -- never more than the n + m of ref64's chain.
    Worst error/bound ratio on an MI355X: the printed line of each case."""
    c, layout = CONFIGS[i], ("csr", "rm", "fm")[i % 3]
    e = _engine(c, i, gpu_device, serve_fused=False)
    assert e.ranks and e.frozen
    ctx, cands = _requests(layout)
    p = _rank(e, ctx, cands, CAND_COUNTS, layout)
    req = np.repeat(np.arange(len(ctx)), CAND_COUNTS)
    full = [np.concatenate([ctx[q], cands[r]]) for r, q in enumerate(req)]
    keys = np.concatenate(full)
    uk = np.unique(keys)
    ref = ref64.reference(c[0], c[1], uk, e.pull(uk), keys, _ptr(full), fm_math=c[2])
    err = np.abs(p.astype(np.float64) - ref.p)
    print("%s %s: worst error/bound %.3g" % (c, layout, float((err / ref.e_p).max())))
    assert (err <= ref.e_p).all()
    assert (ref.y[req == 1] > 31).all() and (p[req == 1] == 1.0).all()         # the upper clamp
    assert (ref.y[req == 8] < -31).all() and (p[req == 8] == F32(1e-6)).all()  # the lower clamp
    assert np.array_equal(_bits(p), _bits(_rank(e, ctx, cands, CAND_COUNTS, layout)))


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 6], ids=["lr", "fm8-standard"])
def test_tiling_and_chunking_change_no_bit(gpu_device, i, tmp_path):
    e = _engine(CONFIGS[i], i, gpu_device)
    rng = np.random.default_rng(11)
    ctx, cands = _keys(rng, 26), [_keys(rng, 13) for _ in range(70)]
    other, before = _keys(rng, 30), [_keys(rng, 13) for _ in range(37)]
    alone = _rank(e, [ctx], cands, [70])
    assert np.array_equal(_bits(alone), _bits(_rank(e, [ctx], cands, [70])))
    assert np.array_equal(_bits(alone), _bits(_rank(e, [other, ctx], before + cands, [37, 70])[37:]))
    assert np.array_equal(_bits(alone), _bits(_rank(e, [ctx], cands[::-1], [70])[::-1]))
    checkpoint.save_serving(e, str(tmp_path / "s"), 0, 1, barrier=lambda: None)
    for max_rows in (64, 4096):
        pred = Predictor(str(tmp_path / "s"), device=gpu_device, max_rows=max_rows)
        assert pred.engine.ranks
        got = pred.rank_keys([other.tolist(), ctx.tolist()],
                             [[k.tolist() for k in before], [k.tolist() for k in cands]])
        assert np.array_equal(_bits(alone), _bits(got[1])) and got[0].shape == (37,)


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 6], ids=["lr", "fm8-standard"])
def test_an_empty_context_scores_like_eval_step(gpu_device, i):
    e = _engine(CONFIGS[i], i, gpu_device, serve_unfused_rows=(0, 0), serve_unfused_rows_latent=(0, 0))
    assert e.serve_fused
    _, cands = _requests("csr")
    want = e.eval_step(_batch(cands, "csr", gpu_device)).cpu().numpy()
    assert np.array_equal(_bits(want), _bits(_rank(e, [np.zeros(0, np.uint64)], cands, [len(cands)])))


@pytest.mark.gpu
def test_rank_step_refuses_what_it_cannot_rank(gpu_device):
    cfg = EngineConfig(table_log2_cap=LOG2, max_rows=64, max_nnz=64 * 8)
    live = Engine(ModelConfig(kind="lr"), OptimConfig(kind="ftrl"), cfg, device=gpu_device)
    mvm = Engine(ModelConfig(kind="mvm", v_dim=4), OptimConfig(kind="frozen"), cfg, device=gpu_device)
    for e in (live, mvm):
        assert not e.ranks
        with pytest.raises(RuntimeError):
            _rank(e, [_keys(np.random.default_rng(0), 3)], [np.arange(100, 104, dtype=np.uint64)], [1])


# ---- CPU -----------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["mvm-snapshot", "crossed-lr", "full-lr"])
def test_the_fallback_is_predict_keys_on_the_expanded_rows(tmp_path, what):
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
    pred = Predictor(str(tmp_path), device=CPU, max_rows=4)
    assert not pred.engine.ranks
    ctx, cf = [[1, 6], [], [40, 11, 3]], [[0, 1], [], [0, 1, 2]]
    cands = [[[9, 2], [30]], [[5, 50, 7]], []]
    df = [[[2, 3], [3]], [[0, 1, 3]], []]
    got = pred.rank_keys(ctx, cands, cf, df)
    rows = [c + k for c, ks in zip(ctx, cands) for k in ks]
    want = pred.predict_keys(rows, [c + k for c, ks in zip(cf, df) for k in ks])
    assert [len(g) for g in got] == [2, 1, 0]
    assert np.array_equal(_bits(np.concatenate(got)), _bits(want))
    with pytest.raises(ValueError):  # short: a context without its candidates
        pred.rank_keys(ctx, cands[:2], cf, df[:2])
    with pytest.raises(ValueError):  # non-monotonic request offsets
        pred.rank_csr(np.arange(3, dtype=np.uint64), [0, 1, 2, 3], np.arange(4, dtype=np.uint64),
                      [0, 1, 2, 3, 4], [0, 3, 2, 4])
