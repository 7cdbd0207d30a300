"""Engine.pool_topk on the fused kernel (k_pool_topk_strip / k_pool_topk_merge,
docs/DESIGN.md §2) against numpy's lexsort of pool_score on the same vectors:
exact equality of idx, and of score bit for bit (a NaN for a NaN).  pool_score
is held to ref64 by test_rank_pool.py.  Vectors are seeded float32 tensors
{c, u.., +0.0} on frozen engines with empty tables."""
import functools

import numpy as np
import pytest
import torch

from test_rank import CONFIGS, F32, _bits, _engine, _keys
from test_rank_pool import _lexsort_topk

from xflow_amd import checkpoint
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Engine
from xflow_amd.serve import Predictor

pytestmark = pytest.mark.gpu
MODELS = {"lr": 0, "fm8": 8, "fm32": 32}  # KP = 2, 10, 34


@functools.lru_cache(maxsize=None)
def _eng(dev, name, **kw):
    D = MODELS[name]
    model = ModelConfig(kind="fm", v_dim=D, fm_math="standard") if D else ModelConfig(kind="lr")
    return Engine(model, OptimConfig(kind="frozen", frozen_from="ftrl"),
                  EngineConfig(table_log2_cap=10, max_rows=64, max_nnz=1024,
                               pool_topk_fused_min=0, **kw), device=dev)  # (at every size)


def _rand(e, name, rng, n):
    v = np.zeros((n, e.pool_width), F32)
    v[:, 0] = rng.normal(0, 1, n)
    v[:, 1:1 + MODELS[name]] = rng.normal(0, 0.3, (n, MODELS[name]))
    return v


def _check(e, ref, cv, pv, k, rows=None):
    """e.pool_topk(cv, pv, k) against lexsort of ref.pool_score on `rows` (all)."""
    cv, pv = (torch.from_numpy(np.ascontiguousarray(x)).to(e.device) for x in (cv, pv))
    idx, score = (t.cpu().numpy() for t in e.pool_topk(cv, pv, k))
    assert idx.shape == score.shape == (len(cv), k) and idx.dtype == np.int32
    for q in range(len(cv)) if rows is None else rows:
        p = ref.pool_score(cv[q:q + 1].contiguous(), pv).cpu().numpy()[0]
        wi, ws = _lexsort_topk(p, k)
        n, nan = len(wi), np.isnan(ws)
        assert np.array_equal(idx[q, :n], wi) and (idx[q, n:] == -1).all(), (q, k)
        assert np.array_equal(np.isnan(score[q, :n]), nan) and not _bits(score[q, n:]).any(), (q, k)
        assert np.array_equal(_bits(score[q, :n])[~nan], _bits(ws)[~nan]), (q, k)
    return idx, score


@pytest.mark.parametrize("k", [1, 7, 32, 33, 100, 1024])
@pytest.mark.parametrize("name", list(MODELS))
def test_edges_of_steps_strips_lists_and_groups(gpu_device, name, k):
    """Strips of 128: one strip, the 128-step edge, two strips, twelve strips
    with lists shorter than k; k > N is padded; k = 1024 merges in several
    rounds; R fills a workgroup's group of requests and starts the next."""
    e, auto = _eng(gpu_device, name, pool_topk_strip=128), _eng(gpu_device, name)
    assert e.pool_topk_fused and auto.pool_topk_fused
    rng = np.random.default_rng(k)
    mq = e.pool_topk_group(k)
    cv = _rand(e, name, rng, mq + 1)
    for N in (1, 127, 128, 129, 1500):
        pv = _rand(e, name, rng, N)
        for R in (1, mq, mq + 1):
            got = _check(e, e, cv[:R], pv, k)
        same = _check(auto, e, cv, pv, k)  # (the automatic strip: one of 1536 at N = 1500)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, same))


@pytest.mark.parametrize("k", [7, 100])
@pytest.mark.parametrize("stream", ["ascending", "descending", "constant", "coarse", "nan"])
def test_streams_that_drive_the_lists(gpu_device, stream, k):
    """ascending: every score survives, a compress per step; descending: none
    after the first k; constant: one tie, by index across steps, compresses and
    strips; coarse: ties straddle every edge; nan: NaN candidates rank last."""
    rng = np.random.default_rng(11)
    for N in (1500, 102) if stream == "nan" else (1500,):
        c = {"ascending": np.linspace(-3, 3, N), "descending": np.linspace(3, -3, N),
             "constant": np.full(N, 0.25), "coarse": np.round(rng.normal(0, 1, N), 1),
             "nan": rng.normal(0, 1, N)}[stream].astype(F32)
        if stream == "nan":
            c[[5, N // 2, N - 1]] = np.nan
        for strip in (128, 0):
            e = _eng(gpu_device, "lr", pool_topk_strip=strip)
            pv, cv = np.zeros((N, e.pool_width), F32), np.zeros((3, e.pool_width), F32)
            pv[:, 0], cv[:, 0] = c, (-0.5, 0.0, 0.5)
            _, score = _check(e, e, cv, pv, k)
            if stream == "coarse":
                p = e.pool_score(torch.from_numpy(cv).to(e.device), torch.from_numpy(pv).to(e.device))
                assert all(len(np.unique(_bits(x))) < N // 2 for x in p.cpu().numpy())
            assert np.isnan(score).any() == (stream == "nan" and N == 102 and k == 100)


def test_more_than_2_31_scores(gpu_device):
    """32 769 x 65 537 = 2 147 581 953 scores: no [R, N] array could be indexed."""
    e = _eng(gpu_device, "lr")
    rng = np.random.default_rng(2)
    cv, pv = _rand(e, "lr", rng, 32769), _rand(e, "lr", rng, 65537)
    _check(e, e, cv, pv, 10, rows=(0, 31, 32, 32767, 32768))


def test_switch_and_chunking(gpu_device, tmp_path):
    rng = np.random.default_rng(4)
    e, off = _eng(gpu_device, "fm8"), _eng(gpu_device, "fm8", pool_topk_fused=False)
    assert not off.pool_topk_fused
    cv, pv = _rand(e, "fm8", rng, 5), _rand(e, "fm8", rng, 1500)
    got = _check(e, off, cv, pv, 10)
    want = off.pool_topk(*(torch.from_numpy(x).to(off.device) for x in (cv, pv)), 10)
    assert all(np.array_equal(_bits(a), _bits(b.cpu().numpy())) for a, b in zip(got, want))
    checkpoint.save_serving(_engine(CONFIGS[6], 6, gpu_device), str(tmp_path / "s"), 0, 1,
                            barrier=lambda: None)
    ctx = [_keys(rng, 26).tolist() for _ in range(3)]
    rows = [_keys(rng, 13).tolist() for _ in range(1500)]
    res = []
    for kw in (dict(), dict(pool_topk_strip=128, pool_max_scores=300)):  # 12 lists of 10 words
        pred = Predictor(str(tmp_path / "s"), device=gpu_device, max_rows=1024,
                         pool_topk_fused_min=0, **kw)
        assert pred.engine.pool_topk_fused
        res.append(pred.rank_pool(ctx, pred.build_pool(rows), top_k=10))
    assert 4 * 300 // (8 * pred.engine.pool_topk_words(1500, 10)) == 1  # one request per chunk
    for (ia, sa), (ib, sb) in zip(*res):
        assert np.array_equal(ia, ib) and np.array_equal(_bits(sa), _bits(sb))
