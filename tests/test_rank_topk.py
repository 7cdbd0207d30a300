"""Segmented top-k of ranking scores (Engine.topk_step: k_topk_tile /
k_topk_merge on the GPU, a partial sort on the CPU; docs/DESIGN.md §2) against
a numpy lexsort per request.  The order is total -- descending sort key
(p > 0 ? p : +0.0f as bits), ties by ascending index -- so indices, score bits
and the -1 / +0.0f padding are all compared exactly, on both backends."""
import functools

import numpy as np
import pytest
import torch

from xflow_amd import checkpoint
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Engine
from xflow_amd.serve import Predictor

F32 = np.float32
CPU = torch.device("cpu")
DEVS = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="hip", marks=pytest.mark.gpu)]
# candidate counts per request, at the edges of the 4096-row tile
SEGS = {
    "below-tile": [4095], "tile": [4096], "above-tile": [4097],
    "ends-on-edges": [4000, 96, 1, 4095, 0, 0, 5],  # no request crosses: no merge owner
    "four-tiles": [100, 3 * 4096 + 7],              # starts mid-tile, one full middle tile
    "six-lists": [5 * 4096 + 1],                    # k = 1024: more than one merge round
    "many-small": [0, 1, 2, 63, 64, 65, 3] * 30,    # 5940 rows: > 64 requests per tile, empties
    "no-request": [], "all-empty": [0, 0, 0],
}
KS = (1, 7, 64, 1024)
PATTERNS = ("uniform", "constant", "seven", "special")


def _dev(request, name):
    return request.getfixturevalue("gpu_device") if name == "cuda" else CPU


@functools.lru_cache(maxsize=None)
def _engine(dev):
    return Engine(ModelConfig(kind="lr"), OptimConfig(kind="ftrl"),
                  EngineConfig(table_log2_cap=10, max_rows=64, max_nnz=64 * 4), device=dev)


def _scores(pattern, rows):
    rng = np.random.default_rng(rows + 1)
    p = rng.random(rows, dtype=F32)
    if pattern == "constant":  # all ties: indices 0 .. k - 1, across tile boundaries
        p[:] = 0.25
    elif pattern == "seven":
        p = rng.choice(np.linspace(0.1, 0.7, 7).astype(F32), rows)
    elif pattern == "special":
        m = rng.random(rows) < 0.5
        p[m] = rng.choice(np.array([np.nan, -0.0, -1.0, 0.0, 1e-42, 1.5, np.inf], F32), int(m.sum()))
    return p


def _select(p, k):
    skey = np.where(p > 0, p, 0).astype(F32).view(np.uint32)
    return np.lexsort((np.arange(len(p)), -(skey.astype(np.int64))))[:k]


def _same(got, want_idx, want_score):
    assert np.array_equal(np.asarray(got[0]), want_idx) and got[0].dtype == np.int32
    assert np.array_equal(np.asarray(got[1], F32).view(np.uint32), want_score.view(np.uint32))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("segs", SEGS)
@pytest.mark.parametrize("dev", DEVS)
def test_topk_step_is_the_lexsort_of_every_request(request, dev, segs, pattern):
    dev = _dev(request, dev)
    rp = np.concatenate([[0], np.cumsum(SEGS[segs])]).astype(np.int64)
    p = _scores(pattern, int(rp[-1]))
    order = [_select(p[a:b], max(KS)) for a, b in zip(rp[:-1], rp[1:])]
    tp, trp = torch.from_numpy(p).to(dev), torch.from_numpy(rp.astype(np.int32)).to(dev)
    for k in KS:
        idx, score = (t.cpu().numpy() for t in _engine(dev).topk_step(tp, trp, k))
        want_idx, want_score = np.full((len(order), k), -1, np.int32), np.zeros((len(order), k), F32)
        for q, o in enumerate(order):
            n = min(k, len(o))
            want_idx[q, :n], want_score[q, :n] = o[:n], p[rp[q]:rp[q + 1]][o[:n]]
        assert idx.shape == (len(order), k)
        _same((idx, score), want_idx, want_score)


@pytest.mark.parametrize("dev", DEVS)
def test_topk_step_refuses_bad_arguments(request, dev):
    dev = _dev(request, dev)
    p, rp = torch.rand(8, device=dev), torch.tensor([0, 3, 8], dtype=torch.int32, device=dev)
    for bad in (lambda: _engine(dev).topk_step(p, rp, 0), lambda: _engine(dev).topk_step(p, rp, 1025),
                lambda: _engine(dev).topk_step(p.double(), rp, 3),
                lambda: _engine(dev).topk_step(p, rp.long(), 3)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("kind", ["lr", "fm8"])
@pytest.mark.parametrize("dev", DEVS)
def test_predictor_top_k_is_the_selection_of_its_scores(request, dev, kind, tmp_path):
    """Requests of 60 / 0 / 700 candidates through the snapshot's Predictor (the
    GPU ranks with k_rank_*, the CPU expands the rows): with top_k the reply is
    the selection of the scores it gives without, also when max_rows cuts the
    700 into chunks that are merged on the host."""
    dev = _dev(request, dev)
    model = ModelConfig(kind="lr") if kind == "lr" else ModelConfig(kind="fm", v_dim=8)
    e = Engine(model, OptimConfig(kind="frozen", frozen_from="ftrl"),
               EngineConfig(table_log2_cap=13, max_rows=512, max_nnz=512 * 16), device=dev)
    rng = np.random.default_rng(3)
    keys = np.arange(100, 4100).astype(np.uint64)
    W = rng.normal(0, 0.05, (len(keys), e.params_per_key)).astype(F32)
    W[:, 0] = np.round(rng.normal(0, 0.3, len(keys)), 1)  # (coarse weights: equal scores occur)
    e.import_weights(keys, W)
    checkpoint.save_serving(e, str(tmp_path / "s"), 0, 1, barrier=lambda: None)
    ctx = [rng.integers(100, 5000, 9).tolist() for _ in range(3)]
    cands = [[rng.integers(100, 5000, 1 + r % 3).tolist() for r in range(n)] for n in (60, 0, 700)]
    for max_rows in (4096, 256):
        pred = Predictor(str(tmp_path / "s"), device=dev, max_rows=max_rows)
        assert pred.engine.ranks == (dev.type == "cuda")
        full = pred.rank_keys(ctx, cands)
        for k in (7, 1024):
            for got, p in zip(pred.rank_keys(ctx, cands, top_k=k), full):
                o = _select(p, k)
                _same(got, o.astype(np.int32), p[o])
    for bad in (0, 1025, 2.5):
        with pytest.raises(ValueError):
            pred.rank_keys(ctx, cands, top_k=bad)
