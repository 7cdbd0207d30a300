"""The LR leader handoff (docs/DESIGN.md section 3): on a one-slice field-major
batch of a multiple of 1024 rows the dedup hands each tile's grouping to the
forward/backward kernel (k_lr_lead) instead of that kernel hashing every
column again.  The per-key gradient sums are the same integers either way and
the forward keeps its per-row summation order, so training with the handoff
on and off (EngineConfig.lead_handoff) must agree bit for bit; against the CPU
backend the tolerance is the one tests/test_determinism.py uses (rtol 1e-4,
atol 1e-6 on the weights, 1e-5 relative on the loss sum).

Reference semantics: per-key gradient sums of a batch (lr_worker.cc:100-119).
"""
import numpy as np
import pytest
import torch

from xflow_amd import native
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Batch, Engine

STEPS = 3
TILE = 1024
CASES = ("hot", "distinct", "twin", "recur", "mixed")


def _keys(case, rows, F, step):
    """[F][rows] keys.  Step 1 uses keys no other step has (a step whose keys
    are all new); step 2 repeats step 0's (slots kept by the scratch table)."""
    base = np.uint64(1 + (step % 2) * (1 << 40))
    r = np.arange(rows, dtype=np.uint64)[None, :]
    f = np.arange(F, dtype=np.uint64)[:, None]
    hot = base + np.uint64(1 << 30) + f + 0 * r          # one leader, rows - 1 followers per tile
    distinct = base + np.uint64(1 << 31) + f * np.uint64(rows) + r  # no followers
    twin = base + np.uint64(1 << 32) + 0 * f + r          # the same key in every field of a row
    recur = base + np.uint64(1 << 33) + f * np.uint64(1000) + r % np.uint64(37)  # within and across tiles
    if case == "mixed":
        rng = np.random.default_rng(100 + step)
        zipf = base + np.uint64(1 << 34) + f * np.uint64(1 << 20) + \
            np.minimum(rng.zipf(1.3, size=(F, rows)), 5000).astype(np.uint64)
        pick = (np.arange(F) + step) % 5
        tabs = [hot, distinct, twin, recur, zipf]
        return np.stack([tabs[pick[j]][j] for j in range(F)])
    return {"hot": hot, "distinct": distinct, "twin": twin, "recur": recur}[case].astype(np.uint64)


def _batches(case, rows, F, steps=STEPS):
    out = []
    for s in range(steps):
        k = np.ascontiguousarray(_keys(case, rows, F, s))
        y = (np.random.default_rng(7 + s).random(rows) < 0.3).astype(np.float32)
        out.append((k, y))
    return out


def _batch(k, y, dev, field_major=True, slice_rows=0):
    keys = k if field_major else np.ascontiguousarray(k.T)
    return Batch(keys=torch.from_numpy(keys.reshape(-1).view(np.int64)).to(dev),
                 labels=torch.from_numpy(y).to(dev), nnz_per_row=k.shape[0],
                 field_major=field_major, slice_rows=slice_rows)


def _engine(dev, rows, F, lead, kind="lr", S=1):
    return Engine(ModelConfig(kind=kind, v_dim=4), OptimConfig(),
                  EngineConfig(table_log2_cap=18, max_rows=rows, max_nnz=rows * F, max_slices=S,
                               lead_handoff=lead), device=dev)


def _train(dev, batches, lead, kind="lr", S=1, field_major=True):
    F, rows = batches[0][0].shape
    eng = _engine(dev, rows, F, lead, kind, S)
    plans = []
    for k, y in batches:
        eng.train_step(_batch(k, y, dev, field_major, rows // S if S > 1 else 0))
        plans.append(eng.native.step_plan(S, rows, F, field_major)["lead"])
    assert not eng.overflowed()
    keys, words = eng.export_table()
    o = np.argsort(keys, kind="stable")
    keys = keys[o]
    words = np.asarray(words).reshape(len(keys), -1)[o]  # (state_words per key, export order)
    return eng, keys, words, eng.pull(keys), eng.read_stats(), plans


def _assert_bit_equal(a, b):
    _, ka, sa, wa, sta, _ = a
    _, kb, sb, wb, stb, _ = b
    np.testing.assert_array_equal(ka, kb)
    np.testing.assert_array_equal(sa, sb)  # the whole slot state ((n, z) words)
    np.testing.assert_array_equal(wa.view(np.uint32), wb.view(np.uint32))
    for name in ("ln_loss", "rows", "positives"):
        assert np.float64(sta[name]).view(np.uint64) == np.float64(stb[name]).view(np.uint64), \
            (name, sta[name], stb[name])


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 2, 39])
@pytest.mark.parametrize("rows", [1024, 2048, 3072])
@pytest.mark.parametrize("case", CASES)
def test_handoff_equals_column_hash_and_cpu(gpu_device, case, rows, F):
    batches = _batches(case, rows, F)
    on = _train(gpu_device, batches, True)
    off = _train(gpu_device, batches, False)
    assert on[5] == [True] * STEPS and off[5] == [False] * STEPS
    _assert_bit_equal(on, off)
    _, kc, _, wc, stc, _ = _train(torch.device("cpu"), batches, True)
    np.testing.assert_array_equal(on[1], kc)
    np.testing.assert_allclose(on[3], wc, rtol=1e-4, atol=1e-6)
    assert on[4]["rows"] == stc["rows"]
    assert abs(on[4]["ln_loss"] - stc["ln_loss"]) <= 1e-5 * abs(stc["ln_loss"])


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["rows1000", "rows1536", "S2", "row_major", "fm"])
def test_fallbacks_plan_off_and_results_independent_of_the_switch(gpu_device, what):
    rows = {"rows1000": 1000, "rows1536": 1536}.get(what, 2048)
    kw = {"S2": dict(S=2), "row_major": dict(field_major=False), "fm": dict(kind="fm")}.get(what, {})
    batches = _batches("mixed", rows, 5)
    on = _train(gpu_device, batches, True, **kw)
    off = _train(gpu_device, batches, False, **kw)
    assert on[5] == [False] * STEPS and off[5] == [False] * STEPS
    _assert_bit_equal(on, off)


@pytest.mark.gpu
def test_eval_after_training_is_independent_of_the_switch(gpu_device):
    batches = _batches("mixed", 2048, 39, STEPS + 1)
    k, y = batches[-1]
    preds = []
    for lead in (True, False):
        eng = _train(gpu_device, batches[:STEPS], lead)[0]
        preds.append(eng.eval_step(_batch(k, y, gpu_device)).cpu().numpy())
    assert np.isfinite(preds[0]).all() and preds[0].std() > 0
    np.testing.assert_array_equal(preds[0].view(np.uint32), preds[1].view(np.uint32))


def test_planner_lead_exactly_where_the_handoff_applies():
    n = native.load()
    models = {"lr": ModelConfig(kind="lr"), "fm": ModelConfig(kind="fm", v_dim=8),
              "mvm": ModelConfig(kind="mvm", v_dim=10)}
    seen = 0
    for model, S, gpu, fmaj, rows, on in [(m, S, g, fm, r, on) for m in models for S in (1, 2, 8)
                                          for g in (True, False) for fm in (True, False)
                                          for r in (0, 1000, 1024, 1536, 2048, 262144)
                                          for on in (True, False)]:
        d = {"model": models[model].native(), "opt": OptimConfig().native(), "gpu": gpu}
        p0 = n.plan_step(dict(d), S)
        p = n.plan_step(dict(d, rows=float(rows), fields=39.0, field_major=fmaj, lead_handoff=on), S)
        want = on and model == "lr" and S == 1 and gpu and fmaj and rows > 0 and rows % TILE == 0
        assert p["lead"] == want, (model, S, gpu, fmaj, rows, on)
        assert not p0["lead"]  # (no batch shape given: off)
        assert p["grad"] == p0["grad"]
        assert {k: v for k, v in p.items() if k != "lead"} == {k: v for k, v in p0.items() if k != "lead"}
        seen += want
    assert seen == 3
    # the kernel's limits: rows of at most 40 features, slots below the follower bit
    d = {"model": models["lr"].native(), "opt": OptimConfig().native(), "rows": 2048.0,
         "field_major": True}
    assert n.plan_step(dict(d, fields=40.0), 1)["lead"]
    assert not n.plan_step(dict(d, fields=41.0), 1)["lead"]
    assert not n.plan_step(dict(d, fields=39.0, scratch_cap=float(1 << 31), max_nnz=float(1 << 29)), 1)["lead"]
    assert n.plan_step(dict(d, fields=39.0, scratch_cap=float(1 << 30), max_nnz=float(1 << 28)), 1)["lead"]
