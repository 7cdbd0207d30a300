"""Bucket-sorted producer regions (docs/DESIGN.md section 3,
EngineConfig.red_local): on a leader-handoff step k_lr_lead writes its gradient
records sorted by reduction bucket and k_red_sum_local sums each bucket from
the workgroups' segments, without the scan and scatter passes.  The record set
is the same and the sums are order-free integers, so training with the switch
on and off must agree bit for bit: engine.pull of every key seen, the
predictions of an eval step and the loss sums.  The CPU backend is a third
opinion within the tolerance tests/test_determinism.py uses (rtol 1e-4, atol
1e-6 on the weights, 1e-5 relative on the loss sum).

Geometry the cases rely on: a bucket is 2^14 slots; the scratch's active
capacity is at least 2^16 (4 buckets) and the first step of an engine runs at
the allocation's capacity.  A sum unit is sparse when no wave of it holds more
than 8 rows of 64 records, else dense.

Not covered: a bucket wider than one unit (sub > 0).  It needs an active
scratch capacity above 4096 x 2^14 = 2^26 slots, i.e. a scratch allocation of
several GB: no small EngineConfig reaches it.  Those units run the same
segment walk with the range form's `l < kR` filter.

Reference semantics: per-key gradient sums of a batch (lr_worker.cc:100-119).
"""
import numpy as np
import pytest
import torch

from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Batch, Engine

MIN_CAP = 1 << 16  # kScratchMinCap
STEPS = 3


def _labels(seed, rows):
    return (np.random.default_rng(seed).random(rows) < 0.3).astype(np.float32)


def _skewed(step, rows, F, hot=3000, p_hot=0.25):
    """[F][rows]: a hot vocabulary that comes back every batch plus random
    62-bit keys, new in every batch"""
    rng = np.random.default_rng(1000 + step)
    n = rows * F
    hot_keys = (np.arange(1, hot + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(2)
    k = rng.integers(1, 1 << 62, size=n, dtype=np.int64).astype(np.uint64)
    pick = rng.random(n) < p_hot
    k[pick] = hot_keys[np.minimum(rng.zipf(1.2, size=int(pick.sum())), hot) - 1]
    return np.ascontiguousarray(k.reshape(F, rows)), _labels(step, rows)


def _same(step, rows, F):
    """every occurrence the same key: one record per tile, all of a
    workgroup's leaders in one bucket, every other (workgroup, bucket) segment
    empty and three of the four buckets without a record"""
    return np.full((F, rows), 777 + step % 2, dtype=np.uint64), _labels(step, rows)


def _distinct(step, rows, F):
    """every occurrence its own key: a workgroup's region is full (1024 x F
    records) and, from 8 fields on, a segment holds more than 64 x 8 records:
    dense units"""
    n = rows * F
    k = (np.uint64(1) << np.uint64(62)) + np.uint64(step % 2) * np.uint64(1 << 32) + np.arange(n, dtype=np.uint64)
    return np.ascontiguousarray(k.reshape(F, rows)), _labels(step, rows)


def _per_group(step, rows, F):
    """one key per producer workgroup (1024 rows), another in each: every
    workgroup's leaders fall in one bucket, the workgroups' buckets differ or
    not as the slots fall, and most buckets get nothing"""
    g = (np.arange(rows, dtype=np.uint64) // np.uint64(1024))[None, :]
    k = (np.uint64(0x9E3779B97F4A7C15) * (g + np.uint64(1 + 100 * (step % 2)))) >> np.uint64(2)
    return np.ascontiguousarray(np.repeat(k, F, axis=0)), _labels(step, rows)


PATTERNS = {"skewed": _skewed, "same": _same, "distinct": _distinct, "per_group": _per_group}


def _batch(k, y, dev, field_major=True, slice_rows=0):
    keys = k if field_major else np.ascontiguousarray(k.T)
    return Batch(keys=torch.from_numpy(keys.reshape(-1).view(np.int64)).to(dev),
                 labels=torch.from_numpy(y).to(dev), nnz_per_row=k.shape[0],
                 field_major=field_major, slice_rows=slice_rows)


def _train(dev, batches, on, kind="lr", S=1, field_major=True, scratch_factor=2.5, overflow=False,
           each=None, want_plan=None, count=False):
    """Trains all batches but the last and evaluates the last.  want_plan: the
    plan's red_local of every step (None: on, for a GPU engine)."""
    max_rows = max(k.shape[1] for k, _ in batches)
    F = batches[0][0].shape[0]
    eng = Engine(ModelConfig(kind=kind, v_dim=4), OptimConfig(),
                 EngineConfig(table_log2_cap=18, max_rows=max_rows, max_nnz=max_rows * F, max_slices=S,
                              scratch_factor=scratch_factor, red_local=on), device=dev)
    if count:
        eng.count_records(True)
    if want_plan is None:
        want_plan = on and dev.type == "cuda"
    seen = []
    for step, (k, y) in enumerate(batches[:-1]):
        rows = k.shape[1]
        b = _batch(k, y, dev, field_major, rows // S if S > 1 else 0)
        if overflow:
            # (the capacity monitor reports the flag once the step is queued)
            try:
                eng.train_step(b)
            except RuntimeError as e:
                assert "scratch overflow" in str(e)
        else:
            eng.train_step(b)
        p = eng.native.step_plan(S, rows, F, field_major)
        assert p["red_local"] == want_plan, (step, p)
        assert not p["red_local"] or p["lead"], (step, p)
        seen.append(np.unique(k))
        if each:
            each(eng, step, k)
    assert eng.overflowed() == overflow
    k, y = batches[-1]
    pctr = eng.eval_step(_batch(k, y, dev, field_major)).cpu().numpy()
    keys = np.unique(np.concatenate(seen))
    return dict(eng=eng, keys=keys, w=eng.pull(keys), pctr=pctr, train=eng.read_stats(),
                eval=eng.read_stats(which=1))


def _assert_bit_equal(a, b):
    np.testing.assert_array_equal(a["keys"], b["keys"])
    np.testing.assert_array_equal(a["w"].view(np.uint32), b["w"].view(np.uint32))
    np.testing.assert_array_equal(a["pctr"].view(np.uint32), b["pctr"].view(np.uint32))
    assert np.isfinite(a["pctr"]).all() and len(a["keys"]) > 0
    for which in ("train", "eval"):
        for name in ("ln_loss", "rows", "positives"):
            x, y = a[which][name], b[which][name]
            assert np.float64(x).view(np.uint64) == np.float64(y).view(np.uint64), (which, name, x, y)


def _both(dev, batches, **kw):
    on = _train(dev, batches, True, **kw)
    off = _train(dev, batches, False, **kw)
    _assert_bit_equal(on, off)
    return on, off


@pytest.mark.gpu
@pytest.mark.parametrize("rows,F", [(1024, 1), (2048, 39), (2048, 40)])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_switch_on_equals_off_and_cpu(gpu_device, pattern, rows, F):
    batches = [PATTERNS[pattern](s, rows, F) for s in range(STEPS + 1)]
    on, _ = _both(gpu_device, batches)
    assert on["pctr"].std() > 0 or pattern == "same"
    # The CPU backend adds a key's gradient in float32, occurrence by
    # occurrence: n terms carry a rounding error of up to n x 2^-24 of their
    # magnitude, past the 1e-4 tolerance from a few thousand terms on (one key
    # in all of 2048 x 39 occurrences measured 2.2e-4).  It is a reference only
    # where no key has more than 4096 occurrences in a step -- every pattern
    # at 1024 x 1, skewed and distinct at every shape.
    if max(np.unique(k, return_counts=True)[1].max() for k, _ in batches) > 4096:
        return
    cpu = _train(torch.device("cpu"), batches, True)
    np.testing.assert_array_equal(on["keys"], cpu["keys"])
    np.testing.assert_allclose(on["w"], cpu["w"], rtol=1e-4, atol=1e-6)
    assert on["train"]["rows"] == cpu["train"]["rows"]
    assert abs(on["train"]["ln_loss"] - cpu["train"]["ln_loss"]) <= 1e-5 * abs(cpu["train"]["ln_loss"])


@pytest.mark.gpu
def test_record_counts_are_the_scatter_form_s(gpu_device):
    """the workgroups' record totals (Engine.count_records) come from the
    cursor scan with the switch on and from the running count with it off"""
    batches = [_skewed(s, 2048, 39) for s in range(STEPS + 1)]
    recs = {True: [], False: []}
    for on in (True, False):
        _train(gpu_device, batches, on, count=True,
               each=lambda e, step, k, on=on: recs[on].append(e.take_records()))
    assert recs[True] == recs[False] and all(0 < r <= 2048 * 39 for r in recs[True]), recs


@pytest.mark.gpu
def test_rebuilds_and_a_capacity_change(gpu_device):
    """2048 x 8 with 14-15 K unique keys: the capacity settles at 2^16 and the
    occupancy passes the rebuild threshold every other step; 8192 x 8 then
    grows the capacity, so the bucket geometry (FwdArgs::red_bcap) changes
    between steps: the allocation's 2^18 slots on the first step, 2^16, then
    the grown capacity."""
    batches = [_skewed(s, 2048, 8) for s in range(8)] + [_skewed(20, 8192, 8)] + \
              [_skewed(s, 2048, 8) for s in range(30, 33)]
    stats = {True: [], False: []}
    runs = []
    for on in (True, False):
        runs.append(_train(gpu_device, batches, on,
                           each=lambda e, step, k, on=on: stats[on].append(
                               (e.scratch_stats(), e.batch_capacity()))))
    _assert_bit_equal(*runs)
    assert [s[0]["capacity"] for s in stats[True]] == [s[0]["capacity"] for s in stats[False]]
    st = stats[True]
    assert st[0][1] > MIN_CAP and st[7][1] == MIN_CAP, st  # (the step's own geometry)
    assert st[7][0]["capacity"] == MIN_CAP and st[7][0]["rebuilds"] >= 3, st
    assert st[8][0]["capacity"] > MIN_CAP and st[-1][0]["capacity"] == st[8][0]["capacity"], st
    assert st[-1][1] == st[8][0]["capacity"], st


@pytest.mark.gpu
def test_spilled_batch(gpu_device):
    """Small vocabularies shrink the table to 2^16 slots; a surge of ~64 K
    distinct keys on top of the stale ones fills it and spills into the rest
    of the allocation: that batch's reduction covers the whole allocation,
    2^18 slots (16 buckets instead of 4), with leaders past the active table."""
    rows, F = 8192, 8
    batches = [_skewed(60 + s, rows, F, hot=2000, p_hot=1.0) for s in range(3)]
    for s in (3, 4):
        rng = np.random.default_rng(s)
        pool = rng.integers(0, 1 << 62, size=2_000_000, dtype=np.int64).astype(np.uint64)
        batches.append((np.ascontiguousarray(pool[rng.integers(0, pool.size, size=rows * F)].reshape(F, rows)),
                        _labels(s, rows)))
    batches.append(_skewed(70, rows, F))
    caps = []
    _both(gpu_device, batches, each=lambda e, step, k: caps.append(e.batch_capacity()))
    alloc = 1 << 18  # pow2 >= 2.5 x 8192 x 8
    assert caps[1:4] == [MIN_CAP, MIN_CAP, alloc], caps


@pytest.mark.gpu
def test_full_scratch_trash_leaders_emit_nothing(gpu_device):
    """A scratch allocation of 256 slots for batches of 1024 distinct keys:
    the leaders that find no slot get the trash slot, emit no record, and the
    step is flagged.  Which keys find a slot is a race inside the dedup, so
    the runs are compared on what does not depend on it: every label is 1 and
    every key occurs once, so every key that found a slot has the same state
    -- and the records of a step are exactly the keys that found one."""
    rows = 1024
    # (keys no other step has)
    batches = [((np.uint64(s + 1) << np.uint64(32)) + np.arange(rows, dtype=np.uint64)[None, :],
                np.ones(rows, dtype=np.float32)) for s in range(STEPS + 1)]
    out = {}
    for on in (True, False):
        recs = []
        r = _train(gpu_device, batches, on, scratch_factor=0.2, overflow=True, count=True,
                   each=lambda e, step, k: recs.append(e.take_records()))
        keys, words = r["eng"].export_table()
        out[on] = (recs, len(keys), np.unique(np.asarray(words).reshape(len(keys), -1), axis=0), r)
    # (a step that finds the scratch still full of the last step's keys, before
    # its rebuild, leaves no record at all: every segment empty)
    assert out[True][0] == out[False][0] and all(0 <= n < rows for n in out[True][0]), out[True][0]
    assert out[True][0][0] > 0
    assert out[True][1] == out[False][1] == sum(out[True][0])
    np.testing.assert_array_equal(out[True][2], out[False][2])
    assert len(out[True][2]) == 1
    a, b = out[True][3], out[False][3]
    for which in ("train", "eval"):
        for name in ("ln_loss", "rows", "positives"):
            assert np.float64(a[which][name]).view(np.uint64) == np.float64(b[which][name]).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["rows1000", "rows1536", "S2", "row_major", "fm"])
def test_plan_off_wherever_the_handoff_is_off(gpu_device, what):
    rows = {"rows1000": 1000, "rows1536": 1536}.get(what, 2048)
    kw = {"S2": dict(S=2), "row_major": dict(field_major=False), "fm": dict(kind="fm")}.get(what, {})
    batches = [_skewed(s, rows, 5) for s in range(STEPS + 1)]
    _both(gpu_device, batches, want_plan=False, **kw)


def test_switch_defaults_on_and_the_cpu_plan_is_off():
    assert EngineConfig().red_local is True
    e = Engine(ModelConfig(kind="lr"), OptimConfig(),
               EngineConfig(table_log2_cap=12, max_rows=2048, max_nnz=2048 * 4), device=torch.device("cpu"))
    p = e.native.step_plan(1, 2048, 4, True)
    assert not p["lead"] and not p["red_local"]
    assert "red_local" in e.native.step_plan(1)
