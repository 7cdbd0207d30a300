"""FTRL inside the bucket reduction (docs/DESIGN.md section 3,
EngineConfig.red_apply): on a bucket-sorted leader-handoff step with ranked
outputs k_red_sum_local pushes every key's normalised gradient sum itself --
k_apply_lr16's arithmetic on k_apply_lr16's inputs -- so the step has no
unique-order gradient array and no apply launch.  Every key is pushed once
with the same float, so two engines that differ only in the switch must agree
byte for byte after every step: the pulled weight of every key seen so far,
the loss sums and the table's size.

Geometry the cases rely on: a sum unit is 2^14 scratch slots, a bitmap word 32
of them, a compaction chunk 4096; the scratch's active capacity is at least
2^16 and the first step of an engine runs at the allocation's capacity.  A
unit is sparse when no wave of it holds more than 8 rows of 64 records, else
dense.  A key's scratch home is fmix64(key) & (capacity - 1) while the
parameter table has at most as many slots as the scratch (kernels_dedup.hip).

Reference semantics: the FTRL-Proximal push of a key's batch gradient
(ftrl.h:38-152, lr_worker.cc:100-119).
"""
import numpy as np
import pytest
import torch

from xflow_amd import native
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Batch, Engine
from xflow_amd.testing.hashing import fmix64

MIN_CAP = 1 << 16  # kScratchMinCap
STEPS = 6


def _labels(seed, rows):
    return (np.random.default_rng(seed).random(rows) < 0.3).astype(np.float32)


def _power_law(step, rows, F, hot=3000, p_hot=0.5):
    """[F][rows]: a hot vocabulary with a power-law inside that comes back
    every batch, plus random 62-bit keys new in every batch"""
    rng = np.random.default_rng(1000 + step)
    n = rows * F
    hot_keys = (np.arange(1, hot + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(2)
    k = rng.integers(1, 1 << 62, size=n, dtype=np.int64).astype(np.uint64)
    pick = rng.random(n) < p_hot
    k[pick] = hot_keys[np.minimum(rng.zipf(1.2, size=int(pick.sum())), hot) - 1]
    return np.ascontiguousarray(k.reshape(F, rows)), _labels(step, rows)


def _one_key(step, rows, F):
    """every occurrence of every step the same key: one record per tile and
    field, one stamped slot"""
    return np.full((F, rows), 777, dtype=np.uint64), _labels(step, rows)


def _distinct(step, rows, F):
    """every occurrence its own key, the same keys every other step"""
    n = rows * F
    k = (np.uint64(1) << np.uint64(62)) + np.uint64(step % 2) * np.uint64(1 << 32) + np.arange(n, dtype=np.uint64)
    return np.ascontiguousarray(k.reshape(F, rows)), _labels(step, rows)


def _batch(k, y, dev, field_major=True, slice_rows=0):
    keys = k if field_major else np.ascontiguousarray(k.T)
    return Batch(keys=torch.from_numpy(keys.reshape(-1).view(np.int64)).to(dev),
                 labels=torch.from_numpy(y).to(dev), nnz_per_row=k.shape[0],
                 field_major=field_major, slice_rows=slice_rows)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _pair(dev, batches, want_plan=True, shape=None, overflow=False, each=None, **cfg):
    """Two engines, red_apply on and off, in lockstep over the batches (k, y
    [, batch keywords]).  After every step: the plan says want_plan (a list:
    per step) for the engine with the switch on and False for the other, and
    the pulled weights of every key seen, the loss sums and the table's size
    are byte-identical.  Returns the engines (on, off)."""
    max_rows = max(b[0].shape[1] for b in batches)
    F = batches[0][0].shape[0]
    kw = dict(table_log2_cap=18, max_rows=max_rows, max_nnz=max_rows * F)
    kw.update(cfg)
    engs = [Engine(ModelConfig(kind="lr"), OptimConfig(), EngineConfig(red_apply=on, **kw), device=dev)
            for on in (True, False)]
    seen = np.zeros(0, dtype=np.uint64)
    for step, bt in enumerate(batches):
        k, y = bt[0], bt[1]
        bkw = bt[2] if len(bt) > 2 else {}
        S = 2 if bkw.get("slice_rows") else 1
        for eng in engs:
            if overflow:
                # (the capacity monitor reports the flag once the step is queued)
                try:
                    eng.train_step(_batch(k, y, dev, **bkw))
                except RuntimeError as e:
                    assert "scratch overflow" in str(e)
            else:
                eng.train_step(_batch(k, y, dev, **bkw))
        want = want_plan[step] if isinstance(want_plan, list) else want_plan
        plans = [e.native.step_plan(S, k.shape[1], F, bkw.get("field_major", True)) for e in engs]
        assert plans[0]["red_apply"] == want and not plans[1]["red_apply"], (step, plans)
        assert not want or (plans[0]["red_local"] and plans[0]["red_rank"] and plans[0]["lead"])
        assert plans[0]["grad"] == plans[1]["grad"], (step, plans)  # (the layout is the same)
        assert not want or plans[0]["grad"] == "unique_lr", (step, plans)
        if each:
            each(engs, step, k)
        if overflow:
            continue  # (which keys found a slot is a race: the caller compares)
        seen = np.union1d(seen, k.reshape(-1))
        w = [e.pull(seen) for e in engs]
        np.testing.assert_array_equal(_bits(w[0]), _bits(w[1]), err_msg=f"step {step}")
        st = [e.read_stats() for e in engs]
        for name in ("ln_loss", "rows", "positives"):
            assert np.float64(st[0][name]).view(np.uint64) == np.float64(st[1][name]).view(np.uint64), \
                (step, name, st)
        assert engs[0].table_size() == engs[1].table_size(), step
    assert all(e.overflowed() == overflow for e in engs)
    if not overflow:
        assert np.any(engs[0].pull(seen) != 0)  # (the pushes happened at all)
    return engs


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 2, 39])
@pytest.mark.parametrize("rows", [1024, 2048, 5120])
def test_power_law_on_equals_off(gpu_device, rows, F):
    """repeated keys across steps, and from the second step on carry-over
    rebuilds of the scratch (2^16 active slots)"""
    _pair(gpu_device, [_power_law(s, rows, F) for s in range(STEPS)])


@pytest.mark.gpu
@pytest.mark.parametrize("rows,F", [(1024, 1), (2048, 39), (129 * 1024, 1)])
def test_one_key(gpu_device, rows, F):
    """one stamped slot, one record per tile: a sparse unit, and with 129 tiles
    a dense one (nine segments a wave, which has record slots for eight rows)"""
    _pair(gpu_device, [_one_key(s, rows, F) for s in range(STEPS)])


@pytest.mark.gpu
@pytest.mark.parametrize("rows,F", [(1024, 1), (1024, 2), (2048, 39)])
def test_all_distinct(gpu_device, rows, F):
    """1024 x 1: sparse units, a key per record (1024 x 2 has units of either
    form: ~512 records, eight rows of a wave or nine); 2048 x 39: dense units
    at a third to two thirds occupancy, where keys share bitmap words and sit
    on both sides of chunk and unit boundaries by the thousand"""
    _pair(gpu_device, [_distinct(s, rows, F) for s in range(STEPS)])


def _steered(cap_bits=16):
    """keys by their scratch home modulo 2^16 (every active capacity is a
    multiple of it): two in one bitmap word, two on either side of a chunk
    boundary, two on either side of a unit boundary, one in the last slot"""
    homes = [64, 65, 4095, 4096, (1 << 14) - 1, 1 << 14, (1 << 16) - 1, 40000]
    cand = np.arange(1, 4_000_000, dtype=np.uint64)
    h = fmix64(cand) & np.uint64((1 << cap_bits) - 1)
    keys = []
    for x in homes:
        keys.append(cand[np.flatnonzero(h == np.uint64(x))[0]])
    return np.array(keys, dtype=np.uint64), homes


@pytest.mark.gpu
def test_steered_slots(gpu_device):
    """A table of 2^12 slots, no growth: the dedup's home is fmix64 & (cap - 1)
    and eight keys never collide, so each sits in its home.  The unique list is
    in slot order, which shows that the steering worked."""
    keys, homes = _steered()
    rows, F = 1024, 2
    batches = []
    for s in range(STEPS):
        rng = np.random.default_rng(s)
        k = keys[rng.integers(0, len(keys), size=(F, rows))]
        k[0, :len(keys)] = keys  # (every key in every batch)
        batches.append((np.ascontiguousarray(k), _labels(s, rows)))

    def each(engs, step, k):
        for e in engs:
            cap = e.batch_capacity()
            assert cap % MIN_CAP == 0
            h = fmix64(keys) & np.uint64(cap - 1)
            assert sorted(int(x) % MIN_CAP for x in h) == sorted(homes)
            np.testing.assert_array_equal(e.native.unique_keys(), keys[np.argsort(h, kind="stable")])

    # (max_nnz: a scratch allocation of 2^17 slots, so that the first step,
    # which runs at the allocation's capacity, has whole multiples of 2^16 too)
    _pair(gpu_device, batches, each=each, table_log2_cap=12, table_grow=False, max_nnz=32768)


@pytest.mark.gpu
def test_admission_leaves_unadmitted_keys_alone(gpu_device):
    """min_count 2: a key's first sighting gets no table slot (kNoSlot in the
    unique list) and must be skipped; the hot keys are admitted from the
    second step on"""
    engs = _pair(gpu_device, [_power_law(s, 2048, 5) for s in range(STEPS)], admit_min_count=2)
    seen = np.unique(np.concatenate([_power_law(s, 2048, 5)[0].reshape(-1) for s in range(STEPS)]))
    assert 0 < engs[0].table_size() < len(seen)


@pytest.mark.gpu
def test_spilled_batch(gpu_device):
    """Small vocabularies shrink the scratch to 2^16 slots; a surge of ~64 K
    distinct keys fills it and spills into the rest of the allocation: that
    batch's reduction covers 2^18 slots with leaders past the active table."""
    rows, F = 8192, 8
    batches = [_power_law(60 + s, rows, F, hot=2000, p_hot=1.0) for s in range(3)]
    for s in (3, 4):
        rng = np.random.default_rng(s)
        pool = rng.integers(0, 1 << 62, size=2_000_000, dtype=np.int64).astype(np.uint64)
        batches.append((np.ascontiguousarray(pool[rng.integers(0, pool.size, size=rows * F)].reshape(F, rows)),
                        _labels(s, rows)))
    batches.append(_power_law(70, rows, F))
    caps = []
    _pair(gpu_device, batches, each=lambda engs, step, k: caps.append(engs[0].batch_capacity()))
    assert caps[1:4] == [MIN_CAP, MIN_CAP, 1 << 18], caps


@pytest.mark.gpu
def test_full_scratch_overflows_to_the_trash_slot(gpu_device):
    """A scratch allocation of 256 slots for batches of 1024 distinct keys:
    the leaders that find no slot get the trash slot, emit no record and have
    no unique index, and the step is flagged.  Which keys find a slot is a
    race inside the dedup, so the engines are compared on what does not depend
    on it: every label is 1 and every key occurs once, so every key that found
    a slot has the same state, and both engines hold as many keys."""
    rows = 1024
    batches = [((np.uint64(s + 1) << np.uint64(32)) + np.arange(rows, dtype=np.uint64)[None, :],
                np.ones(rows, dtype=np.float32)) for s in range(STEPS)]
    engs = _pair(gpu_device, batches, overflow=True, scratch_factor=0.2)
    out = []
    for e in engs:
        keys, words = e.export_table()
        out.append((len(keys), np.unique(np.asarray(words).reshape(len(keys), -1), axis=0)))
    assert out[0][0] == out[1][0] > 0
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert len(out[0][1]) == 1 and np.any(out[0][1] != 0)  # (one state, and pushed)
    st = [e.read_stats() for e in engs]
    for name in ("ln_loss", "rows", "positives"):
        assert np.float64(st[0][name]).view(np.uint64) == np.float64(st[1][name]).view(np.uint64)


@pytest.mark.gpu
def test_table_growth_and_snapshots(gpu_device):
    """A table of 2^10 slots that has to grow under ~2 K new keys a step, and
    a capacity monitor one step behind: every step waits for the snapshot of
    the step before, which on a red_apply step the reduction's launch stores."""
    batches = [_power_law(s, 1024, 4, hot=500, p_hot=0.3) for s in range(8)]
    engs = _pair(gpu_device, batches, table_log2_cap=10, monitor_lag=1)
    assert engs[0].table_growths == engs[1].table_growths > 0


@pytest.mark.gpu
def test_fallback_steps_in_the_same_engine(gpu_device):
    """steps the plan does not cover -- rows no multiple of the tile, a
    row-major batch, two slices -- between steps it does: they run the
    separate apply on the same table and stashes"""
    F = 5
    kinds = [("lead", 2048, {}), ("rows1000", 1000, {}), ("lead", 2048, {}),
             ("row_major", 2048, dict(field_major=False)), ("lead", 1024, {}),
             ("S2", 2048, dict(slice_rows=1024)), ("lead", 2048, {})]
    batches = [_power_law(s, rows, F) + (kw,) for s, (_, rows, kw) in enumerate(kinds)]
    _pair(gpu_device, batches, want_plan=[name == "lead" for name, _, _ in kinds], max_slices=2)


# ---- planner (CPU) ---------------------------------------------------------
def _plan(S=1, **kw):
    d = {"model": ModelConfig(kind="lr").native(), "opt": OptimConfig().native(), "gpu": True,
         "rows": 2048.0, "fields": 39.0, "field_major": True}
    d.update(kw)
    return native.load().plan_step(d, S, True)


def test_planner_red_apply_implies_its_three_conditions():
    n = 0
    for S in (1, 2, 8):
        for gpu in (True, False):
            for fmaj in (True, False):
                for rows in (0.0, 1000.0, 1024.0, 262144.0):
                    for model in (ModelConfig(kind="lr"), ModelConfig(kind="fm", v_dim=8)):
                        for opt in ("ftrl", "sgd"):
                            p = _plan(S, gpu=gpu, field_major=fmaj, rows=rows, model=model.native(),
                                      opt=OptimConfig(kind=opt).native())
                            want = (S == 1 and gpu and fmaj and rows >= 1024 and model.kind == "lr"
                                    and opt == "ftrl")
                            assert p["red_apply"] == want, (S, gpu, fmaj, rows, model.kind, opt, p)
                            if p["red_apply"]:
                                assert p["red_local"] and p["red_rank"] and p["lead"] and p["lr16"]
                                n += 1
    assert n == 2


@pytest.mark.parametrize("flag", ["red_apply", "red_local", "red_rank", "lead_handoff"])
def test_planner_any_flag_off_switches_it_off(flag):
    on, off = _plan(), _plan(**{flag: False})
    assert on["red_apply"] and not off["red_apply"]
    # the gradient layout is the separate apply's
    assert on["grad"] == off["grad"] == "unique_lr"
    if flag == "red_apply":  # the switch changes nothing else of the plan
        assert {k: v for k, v in on.items() if k != "red_apply"} == \
            {k: v for k, v in off.items() if k != "red_apply"}


def test_switch_defaults_on_and_the_bare_plan_does_not_report_it():
    assert EngineConfig().red_apply is True
    d = {"model": ModelConfig(kind="lr").native(), "opt": OptimConfig().native()}
    assert "red_apply" not in native.load().plan_step(d, 1)
    e = Engine(ModelConfig(kind="lr"), OptimConfig(),
               EngineConfig(table_log2_cap=12, max_rows=2048, max_nnz=2048 * 4), device=torch.device("cpu"))
    p = e.native.step_plan(1, 2048, 4, True)
    assert p["red_apply"] is False and not p["lead"]
