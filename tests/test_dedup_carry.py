"""Carry-over rebuilds of the GPU dedup scratch (docs/DESIGN.md section 3,
EngineConfig.scratch_carry): a rebuild at an unchanged capacity keeps the
slots the batch just stamped and frees the rest, and the rebuild counter means
occupied slots.  Which slot a key gets never shows in a result (gradients are
integer sums per key, the apply is per key), so training with the switch on
and off must agree bit for bit; against the CPU backend the tolerance is the
one tests/test_determinism.py uses (rtol 1e-4, atol 1e-6).

The shapes are small: 2048 rows x 8 fields give 14-15 K unique keys per batch,
the scratch's smallest capacity (2^16 slots) is then also its allocation, and
the occupancy passes the rebuild threshold (3/8 of the table) in the second
step after a rebuild at the latest.

Reference semantics: the sorted unique keys of a batch (lr_worker.cc:146-166).
"""
import numpy as np
import pytest
import torch

from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Batch, Engine

ROWS, F, STEPS = 2048, 8, 12
CAP = 1 << 16  # kScratchMinCap
CPU = torch.device("cpu")


def _stream(step, rows=ROWS, fields=F, hot=3000, p_hot=0.25):
    """[fields][rows] keys: a small hot vocabulary (the keys that come back
    every batch) plus a tail of random 62-bit keys, new in every batch."""
    rng = np.random.default_rng(1000 + step)
    n = rows * fields
    hot_keys = (np.arange(1, hot + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(2)
    k = rng.integers(1, 1 << 62, size=n, dtype=np.int64).astype(np.uint64)
    pick = rng.random(n) < p_hot
    # (skewed inside the hot set as well)
    k[pick] = hot_keys[np.minimum(rng.zipf(1.2, size=int(pick.sum())), hot) - 1]
    y = (rng.random(rows) < 0.3).astype(np.float32)
    return np.ascontiguousarray(k.reshape(fields, rows)), y


def _distinct(tag, rows, fields=F):
    """all keys different, and different from every other tag's and stream's"""
    n = rows * fields
    k = (np.uint64(1) << np.uint64(62)) + np.uint64(tag) * np.uint64(1 << 32) + np.arange(n, dtype=np.uint64)
    return np.ascontiguousarray(k.reshape(fields, rows)), np.zeros(rows, dtype=np.float32)


def _batch(k, y, dev, field_major=True, slice_rows=0):
    keys = k if field_major else np.ascontiguousarray(k.T)
    return Batch(keys=torch.from_numpy(keys.reshape(-1).view(np.int64)).to(dev),
                 labels=torch.from_numpy(y).to(dev), nnz_per_row=k.shape[0],
                 field_major=field_major, slice_rows=slice_rows)


def _engine(dev, carry, kind="lr", S=1, max_rows=ROWS, fields=F):
    return Engine(ModelConfig(kind=kind, v_dim=4), OptimConfig(),
                  EngineConfig(table_log2_cap=20, max_rows=max_rows, max_nnz=max_rows * fields,
                               max_slices=S, scratch_carry=carry), device=dev)


_BATCHES = {}


def _batches():
    if not _BATCHES:
        _BATCHES["b"] = [_stream(s) for s in range(STEPS + 1)]
        _BATCHES["keys"] = np.unique(np.concatenate([k.reshape(-1) for k, _ in _BATCHES["b"][:STEPS]]))
    return _BATCHES["b"], _BATCHES["keys"]


def _train(dev, carry, kind="lr", S=1, field_major=True):
    batches, seen = _batches()
    eng = _engine(dev, carry, kind, S)
    rows = batches[0][0].shape[1]
    for k, y in batches[:STEPS]:
        eng.train_step(_batch(k, y, dev, field_major, rows // S if S > 1 else 0))
    assert not eng.overflowed()
    k, y = batches[STEPS]
    pctr = eng.eval_step(_batch(k, y, dev, field_major)).cpu().numpy()
    return eng, eng.pull(seen), pctr, eng.read_stats(), eng.read_stats(which=1)


CASES = {"lr": {}, "fm": dict(kind="fm"), "lr_s4": dict(S=4), "lr_row_major": dict(field_major=False)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_results_equal_with_carry_on_and_off_and_cpu(gpu_device, case):
    kw = CASES[case]
    batches, _ = _batches()
    uniq = [len(np.unique(k)) for k, _ in batches]
    assert 12000 <= min(uniq) and max(uniq) <= 16384, uniq  # the capacity stays 2^16
    on = _train(gpu_device, True, **kw)
    off = _train(gpu_device, False, **kw)
    son, soff = on[0].scratch_stats(), off[0].scratch_stats()
    print(case, "carry on", son, "off", soff)
    assert son["capacity"] == soff["capacity"] == CAP
    assert son["rebuilds"] >= 3 and son["carried"] > 0, son
    assert soff["carried"] == 0, soff
    np.testing.assert_array_equal(on[1].view(np.uint32), off[1].view(np.uint32))
    np.testing.assert_array_equal(on[2].view(np.uint32), off[2].view(np.uint32))
    for a, b in ((on[3], off[3]), (on[4], off[4])):  # training and eval loss sums
        for name in ("ln_loss", "rows", "positives"):
            assert np.float64(a[name]).view(np.uint64) == np.float64(b[name]).view(np.uint64), name
    cpu = _train(CPU, True, **kw)
    np.testing.assert_allclose(on[1], cpu[1], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(on[2], cpu[2], rtol=1e-4, atol=1e-6)
    for a, b in ((on[3], cpu[3]), (on[4], cpu[4])):
        assert a["rows"] == b["rows"]
        assert abs(a["ln_loss"] - b["ln_loss"]) <= 1e-4 * abs(b["ln_loss"])


def _prepare(eng, k, y, counts, send):
    """dedup only (the world-1 prepare): returns the engine's unique keys"""
    eng.w_prepare(_batch(k, y, eng.device), 1, counts, send)
    n = eng.n_unique()
    assert int(counts.cpu()[0]) == n
    return send[:n].cpu().numpy().view(np.uint64)


@pytest.mark.gpu
def test_unique_list_exact_after_every_carry_over_rebuild(gpu_device):
    """A kept key behind a freed hole of its chain is claimed again in the hole
    and must still be in the list once."""
    batches, _ = _batches()
    eng = _engine(gpu_device, True)
    counts = torch.zeros(1, dtype=torch.int64, device=gpu_device)
    send = torch.zeros(ROWS * F, dtype=torch.int64, device=gpu_device)
    stats = [eng.scratch_stats()]
    after_rebuild = 0
    for step, (k, y) in enumerate(batches + batches[:3]):
        got = _prepare(eng, k, y, counts, send)
        want = np.unique(k)
        assert len(got) == len(want), (step, len(got), len(want))
        np.testing.assert_array_equal(np.sort(got), want, err_msg=f"step {step}")
        st = eng.scratch_stats()
        # occupied slots: at least the batch, at most the table
        assert len(want) <= st["occupancy"] <= CAP, (step, st)
        if st["rebuilds"] > stats[-1]["rebuilds"]:  # this step's compaction rebuilt
            assert st["carried"] == len(want) == st["occupancy"], (step, st)
        if len(stats) > 1 and stats[-1]["rebuilds"] > stats[-2]["rebuilds"]:
            after_rebuild += 1  # this step ran on the table a carry-over rebuild left
        stats.append(st)
    assert after_rebuild >= 3, stats
    assert not eng.overflowed()


@pytest.mark.gpu
@pytest.mark.parametrize("carry", [True, False])
def test_carry_keeps_the_batch_keys_across_a_rebuild(gpu_device, carry):
    """The batch holds 16 384 distinct keys, a quarter of the table: the most
    a table sized by the 4x headroom holds.  A distinct-key filler before it
    is the least that makes the batch's own compaction pass the threshold
    (3/8 of the table with carry-over: 8 200 keys; half of it without: 16 392),
    so that compaction rebuilds.  With carry-over the rebuild keeps exactly
    the batch's keys, and the same batch again claims only the holes: kept
    keys whose chain lost a filler's slot in front of them.  The batch was
    inserted at loads 0.125 .. 0.375; a sequential model of the probing gives
    2 300 - 2 400 such keys (14 %), the bound is a quarter of the batch.
    Observed on gfx950: 2 130 (13 %).  (Behind a fuller table the share is
    larger: 6 852 of 12 925 keys inserted at loads 0.50 .. 0.70 in a build
    with the threshold at half the table.  A key claimed in a hole has moved
    towards its home, so keys that keep coming back settle.)"""
    eng = _engine(gpu_device, carry, max_rows=ROWS + 1)
    counts = torch.zeros(1, dtype=torch.int64, device=gpu_device)
    send = torch.zeros((ROWS + 1) * F, dtype=torch.int64, device=gpu_device)
    filler = 1025 if carry else ROWS + 1
    k, y = _distinct(1, filler)
    assert len(_prepare(eng, k, y, counts, send)) == filler * F
    st = eng.scratch_stats()
    assert st == dict(capacity=CAP, occupancy=filler * F, rebuilds=0, carried=0), st
    k, y = _distinct(2, ROWS)
    uniq = ROWS * F
    assert len(_prepare(eng, k, y, counts, send)) == uniq
    st = eng.scratch_stats()
    assert st["rebuilds"] == 1 and st["capacity"] == CAP, st
    assert st["carried"] == (uniq if carry else 0), st
    assert st["occupancy"] == (uniq if carry else 0), st
    got = _prepare(eng, k, y, counts, send)
    np.testing.assert_array_equal(np.sort(got), np.unique(k))
    st2 = eng.scratch_stats()
    grown = st2["occupancy"] - st["occupancy"]
    print("carry", carry, "unique", uniq, "claimed again by the repeat batch", grown)
    assert st2["rebuilds"] == 1, st2
    if carry:
        assert 0 <= grown < uniq // 4, (grown, uniq)
    else:
        assert grown == uniq, (grown, uniq)
    assert not eng.overflowed()


def _pair(max_rows):
    return [_engine(d, True, max_rows=max_rows) for d in (CPU, torch.device("cuda", 0))]


def _same_as_cpu(engines, keys):
    keys = np.unique(np.concatenate([k.reshape(-1) for k in keys]))
    assert not engines[1].overflowed()
    np.testing.assert_allclose(engines[1].pull(keys), engines[0].pull(keys), rtol=1e-4, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("first", ["distinct", "hot"])
def test_growth_rebuild_keeps_the_full_clear(gpu_device, first):
    """512 rows, then 4096: the capacity grows.  After a first batch of
    distinct keys the growth comes before the insert (k_scratch_grow: eight
    times the occurrences); after a hot first batch (few keys) the insert runs
    at the small capacity and the compaction scan grows it.  Neither carries."""
    engines = _pair(16384)  # (allocation 2^19: the first batch shrinks the table to 2^16)
    if first == "distinct":
        k0, y0 = _stream(50, rows=512, p_hot=0.0)
    else:
        k0, y0 = _stream(50, rows=512, hot=300, p_hot=1.0)
    k1, y1 = _stream(51, rows=4096, p_hot=0.1)
    seen = []
    for i, (k, y) in enumerate([(k0, y0), (k1, y1), (k1, y1)]):
        for e in engines:
            e.train_step(_batch(k, y, e.device))
        seen.append(k)
        st = engines[1].scratch_stats()
        print(first, "step", i, st)
        assert engines[1].n_unique() == len(np.unique(k))
        if i == 0:
            assert st["capacity"] == CAP and st["rebuilds"] == 1 and st["carried"] == 0, st
        else:
            assert st["capacity"] == 2 * CAP and st["carried"] == 0, st
            assert st["rebuilds"] == (1 if first == "distinct" else 2), st
    _same_as_cpu(engines, seen)


@pytest.mark.gpu
def test_spilled_batch_keeps_the_full_clear(gpu_device):
    """Small vocabularies shrink the table to 2^16 slots; a surge of ~64.5 K
    distinct keys on top of the stale ones then fills it and spills into the
    rest of the allocation (as in test_adaptive_scratch_capacity_matches_cpu).
    That batch's rebuild grows the table and carries nothing."""
    rows = 8192
    engines = _pair(rows)
    seen = []
    stats = []
    for step in range(5):
        if step < 3:
            k, y = _stream(60 + step, rows=rows, hot=2000, p_hot=1.0)
        else:
            rng = np.random.default_rng(step)
            pool = rng.integers(0, 1 << 62, size=2_000_000, dtype=np.int64).astype(np.uint64)
            k = np.ascontiguousarray(pool[rng.integers(0, pool.size, size=rows * F)].reshape(F, rows))
            y = (rng.random(rows) < 0.3).astype(np.float32)
        for e in engines:
            e.train_step(_batch(k, y, e.device))
        seen.append(k)
        assert engines[1].n_unique() == len(np.unique(k)), step
        stats.append(engines[1].scratch_stats())
    print(stats)
    assert stats[2]["capacity"] == CAP, stats
    # the surge: more keys than the active table has free slots
    assert len(np.unique(seen[3])) + stats[2]["occupancy"] > CAP
    assert stats[3]["rebuilds"] == stats[2]["rebuilds"] + 1 and stats[3]["carried"] == 0, stats
    assert stats[3]["capacity"] > CAP and stats[3]["occupancy"] == 0, stats
    _same_as_cpu(engines, seen)


@pytest.mark.gpu
def test_stamp_epoch_wrap_with_carry(gpu_device):
    """300 one-tile steps (1024 occurrences) cross the wrap of the byte stamps
    at epoch 255 and several carry-over rebuilds: the unique count is exact in
    every step."""
    rows = 128
    eng = _engine(gpu_device, True)
    counts = torch.zeros(1, dtype=torch.int64, device=gpu_device)
    send = torch.zeros(ROWS * F, dtype=torch.int64, device=gpu_device)
    rebuilds_at = []
    last = 0
    for step in range(300):
        k, y = _stream(2000 + step, rows=rows, hot=400)
        got = _prepare(eng, k, y, counts, send)
        want = np.unique(k)
        assert len(got) == len(want), step
        if step % 16 == 0 or 250 <= step < 262:
            np.testing.assert_array_equal(np.sort(got), want, err_msg=f"step {step}")
            st = eng.scratch_stats()
            if st["rebuilds"] > last:
                rebuilds_at.append(step)
                last = st["rebuilds"]
    st = eng.scratch_stats()
    print(st, rebuilds_at)
    assert st["rebuilds"] >= 3 and st["capacity"] == CAP, st
    assert not eng.overflowed()


def test_config_switch_and_cpu_stats():
    """The switch reaches the native engine on every backend; the CPU backend
    reports its fixed capacity and its claims, and no rebuilds."""
    assert EngineConfig().scratch_carry is True
    for carry in (True, False):
        eng = _engine(CPU, carry)
        k, y = _stream(0)
        eng.train_step(_batch(k, y, CPU))
        st = eng.scratch_stats()
        assert st == dict(capacity=CAP, occupancy=len(np.unique(k)), rebuilds=0, carried=0), st
