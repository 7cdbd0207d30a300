"""Ranked reduction outputs (docs/DESIGN.md section 3, EngineConfig.red_rank):
on a one-slice LR or reference-FM step with slot positions the gradient
reduction (k_red_sum) finds the unique-list index of a slot from the dedup's
stamps and the compaction's chunk offsets, and the compaction writes no
slot -> unique map.  Both ways name the same index -- the unique list is in
slot order -- so training with the switch on and off must agree bit for bit:
the exported table state, the predictions of an eval step, and the loss sums.

Which branch of k_red_sum a case reaches follows from Engine.count_records:
a unit (16 384 LR slots, 8 192 FM slots) with more than 8 192 records takes
the dense branch, any other the register branch.  A step with more records
than units x 8 192 therefore has a dense unit, and a step with at most 8 192
records has none; the cases below assert whichever they claim.

Reference semantics: per-key gradient sums of a batch (lr_worker.cc:100-119,
fm_worker.cc:126-157).
"""
import numpy as np
import pytest
import torch

from xflow_amd import native
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Batch, Engine

MIN_CAP = 1 << 16   # kScratchMinCap
DENSE_AT = 8192     # records of a unit above which it takes the dense branch
UNIT = {"lr": 1 << 14, "fm": 1 << 13}  # slots per k_red_sum unit


def _labels(seed, rows):
    return (np.random.default_rng(seed).random(rows) < 0.3).astype(np.float32)


def _skewed(step, rows, F, hot=3000, p_hot=0.25):
    """[F][rows]: a hot vocabulary that comes back every batch (skewed inside
    as well) plus random 62-bit keys, new in every batch"""
    rng = np.random.default_rng(1000 + step)
    n = rows * F
    hot_keys = (np.arange(1, hot + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(2)
    k = rng.integers(1, 1 << 62, size=n, dtype=np.int64).astype(np.uint64)
    pick = rng.random(n) < p_hot
    k[pick] = hot_keys[np.minimum(rng.zipf(1.2, size=int(pick.sum())), hot) - 1]
    return np.ascontiguousarray(k.reshape(F, rows)), _labels(step, rows)


def _distinct(tag, rows, F):
    n = rows * F
    k = (np.uint64(1) << np.uint64(62)) + np.uint64(tag) * np.uint64(1 << 32) + np.arange(n, dtype=np.uint64)
    return np.ascontiguousarray(k.reshape(F, rows)), _labels(tag, rows)


def _one_key(tag, rows, F):
    return np.full((F, rows), 12345 + tag, dtype=np.uint64), _labels(tag, rows)


def _batch(k, y, dev):
    return Batch(keys=torch.from_numpy(k.reshape(-1).view(np.int64)).to(dev),
                 labels=torch.from_numpy(y).to(dev), nnz_per_row=k.shape[0], field_major=True)


def _train(dev, batches, on, kind="lr", lead=True, scratch_factor=2.5, overflow=False, each=None,
           count=False):
    """Trains all batches but the last, evaluates the last.  each(eng, step,
    k): called after every step; count: with Engine.count_records."""
    max_rows = max(k.shape[1] for k, _ in batches)
    F = batches[0][0].shape[0]
    eng = Engine(ModelConfig(kind=kind, v_dim=4), OptimConfig(),
                 EngineConfig(table_log2_cap=18, max_rows=max_rows, max_nnz=max_rows * F,
                              lead_handoff=lead, scratch_factor=scratch_factor, red_rank=on),
                 device=dev)
    if count:
        eng.count_records(True)
    want_grad = "unique_lr" if kind == "lr" else "unique_fm_bc"
    for step, (k, y) in enumerate(batches[:-1]):
        if overflow:
            # (the capacity monitor reports the flag once the step is queued)
            try:
                eng.train_step(_batch(k, y, dev))
            except RuntimeError as e:
                assert "scratch overflow" in str(e)
        else:
            eng.train_step(_batch(k, y, dev))
        p = eng.native.step_plan(1, k.shape[1], F, True)
        # on: ranked from the stamps; off: the same layout through the map
        assert p["red_rank"] == on and p["grad"] == want_grad and not p["upos"], (step, p)
        if each:
            each(eng, step, k)
    assert eng.overflowed() == overflow
    k, y = batches[-1]
    pctr = eng.eval_step(_batch(k, y, dev)).cpu().numpy()
    keys, words = eng.export_table()
    o = np.argsort(keys, kind="stable")
    keys = keys[o]
    words = np.asarray(words).reshape(len(keys), -1)[o]
    return dict(eng=eng, keys=keys, words=words, pctr=pctr, train=eng.read_stats(),
                eval=eng.read_stats(which=1))


def _assert_bit_equal(a, b):
    np.testing.assert_array_equal(a["keys"], b["keys"])
    np.testing.assert_array_equal(a["words"], b["words"])  # the whole slot state
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


SHAPES = {
    # LR with the leader handoff (k_lr_lead)
    "lr_lead_1024x1": dict(kind="lr", mk=lambda s: _skewed(s, 1024, 1, hot=300)),
    "lr_lead_2048x39": dict(kind="lr", mk=lambda s: _skewed(s, 2048, 39)),
    # LR without it: rows no multiple of the tile (k_lr + ListAgg)
    "lr_1000x39": dict(kind="lr", mk=lambda s: _skewed(s, 1000, 39), lead_plan=False),
    "lr_switch_off_2048x39": dict(kind="lr", mk=lambda s: _skewed(s, 2048, 39), lead=False, lead_plan=False),
    # reference FM: (B, C) pairs, units of 8 192 slots
    "fm_2048x18": dict(kind="fm", mk=lambda s: _skewed(s, 2048, 18)),
    "one_key": dict(kind="lr", mk=lambda s: _one_key(s % 2, 1024, 1)),
    "one_key_fm": dict(kind="fm", mk=lambda s: _one_key(s % 2, 1024, 3)),
    "all_distinct": dict(kind="lr", mk=lambda s: _distinct(s % 2, 2048, 39)),
    "all_distinct_fm": dict(kind="fm", mk=lambda s: _distinct(s % 2, 2048, 5)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(SHAPES))
def test_switch_on_equals_off(gpu_device, case):
    c = SHAPES[case]
    batches = [c["mk"](s) for s in range(4)]
    F, rows = batches[0][0].shape
    on, _ = _both(gpu_device, batches, kind=c["kind"], lead=c.get("lead", True))
    lead = on["eng"].native.step_plan(1, rows, F, True)["lead"]
    assert lead == (c["kind"] == "lr" and c.get("lead_plan", True))


@pytest.mark.gpu
def test_carry_over_rebuilds_and_a_capacity_change(gpu_device):
    """2048 x 8 with 14-15 K unique keys: the capacity settles at 2^16 and the
    occupancy passes the rebuild threshold every other step; 8192 x 8 then
    grows the capacity, and the small batches after it run in the larger
    table."""
    batches = [_skewed(s, 2048, 8) for s in range(8)] + [_skewed(20, 8192, 8)] + \
              [_skewed(s, 2048, 8) for s in range(30, 33)]
    stats = {True: [], False: []}
    runs = []
    for on in (True, False):
        runs.append(_train(gpu_device, batches, on,
                           each=lambda e, step, k, on=on: stats[on].append(e.scratch_stats())))
    _assert_bit_equal(*runs)
    # (the occupancy may differ: a key claimed again in a hole depends on slot placement)
    assert [s["capacity"] for s in stats[True]] == [s["capacity"] for s in stats[False]]
    st = stats[True]
    assert st[7]["capacity"] == MIN_CAP and st[7]["rebuilds"] >= 3 and st[7]["carried"] > 0, st
    assert st[8]["capacity"] > MIN_CAP, st  # (grown before the insert: more occurrences than ever)
    assert st[-1]["capacity"] == st[8]["capacity"], st


@pytest.mark.gpu
def test_stamp_epoch_wrap(gpu_device):
    """300 steps of 1024 x 1 cross the wrap of the byte stamps at epoch 255:
    the stamps are cleared there and the epochs start again at 1."""
    batches = [_skewed(2000 + s, 1024, 1, hot=400) for s in range(301)]
    _both(gpu_device, batches)


@pytest.mark.gpu
def test_spilled_batch(gpu_device):
    """Small vocabularies shrink the table to 2^16 slots; a surge of ~64 K
    distinct keys on top of the stale ones fills it and spills into the rest
    of the allocation (ScratchView::ctl[4]): that batch's compaction and
    reduction cover the whole allocation, 2^18 slots."""
    rows, F = 8192, 8
    batches = [_skewed(60 + s, rows, F, hot=2000, p_hot=1.0) for s in range(3)]
    for s in (3, 4):
        rng = np.random.default_rng(s)
        pool = rng.integers(0, 1 << 62, size=2_000_000, dtype=np.int64).astype(np.uint64)
        batches.append((np.ascontiguousarray(pool[rng.integers(0, pool.size, size=rows * F)].reshape(F, rows)),
                        _labels(s, rows)))
    batches.append(_skewed(70, rows, F))
    stats = []
    on, _ = _both(gpu_device, batches, each=lambda e, step, k: stats.append((e.scratch_stats(), e.n_unique(),
                                                                         e.batch_capacity())))
    st = stats[:5]  # (the run with the switch on)
    assert st[2][0]["capacity"] == MIN_CAP, st
    # the surge: more keys than the active table has free slots
    assert len(np.unique(batches[3][0])) + st[2][0]["occupancy"] > MIN_CAP, st
    assert st[3][1] == len(np.unique(batches[3][0])), st
    # the spill itself: the steps before were compacted and reduced over the
    # 2^16 active slots, the surge's batch over the whole allocation (the
    # compaction scan reports that capacity exactly when ctl[4] is the batch's epoch)
    alloc = 1 << 18  # pow2 >= 2.5 x 8192 x 8
    assert [x[2] for x in st[1:4]] == [MIN_CAP, MIN_CAP, alloc], st
    assert st[3][0]["rebuilds"] == st[2][0]["rebuilds"] + 1 and st[3][0]["capacity"] > MIN_CAP, st


@pytest.mark.gpu
def test_trash_slot(gpu_device):
    """A scratch allocation of 16 slots for batches of 64 distinct keys: the
    keys that find no slot go to the trash slot (index 16, past the capacity
    the compaction covered: no unique index), their gradients are dropped and
    the step is flagged.  64 occurrences are one wavefront of the insert
    kernel, so which keys find a slot is decided inside single CAS
    instructions of that wave and is the same in both runs."""
    batches = [_distinct(s, 64, 1) for s in range(4)]
    on, off = _both(gpu_device, batches, scratch_factor=0.2, overflow=True)
    assert 0 < len(on["keys"]) <= 3 * 16  # (16 slots a step, cleared by the rebuilds)


DENSE_ROWS = {"lr": 3072, "fm": 5120}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lr", "fm"])
def test_dense_branch(gpu_device, kind):
    """39 columns of 400 keys each, row r of a column holding key (r + c) mod
    400: 15 600 unique keys, so the capacity settles at 2^16 slots (4 LR units,
    8 FM units), and 400 or more consecutive rows hold all 400 keys of every
    column -- a producer workgroup of 1024 rows leaves 39 x 400 = 15 600
    records, one per key.  The 3 workgroups of 3072 LR rows and the 5 of 5120
    FM rows then leave more records than units x 8 192 (narrower workgroups
    would leave more still), which the record count asserts: at least one
    unit of every step sums densely.

    The loss sums compare bit for bit although the workgroups add to them in
    any order: a term is a float widened to double, and with predictions
    inside (0.01, 0.99) -- three steps from zero weights; asserted on the eval
    step -- every term is a multiple of 2^-30 below 2^3, so a sum of fewer
    than 2^14 of them (3 x 5120 rows) is exact in 53 bits."""
    rows, F, V = DENSE_ROWS[kind], 39, 400
    vocab = (np.arange(1, F * V + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(2)
    r = np.arange(rows)[None, :]
    c = np.arange(F)[:, None]
    batches = []
    for s in range(4):
        k = vocab[c * V + (r + 7 * c + 37 * s) % V]
        batches.append((np.ascontiguousarray(k), _labels(s, rows)))
    assert len(np.unique(batches[0][0])) == F * V
    recs = []
    on, _ = _both(gpu_device, batches, kind=kind, lead=False, count=True,
                  each=lambda e, step, k: recs.append((step, e.take_records(), e.batch_capacity())))
    print(kind, recs)
    assert on["pctr"].min() > 0.01 and on["pctr"].max() < 0.99
    for step, rec, cap in recs:
        if step > 0:  # (the first step runs at the allocation's capacity)
            assert cap == MIN_CAP
            assert rec > (cap // UNIT[kind]) * DENSE_AT, (step, rec, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lr", "fm"])
def test_register_branch(gpu_device, kind):
    """1024 x 4: at most 4096 records a step, so no unit passes 8 192 and
    every unit with records keeps them in registers."""
    batches = [_skewed(s, 1024, 4, hot=500) for s in range(4)]
    recs = []
    _both(gpu_device, batches, kind=kind, count=True, each=lambda e, step, k: recs.append(e.take_records()))
    assert len(recs) == 6 and all(0 < r <= DENSE_AT for r in recs), recs


def test_planner_red_rank_exactly_where_it_applies():
    n = native.load()
    models = {"lr": ModelConfig(kind="lr"), "fm_ref": ModelConfig(kind="fm", v_dim=8, fm_math="reference"),
              "fm_std": ModelConfig(kind="fm", v_dim=8, fm_math="standard"),
              "mvm": ModelConfig(kind="mvm", v_dim=10)}
    seen = 0
    for model in models:
        for opt in ("ftrl", "sgd"):
            for S in (1, 2, 8, 64):
                for gpu in (True, False):
                    for on in (True, False):
                        d = {"model": models[model].native(), "opt": OptimConfig(kind=opt).native(), "gpu": gpu}
                        p = n.plan_step(dict(d, red_rank=on), S)
                        p0 = n.plan_step(dict(d, red_rank=False), S)
                        want = on and gpu and S == 1 and ((model == "lr" and opt == "ftrl") or model == "fm_ref")
                        assert p["red_rank"] == want, (model, opt, S, gpu, on, p)
                        assert not p0["red_rank"]
                        # the switch changes nothing else of the plan
                        assert {k: v for k, v in p.items() if k != "red_rank"} == \
                            {k: v for k, v in p0.items() if k != "red_rank"}
                        seen += want
    assert seen == 3
    assert EngineConfig().red_rank is True
    # the CPU backend plans it off whatever the switch says
    e = Engine(ModelConfig(kind="lr"), OptimConfig(), EngineConfig(table_log2_cap=12, max_rows=64, max_nnz=1024),
               device=torch.device("cpu"))
    assert not e.native.step_plan(1)["red_rank"]
