"""Feature admission (EngineConfig.admit_min_count, docs/DESIGN.md §2): a
training pull inserts a key only once the blocked counting filter in front
of the table has seen it admit_min_count times.

The oracle is a pure-Python model of the filter and the three-phase decision
(FilterModel) on the hash mirrored in xflow_amd/testing/hashing.py: per
inserting pull, every entry whose key is not in the table adds 1 (saturating
at 255) to both of its counters, then every such entry reads both counters
and its key is admitted iff min(c0, c1) >= admit_min_count.
"""
import json
import logging
import os

import numpy as np
import pytest
import torch

from xflow_amd import checkpoint
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Batch, Engine
from xflow_amd.testing.hashing import admit_pos, normal_init

CPU = torch.device("cpu")
NO_SLOT = 0xFFFFFFFF

DEVICES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]


@pytest.fixture
def device(request):
    if request.param == "cpu":
        return CPU
    return request.getfixturevalue("gpu_device")


# (model kind, fm_math): LR, reference FM, standard FM, MVM
MODELS = [("lr", "reference"), ("fm", "reference"), ("fm", "standard"), ("mvm", "reference")]
MODEL_IDS = ["lr", "fm-ref", "fm-std", "mvm"]


class FilterModel:
    """The filter, the decision and the table's key set."""

    def __init__(self, log2, min_count):
        self.log2, self.min_count = log2, min_count
        self.c = np.zeros(1 << log2, dtype=np.uint8)
        self.table = set()

    def pull(self, entries):
        """One inserting pull over `entries` (one key per entry); returns the
        keys it admits."""
        absent = np.array([k for k in entries if int(k) not in self.table], dtype=np.uint64)
        if len(absent) == 0:
            return set()
        c0, c1 = admit_pos(absent, self.log2)
        for a, b in zip(c0, c1):
            for i in (a, b):
                if self.c[i] < 255:
                    self.c[i] += 1
        ok = np.minimum(self.c[c0], self.c[c1]) >= self.min_count
        new = {int(k) for k in absent[ok]}
        self.table |= new
        return new

    def step(self, batch_keys):
        return self.pull(np.unique(batch_keys))

    def counts(self, keys):
        c0, c1 = admit_pos(np.asarray(keys, dtype=np.uint64), self.log2)
        return np.minimum(self.c[c0], self.c[c1])


def _key(f, i):
    return (f * 1_000_003 + i + 1) * 0x9E3779B97F4A7C15 % (1 << 64)


def _batch(rows_keys, labels, device, slice_rows=0, fgid=None):
    """CSR batch from a list of per-row key lists (field = position)."""
    keys = np.array([k for r in rows_keys for k in r], dtype=np.uint64)
    rp = np.cumsum([0] + [len(r) for r in rows_keys]).astype(np.int32)
    fg = np.array([j for r in rows_keys for j in range(len(r))], dtype=np.int32) if fgid is None \
        else np.asarray(fgid, dtype=np.int32)
    return Batch(keys=torch.from_numpy(keys.view(np.int64)).to(device),
                 labels=torch.from_numpy(np.asarray(labels, dtype=np.float32)).to(device),
                 row_ptr=torch.from_numpy(rp).to(device), fgid=torch.from_numpy(fg).to(device),
                 slice_rows=slice_rows)


def _schedule(steps=8, rows=32, fields=4, seed=5, p_once=0.12, key=None):
    """Per step a list of rows of `fields` keys: keys that occur every step
    (rows 0-4), keys with periods 2 and 3, keys that occur once, and in steps
    2 and 5 one key five times in the batch and nowhere else.  key(f, i): the
    key of id i in field f (_key)."""
    key = key or _key
    rng = np.random.default_rng(seed)
    out, fresh = [], 1000
    for t in range(steps):
        batch = []
        for r in range(rows):
            row = []
            for f in range(fields):
                u = rng.random()
                if r < 5:
                    i = r                                   # every step
                elif t in (2, 5) and f == 0 and r < 10:
                    i = 900                                 # five times in this batch
                elif u < p_once:
                    fresh += 1
                    i = fresh                               # once
                elif u < 0.5:
                    i = 100 + int(rng.integers(0, 6)) if t % 2 == 0 else int(rng.integers(0, 5))
                else:
                    i = 200 + int(rng.integers(0, 6)) if t % 3 == 0 else 5 + int(rng.integers(0, 5))
                row.append(key(f, i))
            batch.append(row)
        out.append(batch)
    return out


def _labels(rows, t):
    return ((np.arange(rows) * 7 + t) % 3 == 0).astype(np.float32)


def _flat(batch):
    return np.array([k for r in batch for k in r], dtype=np.uint64)


def _no_shared_counter(keys, log2):
    c0, c1 = admit_pos(np.asarray(keys, dtype=np.uint64), log2)
    return len(np.unique(np.concatenate([c0, c1]))) == 2 * len(keys)


def _engine(device, kind="lr", fm_math="reference", opt="ftrl", S=1, rows=64, nnz=1024, **cfg):
    cfg.setdefault("table_log2_cap", 16)
    # (MVM: initial latent values of order 1 keep the products of the field
    # sums, and so the gradients, live -- as tests/test_csr_slices.py does;
    # N(0,1) * 0.25 leaves every FTRL weight at exactly 0)
    o = OptimConfig(kind=opt, sgd_v_init=0.9, v_init_scale=1.0) if kind == "mvm" \
        else OptimConfig(kind=opt)
    return Engine(ModelConfig(kind=kind, v_dim=4, fm_math=fm_math, mvm_math="fixed"), o,
                  EngineConfig(max_rows=rows, max_nnz=nnz, max_slices=S, **cfg), device=device)


def _export(eng):
    k, w = eng.export_table()
    w = np.asarray(w).reshape(len(k), eng.state_words)
    o = np.argsort(k)
    return np.asarray(k)[o], w[o]


# ---- 1. exact admission step ------------------------------------------------
@pytest.mark.parametrize("S", [1, 4, 8])
@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_exact_admission_step(device, model, opt, S):
    """After every step the table holds exactly the keys with at least 3
    step-sightings (a key five times in one batch counts once), on the fused
    (S = 1), slice-group and CSR layouts."""
    LOG2, MIN = 22, 3
    sched = _schedule()
    allk = np.unique(np.concatenate([_flat(b) for b in sched]))
    assert 150 <= len(allk) <= 300
    assert _no_shared_counter(allk, LOG2)  # precondition: the filter counts exactly
    eng = _engine(device, model[0], model[1], opt, S, admit_min_count=MIN, admit_log2=LOG2)
    assert eng.admit_bytes() == 1 << LOG2
    fm = FilterModel(LOG2, MIN)
    seen = {}
    for t, b in enumerate(sched):
        eng.train_step(_batch(b, _labels(len(b), t), device, slice_rows=len(b) // S))
        fm.step(_flat(b))
        for k in np.unique(_flat(b)):
            seen[int(k)] = seen.get(int(k), 0) + 1
        want = np.array(sorted(fm.table), dtype=np.uint64)
        # (no shared counters: the model is the exact count)
        assert fm.table == {k for k, c in seen.items() if c >= MIN}
        assert eng.table_size() == len(want)
        np.testing.assert_array_equal(_export(eng)[0], want)
    assert not eng.overflowed()
    assert _key(0, 900) not in fm.table and seen[_key(0, 900)] == 2  # 10 occurrences, 2 steps
    assert 0 < len(fm.table) < len(allk)
    np.testing.assert_array_equal(eng.admit_counts(allk), fm.counts(allk))


# ---- 2. unadmitted keys neither train nor disturb -----------------------------
def _anchored(steps=8, rows=32, seed=9):
    """Rows of (anchor, 3 more keys): one of four anchor keys, which occur in
    every step, in every row -- so dropping unadmitted occurrences empties
    whole steps (the first) but never a single row."""
    base = _schedule(steps, rows, 3, seed)
    return [[[_key(7, r % 4)] + row for r, row in enumerate(b)] for b in base]


@pytest.mark.parametrize("S", [1, 8])
@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_unadmitted_keys_neither_train_nor_disturb(device, S):
    """LR-FTRL with admit_min_count = 2 on full batches == admission off on
    the batches without the occurrences the model calls unadmitted, bitwise:
    an unadmitted LR key adds 0.0 to its row and its gradient is dropped.

    Every row lists its unadmitted occurrences last, in both runs, so that
    removing them leaves each remaining occurrence at its position in the
    row: the GPU gradient reduction rounds a workgroup's partial sum per row
    position (model_common.h ListAgg::column), with or without admission,
    so a key's bits depend on the positions of its occurrences."""
    LOG2, MIN = 22, 2
    sched = _anchored()
    allk = np.unique(np.concatenate([_flat(b) for b in sched]))
    assert _no_shared_counter(allk, LOG2)
    a = _engine(device, S=S, admit_min_count=MIN, admit_log2=LOG2)
    b = _engine(device, S=S)
    fm = FilterModel(LOG2, MIN)
    trained_b = 0
    for t, rows in enumerate(sched):
        lab = _labels(len(rows), t)
        fm.step(_flat(rows))  # (the order inside a row does not matter to the model)
        rows = [sorted(r, key=lambda k: int(k) not in fm.table) for r in rows]
        a.train_step(_batch(rows, lab, device, slice_rows=len(rows) // S))
        kept = [[k for k in r if int(k) in fm.table] for r in rows]
        if not any(kept):
            continue  # the whole step is unadmitted
        assert all(kept), "a single row became empty"
        fg = [j for r in rows for j, k in enumerate(r) if int(k) in fm.table]
        b.train_step(_batch(kept, lab, device, slice_rows=len(rows) // S, fgid=fg))
        trained_b += 1
    assert 0 < trained_b < len(sched)
    ka, wa = _export(a)
    kb, wb = _export(b)
    assert 0 < len(ka) < len(allk)
    np.testing.assert_array_equal(ka, kb)
    assert np.abs(wa.view(np.float32)).max() > 0
    np.testing.assert_array_equal(wa, wb)


# ---- 3. order-free under collisions -------------------------------------------
def _collide_run(device, sched, min_count):
    eng = _engine(device, rows=128, nnz=1024, admit_min_count=min_count, admit_log2=6)
    for t, b in enumerate(sched):
        eng.train_step(_batch(b, _labels(len(b), t), device))
    assert not eng.overflowed()
    return _export(eng) + (eng.admit_export(),)


@pytest.mark.gpu
@pytest.mark.parametrize("min_count", [2, 4])
def test_order_free_under_collisions(gpu_device, min_count):
    """A one-block filter (64 counters for ~300 keys): two GPU runs give
    bitwise-equal tables and filters; the filter and the admitted key set
    equal the CPU backend's and the Python model's (the model holds no
    weights; GPU and CPU weights are compared in test 4); every key the exact
    count admits is in the table -- a collision only admits early."""
    sched = _schedule(steps=6, rows=48, fields=4, seed=21, p_once=0.3)
    allk = np.unique(np.concatenate([_flat(b) for b in sched]))
    assert 250 <= len(allk) <= 400
    k1, w1, f1 = _collide_run(gpu_device, sched, min_count)
    k2, w2, f2 = _collide_run(gpu_device, sched, min_count)
    np.testing.assert_array_equal(k1, k2)
    np.testing.assert_array_equal(w1, w2)
    np.testing.assert_array_equal(f1, f2)
    kc, _, fc = _collide_run(CPU, sched, min_count)
    np.testing.assert_array_equal(k1, kc)
    np.testing.assert_array_equal(f1, fc)
    fm = FilterModel(6, min_count)
    seen = {}
    for b in sched:
        fm.step(_flat(b))
        for k in np.unique(_flat(b)):
            seen[int(k)] = seen.get(int(k), 0) + 1
    np.testing.assert_array_equal(k1, np.array(sorted(fm.table), dtype=np.uint64))
    np.testing.assert_array_equal(f1, fm.c)
    exact = {k for k, c in seen.items() if c >= min_count}
    assert exact <= set(int(k) for k in k1)
    assert len(exact) < len(k1)  # (and collisions did admit some early)


# ---- 4. GPU == CPU backend with admission on ------------------------------------
# MVM's gradient of a key divides the row's product by 1 + v of that key, so
# its condition number in v is 1 / |1 + v|.  A key's first v is the lazy
# N(0,1) init (v_init_scale 1.0 here), computed with logf / cosf, which the
# device and the host libm may round differently in the last bits: allow 4 ulp
# of a float in [1, 2), 4 * 2^-23 = 4.8e-7.  For that input difference to stay a
# tenth of the comparison's rtol (2e-4), |1 + v| must be at least
# 4.8e-7 / 2e-5 = 0.024.  The MVM comparison therefore runs on keys that meet
# this bound in every dim (about 1 % of N(0,1) values do not) -- a
# precondition of comparing the two backends at this tolerance, asserted
# below, like the "no shared counter" one of test 1.
MVM_MIN_1PV = 4 * 2.0 ** -23 / (2e-4 / 10)


def _mvm_conditioned(keys):
    k = np.asarray(keys, dtype=np.uint64)
    v = np.stack([normal_init(k, d) for d in range(4)], axis=1)
    return (np.abs(1.0 + v) >= MVM_MIN_1PV).all(axis=1)


def _mvm_key(f, i):
    """_key(f, i), or the first of _key(f, i + 100000 * j) that is conditioned."""
    while not _mvm_conditioned([_key(f, i)])[0]:
        i += 100000
    return _key(f, i)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
@pytest.mark.parametrize("model", MODELS, ids=MODEL_IDS)
def test_gpu_equals_cpu_backend(gpu_device, model, opt):
    """8 fields x 64 rows x 6 steps, admit_min_count = 2.  The key sets and
    the filters are equal; LR tables are bitwise equal; FM and MVM weights
    within the tolerance of the project's GPU-vs-CPU check on tiny batches
    (tests/test_csr_slices.py test_csr_steps_with_empty_and_tiny_batches:
    rtol 2e-4, atol 1e-6 on the pulled weights).

    LR: every key occurs at most once per batch (and 1 to 4 times over the
    steps).  The backends sum a key's occurrences differently -- the GPU
    exactly in fixed point and rounds once, the CPU in a sequential float
    loop (tests/test_determinism.py) -- so with or without admission their LR
    tables are bitwise equal only where each sum has one term.  Measured on
    the schedule the other models use here (keys repeat inside a batch):
    max |dw| 7.0e-10 (FTRL, 69 of 354 state words differ) and 7.3e-12 (SGD,
    30 of 354).

    MVM: on keys whose lazy init meets MVM_MIN_1PV (above).  On the same
    schedule without that precondition one key has a first v of -0.99984 in
    dim 1 (1 + v = 1.6e-4) and its first push differs between the backends
    by 6.4e-4 relative (6.8e-5 absolute; 1 of 708 weights, with FTRL) -- and
    by 5.7e-4 with admission off: a property of that key's init, not of
    admission."""
    if model[0] == "lr":
        sched = [[[_key(f, r + 19 * t) for f in range(8)] for r in range(64)]
                 for t in range(6)]
    elif model[0] == "mvm":
        sched = _schedule(steps=6, rows=64, fields=8, seed=33, key=_mvm_key)
        assert _mvm_conditioned(np.unique(np.concatenate([_flat(b) for b in sched]))).all()
    else:
        sched = _schedule(steps=6, rows=64, fields=8, seed=33)
    out = []
    for dev in (gpu_device, CPU):
        eng = _engine(dev, model[0], model[1], opt, rows=64, nnz=1024, admit_min_count=2,
                      admit_log2=20)
        for t, b in enumerate(sched):
            eng.train_step(_batch(b, _labels(len(b), t), dev))
        assert not eng.overflowed()
        k, w = _export(eng)
        out.append((k, w, eng.pull(k), eng.admit_export()))
    (gk, gw, gp, gf), (ck, cw, cp, cf) = out
    allk = np.unique(np.concatenate([_flat(b) for b in sched]))
    assert 0 < len(gk) < len(allk)
    np.testing.assert_array_equal(gk, ck)
    np.testing.assert_array_equal(gf, cf)
    assert np.abs(cp).max() > 0
    if model[0] == "lr":
        diff = np.abs(gp - cp).max()
        print("LR GPU vs CPU: max |dw| =", diff, "differing words:", int((gw != cw).sum()))
        np.testing.assert_array_equal(gw, cw)
    else:
        np.testing.assert_allclose(gp, cp, rtol=2e-4, atol=1e-6)


# ---- 5. saturation --------------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_saturation(device):
    """One key, admit_min_count = 255: absent after 254 steps, present after
    255; its estimate stays 255, also after five sightings of a second key
    that shares a counter with it."""
    LOG2 = 6
    k1 = _key(0, 0)
    a0, a1 = (int(x[0]) for x in admit_pos(np.array([k1], dtype=np.uint64), LOG2))
    k2 = None
    for i in range(1, 10000):
        b0, b1 = (int(x[0]) for x in admit_pos(np.array([_key(1, i)], dtype=np.uint64), LOG2))
        if len({a0, a1} & {b0, b1}) == 1:
            k2 = _key(1, i)
            break
    assert k2 is not None
    eng = _engine(device, rows=4, nnz=16, admit_min_count=255, admit_log2=LOG2)
    one = _batch([[k1]], [1.0], device)
    for t in range(1, 261):
        eng.train_step(one)
        if t == 254:
            assert eng.table_size() == 0
            assert eng.admit_counts([k1])[0] == 254
        if t == 255:
            assert eng.table_size() == 1
            np.testing.assert_array_equal(_export(eng)[0], [k1])
    assert eng.admit_counts([k1])[0] == 255
    two = _batch([[k2]], [0.0], device)
    for _ in range(5):
        eng.train_step(two)
    assert eng.admit_counts([k1])[0] == 255
    assert eng.admit_counts([k2])[0] == 5
    f = eng.admit_export()
    assert f.max() == 255 and int((f == 255).sum()) == 2
    assert eng.table_size() == 1 and not eng.overflowed()


# ---- 6. lookups never count -------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_lookups_never_count(device):
    eng = _engine(device, kind="fm", admit_min_count=2, admit_log2=16)
    rows = _schedule(steps=1, rows=16, fields=4, seed=2)[0]
    keys = np.unique(_flat(rows))
    b = _batch(rows, _labels(16, 0), device)
    for _ in range(3):
        eng.eval_step(b)
        eng.pull(keys)
    assert eng.table_size() == 0
    assert not eng.admit_counts(keys).any() and not eng.admit_export().any()
    # explicit inserts bypass the filter
    eng.push(keys[:5], np.ones((5, eng.params_per_key), np.float32))
    assert eng.table_size() == 5
    other = _engine(device, kind="fm", admit_min_count=2, admit_log2=16)
    k, w = eng.export_table()
    other.import_table(k, w)
    assert other.table_size() == 5
    np.testing.assert_array_equal(_export(other)[0], np.sort(keys[:5]))
    assert not eng.admit_export().any() and not other.admit_export().any()
    # ... and a training step counts only the keys that are not in the table
    eng.train_step(b)
    assert eng.table_size() == 5
    np.testing.assert_array_equal(eng.admit_counts(keys), [0] * 5 + [1] * (len(keys) - 5))


# ---- 7. two sources in one s_pull ---------------------------------------------------
@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_two_sources_in_one_s_pull(device):
    """A sighting in s_pull is one received entry: the same key from two
    sources is sighted twice in the call, and both entries decide alike."""
    k, other = _key(3, 1), _key(3, 2)
    recv = torch.from_numpy(np.array([k, other, k], dtype=np.uint64).view(np.int64)).to(device)
    for min_count, admitted in ((2, True), (3, False)):
        eng = _engine(device, admit_min_count=min_count, admit_log2=16)
        vals = torch.zeros(3, eng.value_width, dtype=torch.float32, device=device)
        eng.s_pull(recv, 3, vals, insert=True, buf=0, offsets=[0, 2, 3])
        s = eng.server_slots(0)
        assert s[1] == NO_SLOT  # one sighting
        if admitted:
            assert s[0] != NO_SLOT and s[0] == s[2]
            assert eng.table_size() == 1
            np.testing.assert_array_equal(_export(eng)[0], [k])
        else:
            assert s[0] == NO_SLOT and s[2] == NO_SLOT
            assert eng.table_size() == 0
        assert not eng.overflowed()
        np.testing.assert_array_equal(eng.admit_counts([k, other]), [2, 1])
        # a lookup-only s_pull neither counts nor inserts
        eng.s_pull(recv, 3, vals, insert=False, buf=1, offsets=[0, 2, 3])
        np.testing.assert_array_equal(eng.admit_counts([k, other]), [2, 1])
        assert eng.table_size() == (1 if admitted else 0)


# ---- 8. growth ----------------------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_growth(device):
    """A 16-slot table that grows by segment splits during the run still
    holds exactly the model's keys; an s_pull buffer pulled before a split
    and applied after it skips its unadmitted entries."""
    LOG2, MIN = 20, 2
    sched = _schedule(steps=8, rows=32, fields=4, seed=13)
    allk = np.unique(np.concatenate([_flat(b) for b in sched]))
    assert _no_shared_counter(allk, LOG2)
    eng = _engine(device, table_log2_cap=4, table_grow=True, admit_min_count=MIN, admit_log2=LOG2)
    fm = FilterModel(LOG2, MIN)
    for t, b in enumerate(sched):
        eng.train_step(_batch(b, _labels(len(b), t), device))
        fm.step(_flat(b))
        assert eng.table_size() == len(fm.table)
    assert eng.table_splits >= 1 and not eng.overflowed()
    np.testing.assert_array_equal(_export(eng)[0], np.array(sorted(fm.table), dtype=np.uint64))
    # s_pull: keys seen once so far (admitted by this sighting), new keys
    # (not admitted) and present keys; then a split; then the apply
    once = [k for k in allk if fm.counts([k])[0] == 1][:6]
    new = [_key(9, i) for i in range(6)]
    old = sorted(fm.table)[:4]
    assert len(once) == 6 and _no_shared_counter(np.concatenate([allk, new]), LOG2)
    recv_np = np.array(once + new + old, dtype=np.uint64)
    n = len(recv_np)
    recv = torch.from_numpy(recv_np.view(np.int64)).to(device)
    vals = torch.zeros(n, eng.value_width, dtype=torch.float32, device=device)
    before = eng.pull(recv_np).copy()
    eng.s_pull(recv, n, vals, insert=True, buf=0, offsets=[0, n])
    fm.pull(recv_np)
    s0 = eng.server_slots(0)
    np.testing.assert_array_equal(s0 == NO_SLOT, [False] * 6 + [True] * 6 + [False] * 4)
    splits = eng.table_splits
    cap_log2 = int(np.log2(eng.table_capacity - 1)) + 1
    eng.grow_table(cap_log2 + 2)
    assert eng.table_splits > splits
    s1 = eng.server_slots(0)
    np.testing.assert_array_equal(s1 == NO_SLOT, s0 == NO_SLOT)
    assert (s1 != s0).any()  # (keys moved: the slots were looked up again)
    grads = torch.ones(n, dtype=torch.float32, device=device)
    eng.s_apply(recv, grads, None, [0, n], 1, buf=0)
    eng.end_step()
    assert not eng.overflowed()
    assert eng.table_size() == len(fm.table)
    np.testing.assert_array_equal(_export(eng)[0], np.array(sorted(fm.table), dtype=np.uint64))
    after = eng.pull(recv_np)
    assert (after[:6] != 0).all() and (after[12:] != before[12:]).all()  # applied
    assert (after[6:12] == 0).all()                                     # skipped


# ---- 9. checkpoint ----------------------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_checkpoint_resume(device, tmp_path, caplog):
    LOG2, MIN = 18, 3
    sched = _schedule(steps=8, rows=32, fields=4, seed=17)
    mk = lambda **kw: _engine(device, kind="fm", **kw)

    def run(eng, steps):
        for t in steps:
            eng.train_step(_batch(sched[t], _labels(len(sched[t]), t), device))

    full = mk(admit_min_count=MIN, admit_log2=LOG2)
    run(full, range(8))
    a = mk(admit_min_count=MIN, admit_log2=LOG2)
    run(a, range(4))
    d = str(tmp_path / "on")
    checkpoint.save(a, d, 0, 1, meta={"epoch": 0})
    meta = json.load(open(os.path.join(d, "meta.json")))
    assert meta["admit_min_count"] == MIN and meta["admit_log2"] == LOG2
    assert sorted(os.listdir(d)) == [checkpoint.admit_name(0, 1), "meta.json",
                                     checkpoint.shard_name(0, 1)]
    b = mk(admit_min_count=MIN, admit_log2=LOG2)
    checkpoint.load(b, d, 0, 1)
    np.testing.assert_array_equal(b.admit_export(), a.admit_export())
    run(b, range(4, 8))
    kf, wf = _export(full)
    kb, wb = _export(b)
    assert 0 < len(kf)
    np.testing.assert_array_equal(kb, kf)
    np.testing.assert_array_equal(wb, wf)
    np.testing.assert_array_equal(b.admit_export(), full.admit_export())
    assert full.admit_export().any()

    # another filter size: the table loads, the filter starts empty, the log says so
    c = mk(admit_min_count=MIN, admit_log2=LOG2 + 1)
    with caplog.at_level(logging.WARNING, logger="xflow_amd.checkpoint"):
        checkpoint.load(c, d, 0, 1)
    assert any("sightings again" in r.getMessage() for r in caplog.records)
    assert not c.admit_export().any()
    np.testing.assert_array_equal(_export(c)[0], _export(a)[0])

    # admission off: today's files and meta.json keys
    off = mk()
    run(off, range(2))
    d2 = str(tmp_path / "off")
    checkpoint.save(off, d2, 0, 1, meta={"epoch": 0})
    assert sorted(os.listdir(d2)) == ["meta.json", checkpoint.shard_name(0, 1)]
    assert sorted(json.load(open(os.path.join(d2, "meta.json")))) == \
        ["epoch", "model", "optim", "world"]


# ---- 10. off is off -----------------------------------------------------------------------
def test_config_range():
    for bad in (dict(admit_min_count=0), dict(admit_min_count=256), dict(admit_log2=5),
                dict(admit_log2=33)):
        with pytest.raises(ValueError):
            _engine(CPU, **bad)
    # automatic size: min(32, largest log2 capacity + 1)
    e = _engine(CPU, table_log2_cap=10, max_log2_cap=14, admit_min_count=2)
    assert e.admit_log2 == 15 and e.admit_bytes() == 1 << 15
    e = _engine(CPU, table_log2_cap=10, table_grow=False, admit_min_count=2)
    assert e.admit_log2 == 11
    assert _engine(CPU).admit_bytes() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("model", [MODELS[0], MODELS[2]], ids=["lr", "fm-std"])
def test_off_is_off(gpu_device, model):
    """admit_min_count = 1: no filter, and the table of a short run equals
    that of an engine built without the new arguments, bitwise."""
    sched = _schedule(steps=4, rows=32, fields=4, seed=3)
    n = __import__("xflow_amd.native", fromlist=["load"]).load()
    m = ModelConfig(kind=model[0], v_dim=4, fm_math=model[1])
    old = n.Engine(m.native(), OptimConfig().native(), table_log2_cap=16, max_rows=64,
                   max_nnz=1024, device=gpu_device.index)
    new = _engine(gpu_device, model[0], model[1], admit_min_count=1)
    assert new.admit_bytes() == 0 and old.admit_bytes == 0
    assert not new.admit_counts(np.unique(_flat(sched[0]))).any()
    for t, b in enumerate(sched):
        bt = _batch(b, _labels(len(b), t), gpu_device)
        new.train_step(bt)
        old.set_stream(torch.cuda.current_stream(gpu_device).cuda_stream)
        old.train_step(bt.view())
    kn, wn = _export(new)
    ko, wo = old.export_table()
    o = np.argsort(ko)
    assert len(kn) == len(np.unique(np.concatenate([_flat(b) for b in sched])))
    np.testing.assert_array_equal(kn, np.asarray(ko)[o])
    np.testing.assert_array_equal(wn, np.asarray(wo).reshape(len(ko), -1)[o])
