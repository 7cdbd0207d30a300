"""Delta checkpoints (EngineConfig.delta_track, docs/DESIGN.md §2): a filter of
2^L bits indexed by key hash marks every key whose state may have changed;
Engine.delta_export / save_delta write only the table's keys whose bit is set,
and checkpoint.save(..., delta_base=) / load chain such versions.

The filter is modelled in numpy from the key sets the test feeds the engine
(delta_bit in Python ints), so the bit count, the exported set and the
reconstructed table are all held to exact values, on both backends.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import DATA
from helpers import random_csr, to_batch
from xflow_amd import checkpoint
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig, TrainConfig
from xflow_amd.engine import Engine
from xflow_amd.testing.hashing import fmix64_int, owner_of

CPU = torch.device("cpu")
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
M64 = (1 << 64) - 1
DELTA_SALT = 0xE7037ED1A0B428DB
TRAIN, TEST = os.path.join(DATA, "small_train"), os.path.join(DATA, "small_test")


@pytest.fixture
def device(request):
    if request.param == "cpu":
        return CPU
    return request.getfixturevalue("gpu_device")


def _engine(device, kind="lr", opt="ftrl", fm_math="reference", rows=256, fields=8, slices=1,
            track=True, log2=30, cap=12, **cfg):
    return Engine(ModelConfig(kind=kind, v_dim=4, fm_math=fm_math), OptimConfig(kind=opt),
                  EngineConfig(table_log2_cap=cap, max_rows=rows, max_nnz=rows * (fields + 4),
                               max_slices=slices, delta_track=track,
                               delta_log2=log2 if track else 0, **cfg), device=device)


def _bit(key, L):
    """delta_bit (csrc/include/xflow/common.h) in Python ints."""
    key = int(key)
    if key == M64:
        key = M64 - 1
    return fmix64_int(key ^ DELTA_SALT) & ((1 << L) - 1)


def _bits(keys, L):
    return {_bit(k, L) for k in np.asarray(keys, dtype=np.uint64).tolist()}


def _sorted(keys, words, W):
    keys = np.asarray(keys, dtype=np.uint64)
    words = np.asarray(words, dtype=np.uint32).reshape(len(keys), W)
    o = np.argsort(keys)
    return keys[o], words[o]


def _export(e):
    k, w = e.export_table()
    return _sorted(k, w, e.state_words)


def _delta(e):
    k, w = e.delta_export()
    assert len(k) == e.delta_count()
    return _sorted(k, w, e.state_words)


def _rand_keys(rng, n):
    return np.unique(rng.integers(1, 1 << 62, size=n + n // 4 + 8, dtype=np.int64))[:n] \
        .astype(np.uint64)


def _preload(e, rng, n):
    """n keys no batch touches, with small positive float state words."""
    keys = _rand_keys(rng, n) | (np.uint64(1) << np.uint64(62))
    w = (rng.integers(1, 1 << 20, size=(n, e.state_words)).astype(np.float32) / (1 << 16)) \
        .view(np.uint32)
    if e.layout["kind"] != 0:
        w[:, -1] = 1  # the pushed flag (latent models): the states are taken as they are
    e.import_table(keys, w.reshape(-1))
    return keys


def _batch(device, seed, rows=64, fields=8, slice_rows=0):
    k, rp, fg, lab = random_csr(rows, fields=fields, vocab=300, seed=seed)
    return k, to_batch(k, rp, fg, lab, device, slice_rows=slice_rows)


def _rebuild(live, parts, **kw):
    """A fresh engine of live's configuration with the (keys, words) parts
    upserted in order; returns its sorted full export."""
    f = Engine(live.model, live.optim, EngineConfig(table_log2_cap=14, max_rows=256, max_nnz=4096),
               device=live.device)
    for k, w in parts:
        if len(k):
            f.import_table(k, np.asarray(w).reshape(-1))
    return _export(f)


def _assert_same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


# ---- 1. definition ------------------------------------------------------------------
def _mark(e, keys):
    """Mark a key set through push_host (zero gradients): every key is inserted."""
    if len(keys):
        e.push(keys, np.zeros((len(keys), e.params_per_key), dtype=np.float32))


def _s_pull_mark(e, keys):
    """Mark n received entries (duplicates allowed) through s_pull(insert)."""
    n = len(keys)
    recv = torch.from_numpy(np.asarray(keys, dtype=np.uint64).view(np.int64)).to(e.device)
    vals = torch.zeros(max(n, 1), e.value_width, dtype=torch.float32, device=e.device)
    e.s_pull(recv, n, vals, insert=True, buf=0, offsets=[0, n])


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 513, 5000])
def test_filter_matches_model(device, n):
    """bits_set and delta_count equal the numpy model's for a known key set."""
    L = 16
    e = _engine(device, log2=L, cap=14, rows=1024)
    assert e.delta_stats() == {"log2": L, "bits_set": 0, "needs_full": False}
    keys = _rand_keys(np.random.default_rng(n), n)
    _s_pull_mark(e, keys)
    want = _bits(keys, L)
    st = e.delta_stats()
    assert st["bits_set"] == len(want) and not st["needs_full"]
    assert e.table_size() == n
    # every key of the table is marked: the delta is the table
    assert e.delta_count() == n
    _assert_same(_delta(e), _export(e))
    e.delta_clear()
    assert e.delta_stats()["bits_set"] == 0 and e.delta_count() == 0


@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_filter_one_key_many_entries(device):
    """A launch whose entries are all one key sets one bit."""
    e = _engine(device, log2=12, rows=1024)
    k = np.uint64(0x1234567890ABCDEF)
    _s_pull_mark(e, np.full(5000, k, dtype=np.uint64))
    assert e.delta_stats()["bits_set"] == 1 and e.delta_count() == 1
    np.testing.assert_array_equal(e.delta_export()[0], [k])


@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_filter_contended_words(device):
    """2^10 bits, 5000 keys: every 32-bit word is hit by many lanes at once
    (the contended atomicOr), then the same keys again (the already-set
    skip) change nothing; untouched preloaded keys that share a bit count."""
    L = 10
    e = _engine(device, log2=L, cap=14, rows=1024)
    rng = np.random.default_rng(3)
    old = _preload(e, rng, 700)
    e.delta_clear()
    keys = _rand_keys(rng, 5000)
    _s_pull_mark(e, keys)
    want = _bits(keys, L)
    assert len(want) < (1 << L)  # (5000 keys leave a few of the 1024 bits clear)
    assert e.delta_stats()["bits_set"] == len(want)
    hit = sum(_bit(k, L) in want for k in old.tolist())
    assert e.delta_count() == len(keys) + hit
    _s_pull_mark(e, keys)
    assert e.delta_stats()["bits_set"] == len(want)
    assert e.delta_count() == len(keys) + hit


@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_filter_sanitizes_keys(device):
    """The all-ones key is marked and stored as all-ones - 1 (sanitize_key)."""
    L = 20
    e = _engine(device, log2=L)
    keys = np.array([M64, 0, 1, M64 - 2], dtype=np.uint64)
    _mark(e, keys)
    want = _bits([M64 - 1, 0, 1, M64 - 2], L)
    assert e.delta_stats()["bits_set"] == len(want) == 4
    np.testing.assert_array_equal(np.sort(e.delta_export()[0]),
                                  np.array([0, 1, M64 - 2, M64 - 1], dtype=np.uint64))
    # both spellings are one key
    _mark(e, np.array([M64 - 1], dtype=np.uint64))
    assert e.delta_stats()["bits_set"] == 4 and e.delta_count() == 4


def test_lookups_never_mark():
    e = _engine(CPU, log2=20)
    k, b = _batch(CPU, 1)
    e.train_step(b)
    e.delta_clear()
    e.eval_step(b)
    e.pull(np.unique(k))
    recv = torch.from_numpy(np.unique(k).view(np.int64))
    vals = torch.zeros(len(recv), e.value_width)
    e.s_pull(recv, len(recv), vals, insert=False, buf=1)
    assert e.delta_stats()["bits_set"] == 0 and e.delta_count() == 0


def test_config_validation():
    for bad in (9, 35, -1):
        with pytest.raises(ValueError):
            _engine(CPU, log2=bad)
    assert _engine(CPU, log2=0, table_grow=False, cap=10).delta_stats()["log2"] == 12
    assert _engine(CPU, log2=0, max_log2_cap=20).delta_stats()["log2"] == 22


# ---- 2. the exported set, exactly ---------------------------------------------------
@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("L", [10, 30])
def test_exported_set_is_the_marked_keys(device, L):
    e = _engine(device, log2=L, cap=13)
    rng = np.random.default_rng(5)
    old = _preload(e, rng, 3000)
    e.train_step(_batch(device, 39)[1])
    e.delta_clear()
    ak, aw = _export(e)
    touched = []
    for s in range(3):
        k, b = _batch(device, 40 + s)
        e.train_step(b)
        touched.append(k)
    touched = np.unique(np.concatenate(touched))
    marked = _bits(touched, L)
    assert e.delta_stats()["bits_set"] == len(marked)
    bk, bw = _export(e)
    want = np.array(sorted(k for k in bk.tolist() if _bit(k, L) in marked), dtype=np.uint64)
    dk, dw = _delta(e)
    np.testing.assert_array_equal(dk, want)
    np.testing.assert_array_equal(dw, bw[np.searchsorted(bk, dk)])
    false_pos = np.setdiff1d(dk, touched)
    if L == 10:
        assert len(false_pos) >= 1  # (3000 untouched keys over 1024 bits)
        assert np.isin(false_pos, ak).all() and np.isin(false_pos, old).any()
    else:
        assert len(false_pos) == 0
    # every new key and every key whose state changed is in the delta
    new = np.setdiff1d(bk, ak)
    at = np.searchsorted(ak, bk[np.isin(bk, ak)])
    changed = bk[np.isin(bk, ak)][(aw[at] != bw[np.isin(bk, ak)]).any(axis=1)]
    assert len(new) and len(changed)
    assert np.isin(new, dk).all() and np.isin(changed, dk).all()


# ---- 3. reconstruction, bit for bit -------------------------------------------------
MODELS = [("lr", "ftrl", "reference"), ("lr", "sgd", "reference"),
          ("fm", "ftrl", "reference"), ("fm", "sgd", "reference"),
          ("fm", "ftrl", "standard"), ("fm", "sgd", "standard"),
          ("mvm", "ftrl", "reference"), ("mvm", "sgd", "reference")]


def _a_then_b(e, device, slice_rows=0, rows=64, steps=(2, 3)):
    """Train, full export at A (filter cleared), train on: (A, delta at B)."""
    for s in range(steps[0]):
        e.train_step(_batch(device, 10 + s, rows=rows, slice_rows=slice_rows)[1])
    a = e.export_table()
    e.delta_clear()
    for s in range(steps[1]):
        e.train_step(_batch(device, 20 + s, rows=rows, slice_rows=slice_rows)[1])
    return a, e.delta_export()


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("kind,opt,fm_math", MODELS)
def test_reconstruction_one_slice(device, kind, opt, fm_math):
    e = _engine(device, kind, opt, fm_math)
    a, d = _a_then_b(e, device)
    assert 0 < len(d[0]) < e.table_size()
    _assert_same(_rebuild(e, [a, d]), _export(e))


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("kind,fm_math", [("lr", "reference"), ("fm", "standard")])
def test_reconstruction_eight_slices(device, kind, fm_math):
    e = _engine(device, kind, "ftrl", fm_math, slices=8)
    a, d = _a_then_b(e, device, slice_rows=8)
    if e.is_gpu:
        assert e.csr_steps == 5  # (the CSR path: Engine::train_step_csr)
    assert 0 < len(d[0]) < e.table_size()
    _assert_same(_rebuild(e, [a, d]), _export(e))


def _phase_step(e, b, device, S=1, csr=False):
    """One world-1 step through the phase API, the received keys presented as
    two sources."""
    nnz = b.keys.numel()
    counts = torch.zeros(1, dtype=torch.int64, device=device)
    send = torch.empty(nnz, dtype=torch.int64, device=device)
    e.w_prepare(b, 1, counts, send)
    n = int(counts.cpu()[0])
    offs = [0, n // 3, n]
    vals = torch.zeros(n, e.value_width, dtype=torch.float32, device=device)
    e.s_pull(send, n, vals, insert=True, buf=0, offsets=offs, keep_weights=True)
    if csr:
        cnt = torch.zeros(n, dtype=torch.int32, device=device)
        ent = torch.zeros(e.cfg.max_nnz * int(e.native.csr_entry_bytes), dtype=torch.uint8,
                          device=device)
        tot = torch.zeros(1, dtype=torch.int64, device=device)
        e._sync_stream()
        e.native.w_forward_backward_csr(b.view(), vals.data_ptr(), n, S, 0, cnt.data_ptr(),
                                        ent.data_ptr(), counts.data_ptr(), 1, tot.data_ptr())
        e.native.s_apply_csr(send.data_ptr(), cnt.data_ptr(), ent.data_ptr(), offs, S, 0)
    else:
        grads = torch.zeros(n, S * e.grad_width, dtype=torch.float32, device=device)
        masks = torch.zeros(n, dtype=torch.int32, device=device) if S > 1 else None
        e.w_forward_backward(b, vals, n, grads, masks, S)
        e.s_apply(send, grads, masks, offs, S, buf=0)
    e.w_finish()


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("kind", ["lr", "fm"])
def test_reconstruction_phase_api(device, kind):
    e = _engine(device, kind)
    for s in range(2):
        _phase_step(e, _batch(device, 10 + s)[1], device)
    a = e.export_table()
    e.delta_clear()
    touched = []
    for s in range(2):
        k, b = _batch(device, 20 + s)
        _phase_step(e, b, device)
        touched.append(k)
    d = e.delta_export()
    np.testing.assert_array_equal(np.sort(d[0]), np.unique(np.concatenate(touched)))
    assert len(d[0]) < e.table_size()
    _assert_same(_rebuild(e, [a, d]), _export(e))


@pytest.mark.gpu
def test_reconstruction_phase_api_csr(gpu_device):
    """s_apply_csr of received entries from two sources (GPU: the CSR exchange)."""
    S = 8
    e = _engine(gpu_device, "lr", slices=S)
    assert e.native.csr_exchange(S)
    for s in range(2):
        _phase_step(e, _batch(gpu_device, 10 + s, slice_rows=8)[1], gpu_device, S, csr=True)
    a = e.export_table()
    e.delta_clear()
    for s in range(2):
        _phase_step(e, _batch(gpu_device, 20 + s, slice_rows=8)[1], gpu_device, S, csr=True)
    d = e.delta_export()
    assert 0 < len(d[0]) < e.table_size()
    _assert_same(_rebuild(e, [a, d]), _export(e))


def test_apply_after_clear_marks_again():
    """A server buffer pulled before delta_clear and applied after it: the
    apply marks the buffer's keys itself."""
    e = _engine(CPU)
    k, b = _batch(CPU, 1)
    e.train_step(b)
    keys = np.unique(k)[:20]
    recv = torch.from_numpy(keys.view(np.int64))
    vals = torch.zeros(20, e.value_width)
    e.s_pull(recv, 20, vals, insert=True, buf=0, offsets=[0, 20])
    a = e.export_table()
    e.delta_clear()
    e.s_apply(recv, torch.ones(20), None, [0, 20], 1, buf=0)
    e.end_step()
    d = e.delta_export()
    np.testing.assert_array_equal(np.sort(d[0]), keys)
    _assert_same(_rebuild(e, [a, d]), _export(e))


@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_reconstruction_with_admission(device):
    """admit_min_count = 2: a key seen once is marked, absent and not exported."""
    L = 30
    e = _engine(device, log2=L, admit_min_count=2, admit_log2=16)
    seen = []
    for s in range(2):
        k, b = _batch(device, 10 + s)
        e.train_step(b)
        seen.append(k)
    a = e.export_table()
    e.delta_clear()
    touched = []
    for s in range(3):
        k, b = _batch(device, 20 + s)
        e.train_step(b)
        touched.append(k)
    touched = np.unique(np.concatenate(touched))
    dk, dw = e.delta_export()
    bk, _ = _export(e)
    absent = np.setdiff1d(touched, bk)
    assert len(absent) > 0  # (keys sighted once only)
    assert e.delta_stats()["bits_set"] == len(_bits(touched, L))
    np.testing.assert_array_equal(np.sort(dk), np.intersect1d(touched, bk))
    _assert_same(_rebuild(e, [a, (dk, dw)]), _export(e))


@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_reconstruction_across_splits(device):
    """The table splits to a segment count that is no power of two between A
    and B: the filter is indexed by key hash, so re-packed slots do not matter."""
    e = _engine(device, cap=10, rows=16, fields=8)
    rng = np.random.default_rng(9)
    _preload(e, rng, 500)
    a = e.export_table()
    e.delta_clear()
    assert e.table_geometry["segments"] == 1
    odd = False
    for s in range(40):
        keys = _rand_keys(np.random.default_rng(100 + s), 128)
        rp = (np.arange(17) * 8).astype(np.int32)
        b = to_batch(keys, rp, np.tile(np.arange(8, dtype=np.int32), 16),
                     (np.arange(16) % 3 == 0).astype(np.float32), device)
        e.train_step(b)
        n = e.table_geometry["segments"]
        if n & (n - 1):
            odd = True
            break
    assert odd and e.table_splits >= 2 and not e.overflowed()
    d = e.delta_export()
    assert len(d[0]) == e.table_size() - 500
    _assert_same(_rebuild(e, [a, d]), _export(e))


@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_reconstruction_push_host(device):
    e = _engine(device, "fm")
    e.train_step(_batch(device, 1)[1])
    a = e.export_table()
    e.delta_clear()
    keys = np.concatenate([a[0][:5], np.array([7, 8, 9], dtype=np.uint64)])
    e.push(keys, np.full((len(keys), e.params_per_key), 0.25, dtype=np.float32))
    d = e.delta_export()
    np.testing.assert_array_equal(np.sort(d[0]), np.sort(keys))
    _assert_same(_rebuild(e, [a, d]), _export(e))


@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_two_deltas_in_order(device):
    e = _engine(device, "fm", fm_math="standard")
    e.train_step(_batch(device, 1)[1])
    a = e.export_table()
    e.delta_clear()
    e.train_step(_batch(device, 2)[1])
    e.train_step(_batch(device, 3)[1])
    d1 = e.delta_export()
    mid = _export(e)
    e.delta_clear()
    e.train_step(_batch(device, 3)[1])
    e.train_step(_batch(device, 4)[1])
    d2 = e.delta_export()
    _assert_same(_rebuild(e, [a, d1]), mid)
    _assert_same(_rebuild(e, [a, d1, d2]), _export(e))
    # (the order matters: a key of both deltas takes the newer state)
    both = np.intersect1d(d1[0], d2[0])
    assert len(both) > 0


# ---- 4. what a delta cannot carry ---------------------------------------------------
@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_needs_full(device):
    e = _engine(device)
    e.push(np.arange(1, 40, dtype=np.uint64), np.ones((39, 1), dtype=np.float32))
    assert not e.delta_stats()["needs_full"] and not e.delta_needs_full
    # a prune that drops nothing (every weight is away from zero: |z| = 1 > lambda1)
    assert e.prune() == 0
    assert not e.delta_stats()["needs_full"]
    # a prune that drops a key: zero state
    e.push(np.array([77], dtype=np.uint64), np.zeros((1, 1), dtype=np.float32))
    assert e.prune() >= 1
    assert e.delta_stats()["needs_full"] and e.delta_needs_full
    e.delta_clear()
    assert e.delta_stats() == {"log2": 30, "bits_set": 0, "needs_full": False}
    k, w = e.export_table()
    e.import_table(k[:3], w.reshape(len(k), -1)[:3].reshape(-1))
    assert e.delta_stats()["needs_full"]
    e.delta_clear()
    e.prefill(10)
    assert e.delta_stats()["needs_full"]
    e.delta_clear()
    assert not e.delta_stats()["needs_full"]


@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_tracking_off(device):
    """No filter, no side effect: the trained table is bit-equal."""
    on, off = _engine(device, "fm"), _engine(device, "fm", track=False)
    for s in range(3):
        for e in (on, off):
            e.train_step(_batch(device, 30 + s)[1])
    assert off.delta_stats() == {"log2": 0, "bits_set": 0, "needs_full": False}
    assert off.delta_log2 == 0
    for call in (off.delta_export, off.delta_count):
        with pytest.raises(RuntimeError, match="tracking is off"):
            call()
    off.delta_clear()  # (a no-op)
    _assert_same(_export(on), _export(off))


# ---- 5. the checkpoint layer --------------------------------------------------------
NB = lambda: None  # noqa: E731  (single process: no barrier)


def _ver(root, i):
    return checkpoint.version_dir(str(root), i)


def _name(root, i):
    return os.path.basename(_ver(root, i))


def _loaded(live, d, rank=0, world=1):
    f = Engine(live.model, live.optim, EngineConfig(table_log2_cap=14, max_rows=256, max_nnz=4096,
                                                    delta_track=True, delta_log2=20))
    checkpoint.load(f, d, rank, world)
    assert f.delta_stats() == {"log2": 20, "bits_set": 0, "needs_full": False}
    return f


def test_chain_full_delta_delta_full_delta(tmp_path):
    e = _engine(CPU, "fm", log2=20)
    snaps, kinds = {}, {}
    for i in range(1, 6):
        e.train_step(_batch(CPU, i)[1])
        base = None if i in (1, 4) else _name(tmp_path, i - 1)
        p = checkpoint.save(e, _ver(tmp_path, i), 0, 1, meta={"epoch": i}, barrier=NB,
                            delta_base=base)
        kinds[i] = os.path.basename(p).split("-")[0]
        snaps[i] = _export(e)
        assert e.delta_stats()["bits_set"] == 0  # (cleared once the file is durable)
    assert kinds == {1: "shard", 2: "delta", 3: "delta", 4: "shard", 5: "delta"}
    assert checkpoint.shard_keys(os.path.join(_ver(tmp_path, 2), checkpoint.delta_name(0, 1))) \
        < len(snaps[2][0])
    for i in range(1, 6):
        meta = checkpoint.load_meta(_ver(tmp_path, i))
        assert meta.get("delta_base") == (None if i in (1, 4) else _name(tmp_path, i - 1))
        assert meta["epoch"] == i
        _assert_same(_export(_loaded(e, _ver(tmp_path, i))), snaps[i])
    assert [os.path.basename(d) for d in checkpoint.chain(_ver(tmp_path, 3))] == \
        [_name(tmp_path, i) for i in (1, 2, 3)]
    hdr, _, _ = checkpoint.read_shard(os.path.join(_ver(tmp_path, 2), checkpoint.delta_name(0, 1)))
    assert hdr[7] == 1
    hdr, _, _ = checkpoint.read_shard(os.path.join(_ver(tmp_path, 1), checkpoint.shard_name(0, 1)))
    assert hdr[7] == 0
    # a resumed engine goes on with a delta on the version it loaded
    f = _loaded(e, _ver(tmp_path, 5))
    for x in (e, f):
        x.train_step(_batch(CPU, 6)[1])
    p = checkpoint.save(f, _ver(tmp_path, 6), 0, 1, barrier=NB, delta_base=_name(tmp_path, 5))
    assert os.path.basename(p) == checkpoint.delta_name(0, 1)
    _assert_same(_export(_loaded(e, _ver(tmp_path, 6))), _export(e))


def test_publish_keeps_chain_links(tmp_path):
    e = _engine(CPU, log2=20)
    # 1 full, 2 delta, 3 delta, 4 full, 5 delta, 6 delta
    for i in range(1, 7):
        e.train_step(_batch(CPU, i)[1])
        base = None if i in (1, 4) else _name(tmp_path, i - 1)
        checkpoint.save(e, _ver(tmp_path, i), 0, 1, barrier=NB, delta_base=base)
        if i == 3:
            checkpoint.publish(str(tmp_path), 3, keep=2)
            # tips 2 and 3 need 1
            assert sorted(os.listdir(tmp_path)) == ["LATEST"] + [_name(tmp_path, j) for j in (1, 2, 3)]
        if i == 5:
            checkpoint.publish(str(tmp_path), 5, keep=2)
            # tips 4 and 5 need nothing older
            assert sorted(os.listdir(tmp_path)) == ["LATEST"] + [_name(tmp_path, j) for j in (4, 5)]
    checkpoint.publish(str(tmp_path), 6, keep=2)
    assert sorted(os.listdir(tmp_path)) == ["LATEST"] + [_name(tmp_path, j) for j in (4, 5, 6)]
    assert checkpoint.latest(str(tmp_path)) == _ver(tmp_path, 6)
    _assert_same(_export(_loaded(e, _ver(tmp_path, 6))), _export(e))


def test_publish_full_only_root_unchanged(tmp_path):
    e = _engine(CPU, track=False)
    e.train_step(_batch(CPU, 1)[1])
    for i in range(1, 5):
        checkpoint.save(e, _ver(tmp_path, i), 0, 1, barrier=NB)
        checkpoint.publish(str(tmp_path), i, keep=2)
        assert sorted(os.listdir(tmp_path)) == \
            ["LATEST"] + [_name(tmp_path, j) for j in range(max(1, i - 1), i + 1)]


def _two_ranks(seed_steps):
    """Two engines holding the two owners' shards of the same training."""
    es = [_engine(CPU, "fm", log2=20) for _ in range(2)]
    return es


def _train_owned(es, seed):
    k, rp, fg, lab = random_csr(64, fields=8, vocab=300, seed=seed)
    for r, e in enumerate(es):
        # each rank pushes the keys it owns (world 2)
        uk = np.unique(k)
        mine = uk[owner_of(uk, 2) == r]
        e.push(mine, np.full((len(mine), e.params_per_key), 0.125 * (seed % 5 + 1),
                             dtype=np.float32))


def test_resharded_chain(tmp_path):
    es = _two_ranks(0)
    root, flat = tmp_path / "chain", tmp_path / "full"
    for i in range(1, 4):
        _train_owned(es, i)
        base = None if i == 1 else _name(root, i - 1)
        for r in (1, 0):  # (rank 0 writes meta.json: last)
            p = checkpoint.save(es[r], _ver(root, i), r, 2, barrier=NB, delta_base=base)
            assert os.path.basename(p).startswith("shard-" if i == 1 else "delta-")
    # a full save of the same state (tracking needs no clear filter for it)
    twins = [Engine(es[0].model, es[0].optim, EngineConfig(table_log2_cap=14, max_rows=256,
                                                           max_nnz=4096)) for _ in range(2)]
    for r in (1, 0):
        k, w = es[r].export_table()
        twins[r].import_table(k, w)
        checkpoint.save(twins[r], str(flat), r, 2, barrier=NB)
    for world in (1, 3):
        for rank in range(world):
            a = _export(_loaded(es[0], _ver(root, 3), rank, world))
            b = _export(_loaded(es[0], str(flat), rank, world))
            assert len(a[0]) > 0
            _assert_same(a, b)
    # same world: each rank its own files
    for r in range(2):
        _assert_same(_export(_loaded(es[0], _ver(root, 3), r, 2)), _export(es[r]))


def test_missing_link_raises(tmp_path):
    import shutil

    e = _engine(CPU, log2=20)
    for i in range(1, 4):
        e.train_step(_batch(CPU, i)[1])
        checkpoint.save(e, _ver(tmp_path, i), 0, 1, barrier=NB,
                        delta_base=None if i == 1 else _name(tmp_path, i - 1))
    shutil.rmtree(_ver(tmp_path, 2))
    with pytest.raises(FileNotFoundError, match=_name(tmp_path, 2)):
        checkpoint.load(_engine(CPU, log2=20), _ver(tmp_path, 3), 0, 1)
    os.remove(os.path.join(_ver(tmp_path, 3), checkpoint.delta_name(0, 1)))
    with pytest.raises(FileNotFoundError):
        checkpoint.chain_files(_ver(tmp_path, 3))


def test_save_falls_back_to_full(tmp_path):
    def kind(p):
        return os.path.basename(p).split("-")[0]

    e = _engine(CPU, log2=20)
    e.train_step(_batch(CPU, 1)[1])
    assert kind(checkpoint.save(e, _ver(tmp_path, 1), 0, 1, barrier=NB)) == "shard"
    e.train_step(_batch(CPU, 2)[1])
    assert kind(checkpoint.save(e, _ver(tmp_path, 2), 0, 1, barrier=NB,
                                delta_base=_name(tmp_path, 1))) == "delta"
    # after a prune that dropped a key
    e.push(np.array([5], dtype=np.uint64), np.zeros((1, 1), dtype=np.float32))
    assert e.prune() >= 1
    p = checkpoint.save(e, _ver(tmp_path, 3), 0, 1, barrier=NB, delta_base=_name(tmp_path, 2))
    assert kind(p) == "shard" and "delta_base" not in checkpoint.load_meta(_ver(tmp_path, 3))
    _assert_same(_export(_loaded(e, _ver(tmp_path, 3))), _export(e))
    # a missing base
    e.train_step(_batch(CPU, 3)[1])
    assert kind(checkpoint.save(e, _ver(tmp_path, 4), 0, 1, barrier=NB,
                                delta_base=_name(tmp_path, 9))) == "shard"
    # a changed world size (the base was written by one rank)
    e.train_step(_batch(CPU, 4)[1])
    assert kind(checkpoint.save(e, _ver(tmp_path, 5), 0, 2, barrier=NB,
                                delta_base=_name(tmp_path, 4))) == "shard"
    # tracking off
    off = _engine(CPU, track=False)
    off.train_step(_batch(CPU, 1)[1])
    checkpoint.save(off, _ver(tmp_path, 6), 0, 1, barrier=NB)
    assert kind(checkpoint.save(off, _ver(tmp_path, 7), 0, 1, barrier=NB,
                                delta_base=_name(tmp_path, 6))) == "shard"


# ---- 6. trainer and serving ---------------------------------------------------------
def _trainer(tmp_path, device, epochs, root, metrics="", delta=True):
    from xflow_amd.trainer import Trainer

    cfg = TrainConfig(train_prefix=TRAIN, test_prefix=TEST, epochs=epochs, threads=8,
                      pred_dir=str(tmp_path), write_pred=False, init_push=False,
                      resume_dir=str(root), save_every=1, save_delta=delta, delta_full_every=3,
                      metrics_file=metrics,
                      model=ModelConfig(kind="lr"), optim=OptimConfig(),
                      engine=EngineConfig(table_log2_cap=14, delta_log2=20))
    return Trainer(cfg, device=device)


def _run(tmp_path, device, epochs, root, metrics="", resume=False, delta=True):
    t = _trainer(tmp_path, device, epochs, root, metrics, delta)
    try:
        if resume:
            assert t.resume(str(root)) is not None
            t.train_epochs(epochs - t.epoch)
        else:
            t.train_epochs(epochs)
        return _export(t.table)
    finally:
        t.close()


def test_trainer_writes_the_pattern(tmp_path):
    root, mf = tmp_path / "ck", str(tmp_path / "m.jsonl")
    final = _run(tmp_path, CPU, 5, root, metrics=mf)
    recs = [json.loads(x) for x in open(mf)]
    eps = [r for r in recs if r.get("event") == "epoch"]
    assert [r["ckpt_kind"] for r in eps] == ["full", "delta", "delta", "full", "delta"]
    # publish(keep=2) kept tips 4, 5: a full version and its delta
    assert sorted(os.listdir(root)) == ["LATEST", _name(root, 4), _name(root, 5)]
    assert os.path.exists(os.path.join(_ver(root, 4), checkpoint.shard_name(0, 1)))
    assert os.path.exists(os.path.join(_ver(root, 5), checkpoint.delta_name(0, 1)))
    assert eps[3]["ckpt_keys"] == len(final[0]) == eps[4]["table_keys"]
    assert 0 < eps[4]["ckpt_keys"] <= eps[3]["ckpt_keys"]
    assert eps[4]["ckpt_keys"] == checkpoint.shard_keys(
        os.path.join(_ver(root, 5), checkpoint.delta_name(0, 1)))


@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_resume_from_chain_equals_uninterrupted(tmp_path, device):
    whole = _run(tmp_path, device, 4, tmp_path / "a")
    _run(tmp_path, device, 2, tmp_path / "b")
    assert "delta_base" in checkpoint.load_meta(checkpoint.latest(str(tmp_path / "b")))
    resumed = _run(tmp_path, device, 4, tmp_path / "b", resume=True)
    _assert_same(resumed, whole)
    # the resumed run went on with the chain: full, delta | delta, full
    metas = [checkpoint.load_meta(_ver(tmp_path / "b", i)) for i in (3, 4)]
    assert "delta_base" in metas[0] and "delta_base" not in metas[1]


def test_predictor_on_a_delta_tip(tmp_path):
    from xflow_amd.serve import Predictor

    _run(tmp_path, CPU, 2, tmp_path / "d")
    _run(tmp_path, CPU, 2, tmp_path / "f", delta=False)
    tip = checkpoint.latest(str(tmp_path / "d"))
    assert "delta_base" in checkpoint.load_meta(tip)
    assert "delta_base" not in checkpoint.load_meta(checkpoint.latest(str(tmp_path / "f")))
    text = open(TEST + "-00000", "rb").read()
    pd = Predictor(str(tmp_path / "d"), device=CPU, max_rows=256)
    pf = Predictor(str(tmp_path / "f"), device=CPU, max_rows=256)
    assert pd.keys == pf.keys > 0
    a, b = pd.predict_libffm(text), pf.predict_libffm(text)
    assert len(a) > 0
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_cli_flags():
    from xflow_amd.cli import build_parser, config_from_args

    args = [TRAIN, TEST, "0", "3", "--cpu"]
    cfg = config_from_args(build_parser().parse_args(
        args + ["--save-delta", "--delta-full-every", "4", "--delta-log2", "20"]))
    assert cfg.save_delta and cfg.delta_full_every == 4
    assert cfg.engine.delta_track and cfg.engine.delta_log2 == 20
    off = config_from_args(build_parser().parse_args(args))
    assert not off.save_delta and not off.engine.delta_track and off.delta_full_every == 8
