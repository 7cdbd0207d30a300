"""The three checkpoint files, byte for byte (csrc/engine/engine_io.cpp).

Each file is parsed with numpy straight from its documented layout and held
to the arrays the matching export returns -- same keys, same words, same
order -- so the file writer and the host export cannot drift apart:

  save / save_delta   8-byte magic "XFLOWTB1", int32[8] (hdr[7]: 1 for a
                      delta), u64 n, u64 keys[n], u32 words[n][state_words]
  save_serving        8-byte magic "XFLOWSW1", int32[6] {model kind, v_dim,
                      fm_math, mvm_math, P, optimiser kind}, u64 keys of the
                      table, u64 n, u64 keys[n], f32 weights[n][P]

What the existing suites already hold (round trips, the filter's key set, the
snapshot's weights) is not repeated here.
"""
import numpy as np
import pytest
import torch

from helpers import to_batch
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Engine

CPU = torch.device("cpu")
ROWS, FIELDS, STEPS = 128, 8, 3
MODELS = [("lr", "reference"), ("fm", "reference")]


def _engine(device, kind="lr", fm_math="reference"):
    return Engine(ModelConfig(kind=kind, v_dim=4, fm_math=fm_math), OptimConfig(kind="ftrl"),
                  EngineConfig(table_log2_cap=10, max_log2_cap=14, max_rows=ROWS,
                               max_nnz=ROWS * FIELDS, delta_track=True), device=device)


def _step(e, seed):
    """ROWS x FIELDS keys that occur once, in this step only.  Every forward
    then reads zero weights (p = 0.5 exactly), every key's gradient is the one
    addend (0.5 - y) / 128, and the FTRL update is IEEE basic operations
    (tests/test_apply_exact.py): the table is the same bits on both backends,
    with no float sum whose order, or expf whose last bit, could differ."""
    n = ROWS * FIELDS
    keys = (np.arange(1, n + 1, dtype=np.uint64) + np.uint64(seed * n)) * np.uint64(0x9E3779B97F4A7C15)
    labels = (np.random.default_rng(seed).random(ROWS) < 0.3).astype(np.float32)
    e.train_step(to_batch(keys, np.arange(0, n + 1, FIELDS, dtype=np.int32),
                          np.tile(np.arange(FIELDS, dtype=np.int32), ROWS), labels, e.device))


def _trained(device, kind="lr", fm_math="reference"):
    """Two steps, the filter cleared, the third: the delta is a proper subset."""
    e = _engine(device, kind, fm_math)
    for s in range(STEPS):
        if s == STEPS - 1:
            e.delta_clear()
        _step(e, s)
    return e


def _read_shard(path, W):
    raw = open(path, "rb").read()
    hdr = np.frombuffer(raw, dtype=np.int32, count=8, offset=8)
    n = int(np.frombuffer(raw, dtype=np.uint64, count=1, offset=40)[0])
    assert len(raw) == 48 + n * (8 + 4 * W)
    keys = np.frombuffer(raw, dtype=np.uint64, count=n, offset=48)
    words = np.frombuffer(raw, dtype=np.uint32, count=n * W, offset=48 + 8 * n)
    return raw[:8], hdr, keys, words


def _read_serving(path, P):
    raw = open(path, "rb").read()
    hdr = np.frombuffer(raw, dtype=np.int32, count=6, offset=8)
    total, n = (int(x) for x in np.frombuffer(raw, dtype=np.uint64, count=2, offset=32))
    assert len(raw) == 48 + n * (8 + 4 * P)
    keys = np.frombuffer(raw, dtype=np.uint64, count=n, offset=48)
    weights = np.frombuffer(raw, dtype=np.uint32, count=n * P, offset=48 + 8 * n)
    return raw[:8], hdr, total, keys, weights


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


@pytest.mark.parametrize("kind,fm_math", MODELS)
def test_save_file_is_the_export(tmp_path, kind, fm_math):
    e = _trained(CPU, kind, fm_math)
    L, W = e.layout, e.state_words
    for name, write, export, delta in (("full", e.save, e.export_table, 0),
                                       ("delta", e.save_delta, e.delta_export, 1)):
        path = str(tmp_path / name)
        write(path)
        magic, hdr, keys, words = _read_shard(path, W)
        k, w = export()
        assert magic == b"XFLOWTB1"
        # (p_w = 1: LR and FM keep one linear weight per key)
        assert hdr.tolist() == [1, L["kind"], 4, L["P"], 1, L["opt"], L["stride"], delta]
        assert len(k) > 0 and keys.tobytes() == np.asarray(k, dtype=np.uint64).tobytes()
        assert words.tobytes() == np.asarray(w, dtype=np.uint32).tobytes()
    assert 0 < e.delta_count() < e.table_size()


@pytest.mark.parametrize("kind,fm_math", MODELS)
def test_serving_file_is_the_export(tmp_path, kind, fm_math):
    e = _trained(CPU, kind, fm_math)
    P = e.params_per_key
    path = str(tmp_path / "weights.xfw")
    assert e.save_serving(path) > 0
    magic, hdr, total, keys, weights = _read_serving(path, P)
    k, w = e.export_weights()
    m = e.model.native()
    assert magic == b"XFLOWSW1"
    assert hdr.tolist() == [m["kind"], 4, m["fm_math"], m["mvm_math"], P, e.layout["opt"]]
    assert total == e.table_size()
    assert keys.tobytes() == np.asarray(k, dtype=np.uint64).tobytes()
    assert weights.tobytes() == _bits(w).tobytes()


def _sorted_export(e):
    k, w = e.export_table()
    o = np.argsort(k)
    return np.asarray(k)[o].tobytes() + np.asarray(w).reshape(len(k), e.state_words)[o].tobytes()


def test_failed_save_and_load_leave_the_engine_whole(tmp_path):
    e = _trained(CPU)
    with pytest.raises(RuntimeError, match="cannot open"):
        e.save(str(tmp_path / "no_such_dir" / "shard"))
    with pytest.raises(RuntimeError, match="cannot open"):
        e.load(str(tmp_path / "no_such_file"))
    good = str(tmp_path / "good")
    e.save(good)
    raw = open(good, "rb").read()
    n = e.table_size()
    assert n > 8
    cut, magic = str(tmp_path / "cut"), str(tmp_path / "magic")
    open(cut, "wb").write(raw[:48 + 8 * (n // 2) + 3])  # (inside the key array)
    open(magic, "wb").write(b"XFLOWTB2" + raw[8:])
    before = _sorted_export(e)
    for seed, (path, what) in enumerate(((cut, "truncated checkpoint"), (magic, "bad checkpoint"))):
        with pytest.raises(RuntimeError, match=what):
            e.load(path)
        assert _sorted_export(e) == before
        _step(e, 10 + seed)
        assert not e.overflowed()
        before = _sorted_export(e)


@pytest.mark.gpu
def test_gpu_files_equal_the_cpu_engines(tmp_path, gpu_device):
    """After the same three steps the three files hold the same (key, value)
    pairs on both backends; slot order differs, so both sides are sorted by
    key.  A narrower table state than ordinary batches give: with repeated
    keys the backends sum a key's gradients in different orders and agree to
    rtol 1e-4 only (tests/test_determinism.py), so _step's keys occur once and
    no (n, z) accumulates over steps.  What is compared is the files."""
    def by_key(magic, hdr, *rest):
        *counts, keys, vals = rest
        o = np.argsort(keys)
        return (magic, hdr.tolist(), counts, keys[o].tobytes(),
                vals.reshape(len(keys), -1)[o].tobytes())

    files = {}
    for dev in (gpu_device, CPU):
        e = _trained(dev)
        full, delta, serving = (str(tmp_path / (dev.type + n)) for n in ("full", "delta", "serving"))
        e.save(full)
        e.save_delta(delta)
        e.save_serving(serving)
        files[dev.type] = [by_key(*_read_shard(full, e.state_words)),
                           by_key(*_read_shard(delta, e.state_words)),
                           by_key(*_read_serving(serving, e.params_per_key))]
    for g, c in zip(files["cuda"], files["cpu"]):
        assert len(g[3]) > 0 and g == c
