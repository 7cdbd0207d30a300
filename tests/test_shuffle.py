"""Per-epoch row shuffling on the device (Engine.shuffle_batch,
shuffle_permutation, TrainConfig.shuffle; docs/DESIGN.md §9).

The reference in every test is the Python-int / numpy code in this file: the
permutation as the design writes it down (`ref_perm`), and a numpy gather by
it.  Integers are compared exactly and labels by bit pattern, on the CPU
backend and (marked gpu) on the HIP backend.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import DATA
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig, TrainConfig
from xflow_amd.engine import Batch, Engine, shuffle_permutation

DEVS = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
ROWS = [0, 1, 2, 63, 64, 65, 257, 1025]  # wave, workgroup, tile and scan-block edges
MAX_ROWS = 20001  # (> 16384 rows: the CSR scan's three-launch form)


# ---- the definition, in Python ints ----------------------------------------
def fmix(h):
    h &= M64
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & M64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & M64
    h ^= h >> 33
    return h


def ref_perm(n, seed):
    """pi(i) for i in [0, n): 4 Feistel rounds on 2h bits, cycle-walked."""
    if n <= 1:
        return np.arange(n, dtype=np.int64)
    b = (n - 1).bit_length()
    h = max(1, (b + 1) // 2)
    mask = (1 << h) - 1
    ks = [fmix((seed + GOLDEN * (r + 1)) & M64) for r in range(4)]
    out = np.empty(n, dtype=np.int64)
    for i in range(n):
        x = i
        while True:
            L, R = x >> h, x & mask
            for k in ks:
                L, R = R, (L ^ fmix(R ^ k)) & mask
            x = (L << h) | R
            if x < n:
                break
        out[i] = x
    return out


_perms = {}


def perm(n, seed):
    """ref_perm, computed once per (n, seed) and shared (read-only)."""
    if (n, seed) not in _perms:
        p = ref_perm(n, seed)
        p.setflags(write=False)
        _perms[(n, seed)] = p
    return _perms[(n, seed)]


@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 64, 65, 257, 4097])
def test_permutation_is_the_definition(n):
    for seed in (0, 1, 2 ** 63 + 5, 2 ** 64 - 1):
        got = shuffle_permutation(n, seed)
        assert got.dtype == np.int64 and got.shape == (n,)
        assert np.array_equal(got, perm(n, seed)), (n, seed)
        assert np.array_equal(np.sort(got), np.arange(n)), (n, seed)


@pytest.mark.parametrize("seed", range(8))
def test_permutation_mixes(seed):
    """n = 4096: the mean displacement is a uniform permutation's 1/3 within
    [0.30, 0.37] (about 9 sigma: sigma = sqrt(1/18/4096) = 0.0037), and at
    most 16 of the 4095 neighbouring pairs stay neighbours (uniform: ~2)."""
    n = 4096
    p = perm(n, seed)
    assert np.array_equal(shuffle_permutation(n, seed), p)
    disp = np.abs(p - np.arange(n)).mean() / n
    kept = int(np.sum(np.abs(np.diff(p)) == 1))
    print("seed", seed, "mean displacement", disp, "neighbours kept", kept)
    assert 0.30 <= disp <= 0.37
    assert kept <= 16


# ---- Engine.shuffle_batch ---------------------------------------------------
@pytest.fixture(autouse=True)
def _gpu_cases_need_the_gpu(request):
    """Every case marked gpu goes through the suite's gpu_device fixture."""
    if request.node.get_closest_marker("gpu"):
        request.getfixturevalue("gpu_device")


def _dev(name):
    return torch.device("cuda", 0) if name == "cuda" else torch.device("cpu")


_engines = {}


def _engine(devname):
    if devname not in _engines:
        _engines[devname] = Engine(ModelConfig(), OptimConfig(),
                                   EngineConfig(table_log2_cap=8, max_rows=MAX_ROWS,
                                                max_nnz=1 << 18), device=_dev(devname))
    return _engines[devname]


def _labels(rng, rows):
    y = rng.standard_normal(rows).astype(np.float32)
    y[::7] = -0.0  # (compared by bit pattern)
    return y


def _csr(rows, with_fgid, seed):
    """Rows of 0..5 entries, a third of them empty, one of 300 entries."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 6, rows)
    lens[rng.random(rows) < 0.33] = 0
    if rows:
        lens[rows // 2] = 300
    rp = np.zeros(rows + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    nnz = int(rp[-1])
    return dict(keys=rng.integers(-2 ** 63, 2 ** 63 - 1, nnz, dtype=np.int64),
                labels=_labels(rng, rows), row_ptr=rp, F=0,
                fgid=rng.integers(0, 40, nnz).astype(np.int32) if with_fgid else None)


def _fixed(rows, F, with_fgid, seed, compact=False):
    rng = np.random.default_rng(seed)
    if compact:  # u32 keys in int32, most with the top bit set
        keys = rng.integers(-2 ** 31, 2 ** 29, rows * F, dtype=np.int64).astype(np.int32)
    else:
        keys = rng.integers(-2 ** 63, 2 ** 63 - 1, rows * F, dtype=np.int64)
    return dict(keys=keys, labels=_labels(rng, rows), row_ptr=None, F=F,
                fgid=rng.integers(0, 40, rows * F).astype(np.int32) if with_fgid else None)


def _batch(d, dev):
    def t(a):
        return None if a is None else torch.from_numpy(a.copy()).to(dev)
    return Batch(keys=t(d["keys"]), labels=t(d["labels"]), row_ptr=t(d["row_ptr"]),
                 fgid=t(d["fgid"]), nnz_per_row=d["F"], slice_rows=3)


def _rows_of(keys, labels, row_ptr, fgid, F):
    """[(label bits, keys of the row, fgid of the row)] of row-major / CSR arrays."""
    rows = len(labels)
    rp = row_ptr if row_ptr is not None else np.arange(rows + 1) * F
    bits = labels.view(np.uint32)
    return [(int(bits[r]), tuple(keys[rp[r]:rp[r + 1]].tolist()),
             tuple(fgid[rp[r]:rp[r + 1]].tolist()) if fgid is not None else ())
            for r in range(rows)]


def _check(devname, d, seed, field_major=None):
    """shuffle_batch(d) == the numpy gather by ref_perm, exactly; the same
    multiset of rows; the source untouched; slice_rows carried over."""
    eng, dev = _engine(devname), _dev(devname)
    src = _batch(d, dev)
    out = eng.shuffle_batch(src, seed, field_major=field_major)
    rows, F = len(d["labels"]), d["F"]
    pi = perm(rows, seed & M64)
    fixed = d["row_ptr"] is None
    fm = fixed if field_major is None else field_major
    assert out.field_major == fm and out.slice_rows == 3 and out.nnz_per_row == F
    assert out.keys.dtype == torch.int64 and out.rows == rows and out.nnz == len(d["keys"])
    out.check(dev)
    wide = d["keys"].astype(np.int64) & 0xFFFFFFFF if d["keys"].dtype == np.int32 else d["keys"]
    got_k, got_y = out.keys.cpu().numpy(), out.labels.cpu().numpy()
    got_g = out.fgid.cpu().numpy() if out.fgid is not None else None
    assert (got_g is None) == (d["fgid"] is None)
    assert np.array_equal(got_y.view(np.uint32), d["labels"][pi].view(np.uint32))
    if fixed:
        assert out.row_ptr is None
        if fm:  # back to row-major for the comparison
            got_k = np.ascontiguousarray(got_k.reshape(F, rows).T).reshape(-1)
            if got_g is not None:
                got_g = np.ascontiguousarray(got_g.reshape(F, rows).T).reshape(-1)
        assert np.array_equal(got_k, wide.reshape(rows, F)[pi].reshape(-1))
        if got_g is not None:
            assert np.array_equal(got_g, d["fgid"].reshape(rows, F)[pi].reshape(-1))
        got_rp = None
    else:
        rp = d["row_ptr"]
        got_rp = out.row_ptr.cpu().numpy()
        want_rp = np.zeros(rows + 1, np.int32)
        want_rp[1:] = np.cumsum(np.diff(rp)[pi])
        assert got_rp.dtype == np.int32 and np.array_equal(got_rp, want_rp)
        idx = (np.concatenate([np.arange(rp[p], rp[p + 1]) for p in pi]) if rows
               else np.zeros(0, np.int64)).astype(np.int64)
        assert np.array_equal(got_k, wide[idx])
        if got_g is not None:
            assert np.array_equal(got_g, d["fgid"][idx])
    # the same rows, the same model inputs
    assert sorted(_rows_of(got_k, got_y, got_rp, got_g, F)) == \
        sorted(_rows_of(wide, d["labels"], d["row_ptr"], d["fgid"], F))
    # the source is left as it was
    for name in ("keys", "labels", "row_ptr", "fgid"):
        if d[name] is not None:
            a, b = getattr(src, name).cpu().numpy(), d[name]
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    return out


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("with_fgid", [False, True])
def test_shuffle_csr(devname, with_fgid):
    for rows in ROWS:
        _check(devname, _csr(rows, with_fgid, seed=rows), seed=11 + rows)


@pytest.mark.parametrize("devname", DEVS)
def test_shuffle_csr_many_rows(devname):
    """More rows than one scan launch covers (the offsets' multi-tile scan),
    short rows; and a seed above 2^63."""
    _check(devname, _csr(MAX_ROWS, True, seed=3), seed=2 ** 64 - 3)


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("field_major", [True, False])
@pytest.mark.parametrize("F", [1, 2, 18, 39, 64])
def test_shuffle_fixed_width(devname, F, field_major):
    for rows in ROWS:
        _check(devname, _fixed(rows, F, with_fgid=rows % 2 == 1, seed=F * 10000 + rows),
               seed=5 + rows, field_major=field_major)
    # the default layout of a fixed-width batch is the step's: field-major
    assert _check(devname, _fixed(65, F, False, seed=1), seed=2).field_major


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("field_major", [True, False])
def test_shuffle_compact_keys(devname, field_major):
    """Compact u32 keys (int32 tensors, the top bit set) come out as u64 below 2^32."""
    for rows, F in ((257, 39), (64, 1), (1025, 18)):
        out = _check(devname, _fixed(rows, F, True, seed=rows, compact=True), seed=77,
                     field_major=field_major)
        k = out.keys.cpu().numpy()
        assert k.min() >= 0 and k.max() < 2 ** 32 and k.max() >= 2 ** 31
    # a compact CSR batch is widened first
    d = _csr(65, True, seed=8)
    d["keys"] = (d["keys"] >> 32).astype(np.int32)
    assert _check(devname, d, seed=9).keys.cpu().numpy().min() >= 0


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("field_major", [True, False])
def test_shuffle_wide_rows_fall_back_to_torch(devname, field_major):
    """More than 64 fields: torch gathers (as Batch.to_field_major), same result."""
    _check(devname, _fixed(257, 65, True, seed=4), seed=6, field_major=field_major)
    _check(devname, _fixed(63, 65, False, seed=4, compact=True), seed=6, field_major=field_major)


@pytest.mark.parametrize("devname", DEVS)
def test_shuffle_rejections(devname):
    eng, dev = _engine(devname), _dev(devname)
    fm = _batch(_fixed(64, 3, True, seed=1), dev).to_field_major(eng)
    with pytest.raises(ValueError, match="field-major"):
        eng.shuffle_batch(fm, 1)
    out = _batch(_fixed(64, 3, True, seed=1), dev)
    with pytest.raises(ValueError, match="field-major"):  # the native check
        eng.native.shuffle_rows(fm.view(), 1, out.keys.data_ptr(), out.fgid.data_ptr(),
                                out.labels.data_ptr(), 0, True, 8)
    big = _batch(_fixed(MAX_ROWS + 1, 1, False, seed=1), dev)
    with pytest.raises(ValueError, match="max_rows"):
        eng.shuffle_batch(big, 1)
    o = _batch(_fixed(MAX_ROWS + 1, 1, False, seed=1), dev)
    with pytest.raises(ValueError, match="max_rows"):
        eng.native.shuffle_rows(big.view(), 1, o.keys.data_ptr(), 0, o.labels.data_ptr(), 0,
                                False, 8)
    with pytest.raises(ValueError, match="field-major"):  # CSR stays CSR
        eng.shuffle_batch(_batch(_csr(5, False, seed=1), dev), 1, field_major=True)


# ---- trainer ----------------------------------------------------------------
def _cfg(**kw):
    kw.setdefault("epochs", 3)
    return TrainConfig(train_prefix=os.path.join(DATA, "small_train"),
                       test_prefix=os.path.join(DATA, "small_test"), threads=8,
                       write_pred=False, model=ModelConfig(kind="lr"),
                       optim=OptimConfig(kind="ftrl"), engine=EngineConfig(table_log2_cap=14),
                       **kw)


def _table(t):
    k, w = t.table.export_table()
    o = np.argsort(k)
    return k[o], w.reshape(len(k), -1)[o]


def _run(cfg, device="cpu", epochs=3):
    """(sorted table, samples of each epoch) after `epochs` epochs, one at a time."""
    from xflow_amd.trainer import Trainer

    t = Trainer(cfg, device=torch.device(device))
    try:
        per_epoch = []
        for _ in range(epochs):
            s0 = t.samples
            t.train_epochs(1)
            per_epoch.append(t.samples - s0)
        return _table(t), per_epoch
    finally:
        t.close()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_trainer_shuffle_is_seeded(tmp_path):
    """CPU backend, bundled data, 8 threads, LR-FTRL: one seed, one table;
    another seed or no shuffle, another table; the same rows every epoch."""
    m = str(tmp_path / "m.jsonl")
    a, na = _run(_cfg(shuffle=True, shuffle_seed=1, metrics_file=m))
    a2, na2 = _run(_cfg(shuffle=True, shuffle_seed=1))
    b, nb = _run(_cfg(shuffle=True, shuffle_seed=2))
    c, nc = _run(_cfg())
    assert _same(a, a2)
    assert not _same(a, b) and not _same(a, c) and not _same(b, c)
    assert na == na2 == nb == nc and na[0] > 0
    # the rows are the same, so are the keys the table holds
    assert np.array_equal(a[0], c[0]) and np.array_equal(b[0], c[0])
    recs = [json.loads(line) for line in open(m)]
    eps = [r for r in recs if r.get("event") == "epoch"]
    assert len(eps) == 3 and all(r["shuffle"] is True and r["shuffle_seed"] == 1 for r in eps)


@pytest.mark.parametrize("block_bytes", [2 << 20, 8192])
def test_trainer_shuffle_resumes_like_uninterrupted(tmp_path, block_bytes):
    """2 epochs, checkpoint, resume, 1 epoch == 3 epochs straight, bit for bit
    (one block, and several)."""
    from xflow_amd.trainer import Trainer

    def cfg():
        return _cfg(shuffle=True, shuffle_seed=5, train_block_bytes=block_bytes)

    straight, _ = _run(cfg())
    root = str(tmp_path / "ck")
    t = Trainer(cfg(), device=torch.device("cpu"))
    t.train_epochs(2)
    t.save_versioned(root)
    t.close()
    t = Trainer(cfg(), device=torch.device("cpu"))
    assert t.resume(root) is not None and t.epoch == 2
    t.train_epochs(1)
    resumed = _table(t)
    t.close()
    assert _same(straight, resumed)
    # (an epoch's order depends on the epoch: 3 x epoch 0 is another table)
    t = Trainer(cfg(), device=torch.device("cpu"))
    for _ in range(3):
        t.epoch = 0
        t.train_epochs(1)
    assert not _same(straight, _table(t))
    t.close()


def _xfb_shard(d, rows=603, F=7):
    """A fixed-width compact-key .xfb train shard (and a test shard)."""
    from xflow_amd.data import binfmt

    rng = np.random.default_rng(12)
    for name, n in (("tr-00000.xfb", rows), ("te-00000.xfb", 64)):
        keys = rng.integers(0, 3000, n * F).astype(np.uint64) + (1 << 31)
        labels = (rng.random(n) < 0.3).astype(np.float32)
        binfmt.write(str(d / name), labels, np.arange(n + 1) * F, keys,
                     np.tile(np.arange(F, dtype=np.int32), n), compact=True)
    return dict(train_prefix=str(d / "tr"), test_prefix=str(d / "te"), threads=8, block_rows=256,
                write_pred=False, model=ModelConfig(kind="lr"), optim=OptimConfig(kind="ftrl"),
                engine=EngineConfig(table_log2_cap=14))


@pytest.mark.parametrize("devname", DEVS)
def test_trainer_shuffle_fixed_width_blocks(devname, tmp_path):
    """Fixed-width compact blocks (the fused shuffle + transpose + widen), 3
    blocks with a dropped tail: reproducible, the same rows as without."""
    kw = _xfb_shard(tmp_path)
    a, na = _run(TrainConfig(shuffle=True, shuffle_seed=3, **kw), devname, epochs=2)
    a2, _ = _run(TrainConfig(shuffle=True, shuffle_seed=3, **kw), devname, epochs=2)
    c, nc = _run(TrainConfig(**kw), devname, epochs=2)
    assert _same(a, a2) and not _same(a, c)
    assert na == nc == [600, 600]
    assert np.array_equal(a[0], c[0])


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [False, True])
def test_trainer_gpu_resident_shuffle_equals_streamed(gpu_device, gpu_parse):
    """One block: --resident --shuffle (the recorded pre-shuffle batch, laid
    out again every epoch) == --shuffle re-reading the shard, bit for bit."""
    a, na = _run(_cfg(shuffle=True, shuffle_seed=9, gpu_parse=gpu_parse), "cuda")
    b, nb = _run(_cfg(shuffle=True, shuffle_seed=9, gpu_parse=gpu_parse, resident=True), "cuda")
    assert _same(a, b) and na == nb and na[0] > 0
    c, _ = _run(_cfg(gpu_parse=gpu_parse, resident=True), "cuda")
    assert not _same(a, c)


@pytest.mark.gpu
def test_trainer_gpu_resident_shuffle_several_blocks(gpu_device):
    """Several blocks: the block order differs from the streamed run's by
    design; the epochs' sample counts do not, and the run is reproducible."""
    kw = dict(shuffle=True, shuffle_seed=9, train_block_bytes=8192)
    a, na = _run(_cfg(resident=True, **kw), "cuda")
    a2, na2 = _run(_cfg(resident=True, **kw), "cuda")
    b, nb = _run(_cfg(**kw), "cuda")
    assert _same(a, a2)
    assert na == na2 == nb and na[0] > 0
    assert np.array_equal(a[0], b[0])


def test_trainer_shuffle_rejections(tmp_path):
    from xflow_amd.data import binfmt
    from xflow_amd.trainer import Trainer

    with pytest.raises(ValueError, match="serial"):
        Trainer(_cfg(shuffle=True, serial_slices=True), device=torch.device("cpu"))
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 50, (64, 3)).astype(np.uint64)
    binfmt.write_packed(str(tmp_path / "p-00000.xfb"), (rng.random(64) < 0.5).astype(np.float32),
                        keys)
    cfg = TrainConfig(train_prefix=str(tmp_path / "p"), test_prefix=str(tmp_path / "p"), threads=8,
                      shuffle=True, model=ModelConfig(kind="lr"))
    with pytest.raises(ValueError, match="packed"):
        Trainer(cfg, device=torch.device("cpu"))


def test_cli_flags():
    from xflow_amd.cli import build_parser, config_from_args

    cfg = config_from_args(build_parser().parse_args(
        ["tr", "te", "0", "3", "--shuffle", "--shuffle-seed", "7", "--resident"]))
    assert cfg.shuffle and cfg.shuffle_seed == 7 and cfg.resident
    off = config_from_args(build_parser().parse_args(["tr", "te", "0", "3"]))
    assert not off.shuffle and off.shuffle_seed == 0
