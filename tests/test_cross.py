"""Feature crosses computed on the device (Engine.cross_batch, cross_keys,
TrainConfig.crosses / --cross; docs/DESIGN.md §9).

The reference in every test is the model in this file: `ref_key`, the cross
key in Python ints with Python's own fmix64; `_ops`, the first-occurrence
operand lookup; and a plain concatenation.  (`np_keys` is the same hash on
numpy uint64 arrays, checked against the Python ints first, so that the
larger cases stay quick.)  Every comparison is exact, on the CPU backend and
(marked gpu) on the HIP backend.
"""
import dataclasses
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import DATA
from xflow_amd import checkpoint
from xflow_amd.config import (EngineConfig, ModelConfig, OptimConfig, TrainConfig, check_crosses,
                              parse_crosses)
from xflow_amd.engine import Batch, Engine, cross_keys, sanitize_key

DEVS = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
M64 = (1 << 64) - 1
SALT = 0xC3A5C85C97CB3127
NONE = M64  # a missing operand
ROWS = [1, 63, 64, 65, 255, 256, 257]  # wave and tile edges
MAX_ROWS = 1100


# ---- the definition ---------------------------------------------------------
def fmix(h):
    h &= M64
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & M64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & M64
    h ^= h >> 33
    return h


def ref_key(fields, ops, h_forced=None):
    """cross_key in Python ints (h_forced: the hash before sanitizing)."""
    h = fmix(SALT + len(fields))
    for f, v in zip(fields, ops):
        h = fmix(h ^ (f & 0xFFFFFFFF))
        h = fmix(h ^ v)
    if h_forced is not None:
        h = h_forced
    return M64 - 1 if h == M64 else h


def np_fmix(h):
    h = h.copy()
    h ^= h >> np.uint64(33)
    h *= np.uint64(0xFF51AFD7ED558CCD)
    h ^= h >> np.uint64(33)
    h *= np.uint64(0xC4CEB9FE1A85EC53)
    h ^= h >> np.uint64(33)
    return h


def np_keys(fields, ops):
    """ref_key over a [rows, m] uint64 array."""
    ops = np.asarray(ops, dtype=np.uint64).reshape(-1, len(fields))
    with np.errstate(over="ignore"):
        h = np_fmix(np.full(len(ops), (SALT + len(fields)) & M64, dtype=np.uint64))
        for i, f in enumerate(fields):
            h = np_fmix(h ^ np.uint64(f & 0xFFFFFFFF))
            h = np_fmix(h ^ ops[:, i])
    h[h == np.uint64(M64)] = np.uint64(M64 - 1)
    return h


def test_cross_keys_is_the_definition():
    rng = np.random.default_rng(1)
    for fields in ((3, 7), (7, 3), (1, 2, 5), (0, 70, 2, 9), (2 ** 31 - 1, 0)):
        ops = rng.integers(0, 2 ** 64, (40, len(fields)), dtype=np.uint64)
        ops[::5, 0] = NONE  # a missing operand is hashed like a value
        ops[3] = NONE
        want = np.array([ref_key(fields, [int(v) for v in row]) for row in ops], dtype=np.uint64)
        got = cross_keys(fields, ops)
        assert got.dtype == np.uint64 and np.array_equal(got, want), fields
        assert np.array_equal(np_keys(fields, ops), want), fields
        # int64 bit patterns (batch keys) are taken as u64
        assert np.array_equal(cross_keys(fields, ops.view(np.int64)), want)
    # the order is part of the feature, so is the arity, so is a missing operand
    a, b = 0x1234, 0xABCDEF
    assert cross_keys((3, 7), [[a, b]])[0] != cross_keys((7, 3), [[a, b]])[0]
    assert cross_keys((3, 7), [[a, b]])[0] != cross_keys((7, 3), [[b, a]])[0]
    assert cross_keys((3, 7), [[a, NONE]])[0] != cross_keys((3, 7), [[a, b]])[0]
    assert cross_keys((3, 7), [[a, NONE]])[0] != cross_keys((3, 7, 1), [[a, NONE, NONE]])[0]
    assert int(cross_keys((3, 7), [[a, b]])[0]) == ref_key((3, 7), (a, b))


def test_a_key_that_hashes_to_all_ones_is_sanitized():
    assert sanitize_key(M64) == M64 - 1 and sanitize_key(M64 - 1) == M64 - 1
    assert sanitize_key(0) == 0 and sanitize_key(12345) == 12345
    assert ref_key((3, 7), (1, 2), h_forced=M64) == M64 - 1


# ---- batches and their reference --------------------------------------------
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
                                                max_nnz=1 << 17), device=_dev(devname))
    return _engines[devname]


def _labels(rng, rows):
    y = rng.standard_normal(rows).astype(np.float32)
    y[::7] = -0.0  # (compared by bit pattern)
    return y


def _fixed(rows, F, seed, fgid=None, compact=False):
    """fgid: None, or 'perm' (every row a permutation of fields that leaves
    some out and repeats one)."""
    rng = np.random.default_rng(seed)
    if compact:  # u32 keys in int32, most with the top bit set
        keys = rng.integers(-2 ** 31, 2 ** 29, rows * F, dtype=np.int64).astype(np.int32)
    else:
        keys = rng.integers(-2 ** 63, 2 ** 63 - 1, rows * F, dtype=np.int64)
        keys[::11] = -1  # a raw key of all ones reads as missing
    g = None
    if fgid:
        # unsorted ids out of F + 3 fields: some missing in every row; every
        # third row repeats its first field at the end
        g = np.stack([rng.permutation(F + 3)[:F] for _ in range(rows)]).astype(np.int32) \
            if rows else np.zeros((0, F), np.int32)
        g[::3, F - 1] = g[::3, 0]
        g = g.reshape(-1)
    return dict(keys=keys, labels=_labels(rng, rows), row_ptr=None, F=F, fgid=g)


def _csr(rows, seed, max_field=70):
    """Rows of 0..6 entries, a third empty, one of 300 entries whose only
    occurrence of field 5 is its last entry; field ids up to max_field; the
    last row empty."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 7, rows)
    lens[rng.random(rows) < 0.33] = 0
    if rows > 2:
        lens[rows // 2] = 300
    lens[rows - 1:] = 0
    rp = np.zeros(rows + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    nnz = int(rp[-1])
    g = rng.integers(0, max_field + 1, nnz).astype(np.int32)
    if rows > 2:
        a, b = rp[rows // 2], rp[rows // 2 + 1]
        g[a:b][g[a:b] == 5] = 6
        g[b - 1] = 5
    return dict(keys=rng.integers(-2 ** 63, 2 ** 63 - 1, nnz, dtype=np.int64),
                labels=_labels(rng, rows), row_ptr=rp, F=0, fgid=g)


def _batch(d, dev, field_major=False):
    def t(a):
        return None if a is None else torch.from_numpy(a.copy()).to(dev)
    keys, fg = d["keys"], d["fgid"]
    if field_major:
        rows = len(d["labels"])
        keys = np.ascontiguousarray(keys.reshape(rows, d["F"]).T).reshape(-1)
    return Batch(keys=t(keys), labels=t(d["labels"]), row_ptr=t(d["row_ptr"]), fgid=t(fg),
                 nnz_per_row=d["F"], slice_rows=3, field_major=field_major)


def _wide(d):
    k = d["keys"]
    return (k.astype(np.int64) & 0xFFFFFFFF if k.dtype == np.int32 else k).view(np.uint64)


def _ops(d, fields):
    """[rows, m] operands: with fgid the key of the row's first occurrence of
    the field id, without it occurrence `field` of the row, NONE otherwise."""
    rows = len(d["labels"])
    k = _wide(d)
    rp = d["row_ptr"] if d["row_ptr"] is not None else np.arange(rows + 1) * d["F"]
    out = np.full((rows, len(fields)), NONE, dtype=np.uint64)
    for r in range(rows):
        a, b = int(rp[r]), int(rp[r + 1])
        for i, f in enumerate(fields):
            if d["fgid"] is None:
                if f < b - a:
                    out[r, i] = k[a + f]
            else:
                hit = np.flatnonzero(d["fgid"][a:b] == f)
                if len(hit):
                    out[r, i] = k[a + hit[0]]
    return out


def ref_cross(d, X, fgid_base=None):
    """(keys u64 row-major / CSR, row_ptr or None, fgid or None) of d crossed."""
    rows, C = len(d["labels"]), len(X)
    k = _wide(d)
    ck = (np.stack([np_keys(c, _ops(d, c)) for c in X], axis=1) if rows
          else np.zeros((0, C), np.uint64))
    cg = np.tile(np.arange(C, dtype=np.int32) + (fgid_base or 0), (rows, 1))
    if d["row_ptr"] is None:
        F = d["F"]
        keys = np.concatenate([k.reshape(rows, F), ck], axis=1).reshape(-1)
        fg = (np.concatenate([d["fgid"].reshape(rows, F), cg], axis=1).reshape(-1)
              if fgid_base is not None else None)
        return keys, None, fg
    rp = d["row_ptr"]
    want_rp = (rp.astype(np.int64) + C * np.arange(rows + 1)).astype(np.int32)
    keys = np.concatenate([np.concatenate([k[rp[r]:rp[r + 1]], ck[r]]) for r in range(rows)]
                          + [np.zeros(0, np.uint64)])
    fg = (np.concatenate([np.concatenate([d["fgid"][rp[r]:rp[r + 1]], cg[r]]) for r in range(rows)]
                         + [np.zeros(0, np.int32)]) if fgid_base is not None else None)
    return keys, want_rp, fg


def _crosses(F, C, seed, span=None):
    """C distinct crosses of arities 2, 3, 4 in turn over fields [0, span):
    span = F + 2 reaches operands the rows do not have."""
    rng = np.random.default_rng(seed)
    span = span or F + 2
    out = []
    while len(out) < C:
        m = min(2 + len(out) % 3, span)
        c = tuple(int(f) for f in rng.permutation(span)[:m])
        if c not in out:
            out.append(c)
    return out


def _check(devname, d, X, field_major=None, fgid_base=None, src_field_major=False, seed=None):
    """cross_batch(d) == ref_cross(d), exactly; the source untouched."""
    eng, dev = _engine(devname), _dev(devname)
    src = _batch(d, dev, src_field_major)
    out = eng.cross_batch(src, X, seed=seed, field_major=field_major, fgid_base=fgid_base)
    rows, F, C = len(d["labels"]), d["F"], len(X)
    fixed = d["row_ptr"] is None
    fm = fixed if field_major is None else field_major
    assert out.field_major == fm and out.slice_rows == 3
    assert out.nnz_per_row == (F + C if fixed else 0)
    assert out.keys.dtype == torch.int64 and out.rows == rows
    assert out.nnz == len(d["keys"]) + C * rows
    out.check(dev)
    want_k, want_rp, want_g = ref_cross(d, X, fgid_base)
    got_k = out.keys.cpu().numpy().view(np.uint64)
    got_g = out.fgid.cpu().numpy() if out.fgid is not None else None
    assert (got_g is None) == (fgid_base is None)
    if fm:  # back to row-major for the comparison
        got_k = np.ascontiguousarray(got_k.reshape(F + C, rows).T).reshape(-1)
        if got_g is not None:
            got_g = np.ascontiguousarray(got_g.reshape(F + C, rows).T).reshape(-1)
    assert np.array_equal(got_k, want_k)
    if got_g is not None:
        assert got_g.dtype == np.int32 and np.array_equal(got_g, want_g)
    if fixed:
        assert out.row_ptr is None
    else:
        got_rp = out.row_ptr.cpu().numpy()
        assert got_rp.dtype == np.int32 and np.array_equal(got_rp, want_rp)
    assert np.array_equal(out.labels.cpu().numpy().view(np.uint32), d["labels"].view(np.uint32))
    ref_src = _batch(d, torch.device("cpu"), src_field_major)
    for name in ("keys", "labels", "row_ptr", "fgid"):
        if getattr(ref_src, name) is not None:
            assert torch.equal(getattr(src, name).cpu(), getattr(ref_src, name)), name
    return out


# ---- fixed width ------------------------------------------------------------
@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("field_major", [True, False])
@pytest.mark.parametrize("F,C", [(2, 3), (3, 16), (39, 13), (60, 4)])
def test_cross_fixed_width(devname, F, C, field_major):
    """No field ids: the operand is the occurrence's index (>= F: missing).
    F = 60, C = 4 fills the 64-column tile."""
    X = _crosses(F, C, seed=F)
    assert {len(c) for c in X} == ({2, 3, 4} if C >= 3 else {2, 3})
    assert any(f >= F for c in X for f in c)
    for rows in [0] + ROWS:
        _check(devname, _fixed(rows, F, seed=F * 1000 + rows), X, field_major=field_major)


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("field_major", [True, False])
def test_cross_fixed_width_compact_keys(devname, field_major):
    """Compact u32 keys (int32, the top bit set) are crossed as zero-extended u64."""
    for rows, F in ((257, 39), (64, 2)):
        d = _fixed(rows, F, seed=rows, compact=True)
        out = _check(devname, d, _crosses(F, 4, seed=3), field_major=field_major)
        k = out.keys.cpu().numpy().reshape(F + 4, rows) if field_major else \
            out.keys.cpu().numpy().reshape(rows, F + 4).T
        assert k[:F].min() >= 0 and k[:F].max() < 2 ** 32 and k[:F].max() >= 2 ** 31
    d = _fixed(65, 5, seed=1, fgid="perm", compact=True)
    _check(devname, d, _crosses(5, 3, seed=4, span=8), field_major=field_major, fgid_base=100)


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("field_major", [True, False])
@pytest.mark.parametrize("fgid_base", [None, 1000])
def test_cross_fixed_width_with_fgid(devname, field_major, fgid_base):
    """Field ids: unsorted, one repeated (the first occurrence wins), some
    missing; the output ids of the crosses are fgid_base + c."""
    for rows, F, C in ((1, 4, 2), (65, 7, 5), (257, 18, 16), (256, 39, 3)):
        d = _fixed(rows, F, seed=rows + F, fgid="perm")
        X = _crosses(F, C, seed=rows, span=F + 3)
        if rows >= 65:  # the data holds what the case is about
            g = d["fgid"].reshape(rows, F)
            assert np.any(g[:, 0] == g[:, F - 1]) and np.any(np.diff(g, axis=1) < 0)
            ops = _ops(d, X[0])
            assert np.any(ops == NONE) and np.any(ops != NONE)
        _check(devname, d, X, field_major=field_major, fgid_base=fgid_base)


@pytest.mark.parametrize("devname", DEVS)
def test_cross_first_occurrence_wins(devname):
    """One hand-made row: field 3 twice, field 9 absent."""
    d = dict(keys=np.array([10, 11, 12, 13], np.int64), labels=np.zeros(1, np.float32),
             row_ptr=None, F=4, fgid=np.array([7, 3, 5, 3], np.int32))
    out = _check(devname, d, [(3, 7), (7, 3), (3, 9)], field_major=False, fgid_base=40)
    k = out.keys.cpu().numpy().view(np.uint64)
    assert int(k[4]) == ref_key((3, 7), (11, 10)) and int(k[5]) == ref_key((7, 3), (10, 11))
    assert int(k[6]) == ref_key((3, 9), (11, NONE))
    assert out.fgid.cpu().numpy().tolist() == [7, 3, 5, 3, 40, 41, 42]


# ---- field-major input -------------------------------------------------------
@pytest.mark.parametrize("devname", DEVS)
def test_cross_field_major_input(devname):
    for F, C in ((2, 3), (39, 13), (64, 16)):  # (no tile: F + C may pass 64)
        X = _crosses(F, C, seed=F + 1)
        for rows in [0] + ROWS:
            _check(devname, _fixed(rows, F, seed=F * 77 + rows), X, src_field_major=True)


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("in_place", [False, True])
def test_cross_field_major_col_stride(devname, in_place):
    """col_stride > rows, and the in-place form: the cross columns go behind
    the input's in the same buffer; nothing else is written."""
    eng, dev = _engine(devname), _dev(devname)
    for rows in (1, 65, 257):
        F, C, stride = 5, 4, rows + 9
        d = _fixed(rows, F, seed=rows)
        X = _crosses(F, C, seed=2)
        want, _, _ = ref_cross(d, X)
        want = want.reshape(rows, F + C).T
        buf = np.full((F + C, stride), 0x5A5A5A5A, np.int64)
        buf[:F, :rows] = d["keys"].reshape(rows, F).T
        src = torch.from_numpy(buf.copy()).to(dev)
        dst = src if in_place else torch.full((F + C, stride + 2), 0x5A5A5A5A, dtype=torch.int64,
                                              device=dev)
        y = torch.from_numpy(d["labels"].copy()).to(dev)
        y_out = torch.empty_like(y)
        v = Batch(keys=src.view(-1)[:F * rows], labels=y, nnz_per_row=F, field_major=True).view()
        v.col_stride = stride
        eng._sync_stream()
        eng.native.cross_rows(v, [list(c) for c in X], 0, None, dst.data_ptr(), 0,
                              y_out.data_ptr(), 0, True, 8, dst.shape[1])
        got = dst.cpu().numpy()
        assert np.array_equal(got[:, :rows].view(np.uint64), want)
        assert np.all(got[:, rows:] == 0x5A5A5A5A)
        assert torch.equal(y_out.cpu().view(torch.int32), y.cpu().view(torch.int32))


# ---- CSR ----------------------------------------------------------------------
@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("fgid_base", [None, 71])
def test_cross_csr(devname, fgid_base):
    """Empty rows, rows without any operand, a 300-entry row whose operand is
    its last entry, field ids up to 70, the last row empty; the new row_ptr."""
    X = [(5, 1), (70, 5, 2), (3, 4, 5, 6), (1, 5), (69, 70)]
    for rows in (0, 1, 255, 256, 257, 1025):
        d = _csr(rows, seed=rows)
        if rows > 2:
            r = rows // 2
            ops = _ops(d, (5,))
            assert ops[r, 0] == _wide(d)[d["row_ptr"][r + 1] - 1]  # the long row's last entry
            assert np.all(_ops(d, X[0])[rows - 1] == NONE)
        _check(devname, d, X, fgid_base=fgid_base)
    # one cross, and sixteen
    d = _csr(257, seed=9, max_field=6)
    _check(devname, d, [(2, 3)], fgid_base=fgid_base)
    _check(devname, d, _crosses(6, 16, seed=1, span=8), fgid_base=fgid_base)


# ---- with a seed --------------------------------------------------------------
@pytest.mark.parametrize("devname", DEVS)
def test_cross_with_seed_is_shuffle_then_cross(devname):
    eng, dev = _engine(devname), _dev(devname)

    def same(a, b):
        assert a.field_major == b.field_major and a.nnz_per_row == b.nnz_per_row
        for name in ("keys", "labels", "row_ptr", "fgid"):
            x, y = getattr(a, name), getattr(b, name)
            assert (x is None) == (y is None), name
            if x is not None:
                assert np.array_equal(x.cpu().numpy().view(np.uint8),
                                      y.cpu().numpy().view(np.uint8)), name

    for rows, F, fg, base in ((257, 39, None, None), (65, 7, "perm", 50), (1, 3, None, None),
                              (256, 5, "perm", None)):
        for compact in (False, True):
            d = _fixed(rows, F, seed=rows, fgid=fg, compact=compact)
            X = _crosses(F, 4, seed=rows, span=F + 3)
            for fm in (True, False):
                a = eng.cross_batch(_batch(d, dev), X, seed=12345, field_major=fm, fgid_base=base)
                sh = eng.shuffle_batch(_batch(d, dev), 12345, field_major=False)
                same(a, eng.cross_batch(sh, X, field_major=fm, fgid_base=base))
    for rows in (1, 257, 1025):
        d = _csr(rows, seed=rows + 1)
        X = [(5, 1), (70, 5, 2)]
        for base in (None, 80):
            a = eng.cross_batch(_batch(d, dev), X, seed=2 ** 64 - 3, fgid_base=base)
            sh = eng.shuffle_batch(_batch(d, dev), 2 ** 64 - 3)
            same(a, eng.cross_batch(sh, X, fgid_base=base))
    # and the shuffle moved something
    d = _fixed(257, 3, seed=5)
    a = eng.cross_batch(_batch(d, dev), [(0, 1)], seed=1, field_major=False)
    b = eng.cross_batch(_batch(d, dev), [(0, 1)], field_major=False)
    assert not torch.equal(a.keys, b.keys)
    assert torch.equal(a.keys.view(257, 4).sort(0).values, b.keys.view(257, 4).sort(0).values)


# ---- what is refused ----------------------------------------------------------
@pytest.mark.parametrize("devname", DEVS)
def test_cross_rejections(devname):
    eng, dev = _engine(devname), _dev(devname)
    # 60 fields + 5 crosses: one column more than the tile holds
    d = _fixed(64, 60, seed=1)
    with pytest.raises(ValueError, match="64"):
        eng.cross_batch(_batch(d, dev), _crosses(60, 5, seed=1))
    o = torch.empty(64 * 65, dtype=torch.int64, device=dev)
    y = torch.empty(64, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="64"):  # the native check
        eng.native.cross_rows(_batch(d, dev).view(), [list(c) for c in _crosses(60, 5, seed=1)], 0,
                              None, o.data_ptr(), 0, y.data_ptr(), 0, True, 8)
    csr = _csr(5, seed=1)
    nofg = dict(csr, fgid=None)
    with pytest.raises(ValueError, match="fgid"):
        eng.cross_batch(_batch(nofg, dev), [(1, 2)])
    rp = torch.empty(6, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="fgid"):
        eng.native.cross_rows(_batch(nofg, dev).view(), [[1, 2]], 0, None, o.data_ptr(), 0,
                              y.data_ptr(), rp.data_ptr(), False, 8)
    with pytest.raises(ValueError, match="field-major"):  # CSR stays CSR
        eng.cross_batch(_batch(csr, dev), [(1, 2)], field_major=True)
    fm = _batch(_fixed(64, 3, seed=1), dev, field_major=True)
    with pytest.raises(ValueError, match="field-major"):
        eng.cross_batch(fm, [(0, 1)], seed=3)
    with pytest.raises(ValueError, match="field-major"):
        eng.cross_batch(dataclasses.replace(fm, fgid=torch.zeros(192, dtype=torch.int32, device=dev)),
                        [(0, 1)])
    with pytest.raises(ValueError, match="fgid_base"):
        eng.cross_batch(_batch(_fixed(64, 3, seed=1), dev), [(0, 1)], fgid_base=5)
    big = _batch(_fixed(MAX_ROWS + 1, 1, seed=1), dev)
    with pytest.raises(ValueError, match="max_rows"):
        eng.cross_batch(big, [(0, 1)])
    with pytest.raises(ValueError, match="max_rows"):
        eng.native.cross_rows(big.view(), [[0, 1]], 0, None, o.data_ptr(), 0, y.data_ptr(), 0,
                              False, 8)
    small = Engine(ModelConfig(), OptimConfig(),
                   EngineConfig(table_log2_cap=8, max_rows=64, max_nnz=64 * 3 + 63), device=dev)
    with pytest.raises(ValueError, match="max_nnz"):
        small.cross_batch(_batch(_fixed(64, 3, seed=1), dev), [(0, 1)])
    with pytest.raises(ValueError, match="max_nnz"):
        small.native.cross_rows(_batch(_fixed(64, 3, seed=1), dev).view(), [[0, 1]], 0, None,
                                o.data_ptr(), 0, y.data_ptr(), 0, False, 8)
    for bad, msg in (([(1,)], "2 to 4"), ([(1, 2, 3, 4, 5)], "2 to 4"), ([(1, -2)], "non-negative"),
                     ([(1, 1)], "repeated"), ([(1, 2), (1, 2)], "twice"), ([], "1 to 16"),
                     ([(i, i + 1) for i in range(17)], "1 to 16")):
        with pytest.raises(ValueError, match=msg):
            eng.cross_batch(_batch(_fixed(4, 3, seed=1), dev), bad)
    for bad in ([[1]], [[1, -2]], []):  # the native check of the spec
        with pytest.raises(ValueError):
            eng.native.cross_rows(_batch(_fixed(4, 3, seed=1), dev).view(), bad, 0, None,
                                  o.data_ptr(), 0, y.data_ptr(), 0, False, 8)


# ---- plumbing: the step trains on crossed batches as on any other ----------------
def _table_of(eng):
    k, w = eng.export_table()
    o = np.argsort(k)
    return k[o], w.reshape(len(k), -1)[o]


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("S", [1, 8])
@pytest.mark.parametrize("kind,v_dim", [("lr", 10), ("fm", 4)])
def test_training_on_crossed_batches_equals_host_appended_keys(devname, kind, v_dim, S):
    dev = _dev(devname)
    rows, F, X = 256, 6, [(0, 1), (5, 2, 3), (1, 0)]
    rng = np.random.default_rng(3)
    blocks = []
    for _ in range(3):
        keys = (rng.integers(0, 50, (rows, F)) + 1000 * np.arange(F)).astype(np.int64).reshape(-1)
        blocks.append(dict(keys=keys, labels=(rng.random(rows) < 0.4).astype(np.float32),
                           row_ptr=None, F=F, fgid=None))

    def engine():
        return Engine(ModelConfig(kind=kind, v_dim=v_dim), OptimConfig(kind="ftrl", alpha=0.5),
                      EngineConfig(table_log2_cap=12, max_rows=rows, max_nnz=rows * (F + 3),
                                   max_slices=S), device=dev)

    a, b = engine(), engine()
    for d in blocks:
        src = dataclasses.replace(_batch(d, dev), slice_rows=rows // S)
        a.train_step(a.cross_batch(src, X))
        want, _, _ = ref_cross(d, X)
        host = Batch(keys=torch.from_numpy(want.view(np.int64).copy()).to(dev), labels=src.labels,
                     nnz_per_row=F + 3, slice_rows=rows // S)
        b.train_step(host.to_field_major(b))
    ta, tb = _table_of(a), _table_of(b)
    assert len(ta[0]) > 3 * 50 and np.array_equal(ta[0], tb[0])
    assert np.array_equal(ta[1], tb[1])
    assert not a.overflowed()


# ---- it learns what it is for ---------------------------------------------------
def _xor_block(dev):
    """Two fields of 8 values, every (a, b) pair 64 times, label (a + b) % 2."""
    a, b = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    a, b = np.tile(a.reshape(-1), 64), np.tile(b.reshape(-1), 64)
    o = np.random.default_rng(0).permutation(4096)
    a, b = a[o], b[o]
    keys = np.stack([100 + a, 200 + b], axis=1).astype(np.int64).reshape(-1)
    return Batch(keys=torch.from_numpy(keys).to(dev),
                 labels=torch.from_numpy(((a + b) % 2).astype(np.float32)).to(dev),
                 nnz_per_row=2, slice_rows=4096 // 8)


@pytest.mark.parametrize("devname", DEVS)
def test_a_cross_learns_the_interaction_lr_cannot(devname):
    """LR on two fields whose label is the parity of their sum: every key
    sees as many positives as negatives, so ln 2 is the optimum of the convex
    loss and no weights do better -- the uncrossed logloss is >= ln 2 - 1e-6.
    With the cross 0x1 every pair has a key of its own, and the same 30
    epochs (FTRL alpha 4, beta 1, no regularisation, 8 slices) must bring the
    logloss below half of that.  Measured on the CPU backend: 0.6931472
    uncrossed, 0.0729 crossed (alpha 1: 0.261; alpha 4, 60 epochs: 0.037)."""
    dev = _dev(devname)
    out = {}
    for crossed in (False, True):
        eng = Engine(ModelConfig(kind="lr"),
                     OptimConfig(kind="ftrl", alpha=4.0, beta=1.0, lambda1=0.0, lambda2=0.0),
                     EngineConfig(table_log2_cap=10, max_rows=4096, max_nnz=4096 * 3,
                                  max_slices=8), device=dev)
        raw = _xor_block(dev)
        b = eng.cross_batch(raw, [(0, 1)]) if crossed else raw.to_field_major(eng)
        for _ in range(30):
            eng.train_step(b)
        p = eng.eval_step(b)
        out[crossed] = eng.eval_metrics(p, b.labels)["ln_logloss"]
        assert eng.table_size() == (16 + 64 if crossed else 16)
    print("logloss uncrossed", out[False], "crossed", out[True])
    assert out[False] >= math.log(2) - 1e-6
    assert out[True] < 0.5 * out[False]


# ---- trainer ----------------------------------------------------------------------
CROSSES = [(3, 7), (1, 2, 5), (16, 17)]


def _cfg(**kw):
    kw.setdefault("epochs", 3)
    kw.setdefault("model", ModelConfig(kind="lr"))
    return TrainConfig(train_prefix=os.path.join(DATA, "small_train"),
                       test_prefix=os.path.join(DATA, "small_test"), threads=8,
                       write_pred=False, optim=OptimConfig(kind="ftrl"),
                       engine=EngineConfig(table_log2_cap=14), **kw)


def _run(cfg, device="cpu", epochs=3):
    from xflow_amd.trainer import Trainer

    t = Trainer(cfg, device=torch.device(device))
    try:
        for _ in range(epochs):
            t.train_epochs(1)
        return _table_of(t.table)
    finally:
        t.close()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _bundled_cross_keys():
    """The cross keys of the bundled train shard, from the host parser."""
    from xflow_amd import native

    blk = native.load().parse_libffm(open(os.path.join(DATA, "small_train-00000"), "rb").read())
    d = dict(keys=np.asarray(blk["keys"]).view(np.int64), labels=np.asarray(blk["labels"]),
             row_ptr=np.asarray(blk["row_ptr"]).astype(np.int32), F=0,
             fgid=np.asarray(blk["fgid"]).astype(np.int32))
    return np.unique(np.concatenate([np_keys(c, _ops(d, c)) for c in CROSSES]))


def test_trainer_cross_is_reproducible_and_adds_keys(tmp_path):
    m = str(tmp_path / "m.jsonl")
    a = _run(_cfg(crosses=CROSSES, metrics_file=m))
    a2 = _run(_cfg(crosses=CROSSES))
    plain = _run(_cfg())
    other = _run(_cfg(crosses=[(7, 3), (1, 2, 5), (16, 17)]))
    assert _same(a, a2) and not _same(a, other)
    # every uncrossed key, plus keys no uncrossed run holds: the shard's cross keys
    assert np.all(np.isin(plain[0], a[0])) and len(a[0]) > len(plain[0])
    new = np.setdiff1d(a[0], plain[0])
    want = _bundled_cross_keys()
    assert len(new) > 0 and np.all(np.isin(new, want))
    # (8 threads drop no row of the 200-row blocks: every cross key is there)
    assert np.array_equal(new, np.setdiff1d(want, plain[0]))
    eps = [json.loads(line) for line in open(m)]
    eps = [r for r in eps if r.get("event") == "epoch"]
    assert len(eps) == 3 and all(r["crosses"] == [list(c) for c in CROSSES] for r in eps)


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("block_bytes", [2 << 20, 8192])
def test_trainer_cross_streamed_equals_resident_cpu(shuffle, block_bytes):
    kw = dict(crosses=CROSSES, shuffle=shuffle, shuffle_seed=4, train_block_bytes=block_bytes)
    a = _run(_cfg(**kw))
    b = _run(_cfg(resident=True, **kw))
    if shuffle and block_bytes == 8192:
        # (several blocks: --resident --shuffle also permutes the block order,
        # by design; the keys are the same)
        assert np.array_equal(a[0], b[0])
    else:
        assert _same(a, b)
    assert not _same(a, _run(_cfg(shuffle=shuffle, shuffle_seed=4, train_block_bytes=block_bytes)))


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [False, True])
@pytest.mark.parametrize("shuffle", [False, True])
def test_trainer_gpu_cross_resident_equals_streamed(gpu_device, gpu_parse, shuffle):
    kw = dict(crosses=CROSSES, shuffle=shuffle, shuffle_seed=9, gpu_parse=gpu_parse)
    a = _run(_cfg(**kw), "cuda")
    b = _run(_cfg(resident=True, **kw), "cuda")
    assert _same(a, b) and len(a[0]) > 0
    assert not _same(a, _run(_cfg(shuffle=shuffle, shuffle_seed=9, gpu_parse=gpu_parse), "cuda"))
    # the device run holds the keys of the CPU run
    assert np.array_equal(a[0], _run(_cfg(crosses=CROSSES, shuffle=shuffle, shuffle_seed=9))[0])


@pytest.mark.parametrize("devname", DEVS)
def test_trainer_cross_fixed_width_blocks(devname, tmp_path):
    """Fixed-width compact .xfb blocks whose columns are not their fields: the
    fused widen + cross + transpose (+ shuffle) pass."""
    from xflow_amd.data import binfmt

    rng = np.random.default_rng(12)
    F = 7
    order = np.array([4, 0, 6, 1, 5, 2, 3], np.int32)  # column j holds field order[j]
    for name, n in (("tr-00000.xfb", 603), ("te-00000.xfb", 64)):
        keys = rng.integers(0, 300, n * F).astype(np.uint64) + (1 << 31)
        labels = (rng.random(n) < 0.3).astype(np.float32)
        binfmt.write(str(tmp_path / name), labels, np.arange(n + 1) * F, keys, np.tile(order, n),
                     compact=True)
    kw = dict(train_prefix=str(tmp_path / "tr"), test_prefix=str(tmp_path / "te"), threads=8,
              block_rows=256, write_pred=False, model=ModelConfig(kind="lr"),
              optim=OptimConfig(kind="ftrl"), engine=EngineConfig(table_log2_cap=14))
    X = [(0, 6), (3, 4, 9)]
    a = _run(TrainConfig(crosses=X, **kw), devname, epochs=2)
    a2 = _run(TrainConfig(crosses=X, **kw), devname, epochs=2)
    s = _run(TrainConfig(crosses=X, shuffle=True, shuffle_seed=3, **kw), devname, epochs=2)
    r = _run(TrainConfig(crosses=X, shuffle=True, shuffle_seed=3, resident=True, **kw), devname,
             epochs=2)
    plain = _run(TrainConfig(**kw), devname, epochs=2)
    assert _same(a, a2) and not _same(a, s) and np.array_equal(a[0], s[0])
    assert np.array_equal(s[0], r[0])
    # the new keys are the cross keys, by field id, of the rows each block
    # trains (its rows % 8 are dropped)
    new = np.setdiff1d(a[0], plain[0])
    rd = binfmt.open_reader(str(tmp_path / "tr-00000.xfb"), 256)
    want = []
    while True:
        blk = rd.next()
        if blk is None:
            break
        n = len(blk["labels"]) // 8 * 8
        k = np.asarray(blk["keys"][:n * F])
        dd = dict(keys=k.view(np.int32) if k.dtype == np.uint32 else k.view(np.int64),
                  labels=np.zeros(n, np.float32), row_ptr=None, F=F,
                  fgid=np.asarray(blk["fgid"][:n * F]).astype(np.int32))
        want += [np_keys(c, _ops(dd, c)) for c in X]
    want = np.unique(np.concatenate(want))
    assert len(new) > 0 and np.array_equal(new, np.setdiff1d(want, plain[0]))


@pytest.mark.parametrize("shuffle", [False, True])
def test_trainer_cross_resumes_like_uninterrupted(tmp_path, shuffle):
    from xflow_amd.trainer import Trainer

    def cfg(**kw):
        return _cfg(crosses=CROSSES, shuffle=shuffle, shuffle_seed=5, **kw)

    straight = _run(cfg())
    root = str(tmp_path / "ck")
    t = Trainer(cfg(), device=torch.device("cpu"))
    t.train_epochs(2)
    t.save_versioned(root)
    t.close()
    meta = checkpoint.load_meta(checkpoint.latest(root))
    assert meta["crosses"] == [list(c) for c in CROSSES] and meta["cross_field_base"] == -1
    assert checkpoint.crosses_of(meta) == (CROSSES, None)
    t = Trainer(cfg(), device=torch.device("cpu"))
    assert t.resume(root) is not None and t.epoch == 2
    t.train_epochs(1)
    resumed = _table_of(t.table)
    t.close()
    assert _same(straight, resumed)
    # another spec, or none, is refused before anything is loaded; both are named
    for other in ([(7, 3), (1, 2, 5), (16, 17)], CROSSES[:2], []):
        t = Trainer(_cfg(crosses=other), device=torch.device("cpu"))
        with pytest.raises(ValueError, match=r"\(3, 7\).*\(16, 17\)") as e:
            t.resume(root)
        assert str(other) in str(e.value)
        assert t.table.table_size() == 0
        with pytest.raises(ValueError, match="crosses"):
            t.load(checkpoint.latest(root))
        t.close()


def test_trainer_cross_mvm_needs_and_records_the_field_base(tmp_path):
    from xflow_amd.trainer import Trainer

    mvm = ModelConfig(kind="mvm", v_dim=4)
    with pytest.raises(ValueError, match="cross-field-base"):
        Trainer(_cfg(crosses=CROSSES, model=mvm), device=torch.device("cpu"))
    cfg = _cfg(crosses=CROSSES, cross_field_base=20, model=mvm, epochs=1)
    t = Trainer(cfg, device=torch.device("cpu"))
    t.train_epochs(1)
    res = t.predict()
    assert res["n"] == 200 and np.isfinite(res["ln_logloss"])
    t.save(str(tmp_path / "ck"))
    assert checkpoint.crosses_of(checkpoint.load_meta(str(tmp_path / "ck"))) == (CROSSES, 20)
    t.close()
    t = Trainer(_cfg(crosses=CROSSES, cross_field_base=21, model=mvm), device=torch.device("cpu"))
    with pytest.raises(ValueError, match="20.*21"):
        t.load(str(tmp_path / "ck"))
    t.close()


def test_trainer_cross_rejections(tmp_path):
    from xflow_amd.data import binfmt
    from xflow_amd.trainer import Trainer

    with pytest.raises(ValueError, match="serial"):
        Trainer(_cfg(crosses=CROSSES, serial_slices=True), device=torch.device("cpu"))
    for bad, msg in (([(1,)], "2 to 4"), ([(1, 1)], "repeated"), ([(1, 2), (1, 2)], "twice"),
                     ([(1, -2)], "non-negative"), ([(i, i + 1) for i in range(17)], "1 to 16")):
        with pytest.raises(ValueError, match=msg):
            Trainer(_cfg(crosses=bad), device=torch.device("cpu"))
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 50, (64, 3)).astype(np.uint64)
    binfmt.write_packed(str(tmp_path / "p-00000.xfb"), (rng.random(64) < 0.5).astype(np.float32),
                        keys)
    cfg = TrainConfig(train_prefix=str(tmp_path / "p"), test_prefix=str(tmp_path / "p"), threads=8,
                      crosses=[(0, 1)], model=ModelConfig(kind="lr"))
    with pytest.raises(ValueError, match="packed"):
        Trainer(cfg, device=torch.device("cpu"))


# ---- checkpoint and serving --------------------------------------------------------
@pytest.mark.parametrize("devname", DEVS)
def test_predictor_crosses_requests_like_the_trainer(devname, tmp_path):
    from xflow_amd.serve import Predictor
    from xflow_amd.trainer import Trainer

    dev = _dev(devname)
    cfg = _cfg(crosses=CROSSES, epochs=2)
    cfg.write_pred, cfg.pred_dir = True, str(tmp_path)
    t = Trainer(cfg, device=dev)
    t.train_epochs(2)
    t.predict()
    t.save(str(tmp_path / "ck"))
    t.close()
    want = [line.split("\t")[0] for line in open(tmp_path / "pred_0_0.txt")]
    p = Predictor(str(tmp_path / "ck"), device=dev, max_rows=64)  # (several chunks)
    assert p.crosses == CROSSES and p.cross_field_base is None
    text = open(os.path.join(DATA, "small_test-00000"), "rb").read()
    got = p.predict_libffm(text)
    assert len(got) == len(want) == 200
    assert ["%g" % float(x) for x in got] == want
    # the crosses matter: the same table without them scores otherwise
    p.crosses = []
    assert ["%g" % float(x) for x in p.predict_libffm(text)] != want
    p.crosses = CROSSES
    with pytest.raises(ValueError, match="crosses"):
        p.predict_keys([[1, 2, 3]])
    with pytest.raises(ValueError, match="crosses"):
        p.predict_csr(np.array([1, 2], np.uint64), np.array([0, 2]))
    one = p.predict_keys([[11, 12, 13]], fields=[[3, 7, 1]])
    assert one.shape == (1,) and 0.0 < float(one[0]) < 1.0


def test_checkpoint_without_crosses_key_loads_and_serves(tmp_path):
    """meta.json as it was before crosses existed: no 'crosses' key."""
    from xflow_amd.serve import Predictor
    from xflow_amd.trainer import Trainer

    cfg = _cfg(epochs=1)
    cfg.write_pred, cfg.pred_dir = True, str(tmp_path)
    t = Trainer(cfg, device=torch.device("cpu"))
    t.train_epochs(1)
    t.predict()
    t.save(str(tmp_path / "ck"))
    t.close()
    meta = checkpoint.load_meta(str(tmp_path / "ck"))
    assert "crosses" not in meta and "cross_field_base" not in meta
    assert checkpoint.crosses_of(meta) == ([], None)
    p = Predictor(str(tmp_path / "ck"), device=torch.device("cpu"))
    assert p.crosses == []
    got = p.predict_libffm(open(os.path.join(DATA, "small_test-00000"), "rb").read())
    assert ["%g" % float(x) for x in got] == \
        [line.split("\t")[0] for line in open(tmp_path / "pred_0_0.txt")]
    assert p.predict_keys([[1, 2, 3]]).shape == (1,)  # (no fields needed)
    t = Trainer(_cfg(), device=torch.device("cpu"))
    t.load(str(tmp_path / "ck"))
    assert t.table.table_size() > 0
    t.close()
    t = Trainer(_cfg(crosses=CROSSES), device=torch.device("cpu"))
    with pytest.raises(ValueError, match="crosses"):
        t.load(str(tmp_path / "ck"))
    t.close()


def test_http_route_refuses_keys_without_fields(tmp_path):
    pytest.importorskip("fastapi")
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from xflow_amd.serve import Predictor, make_app
    from xflow_amd.trainer import Trainer

    t = Trainer(_cfg(crosses=CROSSES, epochs=1), device=torch.device("cpu"))
    t.train_epochs(1)
    t.save(str(tmp_path / "ck"))
    t.close()
    c = TestClient(make_app(Predictor(str(tmp_path / "ck"), device=torch.device("cpu"))))
    r = c.post("/predict", json={"keys": [[1, 2, 3]]})
    assert r.status_code == 400 and "crosses" in r.json()["detail"]
    r = c.post("/predict", json={"keys": [[1, 2, 3]], "fields": [[3, 7, 1]]})
    assert r.status_code == 200 and len(r.json()["pctr"]) == 1


# ---- configuration -------------------------------------------------------------------
def test_parse_crosses():
    assert parse_crosses("3x7,1x2x5") == [(3, 7), (1, 2, 5)]
    assert parse_crosses(" 0x1 ") == [(0, 1)] and parse_crosses("") == []
    assert parse_crosses("3x7,7x3") == [(3, 7), (7, 3)]
    assert check_crosses([[1, 2], (3, 4, 5, 6)]) == [(1, 2), (3, 4, 5, 6)]
    assert len(parse_crosses(",".join("%dx%d" % (i, i + 1) for i in range(16)))) == 16
    for bad, msg in (("3", "2 to 4"), ("1x2x3x4x5", "2 to 4"), ("3x-7", "non-negative"),
                     ("3x3", "repeated"), ("3x7,3x7", "twice"), ("3x7,,1x2", "joined by"),
                     ("axb", "joined by"), ("3 7", "joined by"),
                     (",".join("%dx%d" % (i, i + 1) for i in range(17)), "1 to 16")):
        with pytest.raises(ValueError, match=msg):
            parse_crosses(bad)


def test_cli_flags():
    from xflow_amd.cli import build_parser, config_from_args

    cfg = config_from_args(build_parser().parse_args(
        ["tr", "te", "2", "3", "--cross", "3x7,1x2x5", "--cross-field-base", "40", "--shuffle"]))
    assert cfg.crosses == [(3, 7), (1, 2, 5)] and cfg.cross_field_base == 40 and cfg.shuffle
    off = config_from_args(build_parser().parse_args(["tr", "te", "0", "3"]))
    assert off.crosses == [] and off.cross_field_base == -1
    with pytest.raises(ValueError, match="repeated"):
        config_from_args(build_parser().parse_args(["tr", "te", "0", "3", "--cross", "3x3"]))
