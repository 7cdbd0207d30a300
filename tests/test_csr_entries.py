"""The CSR gradient entries themselves (CsrOut: per-key (off, cnt) and the
(slice, value) entries of k_red_csr / k_red_csr_vec), their packed wire form
(launch_scan_u32, k_csr_pack, k_csr_totals) and the receive scan of
s_apply_csr, against xflow_amd/testing/csr_ref.py.

Structure and LR values are exact.  Which slot -- and so which unique index --
a key gets is a CAS race of the dedup (csrc/hip/kernels_dedup.hip), so device
outputs are always compared per key, through the step's own unique list
(Engine::unique_keys, the send keys of w_prepare), never index by index
between two engines.

Every fused case first asks Engine::red_geometry whether the step's dests fit
the buckets the engine allocated (``needed <= nb``): a CSR step's dests are
unique << slog2, and k_red_scatter has no cursor for a dest beyond the
allocated buckets.  The engine sizes them for max_nnz << slog2(max_slices);
the cases with 256 and 2^14 slices, run at their natural max_nnz, would not
fit an allocation sized for one slice group of 32 (FITS below).
"""
import numpy as np
import pytest
import torch

import test_row_structures as trs
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Batch, Engine
from xflow_amd.testing import apply_ref, csr_ref, ref64
from xflow_amd.testing.hashing import fmix64, owner_of

CSR_HASH = 4096        # kCsrHash: direct-indexed sums above CSR_HASH / 2 records of a window
CSR_REG = 2048         # kCsrReg * kCsrBlock: records a bucket keeps in registers
CSR_WIN = 16           # kCsrWinLog2
VEC_WIN = 15           # kCsrVecWin
SCAN_ONE = 16384       # kScanOneMax
SCAN_TILE = 4096       # kScanTile

MODELS = {
    "lr": (ModelConfig(kind="lr"), OptimConfig(kind="ftrl"), "lr"),
    "fm_ref": (ModelConfig(kind="fm", v_dim=4, fm_math="reference"), OptimConfig(kind="sgd"), "fm_ref"),
    "fm_std4": (ModelConfig(kind="fm", v_dim=4, fm_math="standard"), OptimConfig(kind="sgd"), "rows"),
    "fm_std8": (ModelConfig(kind="fm", v_dim=8, fm_math="standard"), OptimConfig(kind="sgd"), "rows"),
    "mvm": (ModelConfig(kind="mvm", v_dim=4), OptimConfig(kind="sgd", sgd_v_init=0.9), "rows"),
}


# ---- batches -------------------------------------------------------------------
class Spec:
    def __init__(self, keys2d, S, slice_rows, seed=0, fgid2d=None):
        keys2d = np.ascontiguousarray(keys2d, dtype=np.uint64)
        self.rows, self.F = keys2d.shape
        self.keys = keys2d.reshape(-1)
        self.row_ptr = (np.arange(self.rows + 1, dtype=np.int64) * self.F).astype(np.int32)
        self.fgid = (np.tile(np.arange(self.F, dtype=np.int32), self.rows) if fgid2d is None
                     else np.ascontiguousarray(fgid2d, dtype=np.int32).reshape(-1))
        self.labels = (np.random.default_rng(seed).random(self.rows) < 0.3).astype(np.float32)
        self.S, self.slice_rows = S, slice_rows
        self.ukeys = np.unique(self.keys)

    def batch(self, dev):
        return Batch(keys=torch.from_numpy(self.keys.view(np.int64)).to(dev),
                     labels=torch.from_numpy(self.labels).to(dev),
                     row_ptr=torch.from_numpy(self.row_ptr).to(dev),
                     fgid=torch.from_numpy(self.fgid).to(dev), slice_rows=self.slice_rows)


def _case_spec(case, S):
    """A Case of test_row_structures as a Spec-like object."""
    s = Spec.__new__(Spec)
    s.rows, s.F = case.rows, 0
    s.keys, s.row_ptr, s.fgid, s.labels = case.keys, case.row_ptr, case.fgid, case.labels
    s.S, s.slice_rows, s.ukeys = S, -(-case.rows // S), case.ukeys
    return s


def _vocab(n, tag=0):
    return fmix64(np.arange(1, n + 1, dtype=np.uint64) + np.uint64(tag << 32)) >> np.uint64(2)


def mixed(S, per=12, F=6, vocab=200, seed=1):
    """S slices of `per` rows: a key in every row (column 0), a key twice in
    a row (columns 1 and 2 equal), zipf keys elsewhere."""
    rng = np.random.default_rng(seed)
    rows = S * per
    v = _vocab(vocab, 1)
    k = v[np.minimum(rng.zipf(1.3, size=(rows, F)), vocab) - 1]
    k[:, 0] = v[0]
    k[:, 2] = k[:, 1]
    return Spec(k, S, per, seed)


def every_slice(S, nkeys, F=8, tag=2):
    """nkeys keys, each once in every slice: a slice is nkeys / F rows."""
    per = nkeys // F
    v = _vocab(nkeys, tag)
    k = np.tile(v.reshape(per, F), (S, 1))
    return Spec(k, S, per, 3)


def one_row_slices(S):
    """S slices of one row: a key in every row, and one of 64 others."""
    v = _vocab(65, 9)
    return Spec(np.stack([np.full(S, v[0]), v[1 + np.arange(S) % 64]], 1), S, 1, 6)


def distinct(rows, F, S, tag=4):
    k = (np.uint64(1) << np.uint64(61)) + np.uint64(tag << 40) + np.arange(rows * F, dtype=np.uint64)
    return Spec(k.reshape(rows, F), S, rows // S, 5)


# ---- engines ---------------------------------------------------------------------
def _engine(dev, name, spec, max_nnz=None, log2=None):
    m, o, _ = MODELS[name]
    nnz = max(len(spec.keys), 1)
    nuq = len(spec.ukeys)
    log2 = log2 or max(12, int(np.ceil(np.log2(max(nuq, 1) * 2.5))))
    eng = Engine(m, o, EngineConfig(table_log2_cap=log2, max_rows=max(spec.rows, 1),
                                    max_nnz=max_nnz or nnz, max_slices=spec.S), device=dev)
    return eng


def _plant(eng, name, keys, seed=11):
    """Non-zero float32 weights for `keys` (SGD words: w, then the pushed flag)."""
    m = MODELS[name][0]
    P = m.params_per_key
    if all(int(k) in trs.KEY_CLASS for k in keys[:4]):
        W = trs.weights(m, keys)
    else:
        rng = np.random.default_rng(seed)
        W = (0.3 * rng.standard_normal((len(keys), P)) / np.sqrt(8.0 * max(m.v_dim, 1))).astype(np.float32)
        W[:, 0] = (0.3 * rng.standard_normal(len(keys)) / np.sqrt(8.0)).astype(np.float32)
    words = np.zeros((len(keys), eng.state_words), dtype=np.uint32)
    words[:, :P] = W.view(np.uint32)
    words[:, P] = 1
    eng.import_table(keys, words.reshape(-1))
    return W


FITS = "the step's dests need {needed} buckets, the engine allocated {nb}"


def _fused(dev, name, spec, max_nnz=None, plant=False):
    """One train_step on a fresh engine: the step's unique keys, (off, cnt),
    entry words, geometry and the pre-step weights of spec.ukeys."""
    eng = _engine(dev, name, spec, max_nnz)
    if plant:
        _plant(eng, name, spec.ukeys)
    W = eng.pull(spec.ukeys)    # (a lookup: absent keys read their lazy-init weights)
    pre = eng.native.red_geometry(spec.S, len(spec.ukeys))
    assert pre["needed"] <= pre["nb"], FITS.format(**pre)
    b = spec.batch(dev)
    assert eng.slices_of(b) == spec.S
    assert eng.native.step_plan(spec.S)["grad"] == "csr"
    eng.train_step(b)
    uk = eng.native.unique_keys()
    off, cnt, words = eng.native.csr_debug()
    geom = eng.native.red_geometry(spec.S)
    assert eng.csr_steps == 1 and not eng.overflowed()
    assert geom["nuq"] == len(uk) and geom["shift"] == pre["shift"]
    return dict(uk=uk, off=off, cnt=cnt, words=words, geom=geom, W=W)


def _check_structure(spec, name, r):
    """cnt, slice ids, ranges; returns (device entries, expected entries), both
    in ascending-key order."""
    kind = MODELS[name][2]
    P = MODELS[name][0].params_per_key
    exp = csr_ref.expected_structure(spec.keys, spec.row_ptr, spec.slice_rows, spec.S)
    uk = np.asarray(r["uk"], dtype=np.uint64)
    np.testing.assert_array_equal(np.sort(uk), exp.ukeys)
    asc = np.argsort(uk)          # device index of the i-th smallest key
    cnt = np.asarray(r["cnt"], dtype=np.int64)
    np.testing.assert_array_equal(cnt[asc], exp.cnt, err_msg="cnt")
    ew = csr_ref.entry_words(kind, P)
    assert csr_ref.ranges_disjoint(r["off"], cnt, len(r["words"]) // ew)
    got = csr_ref.decode(kind, P, r["off"], cnt, r["words"])
    key_of = np.repeat(np.arange(len(cnt)), cnt)
    assert ((np.diff(got.slices) > 0) | (np.diff(key_of) != 0)).all(), "slice ids ascend strictly"
    got = got.by_key(asc)
    np.testing.assert_array_equal(got.slices, exp.slices, err_msg="slice ids")
    assert int(cnt.sum()) == len(exp.slices)
    return got, exp


def _windows(spec, r, win_log2):
    """Per (bucket, window) of the step: distinct dests and occurrences, from
    the step's own unique order.  Records of a window lie between the two (a
    record is a workgroup's partial sum of one dest)."""
    sl = int(np.ceil(np.log2(spec.S)))
    uk = np.asarray(r["uk"], dtype=np.uint64)
    order = np.argsort(uk)
    idx = order[np.searchsorted(uk[order], spec.keys)].astype(np.int64)
    row_of = np.repeat(np.arange(spec.rows), np.diff(spec.row_ptr))
    dest = (idx << sl) | np.minimum(row_of // spec.slice_rows, spec.S - 1)
    shift = r["geom"]["shift"]
    w = min(shift, win_log2)
    occ = np.bincount(dest >> w)
    dis = np.bincount(np.unique(dest) >> w, minlength=len(occ))
    bocc = np.bincount(dest >> shift)
    bdis = np.bincount(np.unique(dest) >> shift, minlength=len(bocc))
    return dict(sl=sl, shift=shift, occ=occ, dis=dis, bocc=bocc, bdis=bdis)


def _branches(spec, r):
    """Branches of k_red_csr the step certainly reached."""
    w = _windows(spec, r, CSR_WIN)
    out = set()
    if w["shift"] > CSR_WIN:
        out.add("multi_window")
    if w["shift"] <= CSR_WIN and ((w["bocc"] > 0) & (w["bocc"] <= CSR_REG)).any():
        out.add("reg")
    if (w["bdis"] > CSR_REG).any() or w["shift"] > CSR_WIN:
        out.add("not_reg")
    if ((w["occ"] > 0) & (w["occ"] <= CSR_HASH // 2)).any():
        out.add("hash")
    if (w["dis"] > CSR_HASH // 2).any():
        out.add("direct")
    if w["sl"] >= 5:
        out.add("words")
    if w["shift"] > CSR_WIN:      # a bucket with records in two of its windows
        per = np.bincount(np.nonzero(w["occ"])[0] >> (w["shift"] - CSR_WIN))
        if (per >= 2).any():
            out.add("two_live_windows")
    if ((w["occ"] == CSR_HASH // 2) & (w["dis"] == CSR_HASH // 2)).any():
        out.add("exactly_half")
    if w["sl"] == w["shift"] and (w["bdis"] == 1 << w["shift"]).any():
        out.add("full_key")
    if r["geom"]["nuq"] % max(1, (1 << min(w["shift"], CSR_WIN)) >> w["sl"]) != 0:
        out.add("nuq_break")
    return out


# ---- CPU: the helper against ref64 ------------------------------------------------
def _helper_vs_ref64(keys, row_ptr, fgid, labels, rows, S):
    sr = -(-rows // S)
    uk = np.unique(keys)
    ref = ref64.reference("lr", 0, uk, np.zeros((len(uk), 1), np.float32), keys, row_ptr, fgid, labels, sr)
    assert len(ref.slice_rows) == S
    exp = csr_ref.expected_structure(keys, row_ptr, sr, S)
    np.testing.assert_array_equal(exp.ukeys, uk)
    np.testing.assert_array_equal(exp.cnt, ref.touched.sum(1))
    ui, si = np.nonzero(ref.touched)
    np.testing.assert_array_equal(exp.slices, si)
    lr = csr_ref.expected_lr_fresh(keys, row_ptr, labels, sr, S)
    np.testing.assert_array_equal(lr.slices, si)
    # p = 0.5 exactly: ref64's float64 gradient rounds to the same float32
    np.testing.assert_array_equal(lr.values[:, 0], ref.g[ui, si, 0].astype(np.float32))
    np.testing.assert_array_equal(csr_ref.slice_sizes(rows, sr, S), ref.slice_rows)
    # decode reads back what an encoder of the documented formats wrote, from
    # scattered offsets
    rng = np.random.default_rng(0)
    perm = rng.permutation(len(uk))
    off = np.zeros(len(uk), np.int64)
    off[perm] = np.cumsum(exp.cnt[perm]) - exp.cnt[perm] + 3
    for kind, P in (("lr", 1), ("fm_ref", 5), ("rows", 5)):
        ew = csr_ref.entry_words(kind, P)
        nv = {"lr": 1, "fm_ref": 2}.get(kind, P)
        vals = rng.standard_normal((len(si), nv)).astype(np.float32)
        words = np.full((int(exp.cnt.sum()) + 3, ew), 0xA5A5A5A5, np.uint32)
        at = np.repeat(off - exp.start, exp.cnt) + np.arange(len(si))
        words[at, 0] = si
        words[at, 1:1 + nv] = vals.view(np.uint32)
        d = csr_ref.decode(kind, P, off, exp.cnt, words.reshape(-1))
        np.testing.assert_array_equal(d.slices, si)
        np.testing.assert_array_equal(d.bits, vals.view(np.uint32))
        assert csr_ref.ranges_disjoint(off, exp.cnt, len(words))
        assert not csr_ref.ranges_disjoint(np.where(np.arange(len(off)) == perm[1], off[perm[0]], off),
                                           exp.cnt, len(words))
    sl, g, err = csr_ref.from_ref64(ref)
    np.testing.assert_array_equal(sl, si)
    np.testing.assert_array_equal(g, ref.g[ui, si])


def test_helper_agrees_with_ref64_on_the_65_row_case():
    c = trs.CASES["interleaved65"]
    _helper_vs_ref64(c.keys, c.row_ptr, c.fgid, c.labels, c.rows, 8)


def test_helper_agrees_with_ref64_on_a_random_csr_batch():
    from helpers import random_csr
    k, rp, fg, lab = random_csr(500, fields=8, vocab=300, seed=4)
    _helper_vs_ref64(k, rp, fg, lab, 500, 8)


def test_expected_structure_at_the_large_shape():
    s = distinct(32768, 39, 256)   # 1.28 M occurrences: no per-occurrence Python
    e = csr_ref.expected_structure(s.keys, s.row_ptr, s.slice_rows, s.S)
    assert len(e.ukeys) == 32768 * 39 and (e.cnt == 1).all()


# ---- 1. entries of the fused step ---------------------------------------------------
# name -> (spec builder, max_nnz or None, branches the case is built for)
LR_CASES = {
    "S8": (lambda: mixed(8), None, {"reg", "hash", "nuq_break"}),
    "S16": (lambda: mixed(16), None, {"reg", "hash", "nuq_break"}),
    "S32_words": (lambda: mixed(32, per=8), None, {"reg", "hash", "words"}),
    "S9_padded": (lambda: mixed(9), None, {"reg", "hash"}),
    "S33_padded": (lambda: mixed(33, per=8), None, {"reg", "hash", "words"}),
    # one full bucket of 16 384 dests and as many records: direct-indexed sub-windows
    "S256_64keys_every_slice": (lambda: every_slice(256, 64), None, {"not_reg", "direct", "words"}),
    # 256 buckets of 64 records; 2^22 dests over a scratch of 2^16 slots (FITS)
    "S256_distinct_2048x8": (lambda: distinct(2048, 8, 256), None, {"reg", "hash", "words"}),
    # ~1.28 M unique keys, 3.3e8 dests: shift 17, two windows of 2^16 a bucket, both with records
    "S256_distinct_32768x39": (lambda: distinct(32768, 39, 256), None,
                               {"multi_window", "two_live_windows", "not_reg", "hash"}),
    # exactly kCsrHash / 2 = 2048 records and dests in the one window: the last
    # count that takes the hash table (nwin <= kCsrHash / 2), at load 0.5
    "S8_2048_dests": (lambda: every_slice(8, 256), None, {"reg", "hash", "exactly_half"}),
    # the largest S the plan accepts for LR: 2^14 slices of one row each
    # (sl == red_shift(1)); the key in every row fills a whole bucket
    "S16384_one_row_slices": (lambda: one_row_slices(1 << 14), None, {"not_reg", "direct", "words", "full_key"}),
}

_FUSED = {}


def _fused_once(dev, name, case, builder, max_nnz, plant=False):
    key = (name, case)
    if key not in _FUSED:
        spec = builder()
        _FUSED[key] = (spec, _fused(dev, name, spec, max_nnz, plant))
    return _FUSED[key]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(LR_CASES))
def test_lr_fresh_entries_exact(gpu_device, case):
    builder, max_nnz, want = LR_CASES[case]
    spec, r = _fused_once(gpu_device, "lr", case, builder, max_nnz)
    got, exp = _check_structure(spec, "lr", r)
    reached = _branches(spec, r)
    print(case, r["geom"], sorted(reached))
    assert want <= reached, (want, reached, r["geom"])
    lr = csr_ref.expected_lr_fresh(spec.keys, spec.row_ptr, spec.labels, spec.slice_rows, spec.S)
    np.testing.assert_array_equal(lr.slices, got.slices)
    bad = np.nonzero(got.bits[:, 0] != lr.bits[:, 0])[0]
    assert len(bad) == 0, (len(bad), got.values[bad[:4], 0], lr.values[bad[:4], 0])
    # determinism: a second fresh engine, compared per key
    again = _fused(gpu_device, "lr", spec, max_nnz)
    got2, _ = _check_structure(spec, "lr", again)
    np.testing.assert_array_equal(got2.bits, got.bits)


def _vec_chunk(P_nv):
    return min(120 * 1024 // (8 * P_nv), 2048) & ~63


FM_SHAPES = {
    "S8_1024x8": lambda: mixed(8, per=128, F=8, vocab=3000, seed=7),
    "S8_1024keys_every_slice": lambda: every_slice(8, 1024),
    "S8_interleaved65": lambda: _case_spec(trs.CASES["interleaved65"], 8),
    "S64_words": lambda: mixed(64, per=16, F=8, vocab=500, seed=8),
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(FM_SHAPES))
@pytest.mark.parametrize("name", ["fm_ref", "fm_std4", "fm_std8"])
def test_fm_entries_within_the_ref64_bound(gpu_device, name, shape):
    m = MODELS[name][0]
    spec, r = _fused_once(gpu_device, name, shape, FM_SHAPES[shape], None, plant=True)
    got, exp = _check_structure(spec, name, r)
    if shape == "S8_1024keys_every_slice":
        if name == "fm_ref":   # 8192 records in one bucket: not the register form
            assert {"not_reg", "direct"} <= _branches(spec, r), r["geom"]
        else:                  # 8192 distinct dests in one window: several rank chunks
            w = _windows(spec, r, VEC_WIN)
            assert w["dis"].max() > _vec_chunk(1 + m.v_dim), (w["dis"].max(), r["geom"])
    if shape == "S64_words":
        assert int(np.ceil(np.log2(spec.S))) >= 5
    ref = ref64.reference("fm", m.v_dim, spec.ukeys, r["W"], spec.keys, spec.row_ptr, spec.fgid,
                          spec.labels, spec.slice_rows, m.fm_math)
    assert len(ref.slice_rows) == spec.S
    if name == "fm_ref":
        want, bound = csr_ref.fm_ref_bc(ref, r["W"], spec.keys, spec.row_ptr, spec.labels,
                                        spec.slice_rows, spec.S)
    else:
        sl, want, eg = csr_ref.from_ref64(ref)
        np.testing.assert_array_equal(sl, exp.slices)
        bound = eg + csr_ref.quantisation_fm_std(ref, r["W"], spec.keys, spec.row_ptr, spec.labels,
                                                 spec.slice_rows, spec.S)
    err = np.abs(got.values.astype(np.float64) - want)
    assert np.isfinite(got.values).all() and np.abs(got.values).max() > 0
    ratio = trs.worst_ratio(err, bound)
    trs.note_ratio("csr_entry", "gpu", m, ratio)
    assert ratio <= 1.0, (name, shape, ratio)
    again = _fused(gpu_device, name, spec, None, plant=True)
    got2, _ = _check_structure(spec, name, again)
    np.testing.assert_array_equal(got2.bits, got.bits)


def _mvm_spec(shape, dup):
    s = FM_SHAPES[shape]()
    if dup:   # columns 0 and 1 share field 0 (fields 0 .. F - 2 all present): the
        # k_mdup_* passes add to entries
        fg = np.tile(np.maximum(np.arange(s.F, dtype=np.int32) - 1, 0), (s.rows, 1))
        s.fgid = fg.reshape(-1)
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dup", [("S8_1024x8", False), ("S8_1024keys_every_slice", False),
                                       ("S8_1024keys_every_slice", True)])
def test_mvm_entries_within_the_ref64_bound(gpu_device, shape, dup):
    """Fresh latents under SGD with sgd_v_init = 0.9 (read by a lookup before
    the step): field sums 0.9 or 1.8, away from -1.  Values against ref64's g
    within e_g plus csr_ref.quantisation_mvm; the same bits per key on a
    second engine."""
    m = MODELS["mvm"][0]
    spec = _mvm_spec(shape, dup)
    r = _fused(gpu_device, "mvm", spec)
    got, exp = _check_structure(spec, "mvm", r)
    assert (r["W"] > 0).all()
    ref = ref64.reference("mvm", m.v_dim, spec.ukeys, r["W"], spec.keys, spec.row_ptr, spec.fgid,
                          spec.labels, spec.slice_rows, mvm_math=m.mvm_math)
    sl, want, eg = csr_ref.from_ref64(ref)
    np.testing.assert_array_equal(sl, exp.slices)
    bound = eg + csr_ref.quantisation_mvm(ref, r["W"], spec.keys, spec.row_ptr, spec.labels,
                                          spec.slice_rows, spec.S)
    assert np.isfinite(got.values).all() and np.abs(want).max() > 0
    ratio = trs.worst_ratio(np.abs(got.values.astype(np.float64) - want), bound)
    trs.note_ratio("csr_entry" + ("_dup" if dup else ""), "gpu", m, ratio)
    assert ratio <= 1.0, (shape, dup, ratio)
    got2, _ = _check_structure(spec, "mvm", _fused(gpu_device, "mvm", spec))
    np.testing.assert_array_equal(got2.bits, got.bits)


@pytest.mark.gpu
def test_fm_std_multi_window_zero_weights_exact(gpu_device):
    """32 768 x 39 distinct keys, S = 256, every weight imported as zero, SGD:
    p = 0.5, g_w = sum(0.5 - label) / rows exactly, every g_v = 0."""
    spec = distinct(32768, 39, 256, tag=6)
    eng = _engine(gpu_device, "fm_std4", spec)
    P = 5
    words = np.zeros((len(spec.ukeys), eng.state_words), dtype=np.uint32)
    words[:, P] = 1
    eng.import_table(spec.ukeys, words.reshape(-1))
    pre = eng.native.red_geometry(spec.S, len(spec.ukeys))
    assert pre["needed"] <= pre["nb"], FITS.format(**pre)
    eng.train_step(spec.batch(gpu_device))
    off, cnt, w = eng.native.csr_debug()
    r = dict(uk=eng.native.unique_keys(), off=off, cnt=cnt, words=w, geom=eng.native.red_geometry(spec.S))
    got, exp = _check_structure(spec, "fm_std4", r)
    print(r["geom"])
    # (the vector records' larger bucket cap keeps the shift at VEC_WIN + 1
    # here: two windows of 2^15 a bucket)
    assert r["geom"]["shift"] > VEC_WIN, r["geom"]
    lr = csr_ref.expected_lr_fresh(spec.keys, spec.row_ptr, spec.labels, spec.slice_rows, spec.S)
    np.testing.assert_array_equal(got.bits[:, 0], lr.bits[:, 0])
    assert (got.bits[:, 1:] == 0).all()


# ---- 2. the wire form ------------------------------------------------------------------
def _wire(dev, name, spec, world, seq, max_nnz, plant):
    eng = _engine(dev, name, spec, max_nnz)
    if plant:
        _plant(eng, name, spec.ukeys)
    b = spec.batch(dev)
    nnz = max(len(spec.keys), 1)
    counts = torch.zeros(world, dtype=torch.int64, device=dev)
    send = torch.zeros(nnz, dtype=torch.int64, device=dev)
    eng.w_prepare(b, world, counts, send, seq=seq)
    c = counts.cpu().numpy()
    if seq >= 0 and world > 1:
        assert ((c >> 40) == seq).all(), "counts carry the sequence number"
        c = (c & ((1 << 40) - 1)) - 1
    n = int(c.sum())
    skeys = send.cpu().numpy().view(np.uint64)[:n]
    plain = torch.from_numpy(np.ascontiguousarray(c)).to(dev)
    vals = torch.zeros(max(n, 1), eng.value_width, dtype=torch.float32, device=dev)
    eng.s_pull(send, n, vals, insert=True, buf=0, offsets=[0, n], keep_weights=True)
    eb = int(eng.native.csr_entry_bytes)
    pad = 64
    cnt = torch.full((n + pad,), -1515870811, dtype=torch.int32, device=dev)     # 0xA5A5A5A5
    ent = torch.full(((nnz + pad) * eb,), 0xA5, dtype=torch.uint8, device=dev)
    tot = torch.full((world,), -7, dtype=torch.int64, device=dev)
    eng._sync_stream()
    eng.native.w_forward_backward_csr(b.view(), vals.data_ptr(), n, spec.S, 0, cnt.data_ptr(),
                                      ent.data_ptr(), plain.data_ptr(), world, tot.data_ptr())
    eng.native.s_apply_csr(send.data_ptr(), cnt.data_ptr(), ent.data_ptr(), [0, n], spec.S, 0)
    eng.w_finish()
    assert not eng.overflowed()
    return dict(c=c, skeys=skeys, n=n, cnt=cnt.cpu().numpy().view(np.uint32),
                ent=ent.cpu().numpy(), tot=tot.cpu().numpy(), eb=eb, eng=eng)


def _check_wire(spec, name, world, w, fused):
    kind = MODELS[name][2]
    P = MODELS[name][0].params_per_key
    n, skeys = w["n"], w["skeys"]
    np.testing.assert_array_equal(np.sort(skeys), spec.ukeys, err_msg="send keys")
    own = owner_of(skeys, world)
    assert (np.diff(own) >= 0).all(), "owners ascend along the send order"
    np.testing.assert_array_equal(w["c"], np.bincount(own, minlength=world), err_msg="counts")
    exp = csr_ref.expected_structure(spec.keys, spec.row_ptr, spec.slice_rows, spec.S)
    asc = np.argsort(skeys)
    cnt = w["cnt"][:n].astype(np.int64)
    np.testing.assert_array_equal(cnt[asc], exp.cnt, err_msg="cnt_out")
    assert (w["cnt"][n:] == 0xA5A5A5A5).all(), "cnt_out written past n_send"
    total = int(cnt.sum())
    assert (w["ent"][total * w["eb"]:] == 0xA5).all(), "entries written past the packed total"
    doff = np.cumsum(cnt) - cnt
    got = csr_ref.decode(kind, P, doff, cnt, w["ent"][:total * w["eb"]].view(np.uint32)).by_key(asc)
    np.testing.assert_array_equal(got.slices, exp.slices)
    np.testing.assert_array_equal(w["tot"], np.bincount(own, weights=cnt, minlength=world).astype(np.int64),
                                  err_msg="totals")
    np.testing.assert_array_equal(got.bits, fused.bits, err_msg="packed entries vs the fused step's")
    return got


WIRE_SPECS = {
    "lr": lambda: mixed(8, per=64, F=6, vocab=1500, seed=21),
    "fm_ref": lambda: mixed(8, per=64, F=6, vocab=1500, seed=22),
    "fm_std4": lambda: mixed(8, per=64, F=6, vocab=1500, seed=23),
    "mvm": lambda: mixed(8, per=64, F=6, vocab=1500, seed=24),
}
_WIRE_FUSED = {}


@pytest.mark.gpu
@pytest.mark.parametrize("seq", [-1, 5])
@pytest.mark.parametrize("world", [1, 2, 3, 8, 256])
@pytest.mark.parametrize("name", list(WIRE_SPECS))
def test_wire_form(gpu_device, name, world, seq):
    """Every world here takes the owner-partitioned dedup (partition_counts),
    the GPU's only way to group keys by owner: w_prepare uses it for 1 to
    kMaxParts = 1024 owners and refuses any other world before it launches
    anything (test_w_prepare_refuses_world_outside_parts)."""
    plant = name.startswith("fm")
    if name not in _WIRE_FUSED:
        spec = WIRE_SPECS[name]()
        _WIRE_FUSED[name] = (spec, _check_structure(spec, name, _fused(gpu_device, name, spec, None, plant))[0])
    spec, fused = _WIRE_FUSED[name]
    w = _wire(gpu_device, name, spec, world, seq, None, plant)
    if world >= 8:
        assert world < 256 or (w["c"] == 0).any(), "an owner without keys"
    _check_wire(spec, name, world, w, fused)


@pytest.mark.gpu
def test_w_prepare_refuses_world_outside_parts(gpu_device):
    """world = 1025 (> kMaxParts) and world = 0 are host-side argument errors,
    raised before any launch: the same engine then prepares the batch for 256
    owners.  (max_nnz is the wire cases': every owner needs slots of its own in
    the dedup scratch, which is sized by max_nnz.)"""
    keys = _vocab(16, 40)[np.array([[0, 1], [2, 3], [4, 5], [6, 7], [0, 2], [1, 3], [8, 9], [8, 8]])]
    spec = Spec(keys, 1, 8, 41)
    eng = _engine(gpu_device, "lr", spec, max_nnz=8 * 64 * 6)
    b = spec.batch(gpu_device)
    counts = torch.zeros(1025, dtype=torch.int64, device=gpu_device)
    send = torch.zeros(len(spec.keys), dtype=torch.int64, device=gpu_device)
    with pytest.raises(RuntimeError, match="1024"):
        eng.w_prepare(b, 1025, counts, send)
    with pytest.raises(RuntimeError):
        eng.w_prepare(b, 0, counts, send)
    eng.w_prepare(b, 256, counts, send)
    c = counts.cpu().numpy()[:256]
    assert int(c.sum()) == eng.n_unique() == len(spec.ukeys)
    skeys = send.cpu().numpy().view(np.uint64)[:int(c.sum())]
    assert set(skeys.tolist()) == set(spec.ukeys.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("nuq,big", [(4095, False), (4096, False), (4097, False), (4095, True),
                                     (4096, True), (4097, True), (20480, True)])
def test_wire_scan_paths(gpu_device, nuq, big):
    """max_nnz <= 16 384: k_scan_one; above: k_scan_tiles / k_scan_top /
    k_scan_write with the device-side unique count -- 20 480 = 5 x 4 096 is
    k_scan_write's t0 == n branch."""
    v = _vocab(nuq, 30)
    rows = -(-nuq // 32) * 8              # every key in each half (some twice), 8 whole slices
    k = np.resize(v, (rows // 2, 8))
    spec = Spec(np.concatenate([k, k[::-1]]), 8, rows // 8, 31)
    assert len(spec.ukeys) == nuq
    max_nnz = max(len(spec.keys), 1 << 15) if big else len(spec.keys)
    assert (max_nnz > SCAN_ONE) == big
    fused = _check_structure(spec, "lr", _fused(gpu_device, "lr", spec, max_nnz))[0]
    lr = csr_ref.expected_lr_fresh(spec.keys, spec.row_ptr, spec.labels, spec.slice_rows, spec.S)
    np.testing.assert_array_equal(fused.bits, lr.bits)
    for world in (1, 3):
        _check_wire(spec, "lr", world, _wire(gpu_device, "lr", spec, world, -1, max_nnz, False), fused)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 3])
def test_wire_empty_batch(gpu_device, world):
    spec = mixed(8)
    eng = _engine(gpu_device, "lr", spec)
    dev = gpu_device
    b = Batch(keys=torch.zeros(0, dtype=torch.int64, device=dev), labels=torch.zeros(0, device=dev),
              row_ptr=torch.zeros(1, dtype=torch.int32, device=dev),
              fgid=torch.zeros(0, dtype=torch.int32, device=dev), slice_rows=12)
    counts = torch.full((world,), 9, dtype=torch.int64, device=dev)
    send = torch.zeros(8, dtype=torch.int64, device=dev)
    eng.w_prepare(b, world, counts, send)
    assert (counts.cpu().numpy() == -1).all()     # a rank out of data
    vals = torch.zeros(1, eng.value_width, device=dev)
    eng.s_pull(send, 0, vals, insert=True, buf=0, offsets=[0, 0])
    cnt = torch.full((64,), -1515870811, dtype=torch.int32, device=dev)
    ent = torch.full((1024,), 0xA5, dtype=torch.uint8, device=dev)
    tot = torch.full((world,), -7, dtype=torch.int64, device=dev)
    eng._sync_stream()
    eng.native.w_forward_backward_csr(b.view(), vals.data_ptr(), 0, 8, 0, cnt.data_ptr(), ent.data_ptr(),
                                      counts.data_ptr(), world, tot.data_ptr())
    eng.w_finish()
    assert (tot.cpu().numpy() == 0).all()
    assert (cnt.cpu().numpy().view(np.uint32) == 0xA5A5A5A5).all() and (ent.cpu().numpy() == 0xA5).all()
    assert eng.table_size() == 0


# ---- 3. the receive scan -------------------------------------------------------------------
def _receive(dev, n, offsets, cmax=3, sample=None):
    """n distinct keys with cnt in {1..cmax}, ascending slices, dyadic values
    that differ per (i, j); s_pull + s_apply_csr on a fresh LR-FTRL engine; the
    exported (n, z) of `sample` (all keys if None) against apply_ref."""
    rng = np.random.default_rng(n)
    keys = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(1)
    cnt = rng.integers(1, cmax + 1, size=n).astype(np.int64)
    assert cmax == 1 or len(np.unique(cnt)) > 1 or n == 1
    start = np.cumsum(cnt) - cnt
    tot = int(cnt.sum())
    i_of = np.repeat(np.arange(n), cnt)
    j_of = np.arange(tot) - start[i_of]
    # multiples of 2^-10 in (0, 1): (i mod 251 + 1) * 4 + j + 1 over 1024
    val = (((i_of % 251 + 1) * 4 + j_of + 1).astype(np.float32) / np.float32(1024.0)).astype(np.float32)
    val[i_of % 2 == 1] *= np.float32(-1.0)
    ent = np.zeros((tot + 4, 2), np.uint32)
    ent[:tot, 0] = j_of * 2 + (i_of % 2)          # ascending slice ids below 8
    ent[:tot, 1] = val.view(np.uint32)
    S = 8
    log2 = max(12, int(np.ceil(np.log2(n * 2))))
    eng = Engine(ModelConfig(kind="lr"), OptimConfig(kind="ftrl"),
                 EngineConfig(table_log2_cap=log2, max_rows=64, max_nnz=1024, max_slices=S), device=dev)
    kt = torch.from_numpy(keys.view(np.int64)).to(dev)
    vals = torch.zeros(n, eng.value_width, dtype=torch.float32, device=dev)
    eng.s_pull(kt, n, vals, insert=True, buf=0, offsets=offsets)
    ct = torch.from_numpy(cnt.astype(np.uint32).view(np.int32)).to(dev)
    et = torch.from_numpy(ent.view(np.int32)).to(dev)
    eng._sync_stream()
    eng.native.s_apply_csr(kt.data_ptr(), ct.data_ptr(), et.data_ptr(), [int(o) for o in offsets], S, 0)
    k, w = eng.export_table()
    assert len(k) == n and not eng.overflowed()
    w = np.asarray(w, dtype=np.uint32).reshape(n, eng.state_words)
    o = np.argsort(k)
    k, w = k[o], w[o]
    sel = np.arange(n) if sample is None else np.unique(sample)
    order = np.argsort(keys[sel])
    sk = keys[sel][order]
    L = apply_ref.Layout("lr", "ftrl")
    model = apply_ref.ApplyModel(L, OptimConfig(kind="ftrl"), sk, np.zeros((len(sk), 1), np.float32))
    idx = np.arange(len(sk))
    model.insert(idx)
    g = np.zeros((len(sk), cmax, 1), np.float32)
    src = sel[order]
    for j in range(cmax):
        has = cnt[src] > j
        g[has, j, 0] = val[start[src][has] + j]
    model.launch(idx, g=g, cnt=cnt[src])
    at = np.searchsorted(k, sk)
    np.testing.assert_array_equal(k[at], sk)
    want = model.words(idx)
    bad = np.nonzero((w[at] != want).any(1))[0]
    assert len(bad) == 0, (len(bad), src[bad[:5]], w[at][bad[:3]], want[bad[:3]])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 16383, 16384, 16385, 20480])
def test_receive_scan(gpu_device, n):
    _receive(gpu_device, n, [0, n])


@pytest.mark.gpu
@pytest.mark.parametrize("offsets", [[0, 7001, 20481], [0, 4096, 16385, 20481]])
def test_receive_scan_several_sources(gpu_device, offsets):
    """Two and three sources above 16 384 counts: entry offsets are global, so
    a source's keys index the scan at off + o."""
    _receive(gpu_device, offsets[-1], offsets)


@pytest.mark.gpu
def test_receive_scan_carries_past_1024_tiles(gpu_device):
    """4 194 304 + 4 097 counts: k_scan_top's second round of 1 024 tiles takes
    the first round's total as its carry.  cnt in {1, 2}, and the model runs on
    100 000 sampled keys: the first and last key of every 4 096-count tile from
    8 tiles before the 1 024-tile boundary to the end, the last key, and a
    fixed random rest."""
    n = 4194304 + 4097
    t0 = 1024 - 8
    edges = np.concatenate([np.arange(t0, n // SCAN_TILE + 1) * SCAN_TILE,
                            np.arange(t0, n // SCAN_TILE + 1) * SCAN_TILE + SCAN_TILE - 1, [n - 1, 0]])
    edges = edges[edges < n]
    rest = np.random.default_rng(99).choice(n, size=100000 - len(np.unique(edges)), replace=False)
    _receive(gpu_device, n, [0, n], cmax=2, sample=np.concatenate([edges, rest]))
