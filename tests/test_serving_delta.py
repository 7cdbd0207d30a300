"""Serving deltas (docs/DESIGN.md §2): applying a delta to a frozen table against
a dict model written here (inserts, overwrites and deletions, through chains
that wrap a segment end and through segment splits), a training engine's
deltas applied round after round against its own export_weights(), and what
both ends refuse."""
import dataclasses
import functools
import os
import struct

import numpy as np
import pytest
import torch

from xflow_amd import checkpoint
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Batch, Engine
from xflow_amd.testing import hashing

F32 = np.float32
M64 = (1 << 64) - 1
DEVS = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
G = 10  # log2 of the tables' slots at birth: one segment of 2^10, the smallest a test can ask for


def _dev(request, name):
    return request.getfixturevalue("gpu_device") if name == "cuda" else torch.device("cpu")


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _frozen(case, dev, **cfg):
    kind, v_dim, math, src = case
    cfg.setdefault("max_log2_cap", 14)
    return Engine(ModelConfig(kind=kind, v_dim=v_dim, fm_math=math),
                  OptimConfig(kind="frozen", frozen_from=src),
                  EngineConfig(table_log2_cap=G, max_rows=64, max_nnz=8192, **cfg), device=dev)


def _segment(keys, geo):
    """The segment each (sanitized) key lives in (table_home, backend.h)."""
    hi = hashing.fmix64(keys) >> np.uint64(geo["seg_log2"])
    b = hi & np.uint64((1 << geo["level"]) - 1)
    b2 = hi & np.uint64((2 << geo["level"]) - 1)
    return np.where(b < np.uint64(geo["split"]), b2, b)


def _slots(eng, keys):
    """Table slot of each key (0xFFFFFFFF: not in the table), by a lookup pull."""
    t = torch.from_numpy(np.ascontiguousarray(keys).view(np.int64)).to(eng.device)
    out = torch.empty(len(keys) * eng.value_width, dtype=torch.float32, device=eng.device)
    eng.s_pull(t, len(keys), out, insert=False)
    return eng.server_slots(0)[:len(keys)].copy()


def _table(eng):
    """(sorted keys, their P weight words) of every occupied slot; the slot's
    padding words must be zero."""
    k, w = eng.export_table()
    P = eng.params_per_key
    w = w.reshape(len(k), eng.state_words)
    assert not w[:, P:].any()
    o = np.argsort(k)
    return k[o], w[o][:, :P]


class Model:
    """key -> weight bits; an entry whose bits all equal the absent bits is
    removed.  The absent bits are read with pull from an empty frozen engine."""

    def __init__(self, case, dev):
        self.d = {}
        self.empty = _frozen(case, dev)
        self.P = self.empty.params_per_key
        self.used = set()

    def absent(self, skeys):
        return _bits(self.empty.pull(skeys)).reshape(len(skeys), self.P)

    def plant(self, eng, keys, wbits):
        eng.import_weights(keys, wbits.view(F32))
        for k, w in zip(hashing.sanitize_keys(keys).tolist(), wbits):
            self.d[k] = w.copy()
            self.used.add(k)

    def apply(self, eng, keys, wbits):
        """Apply to the engine and to the dict; the engine's counts must be
        the dict's.  Returns the counts."""
        n = len(keys)
        sk = hashing.sanitize_keys(keys)
        ab = self.absent(sk) if n else np.zeros((0, self.P), np.uint32)
        gone = (wbits == ab).all(axis=1)
        want_ins = sum(int(k) not in self.d for k in sk.tolist())
        r = eng.apply_weights_delta(keys, wbits.view(F32))
        for k, w, g in zip(sk.tolist(), wbits, gone):
            self.used.add(k)
            if g:
                self.d.pop(k, None)
            else:
                self.d[k] = w.copy()
        segs = len(set(_segment(sk[gone], eng.table_geometry).tolist()))
        got = (r["inserted"], r["overwritten"], r["dropped"], r["segments_swept"])
        assert got == (want_ins, n - want_ins, int(gone.sum()), segs), (got, r)
        return got

    def check(self, eng):
        assert eng.table_size() == len(self.d)
        k, w = _table(eng)
        want_k = np.array(sorted(self.d), np.uint64)
        assert np.array_equal(k, want_k)
        if len(want_k):
            assert np.array_equal(w, np.stack([self.d[int(x)] for x in want_k]))
        # every key ever used: its bits, or what an absent key reads -- a chain
        # broken by the backward shift would lose a key here
        used = np.array(sorted(self.used), np.uint64)
        if len(used):
            got = _bits(eng.pull(used)).reshape(len(used), self.P)
            ab = self.absent(used)
            want = np.stack([self.d.get(int(x), ab[i]) for i, x in enumerate(used)])
            assert np.array_equal(got, want)


_POOL = np.arange(1, 400001, dtype=np.uint64)
_HOME = (hashing.fmix64(_POOL) & np.uint64((1 << G) - 1)).astype(np.int64)


def _cluster(lo, width, count):
    """count keys whose home in a one-segment 2^G table lies in [lo, lo + width)
    (mod 2^G): inserted together they make one cluster of >= count slots."""
    m = ((_HOME - lo) % (1 << G)) < width
    return _POOL[m][:count].copy()


LONG = _cluster(300, 3, 14)              # one long cluster
WRAP = _cluster((1 << G) - 3, 3, 12)     # a cluster that wraps the segment end


def _base_keys(rng, n):
    return rng.permutation(np.unique(rng.integers(1 << 20, 1 << 30, 2 * n).astype(np.uint64)))[:n]


def _weights(rng, n, P):
    w = rng.standard_normal((n, P)).astype(F32)
    w[w == 0] = 1.0
    return _bits(w).reshape(n, P)


def _fresh(rng, model, n):
    out = []
    while len(out) < n:
        k = int(rng.integers(1 << 20, 1 << 40))
        if k not in model.used and k not in out:
            out.append(k)
    return np.array(out, np.uint64)


def _mixed_delta(rng, model, n_new, n_over, n_del, n_ghost, must_del=()):
    """New keys, overwritten keys, keys set to the absent bits (must_del among
    them) and keys absent before and after, shuffled."""
    have = np.array(sorted(set(model.d) - set(int(k) for k in must_del)), np.uint64)
    pick = rng.permutation(len(have))
    over, dele = have[pick[:n_over]], have[pick[n_over:n_over + n_del]]
    dele = np.concatenate([dele, np.array(list(must_del), np.uint64)])
    new, ghost = _fresh(rng, model, n_new), _fresh(rng, model, n_new + n_ghost)[n_new:]
    keys = np.concatenate([new, over, dele, ghost])
    w = _weights(rng, len(keys), model.P)
    gone = np.concatenate([dele, ghost])
    if len(gone):
        w[len(new) + len(over):] = model.absent(hashing.sanitize_keys(gone))
    o = rng.permutation(len(keys))
    return keys[o], w[o]


OPTS = ("ftrl", "sgd")
CASES = ([("lr", 1, "reference", o) for o in OPTS] +
         [("fm", d, m, o) for d in (1, 8, 10) for m in ("reference", "standard") for o in OPTS] +
         [("mvm", 8, "reference", o) for o in OPTS])


def _scenario(case, dev):
    """A base at load ~0.49 and three deltas; the dict model is checked after
    each.  Returns what a second run, or the other backend, must reproduce."""
    rng = np.random.default_rng(5)
    eng, model = _frozen(case, dev), Model(case, dev)
    # (the other keys' homes keep clear of the two planted clusters)
    cand = np.unique(rng.integers(1 << 20, 1 << 30, 2000).astype(np.uint64))
    home = (hashing.fmix64(cand) & np.uint64((1 << G) - 1)).astype(np.int64)
    cand = cand[((home < 270) | (home > 330)) & (home > 30) & (home < 990)]
    base = np.concatenate([LONG, WRAP, np.array([M64], np.uint64), cand[:500 - 27]])
    w = _weights(rng, len(base), model.P)
    # (the clusters' keys one at a time: which of them sits first, in the
    # middle and last is then the same on both backends, and so is delta 1)
    model.plant(eng, base[26:], w[26:])
    for i in range(26):
        model.plant(eng, base[i:i + 1], w[i:i + 1])
    model.check(eng)
    assert eng.table_geometry["segments"] == 1 and abs(eng.table_size() / (1 << G) - 0.49) < 0.01
    trace = []
    # 1: the first, a middle and the last key of the long cluster and of the
    # one that wraps its segment leave (no split: the sweep alone moves keys)
    s = _slots(eng, np.concatenate([LONG, WRAP]))
    long_o, wrap_o = LONG[np.argsort(s[:14])], WRAP[np.argsort((s[14:].astype(np.int64) + 512) % 1024)]
    assert s[:14].max() - s[:14].min() == 13 and np.ptp((s[14:].astype(np.int64) + 512) % 1024) == 11
    assert s[14:].min() == 0 and s[14:].max() == 1023  # (it does wrap)
    must = [long_o[0], long_o[6], long_o[13], wrap_o[0], wrap_o[5], wrap_o[11]]
    k, w = _mixed_delta(rng, model, 30, 30, 24, 10, must)
    stay = np.array(sorted(set(model.d) - set(hashing.sanitize_keys(k).tolist())), np.uint64)
    before, splits = _slots(eng, stay), eng.table_splits
    c = model.apply(eng, k, w)
    model.check(eng)
    assert min(c) > 0 and eng.table_splits == splits
    assert (before != _slots(eng, stay)).any()  # a surviving key changed slot
    trace.append((c, _table(eng)))
    # 2: a delta that forces segment splits, then sweeps the split table
    k, w = _mixed_delta(rng, model, 2000, 200, 150, 100)
    c = model.apply(eng, k, w)
    model.check(eng)
    assert min(c) > 0 and eng.table_splits > splits and c[3] > 1
    trace.append((c, _table(eng)))
    # 3: the sanitized all-ones key leaves with a third of the table
    k, w = _mixed_delta(rng, model, 300, 700, 800, 50, [M64 - 1])
    c = model.apply(eng, k, w)
    model.check(eng)
    assert min(c) > 0
    trace.append((c, _table(eng)))
    # ... and a delta that empties it
    k = np.array(sorted(model.d), np.uint64)
    c = model.apply(eng, k, model.absent(k))
    model.check(eng)
    assert eng.table_size() == 0 and c[0] == 0 and c[2] == len(k)
    return trace


@functools.lru_cache(maxsize=None)
def _cpu_trace(case):
    return _scenario(case, torch.device("cpu"))


def _same_trace(a, b):
    assert len(a) == len(b)
    for (ca, (ka, wa)), (cb, (kb, wb)) in zip(a, b):
        assert ca == cb and np.array_equal(ka, kb) and np.array_equal(wa, wb)


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_apply_matches_dict_model(request, devname, case):
    """Three deltas and an emptying one against the dict; a second run -- and
    the GPU against the CPU backend -- bit for bit.  (The absent latents of an
    FTRL source are each backend's own lazy init: they never reach the table.)"""
    dev = _dev(request, devname)
    _same_trace(_scenario(case, dev), _cpu_trace(case))


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 5000])
@pytest.mark.parametrize("case", [CASES[0], CASES[7], CASES[-1]], ids=lambda c: "-".join(map(str, c)))
def test_apply_sizes(request, devname, case, n):
    """One delta of n entries on a base at load 0.49: entry i is new, an
    overwrite, a deletion or absent before and after by i % 4 (n = 1: a
    deletion)."""
    dev = _dev(request, devname)
    rng = np.random.default_rng(100 + n)
    eng, model = _frozen(case, dev), Model(case, dev)
    base = _base_keys(rng, 500)
    model.plant(eng, base, _weights(rng, 500, model.P))
    q = n // 4
    n_over, n_del = min(q, 200), min(max(q, 1), 200) if n else 0
    k, w = _mixed_delta(rng, model, q, n_over, n_del, n - q - n_over - n_del)
    assert len(k) == n
    c = model.apply(eng, k, w)
    model.check(eng)
    if n == 0:
        assert c == (0, 0, 0, 0)
    elif n == 1:
        assert c == (0, 1, 1, 1)
    else:
        assert min(c) > 0
    if n == 5000:
        assert eng.table_splits > 0


@pytest.mark.parametrize("devname", DEVS)
def test_fixed_table_refuses_at_its_bound(request, devname):
    """table_grow=False: 500 keys + 320 entries would pass 0.8 of 2^10 slots;
    the call raises and the table is bit-identical.  319 entries are taken."""
    dev = _dev(request, devname)
    case = CASES[2]
    rng = np.random.default_rng(3)
    eng, model = _frozen(case, dev, table_grow=False), Model(case, dev)
    base = _base_keys(rng, 500)
    model.plant(eng, base, _weights(rng, 500, model.P))
    before = _table(eng)
    k, w = _mixed_delta(rng, model, 200, 100, 20, 0)
    with pytest.raises(RuntimeError, match="load bound"):
        eng.apply_weights_delta(k, w.view(F32))
    after = _table(eng)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    model.check(eng)
    c = model.apply(eng, k[:319], w[:319])
    model.check(eng)
    assert eng.table_geometry["segments"] == 1 and c[0] > 0


# ---- 2. end to end: a training engine's deltas ---------------------------------
E2E = [("lr", 1, "reference", OptimConfig(kind="ftrl", lambda1=1e-3)),
       ("fm", 8, "reference", OptimConfig(kind="ftrl")),
       ("mvm", 8, "reference", OptimConfig(kind="sgd", lr=0.05, sgd_v_init=0.5))]
F, VOCAB = 8, 3000


def _batch(rng, rows, dev, vocab=VOCAB):
    keys = rng.integers(1, vocab, size=rows * F).astype(np.int64)
    fg = np.tile(np.arange(F, dtype=np.int32), rows)
    return Batch(keys=torch.from_numpy(keys).to(dev),
                 labels=torch.from_numpy((rng.random(rows) < 0.3).astype(np.float32)).to(dev),
                 fgid=torch.from_numpy(fg).to(dev), nnz_per_row=F, slice_rows=rows)


def _trainer(kind, v_dim, math, optim, dev, **cfg):
    return Engine(ModelConfig(kind=kind, v_dim=v_dim, fm_math=math), optim,
                  EngineConfig(table_log2_cap=12, max_rows=1024, max_nnz=1024 * F, delta_track=True,
                               **cfg), device=dev)


def _frozen_for(tr, dev, **cfg):
    o = dataclasses.replace(tr.optim, kind="frozen", frozen_from=tr.optim.kind)
    return Engine(tr.model, o, EngineConfig(table_log2_cap=G, max_log2_cap=16, max_rows=4100,
                                            max_nnz=4100 * F, **cfg), device=dev)


def _sorted_weights(eng):
    k, w = eng.export_weights()
    o = np.argsort(k)
    return k[o], _bits(w[o]).reshape(len(k), eng.params_per_key)


def _rounds(case, dev, fcfg, tcfg=None, check_eval=True):
    """A full snapshot into a frozen engine, then 3 rounds of {train steps,
    export_weights_delta, delta_clear, apply}.  After each the frozen table is
    the trainer's export_weights(), and scores as a frozen engine built fresh
    from it.  Returns the counts of every round summed."""
    kind, v_dim, math, optim = case
    rng = np.random.default_rng(17)
    tr = _trainer(kind, v_dim, math, optim, dev, **(tcfg or {}))
    for rows in (1024, 512):
        tr.train_step(_batch(rng, rows, dev))
    fz = _frozen_for(tr, dev, **fcfg)
    fz.import_weights(*tr.export_weights())
    tr.delta_clear()
    held = [_batch(rng, rows, dev, 2 * VOCAB) for rows in (1, 65, 4097)]
    tot = np.zeros(4, np.int64)
    for rnd in range(3):
        for rows in (256, 1024, 700)[:2 + rnd % 2]:
            tr.train_step(_batch(rng, rows, dev))
        k, w = tr.export_weights_delta()
        assert len(k) == tr.serving_delta_count() and len(set(k.tolist())) == len(k)
        k2, _ = tr.export_weights_delta()  # (nothing cleared the filter)
        assert np.array_equal(np.sort(k), np.sort(k2))
        tr.delta_clear()
        r = fz.apply_weights_delta(k, w)
        tot += [r["inserted"], r["overwritten"], r["dropped"], r["segments_swept"]]
        want_k, want_w = _sorted_weights(tr)
        got_k, got_w = _table(fz)
        assert fz.table_size() == len(want_k)
        assert np.array_equal(got_k, want_k) and np.array_equal(got_w, want_w)
        if check_eval:
            fresh = _frozen_for(tr, dev, **fcfg)
            fresh.import_weights(want_k, want_w.view(F32))
            for b in held:
                assert np.array_equal(_bits(fz.eval_step(b).cpu().numpy()),
                                      _bits(fresh.eval_step(b).cpu().numpy()))
    return tot


PATHS = [{}, {"serve_fused": True, "serve_unfused_rows": (0, 0), "serve_unfused_rows_latent": (0, 0)},
         {"serve_fused": False}]


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("path", range(3), ids=["default", "one-launch", "unfused"])
@pytest.mark.parametrize("case", E2E, ids=lambda c: f"{c[0]}-{c[3].kind}")
def test_training_deltas_track_the_trainer(request, devname, case, path):
    dev = _dev(request, devname)
    tot = _rounds(case, dev, PATHS[path])
    assert tot[0] > 0 and tot[1] > 0
    if case[0] == "lr":  # lambda1 sends keys to zero (and back): deletions happen
        assert tot[2] > 0 and tot[3] > 0


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("tcfg", [{"delta_log2": 10}, {"admit_min_count": 2, "admit_log2": 16}],
                         ids=["small-filter", "admission"])
def test_filter_cases_stay_exact(request, devname, tcfg):
    """A 2^10-bit filter marks far more keys than were touched (false
    positives re-write unchanged keys with the same bits); with admission the
    keys kept out are in neither table."""
    dev = _dev(request, devname)
    tot = _rounds(E2E[0], dev, {}, tcfg, check_eval=False)
    assert tot[0] + tot[1] > 0
    if "delta_log2" in tcfg:
        tr = _trainer("lr", 1, "reference", E2E[0][3], dev, **tcfg)
        tr.train_step(_batch(np.random.default_rng(1), 1024, dev))
        tr.delta_clear()
        tr.train_step(_batch(np.random.default_rng(2), 16, dev))
        touched = tr.n_unique()
        assert tr.serving_delta_count() > touched  # false positives are present


def test_prune_forces_a_full_serving_version(tmp_path):
    rng = np.random.default_rng(8)
    dev = torch.device("cpu")
    tr = _trainer("lr", 1, "reference", E2E[0][3], dev)
    tr.train_step(_batch(rng, 1024, dev))
    root = str(tmp_path)
    none = lambda: None
    p0 = checkpoint.save_serving(tr, os.path.join(root, "epoch-000001"), 0, 1, barrier=none)
    assert p0.endswith(".xfw")
    tr.train_step(_batch(rng, 256, dev))
    p1 = checkpoint.save_serving(tr, os.path.join(root, "epoch-000002"), 0, 1, barrier=none,
                                 delta_base="epoch-000001")
    assert p1.endswith(".xfwd") and checkpoint.load_meta(os.path.dirname(p1))["delta_base"]
    tr.train_step(_batch(rng, 256, dev))
    assert tr.prune() > 0 and tr.delta_needs_full
    p2 = checkpoint.save_serving(tr, os.path.join(root, "epoch-000003"), 0, 1, barrier=none,
                                 delta_base="epoch-000002")
    assert p2.endswith(".xfw") and "delta_base" not in checkpoint.load_meta(os.path.dirname(p2))
    # a clear the serving writer did not make: the next version is full too
    tr.train_step(_batch(rng, 256, dev))
    tr.delta_clear()
    p3 = checkpoint.save_serving(tr, os.path.join(root, "epoch-000004"), 0, 1, barrier=none,
                                 delta_base="epoch-000003")
    assert p3.endswith(".xfw")


# ---- 3. refusals -----------------------------------------------------------------
def test_refusals(tmp_path):
    dev = torch.device("cpu")
    rng = np.random.default_rng(9)
    tr = _trainer("fm", 8, "reference", OptimConfig(), dev)
    tr.train_step(_batch(rng, 256, dev))
    k, w = tr.export_weights_delta()
    with pytest.raises(RuntimeError, match="frozen"):
        tr.apply_weights_delta(k, w)
    off = Engine(tr.model, tr.optim, EngineConfig(table_log2_cap=G, max_rows=64, max_nnz=512))
    for call in (off.export_weights_delta, off.serving_delta_count,
                 lambda: off.save_serving_delta(str(tmp_path / "x.xfwd"))):
        with pytest.raises(RuntimeError, match="tracking is off"):
            call()
    fz = _frozen_for(tr, dev)
    for call in (fz.export_weights_delta, fz.serving_delta_count,
                 lambda: fz.save_serving_delta(str(tmp_path / "x.xfwd"))):
        with pytest.raises(RuntimeError, match="serving snapshot"):
            call()
    # files: a base and a delta version, then the delta's file damaged
    root = str(tmp_path / "s")
    none = lambda: None
    tr.delta_clear()
    checkpoint.save_serving(tr, os.path.join(root, "epoch-000001"), 0, 1, barrier=none)
    tr.train_step(_batch(rng, 256, dev))
    p = checkpoint.save_serving(tr, os.path.join(root, "epoch-000002"), 0, 1, barrier=none,
                                delta_base="epoch-000001")
    assert p.endswith(checkpoint.serving_delta_name(0, 1))
    good = open(p, "rb").read()
    assert good[:8] == b"XFLOWSD1"
    hdr = struct.unpack("<6i", good[8:32])
    assert hdr == (1, 8, 0, 0, 9, 0) and struct.unpack("<QQ", good[32:48])[0] == tr.table_size()
    tip = os.path.join(root, "epoch-000002")
    checkpoint.load_serving(_frozen_for(tr, dev), tip)  # (intact: loads)
    for bad, msg in ((b"XFLOWSW1" + good[8:], "not an xflow serving delta"),
                     (good[:-5], "truncated"), (good[:30], "truncated"),
                     (good[:8] + struct.pack("<6i", 1, 8, 0, 0, 9, 1) + good[32:], "does not match"),
                     (good[:8] + struct.pack("<6i", 2, 8, 0, 0, 9, 0) + good[32:], "does not match")):
        open(p, "wb").write(bad)
        with pytest.raises(ValueError, match=msg):
            checkpoint.load_serving(_frozen_for(tr, dev), tip)
    open(p, "wb").write(good)
    with pytest.raises(ValueError, match="P floats per key"):
        fz.apply_weights_delta(k, w[:, :3])
