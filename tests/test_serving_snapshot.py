"""Serving snapshots (docs/DESIGN.md §2): the export rule against a numpy model
written here, bit-identity of pulls and predictions between a source table and
the frozen table built from its export, what a frozen engine refuses, the
files on disk, the offline conversion, the trainer's --save-serving -- and, on
the GPU, the one-launch LR kernel against the float64 reference's bound."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from conftest import DATA

from xflow_amd import checkpoint
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig, TrainConfig
from xflow_amd.engine import Batch, Engine
from xflow_amd.testing import apply_ref, hashing, ref64

F32 = np.float32
M64 = (1 << 64) - 1
DEVS = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
OPT = OptimConfig()


def _dev(request, name):
    return request.getfixturevalue("gpu_device") if name == "cuda" else torch.device("cpu")


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _frozen_of(eng, device, log2=12, **cfg):
    """A frozen engine holding import_weights(export_weights()) of eng."""
    k, w = eng.export_weights()
    o = dataclasses.replace(eng.optim, kind="frozen", frozen_from=eng.optim.kind)
    f = Engine(eng.model, o, EngineConfig(table_log2_cap=log2, **cfg), device=device)
    f.import_weights(k, w)
    return f, k, w


# ---- 1. the export rule against a numpy model ---------------------------------
def _ulp_up(x):
    return np.nextafter(F32(x), F32(np.inf)).astype(F32)


def _planted(L, optim, keys, rng, mode):
    """State words [n, W] for keys: a mixture of what the rule must tell apart
    (mode "mix"), or only droppable / only kept states."""
    n, P = len(keys), L.P
    words = np.zeros((n, L.W), np.uint32)
    st = np.zeros((n, P, L.sp), F32)
    flag = np.ones(n, np.uint32)
    l1 = F32(optim.lambda1)
    for i in range(n):
        c = {"mix": i % 6, "drop": 0, "keep": 1}[mode]
        if c == 0:      # drops: zero state, flag unset (latents read their lazy init)
            flag[i] = 0
        elif c == 1:    # kept: every param non-zero, flag set
            st[i, :, 0] = rng.uniform(0.5, 2.0, P)
            if L.ftrl:
                st[i, :, 1] = rng.choice([-1.0, 1.0], P) * rng.uniform(0.1, 1.0, P)
        elif c == 2:    # FTRL: |z| exactly lambda1 -> weight 0 (w); flag unset
            if L.ftrl:
                st[i, :, 0] = 1.0
                st[i, :, 1] = l1 if i % 2 else -l1
            flag[i] = 0
        elif c == 3:    # FTRL: |z| one ulp above lambda1 -> a tiny non-zero weight: kept
            if L.ftrl:
                st[i, :, 0] = 1.0
                st[i, :, 1] = _ulp_up(l1)
            else:
                st[i, :, 0] = F32(1e-30)
            flag[i] = 0
        elif c == 4:    # flag set, zero state: latents resolve to 0, an absent key's do not
            pass
        else:           # flag set, one non-zero latent (or w for LR)
            st[i, P - 1, 0] = 0.25 if not L.ftrl else 3.0
            if L.ftrl:
                st[i, P - 1, 1] = -0.75
    words[:, :L.sp * P] = st.reshape(n, L.sp * P).view(np.uint32)
    if L.has_flag:
        words[:, L.flag_col] = flag
    return words


def _expected(eng, L, optim, keys, words):
    """(kept keys sorted, their weight bits) by the rule, in numpy: weights by
    apply_ref's recipe, the absent key's by hashing.normal_init (the engine's
    own lazy init is held to it within 4 ulp and then used, as apply_ref does:
    logf / cosf need not agree bit for bit between numpy and the device)."""
    order = np.argsort(keys)
    keys, words = keys[order], words[order]
    P = L.P
    if len(keys) == 0:
        return keys, np.zeros((0, P), np.uint32)
    fresh = Engine(eng.model, eng.optim, EngineConfig(table_log2_cap=8, max_rows=16, max_nnz=64),
                   device=eng.device)
    lazy = apply_ref.lazy_weights(fresh, keys)
    want = np.zeros((len(keys), P), F32)
    for p in range(L.p_w, P):
        want[:, p] = (hashing.normal_init(keys, p - L.p_w, optim.seed) * F32(optim.v_init_scale)
                      if L.ftrl else F32(optim.sgd_v_init))
    ulp = np.abs(_bits(lazy).astype(np.int64) - _bits(want).astype(np.int64))
    assert ulp.max(initial=0) <= 4
    m = apply_ref.ApplyModel(L, optim, keys, lazy)
    m.plant(np.arange(len(keys)), words)
    w = m.weights()
    absent = np.where(m.latent[None, :], lazy, F32(0.0)).astype(F32)
    keep = (_bits(w) != _bits(absent)).any(axis=1)
    return keys[keep], _bits(w[keep])


RULE_CASES = [(k, o, d) for k in ("lr", "fm", "mvm") for o in ("ftrl", "sgd")
              for d in ((1, 8, 10) if k != "lr" else (1,))]


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("kind,opt,v_dim", RULE_CASES)
def test_export_rule_matches_numpy_model(request, devname, kind, opt, v_dim):
    dev = _dev(request, devname)
    model = ModelConfig(kind=kind, v_dim=v_dim)
    optim = OptimConfig(kind=opt)
    L = apply_ref.Layout(kind, opt, v_dim)
    rng = np.random.default_rng(11)
    for n, mode, log2 in ((0, "mix", 8), (1, "keep", 8), (1, "drop", 8), (5000, "mix", 11),
                          (300, "drop", 10), (300, "keep", 10)):
        eng = Engine(model, optim, EngineConfig(table_log2_cap=log2, max_rows=16, max_nnz=64),
                     device=dev)
        keys = rng.choice(1 << 40, size=n, replace=False).astype(np.uint64)
        if n >= 300:
            keys[0] = np.uint64(M64)  # stored as 2^64 - 2 (sanitize_key)
        words = _planted(L, optim, keys, rng, mode)
        eng.import_table(keys, words.reshape(-1))
        if n == 5000:  # (2^11 slots grew by segment splits)
            assert eng.table_geometry["segments"] >= 3
        skeys = hashing.sanitize_keys(keys)
        want_k, want_w = _expected(eng, L, optim, skeys, words)
        got_k, got_w = eng.export_weights()
        order = np.argsort(got_k)
        assert eng.export_weights_count() == len(want_k)
        assert np.array_equal(got_k[order], want_k)
        assert np.array_equal(_bits(got_w[order]).reshape(len(want_k), L.P), want_w)
        if mode == "drop":
            assert len(got_k) == 0
        if mode == "keep":
            assert len(got_k) == n
        if n >= 300 and mode == "keep":
            assert np.uint64(M64 - 1) in got_k and np.uint64(M64) not in got_k


def test_rule_edges_stated():
    """What the docs promise, stated: an LR key with |z| == lambda1 is dropped
    and one ulp above is kept; a pushed FM key with zero latents is kept, an
    unpushed one dropped."""
    l1 = F32(OPT.lambda1)
    eng = Engine(ModelConfig(kind="lr"), OPT, EngineConfig(table_log2_cap=8, max_rows=16, max_nnz=64))
    st = np.array([[1.0, l1], [1.0, -l1], [1.0, _ulp_up(l1)], [0.0, 0.0]], F32)
    eng.import_table(np.array([5, 6, 7, 8], np.uint64), st.view(np.uint32).reshape(-1))
    k, w = eng.export_weights()
    assert k.tolist() == [7] and w[0, 0] != 0.0
    fm = Engine(ModelConfig(kind="fm", v_dim=2), OPT,
                EngineConfig(table_log2_cap=8, max_rows=16, max_nnz=64))
    W = fm.state_words
    words = np.zeros((2, W), np.uint32)
    words[0, 6] = 1  # key 1: pushed flag set, zero state; key 2: flag unset
    fm.import_table(np.array([1, 2], np.uint64), words.reshape(-1))
    k, w = fm.export_weights()
    assert k.tolist() == [1] and not w.any()
    assert fm.pull([2])[0, 1] != 0.0  # (what the absent key reads)


# ---- 2. pull identity -----------------------------------------------------------
ROWS, SLICE = 2048, 256
MODELS = [("lr", 10, "reference"), ("fm", 8, "reference"), ("fm", 4, "standard"), ("mvm", 8, "reference")]


def _train_batch(rng, rows, F, vocab, dev):
    keys = rng.integers(1, vocab, size=rows * F).astype(np.int64)
    fg = np.tile(np.arange(F, dtype=np.int32), rows)
    return Batch(keys=torch.from_numpy(keys).to(dev),
                 labels=torch.from_numpy((rng.random(rows) < 0.3).astype(np.float32)).to(dev),
                 fgid=torch.from_numpy(fg).to(dev), nnz_per_row=F, slice_rows=SLICE)


def _eval_batches(rng, vocab, dev):
    """CSR with an empty row and a 300-entry row; fixed width 1, 39 and 64,
    row-major and field-major."""
    out = []
    lens = rng.integers(1, 12, size=40)
    lens[3], lens[17] = 0, 300
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    keys = rng.integers(1, 2 * vocab, size=int(rp[-1])).astype(np.int64)
    fg = rng.integers(0, 6, size=int(rp[-1])).astype(np.int32)
    out.append(("csr", Batch(keys=torch.from_numpy(keys).to(dev),
                             labels=torch.zeros(40, device=dev), fgid=torch.from_numpy(fg).to(dev),
                             row_ptr=torch.from_numpy(rp).to(dev))))
    for F in (1, 39, 64):
        rows = 70
        keys = rng.integers(1, 2 * vocab, size=rows * F).astype(np.int64)
        fg = np.tile(np.arange(F, dtype=np.int32) % 6, rows)
        b = Batch(keys=torch.from_numpy(keys).to(dev), labels=torch.zeros(rows, device=dev),
                  fgid=torch.from_numpy(fg).to(dev), nnz_per_row=F)
        out.append((f"row-major {F}", b))
        out.append((f"field-major {F}", b.to_field_major()))
    return out


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("opt", ["ftrl", "sgd"])
@pytest.mark.parametrize("kind,v_dim,fm_math", MODELS)
def test_pull_and_eval_identity(request, devname, kind, v_dim, fm_math, opt):
    dev = _dev(request, devname)
    model = ModelConfig(kind=kind, v_dim=v_dim, fm_math=fm_math)
    optim = OptimConfig(kind=opt, lr=0.05)
    cfg = dict(max_rows=ROWS, max_nnz=ROWS * 8, max_slices=ROWS // SLICE)
    eng = Engine(model, optim, EngineConfig(table_log2_cap=13, **cfg), device=dev)
    rng = np.random.default_rng(5)
    vocab = 3000
    for _ in range(3):
        eng.train_step(_train_batch(rng, ROWS, 8, vocab, dev))
    if eng.is_gpu:
        torch.cuda.synchronize()
    # (keys the run never pushed, present with their flag unset: dropped)
    eng.import_table(np.arange(10_000, 10_050, dtype=np.uint64),
                     np.zeros(50 * eng.state_words, np.uint32))
    frz, k, w = _frozen_of(eng, dev, log2=13, serve_fused=False, **cfg)
    allk, _ = eng.export_table()
    assert frz.frozen and not frz.serve_fused and frz.table_size() == len(k)
    dropped = np.setdiff1d(allk, k)
    assert len(dropped) >= 50 or kind == "lr"
    unseen = np.arange(1 << 50, (1 << 50) + 1000, dtype=np.uint64)
    for name, probe in (("kept", k), ("dropped", dropped), ("unseen", unseen)):
        if len(probe):
            assert np.array_equal(_bits(eng.pull(probe)), _bits(frz.pull(probe))), name
    for name, b in _eval_batches(rng, vocab, dev):
        a = eng.eval_step(b).cpu().numpy()
        c = frz.eval_step(b).cpu().numpy()
        assert np.array_equal(_bits(a), _bits(c)), name


# ---- 3. the one-launch LR kernel (GPU) ---------------------------------------------
FUSED_ROWS = 4097
_fused_cache = {}


def _fused_table():
    """Planted LR weights: 4000 ordinary keys, and keys 1..8 worth +-12 each so
    that a few of them push a logit past either sigmoid clamp."""
    rng = np.random.default_rng(23)
    keys = np.concatenate([np.arange(1, 9), np.arange(100, 4100)]).astype(np.uint64)
    w = rng.normal(0, 0.3, len(keys)).astype(F32)
    w[:4], w[4:8] = 12.0, -12.0
    return keys, w.reshape(-1, 1)


def _fused_case(layout):
    """(keys [nnz], row_ptr, ref64) of FUSED_ROWS rows, computed once."""
    if layout in _fused_cache:
        return _fused_cache[layout]
    rng = np.random.default_rng(100 + FUSED_LAYOUTS.index(layout))
    tk, tw = _fused_table()
    R = FUSED_ROWS
    if layout == "csr":
        lens = rng.integers(1, 20, size=R)
        lens[2], lens[70] = 0, 300
        lens[5], lens[6] = 7, 4  # (room for the three keys that cross a clamp)
    else:
        lens = np.full(R, int(layout.split("-")[1]))
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    # present and absent keys mixed (absent: >= 5000)
    keys = rng.integers(100, 8000, size=int(rp[-1])).astype(np.uint64)
    keys[(keys >= 4100) & (keys < 5000)] += 1000
    for r, fill in ((0, 6000), (5, 1), (6, 5)):  # only absent keys; past +30; past -30
        lo, hi = int(rp[r]), int(rp[r + 1])
        if fill == 6000:
            keys[lo:hi] = 6000 + np.arange(hi - lo)
        elif hi - lo >= 3:
            keys[lo:lo + 3] = fill + np.arange(3)
            keys[lo + 3:hi] = 6000
    uk = np.unique(keys)
    W = np.zeros((len(uk), 1), F32)
    hit = np.isin(uk, tk)
    W[hit] = tw[np.searchsorted(tk, uk[hit])]
    ref = ref64.reference("lr", 0, uk, W, keys, rp)
    _fused_cache[layout] = (keys, rp, ref)
    return _fused_cache[layout]


def _fused_batch(layout, rows, dev):
    keys, rp, ref = _fused_case(layout)
    n = int(rp[rows])
    k = keys[:n].view(np.int64)
    labels = torch.zeros(rows, device=dev)
    if layout == "csr":
        return Batch(keys=torch.from_numpy(k.copy()).to(dev), labels=labels,
                     row_ptr=torch.from_numpy(rp[:rows + 1].astype(np.int32)).to(dev))
    kind, F = layout.split("-")
    F = int(F)
    if kind == "fm":
        k = k.reshape(rows, F).T
    return Batch(keys=torch.from_numpy(np.ascontiguousarray(k).reshape(-1)).to(dev), labels=labels,
                 nnz_per_row=F, field_major=kind == "fm")


FUSED_LAYOUTS = ["csr", "rm-1", "fm-1", "rm-39", "fm-39", "rm-64", "fm-64"]


@pytest.fixture(scope="module")
def fused_engines(gpu_device):
    cfg = dict(table_log2_cap=14, max_rows=FUSED_ROWS, max_nnz=FUSED_ROWS * 64)
    o = OptimConfig(kind="frozen")
    tk, tw = _fused_table()
    out = {}
    for name, fused, fill in (("fused", True, True), ("plain", False, True), ("empty", True, False)):
        # ((0, 0): the one-launch kernel at every batch size, also where the
        # engine would pick the three launches)
        e = Engine(ModelConfig(kind="lr"), o,
                   EngineConfig(serve_fused=fused, serve_unfused_rows=(0, 0), **cfg),
                   device=gpu_device)
        if fill:
            e.import_weights(tk, tw)
        out[name] = e
    # the same weights in a table of 512-slot segments that grew by splits and
    # stopped mid-level (split > 0): table_home's two moduli, chains that wrap
    # inside a segment
    g = Engine(ModelConfig(kind="lr"), o,
               EngineConfig(serve_unfused_rows=(0, 0), grow_start=0.3, grow_load=0.6,
                            **dict(cfg, table_log2_cap=9)), device=gpu_device)
    for i in range(0, len(tk), 500):
        g.import_weights(tk[i:i + 500], tw[i:i + 500])
    geo = g.table_geometry
    assert geo["split"] > 0 and geo["segments"] >= 3 and g.table_size() == len(tk), geo
    out["grown"] = g
    assert out["fused"].serve_fused and not out["plain"].serve_fused
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("layout", FUSED_LAYOUTS)
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257, 4097])
def test_fused_lr_within_the_reference_bound(gpu_device, fused_engines, rows, layout):
    _, rp, ref = _fused_case(layout)
    b = _fused_batch(layout, rows, gpu_device)
    p1 = fused_engines["fused"].eval_step(b).cpu().numpy()
    p2 = fused_engines["fused"].eval_step(b).cpu().numpy()
    assert np.array_equal(_bits(p1), _bits(p2))  # deterministic run to run
    err = np.abs(p1.astype(np.float64) - ref.p[:rows])
    worst = float((err / ref.e_p[:rows]).max())
    print(f"fused {layout} rows {rows}: worst error/bound {worst:.3g}")
    assert (err <= ref.e_p[:rows]).all()
    if layout != "rm-1" and layout != "fm-1" and rows > 6:
        assert ref.y[5] > 30.0 and p1[5] == 1.0          # past the upper clamp
        assert ref.y[6] < -30.0 and p1[6] == F32(1e-6)   # past the lower clamp
    assert p1[0] == 0.5                                   # a row of only absent keys
    # the unfused path on the same frozen table is within the same bound --
    # and gives the same bits: the engine may pick either path per batch size
    p3 = fused_engines["plain"].eval_step(b).cpu().numpy()
    assert (np.abs(p3.astype(np.float64) - ref.p[:rows]) <= ref.e_p[:rows]).all()
    assert np.array_equal(_bits(p1), _bits(p3))
    # a table that grew by segment splits and stands mid-level
    pg = fused_engines["grown"].eval_step(b).cpu().numpy()
    assert np.array_equal(_bits(pg), _bits(p1))
    # a table of 0 keys: every key is absent
    p0 = fused_engines["empty"].eval_step(b).cpu().numpy()
    assert (p0 == 0.5).all()


# ---- 4. refusals ---------------------------------------------------------------------
def test_frozen_engine_refuses_training_and_training_checkpoints(tmp_path):
    o = OptimConfig(kind="frozen")
    m = ModelConfig(kind="lr")
    cfg = EngineConfig(table_log2_cap=8, max_rows=16, max_nnz=64)
    f = Engine(m, o, cfg)
    f.import_weights(np.array([3], np.uint64), np.array([[0.5]], F32))
    b = Batch(keys=torch.tensor([3, 4], dtype=torch.int64), labels=torch.zeros(2), nnz_per_row=1)
    keys = torch.tensor([3], dtype=torch.int64)
    vals = torch.zeros(1, f.value_width)
    calls = {
        "train_step": lambda: f.train_step(b),
        "train_view": lambda: f.train_view(b.view()),
        "push": lambda: f.push([3], [0.1]),
        "s_pull(insert=True)": lambda: f.s_pull(keys, 1, vals, insert=True),
        "s_apply": lambda: f.s_apply(keys, torch.zeros(1), None, [0, 1], 1),
        "s_apply_csr": lambda: f.native.s_apply_csr(keys.data_ptr(), 0, 0, [0, 1], 1, 0),
        "prune": lambda: f.prune(),
        "save": lambda: f.save(str(tmp_path / "x.xftb")),
        "save_delta": lambda: f.save_delta(str(tmp_path / "d.xftb")),
        "delta_track": lambda: Engine(m, o, dataclasses.replace(cfg, delta_track=True)),
        "admit_min_count": lambda: Engine(m, o, dataclasses.replace(cfg, admit_min_count=2)),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="serving snapshot"):
            call()
    f.s_pull(keys, 1, vals, insert=False)  # (a lookup is what a snapshot is for)
    assert vals[0, 0] == 0.5 and f.pull([3, 4]).reshape(-1).tolist() == [0.5, 0.0]
    with pytest.raises(RuntimeError, match="frozen"):
        Engine(m, OPT, cfg).import_weights(np.array([3], np.uint64), np.array([[0.5]], F32))


# ---- 5. disk and surface ------------------------------------------------------------------
def _small_source(kind="fm"):
    model = ModelConfig(kind=kind, v_dim=4)
    eng = Engine(model, OptimConfig(), EngineConfig(table_log2_cap=13, max_rows=512, max_nnz=4096,
                                                    max_slices=2))
    rng = np.random.default_rng(2)
    for _ in range(3):
        keys = rng.integers(1, 1500, size=512 * 8).astype(np.int64)
        eng.train_step(Batch(keys=torch.from_numpy(keys),
                             labels=torch.from_numpy((rng.random(512) < 0.4).astype(np.float32)),
                             fgid=torch.from_numpy(np.tile(np.arange(8, dtype=np.int32), 512)),
                             nnz_per_row=8, slice_rows=256))
    eng.import_table(np.arange(50_000, 50_040, dtype=np.uint64),
                     np.zeros(40 * eng.state_words, np.uint32))
    return eng


@pytest.mark.parametrize("world", [1, 3])
def test_save_serving_loads_into_one_predictor(tmp_path, world):
    from xflow_amd.serve import Predictor

    src = _small_source()
    allk, allw = src.export_table()
    allw = allw.reshape(len(allk), -1)
    out = str(tmp_path / "snap")
    for r in reversed(range(world)):  # (rank 0 last: it writes meta.json)
        part = Engine(src.model, src.optim, EngineConfig(table_log2_cap=13, max_rows=16, max_nnz=64))
        mine = hashing.owner_of(allk, world) == r
        part.import_table(allk[mine], allw[mine].reshape(-1))
        checkpoint.save_serving(part, out, r, world, meta={"epoch": 3}, barrier=lambda: None)
    meta = checkpoint.load_meta(out)
    k, w = src.export_weights()
    assert meta["kind"] == "serving" and meta["world"] == world and meta["epoch"] == 3
    assert meta["keys_total"] == len(allk) and meta["keys_kept"] == len(k) < len(allk)
    assert meta["optim"]["kind"] == "ftrl"
    hdr, fk, fw = checkpoint.read_serving(os.path.join(out, checkpoint.serving_name(0, world)))
    assert hdr[:6] == (1, 4, 0, 0, 5, 0) and fw.shape == (len(fk), 5)
    p = Predictor(out, device=torch.device("cpu"), max_rows=64)
    assert p.snapshot and p.engine.frozen and p.keys == len(k)
    assert p.engine.table_capacity >= 2 * len(k)
    probe = np.concatenate([allk, np.arange(1 << 45, (1 << 45) + 100, dtype=np.uint64)])
    assert np.array_equal(_bits(p.engine.pull(probe)), _bits(src.pull(probe)))
    # not a checkpoint to resume from
    with pytest.raises(ValueError, match="serving snapshot"):
        checkpoint.load(src, out, 0, 1)
    with pytest.raises(ValueError, match="serving snapshot"):
        checkpoint.check_compatible(src, meta)


def _train_cfg(out, kind, **kw):
    return TrainConfig(train_prefix=os.path.join(DATA, "small_train"),
                       test_prefix=os.path.join(DATA, "small_test"), epochs=3, threads=8,
                       pred_dir=str(out), write_pred=False, model=ModelConfig(kind=kind, v_dim=4),
                       engine=EngineConfig(table_log2_cap=14), **kw)


def _test_text():
    with open(os.path.join(DATA, "small_test-00000"), "rb") as f:
        return f.read()


def _snapshot_pairs(d):
    ks, ws = [], []
    for p in checkpoint.serving_files(d):
        _, k, w = checkpoint.read_serving(p)
        ks.append(k)
        ws.append(w)
    k, w = np.concatenate(ks), np.concatenate(ws)
    order = np.argsort(k)
    return k[order], _bits(w[order])


def test_serve_export_from_a_full_version_and_a_delta_tip(tmp_path):
    from xflow_amd import serve
    from xflow_amd.trainer import Trainer

    root = tmp_path / "root"
    t = Trainer(_train_cfg(tmp_path, "lr", resume_dir=str(root), save_every=1, save_delta=True),
                device=torch.device("cpu"))
    try:
        t.train()
    finally:
        t.close()
    full, tip = str(root / "epoch-000001"), str(root / "epoch-000003")
    assert "delta_base" not in checkpoint.load_meta(full)
    assert checkpoint.load_meta(tip).get("delta_base")
    for name, src in (("full", full), ("tip", tip)):
        eng = Engine(ModelConfig(kind="lr", v_dim=4), OptimConfig(),
                     EngineConfig(table_log2_cap=14, max_rows=16, max_nnz=64))
        checkpoint.load(eng, src, 0, 1)
        k, w = eng.export_weights()
        order = np.argsort(k)
        got = {}
        for parts in (1, 3):
            out = str(tmp_path / f"snap-{name}-{parts}")
            assert serve.main(["export", "--checkpoint", src, "--out", out, "--parts", str(parts),
                               "--cpu"]) == 0
            assert len(checkpoint.serving_files(out)) == parts
            got[parts] = _snapshot_pairs(out)
            m = checkpoint.load_meta(out)
            assert m["keys_kept"] == len(k) and m["keys_total"] == eng.table_size()
        for parts in (1, 3):
            assert np.array_equal(got[parts][0], k[order]), (name, parts)
            assert np.array_equal(got[parts][1], _bits(w[order])), (name, parts)
    # the versioned root's retention neither counts nor deletes a snapshot
    snap = str(root / "epoch-999999")
    serve.export_snapshot(tip, snap, 1, device=torch.device("cpu"))
    checkpoint.publish(str(root), 3, keep=1)
    assert os.path.exists(os.path.join(snap, "meta.json")) and os.path.exists(tip)


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("kind", ["lr", "mvm"])
def test_trainer_save_serving_predicts_like_the_full_checkpoint(request, tmp_path, devname, kind):
    from xflow_amd.serve import Predictor
    from xflow_amd.trainer import Trainer

    dev = _dev(request, devname)
    kw = dict(crosses=[(1, 2), (3, 4, 5)], cross_field_base=40) if kind == "mvm" else {}
    cfg = _train_cfg(tmp_path, kind, checkpoint_dir=str(tmp_path / "ck"), save_every=1,
                     save_serving=str(tmp_path / "snap"), **kw)
    t = Trainer(cfg, device=dev)
    try:
        t.train()
    finally:
        t.close()
    full = Predictor(str(tmp_path / "ck"), device=dev, max_rows=64)
    # ((0, 0): on the GPU every LR batch goes through the one-launch kernel,
    # also the sizes at which the engine would pick the three launches)
    snap = Predictor(str(tmp_path / "snap"), device=dev, max_rows=64, serve_unfused_rows=(0, 0))
    assert snap.snapshot and not full.snapshot
    assert snap.crosses == full.crosses and snap.cross_field_base == full.cross_field_base
    a, b = full.predict_libffm(_test_text()), snap.predict_libffm(_test_text())
    assert a.shape == (200,)
    assert np.array_equal(_bits(a), _bits(b))
    if kind == "lr" and dev.type == "cuda":
        # (b came from the one-launch kernel: it sums a row in occurrence
        # order, as the forward does; the same bits with the switch off and
        # with the engine's own pick by batch size)
        assert snap.engine.serve_fused
        for kw in (dict(serve_fused=False), dict()):
            other = Predictor(str(tmp_path / "snap"), device=dev, max_rows=64, **kw)
            assert np.array_equal(_bits(a), _bits(other.predict_libffm(_test_text())))
    m = snap.meta
    assert m["keys_kept"] == snap.keys and m["keys_total"] == full.keys
    if kind == "lr":
        assert m["keys_kept"] < m["keys_total"]


def test_cli_flag(tmp_path):
    from xflow_amd.cli import build_parser, config_from_args

    a = build_parser().parse_args([os.path.join(DATA, "small_train"),
                                   os.path.join(DATA, "small_test"), "0", "1",
                                   "--save-serving", str(tmp_path / "s")])
    assert config_from_args(a).save_serving == str(tmp_path / "s")


def test_health_reports_the_snapshot(tmp_path):
    pytest.importorskip("fastapi")
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from xflow_amd.serve import Predictor, make_app

    src = _small_source("lr")
    checkpoint.save_serving(src, str(tmp_path / "s"), 0, 1, barrier=lambda: None)
    c = TestClient(make_app(Predictor(str(tmp_path / "s"), device=torch.device("cpu"))))
    h = c.get("/health").json()
    assert h["snapshot"] is True and h["keys"] == src.export_weights_count()
    assert json.dumps(h)


def test_native_cli_save_serving(tmp_path):
    """xflow_lr --save-serving writes the file load_serving reads: the same
    pairs as the export of the table its --save wrote."""
    import subprocess

    root = os.path.dirname(DATA)
    env = dict(os.environ, XFLOW_DEVICE="-1", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([os.path.join(root, "build", "bin", "xflow_lr"),
                        os.path.join(DATA, "small_train"), os.path.join(DATA, "small_test"), "0",
                        "3", "--threads", "8", "--save", str(tmp_path / "t.xftb"),
                        "--save-serving", str(tmp_path / "s.xfw")],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    hdr, k, w = checkpoint.read_serving(str(tmp_path / "s.xfw"))
    eng = Engine(ModelConfig(kind="lr"), OptimConfig(),
                 EngineConfig(table_log2_cap=14, max_rows=16, max_nnz=64))
    eng.load(str(tmp_path / "t.xftb"))
    ek, ew = eng.export_weights()
    assert hdr[0] == 0 and hdr[4] == 1 and hdr[5] == 0
    assert checkpoint.serving_counts(str(tmp_path / "s.xfw")) == (eng.table_size(), len(ek))
    assert 0 < len(k) < eng.table_size()
    o1, o2 = np.argsort(k), np.argsort(ek)
    assert np.array_equal(k[o1], ek[o2]) and np.array_equal(_bits(w[o1]), _bits(ew[o2]))
