"""One-launch scoring of frozen FM and MVM tables (k_serve_fm / k_serve_mvm,
docs/DESIGN.md §2): the contract is bit identity with the engine's own
dedup -> pull -> forward path (serve_fused=False) on the same frozen engine;
both are also held to ref64's per-row bound."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from conftest import DATA

from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig, TrainConfig
from xflow_amd.engine import Batch, Engine
from xflow_amd.testing import hashing, ref64

F32 = np.float32
ROWS = 4097
ROW_COUNTS = [1, 63, 64, 65, 257, 4097]
FM_LAYOUTS = ["csr", "rm-1", "fm-1", "rm-39", "fm-39", "rm-64", "fm-64"]
MVM_LAYOUTS = ["csr", "rm-18", "fm-18", "rm-39", "fm-39"]
LOG2 = 13  # 4008 planted keys in 8192 slots: load 0.49


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- models, tables, rows --------------------------------------------------------
# (kind, v_dim, math, frozen_from): every v_dim, both maths and both sources
# somewhere; the first of each kind runs every layout at every row count, the
# others six cases each that walk the row counts and rotate the layouts
CONFIGS = [
    ("fm", 8, "reference", "ftrl"), ("fm", 8, "standard", "ftrl"), ("fm", 8, "reference", "sgd"),
    ("fm", 1, "reference", "ftrl"), ("fm", 1, "standard", "sgd"),
    ("fm", 3, "reference", "sgd"), ("fm", 3, "standard", "ftrl"),
    ("fm", 10, "standard", "sgd"), ("fm", 10, "reference", "ftrl"),
    ("fm", 32, "reference", "sgd"), ("fm", 32, "standard", "ftrl"),
    ("mvm", 10, "compat", "sgd"), ("mvm", 10, "fixed", "ftrl"),
    ("mvm", 1, "compat", "ftrl"), ("mvm", 1, "fixed", "sgd"),
    ("mvm", 3, "fixed", "ftrl"), ("mvm", 3, "compat", "sgd"),
    ("mvm", 16, "compat", "ftrl"), ("mvm", 16, "fixed", "sgd"),
]
FULL = {("fm", 8, "reference", "ftrl"), ("mvm", 10, "compat", "sgd")}


def _cases():
    out = []
    for i, c in enumerate(CONFIGS):
        lays = FM_LAYOUTS if c[0] == "fm" else MVM_LAYOUTS
        if c in FULL:
            out += [(c, lay, rows) for lay in lays for rows in ROW_COUNTS]
            continue
        for j, rows in enumerate(ROW_COUNTS):
            lay = lays[(i + j) % len(lays)]
            if rows == 4097 and c[1] > 8:  # (the float64 reference is a Python loop per weight)
                lay = ("csr", lays[1], lays[2])[i % 3]
            out.append((c, lay, rows))
    return out


CASES = _cases()


def _model(c):
    kind, v_dim, math, _ = c
    return ModelConfig(kind=kind, v_dim=v_dim, **({"fm_math": math} if kind == "fm"
                                                  else {"mvm_math": math}))


def _optim(c):
    # an absent key's latents: N(0, 1) * 1e-2 (FTRL) or the constant (SGD) --
    # small for FM, whose reference math squares the sum of a row's latents,
    # near 1 for MVM, whose logit is a product over the row's fields
    return OptimConfig(kind="frozen", frozen_from=c[3],
                       sgd_v_init=0.003 if c[0] == "fm" else 0.9)


def _table(c):
    """4008 planted keys: 1..4 and 5..8 carry the large weights that take a
    row past either sigmoid clamp, 100..4099 ordinary ones."""
    kind, D = c[0], c[1]
    rng = np.random.default_rng(31 + D)
    keys = np.concatenate([np.arange(1, 9), np.arange(100, 4100)]).astype(np.uint64)
    if kind == "fm":
        W = rng.normal(0, 0.05, (len(keys), 1 + D)).astype(F32)
        W[:, 0] = rng.normal(0, 0.3, len(keys))
        W[:4, 0], W[4:8, 0] = 12.0, -12.0
    else:
        W = (rng.uniform(0.7, 1.3, (len(keys), D)) * rng.choice([-1.0, 1.0], (len(keys), D))).astype(F32)
        W[:4], W[4:8] = 3.0, -3.0
    return keys, W


def _fields(kind, layout, rng, R, padded=False):
    """(lens, fgid) of R rows.  MVM field ids: sorted and unique but for row 1
    (unsorted), 2 (a repeated field), 3 (a field below the maximum missing:
    p = 0.5) and 4 (a field id >= 64).

    padded (MVM at a v_dim the kernels run padded, 3 at 4): no row with an
    empty product range.  k_mvm2 starts every kernel-width component of the
    product at 1, so a 'compat' row whose largest field id is 0 -- an empty
    row, a row of field 0 alone -- scores sigmoid(4), not sigmoid(3), on the
    unfused path (measured: p = 0.98201376 against 0.95257413); the fused
    kernel has that path's bits by contract and ref64 rightly refuses both.
    The forward kernels are not this change's to alter; the rows stay out
    until they are."""
    if layout == "csr":
        lens = rng.integers(2 if padded else 1, 20, size=R)
        lens[0], lens[7], lens[70] = 5, 2 if padded else 0, 300
        lens[1:7] = 7
        if kind == "mvm":
            lens[70] = 72  # (fields 0..71: the >= 64 path on a complete row)
    else:
        lens = np.full(R, int(layout.split("-")[1]))
    if kind != "mvm":
        return lens, None
    fg = [np.arange(n, dtype=np.int32) for n in lens]
    if len(fg[1]) >= 3:
        fg[1] = fg[1][::-1].copy()
        fg[2][1:] -= 1               # 0, 0, 1, 2, ..: complete, field 0 twice
        fg[3][2:] += 1               # field 2 missing, below the maximum
        fg[4][-1] = 64 + len(fg[4])  # (its range then has missing fields: p = 0.5 too)
    return lens, np.concatenate(fg) if len(fg) else np.zeros(0, np.int32)


_case_cache = {}


def _case(c, layout):
    """(keys, row_ptr, fgid, ref64) of ROWS rows -- of as many as the
    configuration runs in this layout -- computed once; rm-F and fm-F share it."""
    R = max(rows for cc, lay, rows in CASES if cc == c and lay.split("-")[-1] == layout.split("-")[-1])
    R = max(R, 71)  # (the special rows up to the CSR case's long row 70)
    tag = (c, layout.split("-")[-1])
    if tag in _case_cache:
        return _case_cache[tag]
    kind, D = c[0], c[1]
    rng = np.random.default_rng(200 + len(_case_cache))
    lens, fg = _fields(kind, layout, rng, R,
                       padded=kind == "mvm" and D not in (1, 2, 4, 8, 10, 16, 32))
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    # planted keys and about 30 % that are not in the table (>= 5000)
    keys = rng.integers(100, 5700, size=int(rp[-1])).astype(np.uint64)
    keys[keys >= 4100] += 1000
    if R > 6 and lens[5] >= 3:
        for r, big in ((5, 1), (6, 5)):  # past +30, past -30
            lo, hi = int(rp[r]), int(rp[r + 1])
            keys[lo:hi] = rng.integers(100, 4100, size=hi - lo)
            if kind == "fm":
                keys[lo:lo + min(4, hi - lo)] = big + np.arange(min(4, hi - lo))
            else:
                keys[lo:hi] = 1 + np.arange(hi - lo) % 4
                keys[lo] = big
    lo, hi = int(rp[0]), int(rp[1])
    keys[lo:hi] = 6000 + np.arange(hi - lo)  # a row of absent keys only
    uk = np.unique(keys)
    W = _engines(c)["plain"].pull(uk)  # (absent keys: what the table's source would initialise)
    ref = ref64.reference(kind, D, uk, W, keys, rp, fgid=fg,
                          **({"fm_math": c[2]} if kind == "fm" else {"mvm_math": c[2]}))
    _case_cache[tag] = (keys, rp, fg, ref)
    return _case_cache[tag]


def _batch(c, layout, rows, dev):
    keys, rp, fg, _ = _case(c, layout)
    n = int(rp[rows])
    k = keys[:n].view(np.int64)
    f = None if fg is None else fg[:n]
    labels = torch.from_numpy((np.arange(rows) % 3 == 0).astype(F32)).to(dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).to(dev)
    if layout == "csr":
        return Batch(keys=t(k), labels=labels, fgid=None if f is None else t(f),
                     row_ptr=torch.from_numpy(rp[:rows + 1].astype(np.int32)).to(dev))
    kind, F = layout.split("-")
    F = int(F)
    if kind == "fm":
        k = k.reshape(rows, F).T
        f = None if f is None else f.reshape(rows, F).T
    return Batch(keys=t(k), labels=labels, fgid=None if f is None else t(f), nnz_per_row=F,
                 field_major=kind == "fm")


_eng_cache = {}


def _engines(c, dev=None):
    """The configuration's engines (those of one configuration at a time)."""
    if c in _eng_cache:
        return _eng_cache[c]
    assert dev is not None
    _eng_cache.clear()
    cfg = dict(table_log2_cap=LOG2, max_rows=ROWS, max_nnz=ROWS * 64)
    model, optim = _model(c), _optim(c)
    tk, tw = _table(c)
    out = {}
    for name, kw, fill in (("fused", dict(serve_unfused_rows_latent=(0, 0)), True),
                           ("plain", dict(serve_fused=False), True),
                           ("empty", dict(serve_unfused_rows_latent=(0, 0)), False),
                           ("empty_plain", dict(serve_fused=False), False)):
        e = Engine(model, optim, EngineConfig(**kw, **cfg), device=dev)
        if fill:
            e.import_weights(tk, tw)
        out[name] = e
    g = Engine(model, optim,
               EngineConfig(serve_unfused_rows_latent=(0, 0), grow_start=0.3, grow_load=0.6,
                            **dict(cfg, table_log2_cap=9)), device=dev)
    for i in range(0, len(tk), 500):
        g.import_weights(tk[i:i + 500], tw[i:i + 500])
    geo = g.table_geometry
    assert geo["split"] > 0 and geo["segments"] >= 3 and g.table_size() == len(tk), geo
    out["grown"] = g
    # chains leave the home slot, by construction: a table of 2^LOG2 slots in
    # one level has home = fmix64(key) mod 2^LOG2, and of planted keys that
    # share a home all but one sit further down the chain
    home = hashing.fmix64(tk) & np.uint64((1 << LOG2) - 1)
    geo = out["fused"].table_geometry
    assert geo["split"] == 0 and geo["segments"] << geo["seg_log2"] == 1 << LOG2, geo
    assert len(tk) - len(np.unique(home)) > 500 and out["fused"].table_size() == len(tk)
    _eng_cache[c] = out
    return out


# ---- GPU -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c,layout,rows", CASES,
                         ids=["%s%d-%s-%s-%s-%d" % (*c, lay, rows) for c, lay, rows in CASES])
def test_fused_equals_the_unfused_path(gpu_device, c, layout, rows):
    """Worst error/bound ratios measured on an MI355X: see the printed line of
    each case (all below 1; -s shows them)."""
    e = _engines(c, gpu_device)
    fused, plain = e["fused"], e["plain"]
    assert fused.serve_fused and not plain.serve_fused
    _, rp, fg, ref = _case(c, layout)
    b = _batch(c, layout, rows, gpu_device)
    for x in (fused, plain):
        x.read_stats(True, 1)
    p1 = fused.eval_step(b).cpu().numpy()
    s1 = fused.read_stats(True, 1)
    p3 = plain.eval_step(b).cpu().numpy()
    s3 = plain.read_stats(True, 1)
    assert np.array_equal(_bits(p1), _bits(p3))
    p2 = fused.eval_step(b).cpu().numpy()
    assert np.array_equal(_bits(p1), _bits(p2))  # deterministic run to run
    # the loss counters: the same per-row terms, summed per wave and per
    # workgroup in another grouping (f64 sums of at most 4097 terms)
    assert s1["rows"] == s3["rows"] == rows and s1["positives"] == s3["positives"]
    for name in ("ln_loss", "log2_lik"):
        assert s1[name] == pytest.approx(s3[name], rel=rows * 2.0 ** -52, abs=0.0), name
    assert np.array_equal(_bits(e["grown"].eval_step(b).cpu().numpy()), _bits(p1))
    p0 = e["empty"].eval_step(b).cpu().numpy()  # every key absent (FTRL: the lazy init of each)
    assert e["empty"].serve_fused and not e["empty_plain"].serve_fused
    assert np.array_equal(_bits(p0), _bits(e["empty_plain"].eval_step(b).cpu().numpy()))
    worst = 0.0
    for name, p in (("fused", p1), ("plain", p3)):
        err = np.abs(p.astype(np.float64) - ref.p[:rows])
        worst = max(worst, float((err / ref.e_p[:rows]).max()))
        assert (err <= ref.e_p[:rows]).all(), name
    print("%s %s rows %d: worst error/bound %.3g" % (c, layout, rows, worst))
    F = int(rp[6] - rp[5]) if rows > 6 else 0
    if F >= 3 and rows > 6:
        assert ref.y[5] > 31.0 and p1[5] == 1.0          # past the upper clamp
        assert ref.y[6] < -31.0 and p1[6] == F32(1e-6)   # past the lower clamp
    if c[0] == "mvm" and F >= 3 and rows > 4:
        assert p1[3] == 0.5 and p1[4] == 0.5             # a field below the maximum is missing
        assert ref.y[1] != 0.0 and ref.y[2] != 0.0       # (unsorted; a repeated field: complete rows)


def _small(kind, dev, **kw):
    c = (kind, 8, "reference" if kind == "fm" else "compat", "ftrl")
    tk, tw = _table(c)
    m = _model(c) if kind != "lr" else ModelConfig(kind="lr")
    e = Engine(m, _optim(c), EngineConfig(table_log2_cap=LOG2, max_rows=512, max_nnz=512 * 39, **kw),
               device=dev)
    e.import_weights(tk, tw if kind != "lr" else tw[:, :1])
    return e


def _small_batch(kind, rows, dev):
    rng = np.random.default_rng(rows)
    keys = rng.integers(100, 5700, size=rows * 39).astype(np.int64)
    fg = np.tile(np.arange(39, dtype=np.int32), rows)
    return Batch(keys=torch.from_numpy(keys).to(dev), labels=torch.zeros(rows, device=dev),
                 fgid=torch.from_numpy(fg).to(dev) if kind == "mvm" else None, nnz_per_row=39)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fm", "mvm"])
def test_the_windows_pick_a_path_not_a_result(gpu_device, kind):
    dflt, plain = _small(kind, gpu_device), _small(kind, gpu_device, serve_fused=False)
    lo, hi = dflt.serve_unfused_rows_latent  # (the model's measured window)
    assert (lo, hi) == ((0, 512) if kind == "fm" else (0, (1 << 63) - 1))
    # LR's window does not reach FM / MVM, whatever it is: the engine reports
    # the fused path and, a launch-observable, leaves its dedup scratch untouched
    lrwin = _small(kind, gpu_device, serve_unfused_rows=(0, 1 << 30),
                   serve_unfused_rows_latent=(0, 0))
    # the latent window does: every batch of this engine takes the unfused path
    latwin = _small(kind, gpu_device, serve_unfused_rows_latent=(0, 1 << 30))
    assert dflt.serve_fused and lrwin.serve_fused and latwin.serve_fused and not plain.serve_fused
    inside = [r for r in (1, 64, 128, 300, 512) if lo <= r < hi][:1]
    outside = [r for r in (1, 64, 128, 300, 512) if not lo <= r < hi][:1]
    for rows in inside + outside + [200]:
        b = _small_batch(kind, rows, gpu_device)
        want = _bits(plain.eval_step(b).cpu().numpy())
        for e in (dflt, lrwin, latwin):
            assert np.array_equal(_bits(e.eval_step(b).cpu().numpy()), want), rows
    assert lrwin.scratch_stats()["occupancy"] == 0 and latwin.scratch_stats()["occupancy"] > 0
    # ... and the latent window does not reach LR
    lr = _small("lr", gpu_device, serve_unfused_rows=(0, 0), serve_unfused_rows_latent=(0, 1 << 30))
    lr_plain = _small("lr", gpu_device, serve_fused=False)
    b = _small_batch("lr", 200, gpu_device)
    assert lr.serve_fused
    assert np.array_equal(_bits(lr.eval_step(b).cpu().numpy()), _bits(lr_plain.eval_step(b).cpu().numpy()))
    assert lr.scratch_stats()["occupancy"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("math", ["compat", "fixed"])
def test_padded_mvm_rows_with_an_empty_product_range_keep_the_unfused_bits(gpu_device, math):
    """The rows _fields keeps out of the float64 bound at v_dim 3 (an empty
    row, rows of field 0 alone): bit identity of the two paths holds there
    too, whatever k_mvm2 makes of them (docs/DESIGN.md §2, known issue)."""
    c = ("mvm", 3, math, "sgd")
    tk, tw = _table(c)
    cfg = dict(table_log2_cap=LOG2, max_rows=64, max_nnz=64 * 8)
    fused = Engine(_model(c), _optim(c), EngineConfig(serve_unfused_rows_latent=(0, 0), **cfg),
                   device=gpu_device)
    plain = Engine(_model(c), _optim(c), EngineConfig(serve_fused=False, **cfg), device=gpu_device)
    for e in (fused, plain):
        e.import_weights(tk, tw)
    lens = np.array([1, 0, 1, 3, 1, 0] * 10 + [2, 1, 0, 1, 1])  # 65 rows > one wave
    lens = lens[:64]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rng = np.random.default_rng(9)
    keys = rng.integers(100, 5700, size=int(rp[-1])).astype(np.int64)
    fg = np.concatenate([np.arange(n, dtype=np.int32) for n in lens])
    b = Batch(keys=torch.from_numpy(keys).to(gpu_device), labels=torch.zeros(64, device=gpu_device),
              fgid=torch.from_numpy(fg).to(gpu_device), row_ptr=torch.from_numpy(rp).to(gpu_device))
    assert fused.serve_fused and not plain.serve_fused
    assert np.array_equal(_bits(fused.eval_step(b).cpu().numpy()),
                          _bits(plain.eval_step(b).cpu().numpy()))


@pytest.mark.gpu
def test_fm_mfma_keeps_the_unfused_path(gpu_device):
    model = ModelConfig(kind="fm", v_dim=8, fm_math="standard", fm_mfma=True)
    src = Engine(model, OptimConfig(kind="sgd", lr=0.05),
                 EngineConfig(table_log2_cap=LOG2, max_rows=512, max_nnz=512 * 39), device=gpu_device)
    rng = np.random.default_rng(3)
    for _ in range(2):
        keys = rng.integers(100, 3000, size=512 * 39).astype(np.int64)
        src.train_step(Batch(keys=torch.from_numpy(keys).to(gpu_device),
                             labels=torch.from_numpy((rng.random(512) < 0.3).astype(F32)).to(gpu_device),
                             nnz_per_row=39))
    k, w = src.export_weights()
    frz = Engine(model, dataclasses.replace(src.optim, kind="frozen", frozen_from="sgd"),
                 EngineConfig(table_log2_cap=LOG2, max_rows=512, max_nnz=512 * 39), device=gpu_device)
    frz.import_weights(k, w)
    assert frz.frozen and not frz.serve_fused
    b = _small_batch("fm", 300, gpu_device)
    assert np.array_equal(_bits(src.eval_step(b).cpu().numpy()), _bits(frz.eval_step(b).cpu().numpy()))


@pytest.mark.gpu
def test_fm_snapshot_predicts_like_the_full_checkpoint(gpu_device, tmp_path):
    from xflow_amd.serve import Predictor
    from xflow_amd.trainer import Trainer

    cfg = TrainConfig(train_prefix=os.path.join(DATA, "small_train"),
                      test_prefix=os.path.join(DATA, "small_test"), epochs=2, threads=8,
                      pred_dir=str(tmp_path), write_pred=False, model=ModelConfig(kind="fm", v_dim=8),
                      engine=EngineConfig(table_log2_cap=14), checkpoint_dir=str(tmp_path / "ck"),
                      save_every=1, save_serving=str(tmp_path / "snap"))
    t = Trainer(cfg, device=gpu_device)
    try:
        t.train()
    finally:
        t.close()
    with open(os.path.join(DATA, "small_test-00000"), "rb") as f:
        text = f.read()
    full = Predictor(str(tmp_path / "ck"), device=gpu_device, max_rows=64)
    snap = Predictor(str(tmp_path / "snap"), device=gpu_device, max_rows=64,
                     serve_unfused_rows_latent=(0, 0))
    assert snap.snapshot and not full.snapshot and snap.engine.serve_fused
    a = full.predict_libffm(text)
    assert a.shape == (200,)
    assert np.array_equal(_bits(a), _bits(snap.predict_libffm(text)))
    for kw in (dict(serve_fused=False), dict()):
        other = Predictor(str(tmp_path / "snap"), device=gpu_device, max_rows=64, **kw)
        assert other.engine.serve_fused == (not kw)
        assert np.array_equal(_bits(a), _bits(other.predict_libffm(text)))


# ---- CPU -----------------------------------------------------------------------------
def test_config_field_round_trips():
    assert len(EngineConfig().serve_unfused_rows_latent) == 2
    assert EngineConfig().serve_unfused_rows == (64, 256)  # LR's window stays what it was
    from xflow_amd.serve import Predictor
    import inspect
    assert "serve_unfused_rows_latent" in inspect.signature(Predictor.__init__).parameters
    # EngineConfig -> native config: a window the native constructor does not
    # know would raise here
    c = ("fm", 3, "reference", "ftrl")
    e = Engine(_model(c), _optim(c),
               EngineConfig(table_log2_cap=10, max_rows=16, max_nnz=64,
                            serve_unfused_rows_latent=(3, 17)), device=torch.device("cpu"))
    assert e.cfg.serve_unfused_rows_latent == (3, 17) and e.frozen
    assert e.serve_unfused_rows_latent == (3, 17)  # (the window in force)
    # one negative bound is neither a window nor the model's default
    for bad in ((-1, 5), (3, -1)):
        with pytest.raises(ValueError):
            Engine(_model(c), _optim(c),
                   EngineConfig(table_log2_cap=10, max_rows=16, max_nnz=64,
                                serve_unfused_rows_latent=bad), device=torch.device("cpu"))


def test_predictor_passes_the_window_on(tmp_path):
    from xflow_amd import checkpoint
    from xflow_amd.serve import Predictor
    src = Engine(ModelConfig(kind="fm", v_dim=3), OptimConfig(kind="sgd"),
                 EngineConfig(table_log2_cap=10, max_rows=16, max_nnz=64), device=torch.device("cpu"))
    src.train_step(Batch(keys=torch.arange(1, 33, dtype=torch.int64), labels=torch.ones(8),
                         nnz_per_row=4))
    checkpoint.save_serving(src, str(tmp_path / "snap"), 0, 1, barrier=lambda: None)
    p = Predictor(str(tmp_path / "snap"), device=torch.device("cpu"), max_rows=16,
                  serve_unfused_rows_latent=(5, 9))
    assert p.engine.cfg.serve_unfused_rows_latent == (5, 9)
    assert Predictor(str(tmp_path / "snap"), device=torch.device("cpu"),
                     max_rows=16).engine.cfg.serve_unfused_rows_latent == \
        EngineConfig().serve_unfused_rows_latent


def test_frozen_fm_on_the_cpu_is_unfused_and_scores_as_before():
    dev = torch.device("cpu")
    model = ModelConfig(kind="fm", v_dim=3)
    src = Engine(model, OptimConfig(kind="ftrl"),
                 EngineConfig(table_log2_cap=10, max_rows=16, max_nnz=64), device=dev)
    keys = torch.arange(1, 65, dtype=torch.int64)
    src.train_step(Batch(keys=keys, labels=torch.ones(16), nnz_per_row=4))
    k, w = src.export_weights()
    frz = Engine(model, dataclasses.replace(src.optim, kind="frozen", frozen_from="ftrl"),
                 EngineConfig(table_log2_cap=10, max_rows=16, max_nnz=64), device=dev)
    frz.import_weights(k, w)
    assert frz.frozen and not frz.serve_fused
    b = Batch(keys=torch.arange(30, 94, dtype=torch.int64), labels=torch.zeros(16), nnz_per_row=4)
    assert np.array_equal(_bits(src.eval_step(b).numpy()), _bits(frz.eval_step(b).numpy()))
