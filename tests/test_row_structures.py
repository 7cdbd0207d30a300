"""Forward, loss counters and one-step gradients on hand-built row shapes,
against the float64 per-row reference (xflow_amd/testing/ref64.py) and its
a-priori error bounds -- on the CPU backend and on the GPU.

The batches are written out row by row from a short list of named row
builders (ROWS); each builder names the kernel branch it exists for.  Weights
are put into the table with import_table, read back with Engine.pull, and
those float32 values go to the reference, so the forward is checked apart from
the optimiser.  No bound here comes from what the engine computes: the
prediction bound is e_p = 1/4 N u A + 2 u p (ref64), the gradient bound is
built from it, and the one number that is measured is measured on the plain
fp32 reference update (torch_ref.RefTable.push), see UPDATE_ROUNDING below.
"""
import math

import numpy as np
import pytest
import torch

from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Batch, Engine
from xflow_amd.testing import ref64, torch_ref

U = ref64.U
CPU = torch.device("cpu")
DEVICES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]
WIDTHS = (1, 2, 4, 8, 10, 16, 32)
OPT = OptimConfig()

# The float64 update's own fp32 rounding.  Measured on the reference, not on
# the engine: the largest deviation of torch_ref.RefTable.push (the plain fp32
# closed forms) from the float64 update over GRAD_CASES, relative to the
# parameter's magnitude max(|w before|, |w after|), is 2.71e-7
# (test_update_rounding_is_what_was_measured holds it there).  Times 4 for
# the documented float(1 / alpha) multiply-vs-divide difference and the
# operation order:
UPDATE_ROUNDING_MEASURED = 2.71e-7
UPDATE_ROUNDING = 4 * UPDATE_ROUNDING_MEASURED


@pytest.fixture
def device(request):
    if request.param == "cpu":
        return CPU
    return request.getfixturevalue("gpu_device")


# ---- keys and rows -----------------------------------------------------------
KEY_CLASS = {}  # key -> occurrences of its field in the widest row it is in


def K(f, i, width=1):
    k = ((f * 1_000_003 + i) * 0x9E3779B97F4A7C15) % (1 << 64)
    KEY_CLASS[k] = (f, width)
    return k


def _plain(r):
    return [(f, K(f, (r + f) % 4)) for f in range(6)]


UNSORTED_ORDER = (3, 0, 5, 1, 4, 2)
HOT_KEY = K(0, 99)

# row index -> [(field, key)]
ROWS = {
    # k_mvm2: G = 0 under compat (empty product, y = D), incomplete under
    # fixed; every kernel's len = 0 lanes next to working ones
    "empty": lambda r: [],
    # MVM compat: a row whose only field is 0 (G = 0, y = D)
    "single": lambda r: [(0, K(0, r % 3))],
    # the sorted product path (`!dup && sorted`)
    "plain": _plain,
    # the unsorted product path (`else if (!dup)`, the `while (fgid != g)` search)
    "unsorted": lambda r: [_plain(r)[f] for f in UNSORTED_ORDER],
    # complete == false in the middle of the mask: M = 0, all gradients 0
    "missing_mid": lambda r: [_plain(r)[f] for f in (0, 1, 3, 4)],
    # complete == false from field 0 on (compat: fields 0-4 absent)
    "only_last": lambda r: [(5, K(5, r % 4))],
    # repeated fields: `dup` from the mask, field sums, the atomics / MvmDup gradient
    "dup_field": lambda r: _plain(r)[:5] + [(4, K(4, 7))] + _plain(r)[5:] + [(5, K(5, 7))],
    # the same key twice in one row: two occurrences of one (key, slice) in a row
    "dup_key": lambda r: _plain(r)[:3] + [_plain(r)[2]] + _plain(r)[3:],
    # 300 occurrences next to short rows: the maxlen loops, lane divergence,
    # LR rows beyond the register columns
    "long": lambda r: [(f, K(f, 100 + i, 50)) for f in range(6) for i in range(50)],
    # the `G >= 64 ? ~0ull` mask edge: fixed math G = 64 with 64 mask bits
    "f63": lambda r: [(f, K(f, 200 + r % 2, 12)) for f in range(64)],
    # field 64 sets `dup` (f >= 64); compat G = 64, fixed G = 65 (linear `complete`)
    "f64": lambda r: [(f, K(f, 200 + r % 2, 12)) for f in range(65)],
    # G > 64 under both maths
    "f70": lambda r: [(f, K(f, 200 + r % 2, 12)) for f in range(71)],
    # ... found by the linear search in reversed order
    "f70_unsorted": lambda r: [(f, K(f, 200 + r % 2, 12)) for f in reversed(range(71))],
    # one key in every row: the longest chain of adds onto one gradient
    "hot": lambda r: [(0, HOT_KEY)] + _plain(r)[1:],
}


class Case:
    """A CSR batch built from (builder name) per row, with labels."""

    def __init__(self, name, builders):
        self.name = name
        self.builders = list(builders)
        keys, fg, rp = [], [], [0]
        for r, b in enumerate(self.builders):
            for f, k in ROWS[b](r):
                keys.append(k)
                fg.append(f)
            rp.append(len(keys))
        self.keys = np.array(keys, dtype=np.uint64)
        self.fgid = np.array(fg, dtype=np.int32)
        self.row_ptr = np.array(rp, dtype=np.int32)
        self.rows = len(self.builders)
        self.labels = np.array([1.0 if (r * 5 + 1) % 3 == 0 else 0.0 for r in range(self.rows)],
                               dtype=np.float32)
        self.ukeys = np.unique(self.keys)

    def batch(self, device, slice_rows=0):
        return Batch(keys=torch.from_numpy(self.keys.view(np.int64)).to(device),
                     labels=torch.from_numpy(self.labels).to(device),
                     row_ptr=torch.from_numpy(self.row_ptr).to(device),
                     fgid=torch.from_numpy(self.fgid).to(device), slice_rows=slice_rows)

    def fixed(self, device):
        """The same rows as a fixed-width row-major batch."""
        F = len(self.keys) // self.rows
        assert (np.diff(self.row_ptr) == F).all()
        return Batch(keys=torch.from_numpy(self.keys.view(np.int64)).to(device),
                     labels=torch.from_numpy(self.labels).to(device),
                     fgid=torch.from_numpy(self.fgid).to(device), nnz_per_row=F)


_CYCLE = [b for b in ROWS if b != "empty"] + ["empty"]
CASES = {c.name: c for c in (
    [Case("one_" + b, [b]) for b in ROWS]
    + [Case("interleaved65", ["empty"] + [_CYCLE[i % len(_CYCLE)] for i in range(63)] + ["empty"]),
       Case("empty65", ["empty"] * 65),
       Case("hot1023", ["hot"] * 1023),
       Case("hot1025", ["hot"] * 1025),
       Case("long_among_single", ["single"] * 32 + ["long"] + ["single"] * 32)])}
FIXED = {c.name: c for c in (Case(f"{b}{n}", [b] * n) for b in ("plain", "unsorted")
                             for n in (63, 257))}
ALL_KEYS = np.unique(np.concatenate([c.keys for c in list(CASES.values()) + list(FIXED.values())]))
MAX_ROWS = 1100
MAX_NNZ = max(len(c.keys) for c in list(CASES.values()) + list(FIXED.values()))
assert max(c.rows for c in CASES.values()) <= MAX_ROWS and int(ALL_KEYS.max()) < (1 << 64) - 1
assert min(c.fgid.min() for c in CASES.values() if len(c.fgid)) >= 0
assert max(c.fgid.max() for c in CASES.values() if len(c.fgid)) == 70


# ---- models and weights ------------------------------------------------------
def cfg_id(m):
    math_ = {"lr": "", "fm": m.fm_math[:3], "mvm": m.mvm_math[:3]}[m.kind]
    return f"{m.kind}{math_}{'mfma' if m.fm_mfma else ''}-d{m.v_dim if m.kind != 'lr' else 0}"


def _models(widths, mfma_widths=()):
    out = [ModelConfig(kind="lr")] if 4 in widths else []
    for d in widths:
        out += [ModelConfig(kind="fm", v_dim=d, fm_math="reference"),
                ModelConfig(kind="fm", v_dim=d, fm_math="standard"),
                ModelConfig(kind="mvm", v_dim=d, mvm_math="compat"),
                ModelConfig(kind="mvm", v_dim=d, mvm_math="fixed")]
    out += [ModelConfig(kind="fm", v_dim=d, fm_math="standard", fm_mfma=True) for d in mfma_widths]
    return out


FULL_MODELS = _models((4,), (4,))                       # the whole case table
WIDTH_MODELS = _models([d for d in WIDTHS if d != 4], (1, 2, 8))   # two batches each


def weights(m, keys):
    """float32 [len(keys), P], logits O(1): LR weights and FM w0 / v at scale
    0.3 (over the square root of the widest row's occurrences, v also of D);
    MVM latents of magnitude in [0.8, 1.25] with random signs -- the keys of
    the 64..71-field rows alternate above and below 1 by field so that the
    product stays near 1, the 50 keys per field of the long row are scaled to
    a field sum of magnitude about 0.45 (one sign per field and component: a
    sum of 50 random signs would cancel and leave no bound worth testing)."""
    rng = np.random.default_rng(1234)
    P = m.params_per_key
    W = np.zeros((len(keys), P))
    for i, k in enumerate(keys):
        f, width = KEY_CLASS[int(k)]
        if m.kind == "mvm":
            if width == 12:
                ln = (0.2 if f % 2 == 0 else -0.2) + rng.uniform(-0.02, 0.02, P)
            else:
                ln = rng.uniform(-math.log(1.25), math.log(1.25), P)
            W[i] = np.exp(ln) * rng.choice([-1.0, 1.0], P)
            if width == 50:
                # one sign per (field, component) and a field sum S of magnitude
                # 0.36 .. 0.57: well conditioned, also in the gradient's 1 / (1 + S)
                W[i] = np.abs(W[i]) * np.random.default_rng(f).choice([-1.0, 1.0], P) * 0.45 / 50
        else:
            W[i, 0] = 0.3 * rng.standard_normal() / math.sqrt(width)
            if P > 1:
                W[i, 1:] = 0.3 * rng.standard_normal(P - 1) / math.sqrt(width * m.v_dim)
    return W.astype(np.float32)


def ftrl_state(W):
    """(n, z) float32 whose FTRL weight is close to W (n = 1)."""
    n = np.ones_like(W, dtype=np.float32)
    den = (OPT.beta + 1.0) / OPT.alpha + OPT.lambda2
    z = (-W.astype(np.float64) * den - np.sign(W) * OPT.lambda1).astype(np.float32)
    return n, z


def make_engine(device, m, opt="sgd", keys=None, S=1, csr=True, sum_slices=False,
                max_rows=MAX_ROWS, max_nnz=MAX_NNZ):
    """An engine whose table holds `keys` with weights(m, keys); returns the
    engine and the imported state (SGD: w; FTRL: (n, z))."""
    eng = Engine(m, OptimConfig(kind=opt),
                 EngineConfig(table_log2_cap=12, max_rows=max_rows, max_nnz=max_nnz, max_slices=S,
                              sum_slices=sum_slices, csr=csr), device=device)
    if keys is None:
        return eng, None
    W = weights(m, keys)
    P = m.params_per_key
    words = np.zeros((len(keys), eng.state_words), dtype=np.uint32)
    if opt == "sgd":
        state = (W,)
        words[:, :P] = W.view(np.uint32)
    else:
        state = ftrl_state(W)
        st = np.stack(state, axis=2)           # [U, P, (n, z)]
        words[:, :2 * P] = st.reshape(len(keys), 2 * P).view(np.uint32)
    if m.kind != "lr":
        words[:, P * (1 if opt == "sgd" else 2)] = 1   # pushed: the latents are the state's
    eng.import_table(keys, words.reshape(-1))
    assert eng.table_size() == len(keys)
    return eng, state


_REF = {}


def reference(m, case, W, slice_rows=0):
    """ref64 of a case under model m with pulled weights W (of case.ukeys);
    computed once per (model, case, weights, slicing)."""
    key = (cfg_id(m), case.name, slice_rows, W.tobytes())
    if key not in _REF:
        ref = ref64.reference(m.kind, m.v_dim, case.ukeys, W, case.keys, case.row_ptr, case.fgid,
                              case.labels, slice_rows, m.fm_math, m.mvm_math)
        # no row may sit where its fp32 logit could fall on the other side of a clamp
        margin = ref.N * U * ref.A
        assert (np.abs(np.abs(ref.y) - 30.0) > margin).all(), (cfg_id(m), case.name)
        _REF[key] = ref
    return _REF[key]


def note_ratio(what, who, m, ratio):
    """One line per check for the record (shown with -s): error / bound."""
    print(f"ratio {what} {who} {cfg_id(m).split('-')[0]} {ratio:.4f}")


def worst_ratio(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    r = np.where(err == 0.0, 0.0, err / np.where(bound > 0, bound, 1e-300))
    return float(r.max()) if r.size else 0.0   # (NaN if any error is NaN)


def check_counters(got, ref, what, fails):
    if got["rows"] != ref.counters["rows"] or got["positives"] != ref.counters["positives"]:
        fails.append(f"{what}: rows/positives {got} != {ref.counters}")
    for name in ("ln_loss", "log2_lik"):
        if math.isinf(ref.counters[name]):   # (p = 1 exactly with label 0: -inf by definition)
            if got[name] != ref.counters[name]:
                fails.append(f"{what}: {name} {got[name]!r}, expected {ref.counters[name]!r}")
            continue
        d = abs(got[name] - ref.counters[name])
        if not d <= ref.counter_tol[name]:
            fails.append(f"{what}: {name} {got[name]!r} vs {ref.counters[name]!r}, "
                         f"|d| {d:.3e} > tol {ref.counter_tol[name]:.3e}")


def _dev(device):
    return "cpu" if device.type == "cpu" else "gpu"


# ---- a. predictions, b. eval counters ----------------------------------------
def _eval_cases(device, m, names, fails):
    eng, (W0,) = make_engine(device, m, "sgd", ALL_KEYS)
    for name in names:
        case = CASES[name]
        W = eng.pull(case.ukeys)
        assert np.array_equal(W, W0[np.searchsorted(ALL_KEYS, case.ukeys)])  # (pull is the import)
        ref = reference(m, case, W)
        eng.read_stats(reset=True, which=1)
        p = eng.eval_step(case.batch(device)).cpu().numpy()
        assert np.isfinite(p).all(), name
        err = np.abs(p.astype(np.float64) - ref.p)
        ratio = worst_ratio(err, ref.e_p)
        note_ratio("pred", _dev(device), m, ratio)
        if not ratio <= 1.0:
            r = int(np.argmax(err / ref.e_p))
            fails.append(f"{name}: row {r} ({case.builders[r]}) p {p[r]!r} vs {ref.p[r]!r}, "
                         f"error/bound {ratio:.3g}")
        check_counters(eng.read_stats(which=1), ref, f"{name} eval counters", fails)
    assert not eng.overflowed()
    return eng


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("m", FULL_MODELS, ids=cfg_id)
def test_predictions_and_eval_counters_whole_table(device, m):
    fails = []
    _eval_cases(device, m, list(CASES), fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("m", WIDTH_MODELS, ids=cfg_id)
def test_predictions_and_eval_counters_other_widths(device, m):
    fails = []
    _eval_cases(device, m, ["interleaved65", "hot1025"], fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("m", FULL_MODELS, ids=cfg_id)
def test_predictions_fixed_width_layouts(device, m):
    """plain / unsorted rows at 63 and 257 rows as fixed-width batches:
    row-major, field-major by torch and field-major by the engine's backend."""
    fails = []
    eng, _ = make_engine(device, m, "sgd", ALL_KEYS)
    for name, case in FIXED.items():
        ref = reference(m, case, eng.pull(case.ukeys))
        rm = case.fixed(device)
        for layout, b in (("row_major", rm), ("field_major", rm.to_field_major()),
                          ("field_major_engine", rm.to_field_major(eng))):
            eng.read_stats(reset=True, which=1)
            p = eng.eval_step(b).cpu().numpy()
            assert np.isfinite(p).all(), (name, layout)
            ratio = worst_ratio(np.abs(p.astype(np.float64) - ref.p), ref.e_p)
            note_ratio("pred", _dev(device), m, ratio)
            if not ratio <= 1.0:
                fails.append(f"{name} {layout}: error/bound {ratio:.3g}")
            check_counters(eng.read_stats(which=1), ref, f"{name} {layout} counters", fails)
    assert not fails, "\n".join(fails)


# ---- 4. the bound holds for the plain fp32 reference -------------------------
@pytest.mark.parametrize("m", [m for m in FULL_MODELS + WIDTH_MODELS if not m.fm_mfma], ids=cfg_id)
def test_torch_reference_is_within_the_prediction_bound(m):
    """torch_ref.forward + sigmoid_ref, the independent plain fp32
    implementation, satisfies e_p on every case (it builds the dense
    [rows, G, D] field sums, which at G = 71 is still small here, so no case
    is left out)."""
    names = list(CASES) + list(FIXED) if m.v_dim == 4 or m.kind == "lr" else ["interleaved65", "hot1025"]
    fails = []
    for name in names:
        case = CASES.get(name) or FIXED[name]
        W = weights(m, case.ukeys)
        ref = reference(m, case, W)
        inv = torch.from_numpy(np.searchsorted(case.ukeys, case.keys)).long()
        row_of = torch.from_numpy(np.repeat(np.arange(case.rows), np.diff(case.row_ptr))).long()
        y, _ = torch_ref.forward(m.kind, torch.from_numpy(W), inv, row_of, case.rows,
                                 torch.from_numpy(case.fgid).long(), m.fm_math, m.mvm_math)
        p = torch_ref.sigmoid_ref(y).numpy()
        ratio = worst_ratio(np.abs(p.astype(np.float64) - ref.p), ref.e_p)
        note_ratio("pred", "torch_ref", m, ratio)
        if not ratio <= 1.0:
            fails.append(f"{name}: error/bound {ratio:.3g}")
    assert not fails, "\n".join(fails)


# ---- saturation ---------------------------------------------------------------
SAT_WEIGHTS = np.array([30.0, -30.0, np.nextafter(np.float32(30), np.float32(np.inf)),
                        np.nextafter(np.float32(-30), np.float32(-np.inf)), 40.0, -40.0, 29.0],
                       dtype=np.float32)


def _sat_case(sel):
    keys = np.array([K(0, 300 + i) for i in range(len(SAT_WEIGHTS)) for _ in (0, 1)], dtype=np.uint64)
    labels = np.array([lab for _ in SAT_WEIGHTS for lab in (0.0, 1.0)], dtype=np.float32)
    keys, labels = keys[sel], labels[sel]
    n = len(keys)
    return keys, np.arange(n + 1, dtype=np.int32), np.zeros(n, dtype=np.int32), labels


@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_sigmoid_clamp_edges_bit_exact(device):
    """Single-key LR rows, y = the weight exactly: the clamps are strict at
    +-30, p is bit-equal to the float64 reference rounded to fp32, the
    counters are finite where the definition is and log2_lik is -inf for
    p = 1, label 0; the range flag stays clear through a train step."""
    m = ModelConfig(kind="lr")
    skeys = np.array([K(0, 300 + i) for i in range(len(SAT_WEIGHTS))], dtype=np.uint64)
    eng = Engine(m, OptimConfig(kind="sgd"), EngineConfig(table_log2_cap=10, max_rows=64, max_nnz=64),
                 device=device)
    words = np.zeros((len(skeys), eng.state_words), dtype=np.uint32)
    words[:, 0] = SAT_WEIGHTS.view(np.uint32)
    eng.import_table(skeys, words.reshape(-1))
    assert np.array_equal(eng.pull(skeys)[:, 0], SAT_WEIGHTS)
    allrows = np.ones(2 * len(SAT_WEIGHTS), dtype=bool)
    want_p = np.array([ref64.sigmoid(float(w)) for w in SAT_WEIGHTS for _ in (0, 1)]).astype(np.float32)
    # the strict clamps, stated: exactly 30 is not clamped, the next float is
    assert ref64.sigmoid(30.0) < 1.0 and ref64.sigmoid(float(SAT_WEIGHTS[2])) == 1.0
    assert ref64.sigmoid(-30.0) < 1e-6 and ref64.sigmoid(float(SAT_WEIGHTS[3])) == 1e-6
    finite = np.array([ref64.loss_terms(float(p), float(lab))[1] > -math.inf
                       for p, lab in zip(want_p, _sat_case(allrows)[3])])
    assert 0 < finite.sum() < len(finite)
    for sel in (allrows, finite):
        keys, rp, fg, labels = _sat_case(sel)
        b = Batch(keys=torch.from_numpy(keys.view(np.int64)).to(device),
                  labels=torch.from_numpy(labels).to(device),
                  row_ptr=torch.from_numpy(rp).to(device), fgid=torch.from_numpy(fg).to(device))
        eng.read_stats(reset=True, which=1)
        p = eng.eval_step(b).cpu().numpy()
        assert np.array_equal(p.view(np.uint32), want_p[sel].view(np.uint32)), (p, want_p[sel])
        want = ref64.counters(want_p[sel].astype(np.float64), labels)
        got = eng.read_stats(which=1)
        assert got["rows"] == want["rows"] and got["positives"] == want["positives"]
        terms = [ref64.loss_terms(float(q), float(lab)) for q, lab in zip(want_p[sel], labels)]
        # logf / log2f: 2u relative; 1 - p rounded to fp32: u relative in the argument
        assert math.isfinite(got["ln_loss"])
        assert abs(got["ln_loss"] - want["ln_loss"]) <= sum(2 * U * abs(t[0]) + 2 * U for t in terms)
        if sel is allrows:
            assert want["log2_lik"] == -math.inf and got["log2_lik"] == -math.inf
        else:
            assert math.isfinite(got["log2_lik"])
            assert abs(got["log2_lik"] - want["log2_lik"]) <= sum(2 * U * abs(t[1]) + 2 * U
                                                                 / math.log(2.0) for t in terms)
    keys, rp, fg, labels = _sat_case(allrows)
    eng.train_step(Batch(keys=torch.from_numpy(keys.view(np.int64)).to(device),
                         labels=torch.from_numpy(labels).to(device),
                         row_ptr=torch.from_numpy(rp).to(device)))
    st = eng.read_stats(which=0)
    assert st["rows"] == len(labels) and math.isfinite(st["ln_loss"]) and st["log2_lik"] == -math.inf
    assert not eng.overflowed()   # (bit 1 of the first word is the range flag)


# ---- c. training counters, d. one-step gradients -----------------------------
# kind, fm_math / mvm_math, v_dim, opt, S, csr, sum_slices, case -> the layout planned on the GPU
# (the (model, optimiser, slices) pairs of tests/test_plan_paths.py::CASES,
# then the widths no other test trains: MVM 1, FM / MVM 2 and 32)
GRAD_CASES = [
    ("lr", "", 0, "ftrl", 1, True, False, "interleaved65", "unique_lr"),
    ("lr", "", 0, "ftrl", 8, True, False, "interleaved65", "csr"),
    ("lr", "", 0, "ftrl", 8, False, False, "interleaved65", "unique_lr"),
    ("lr", "", 0, "ftrl", 8, True, True, "interleaved65", "slot_sums"),
    ("lr", "", 0, "sgd", 1, True, False, "interleaved65", "slot_rows"),
    ("lr", "", 0, "ftrl", 1, True, False, "hot1025", "unique_lr"),
    ("fm", "reference", 4, "ftrl", 1, True, False, "interleaved65", "unique_fm_bc"),
    ("fm", "reference", 4, "ftrl", 8, True, False, "interleaved65", "csr"),
    ("fm", "standard", 4, "ftrl", 1, True, False, "interleaved65", "unique_rows"),
    ("fm", "standard", 4, "ftrl", 8, True, False, "interleaved65", "csr"),
    ("fm", "standard", 4, "sgd", 8, False, False, "interleaved65", "unique_rows"),
    ("mvm", "compat", 4, "ftrl", 1, True, False, "interleaved65", "unique_rows"),
    ("mvm", "compat", 4, "sgd", 8, True, False, "interleaved65", "csr"),
    ("mvm", "fixed", 4, "ftrl", 8, False, False, "interleaved65", "slot_rows"),
    ("mvm", "fixed", 4, "sgd", 1, True, False, "hot1025", "unique_rows"),
    ("mvm", "compat", 1, "sgd", 1, True, False, "interleaved65", "slot_rows"),
    ("mvm", "fixed", 1, "ftrl", 1, True, False, "interleaved65", "slot_rows"),
    ("mvm", "fixed", 1, "sgd", 8, True, False, "interleaved65", "slot_rows"),
    ("fm", "reference", 2, "ftrl", 1, True, False, "interleaved65", "unique_fm_bc"),
    ("fm", "standard", 2, "sgd", 1, True, False, "interleaved65", "unique_rows"),
    ("mvm", "compat", 2, "ftrl", 1, True, False, "interleaved65", "unique_rows"),
    ("fm", "reference", 32, "sgd", 1, True, False, "interleaved65", "unique_fm_bc"),
    ("fm", "standard", 32, "ftrl", 1, True, False, "interleaved65", "unique_rows"),
    ("mvm", "fixed", 32, "ftrl", 1, True, False, "interleaved65", "unique_rows"),
]


def grad_id(c):
    return "-".join(str(x) for x in c[:8] if x != "")


def _model_of(c):
    kind, math_, d = c[:3]
    if kind == "fm":
        return ModelConfig(kind="fm", v_dim=d, fm_math=math_)
    if kind == "mvm":
        return ModelConfig(kind="mvm", v_dim=d, mvm_math=math_)
    return ModelConfig(kind="lr")


def _slice_rows(case, S):
    return 0 if S == 1 else -(-case.rows // S)   # whole rows per slice, S slices


def expected_update(ref, opt, state, W, sum_slices):
    """The float64 update of every (key, param) with ref's gradients, and the
    tolerance from evaluating it at g - e, g, g + e (one slice's gradient at a
    time; the deviations add to first order)."""
    Uq, nS, P = ref.g.shape

    def run(i, q, g):
        w = float(W[i, q])
        if opt == "sgd":
            for s in range(len(g)):
                w = ref64.sgd_update(w, g[s], OPT.lr)
            return w
        n, z = float(state[0][i, q]), float(state[1][i, q])
        for s in range(len(g)):
            n, z = ref64.ftrl_update(n, z, w, g[s], OPT.alpha)
            w = ref64.ftrl_weight(z, n, OPT.alpha, OPT.beta, OPT.lambda1, OPT.lambda2)
        return w

    want = np.zeros((Uq, P))
    tol = np.zeros((Uq, P))
    for i in range(Uq):
        ss = [s for s in range(nS) if ref.touched[i, s]]
        for q in range(P):
            g = [ref.g[i, s, q] for s in ss]
            e = [ref.e_g[i, s, q] for s in ss]
            if sum_slices:
                g, e = [sum(g)], [sum(e)]
            w = want[i, q] = run(i, q, g)
            for s in range(len(g)):
                lo = run(i, q, g[:s] + [g[s] - e[s]] + g[s + 1:])
                hi = run(i, q, g[:s] + [g[s] + e[s]] + g[s + 1:])
                tol[i, q] += max(abs(lo - w), abs(hi - w))
            tol[i, q] += UPDATE_ROUNDING * max(abs(w), abs(float(W[i, q])))
    return want, tol


_TRAINED = {}


def _train(device, c):
    """One train_step of a GRAD_CASES entry (once per device and case)."""
    key = (_dev(device), c)
    if key in _TRAINED:
        return _TRAINED[key]
    *_, opt, S, csr, sum_slices, name, layout = c
    m, case = _model_of(c), CASES[c[7]]
    eng, state = make_engine(device, m, opt, case.ukeys, S, csr, sum_slices, max_rows=case.rows,
                             max_nnz=len(case.keys))
    plan = eng.native.step_plan(S)
    W = eng.pull(case.ukeys)
    sr = _slice_rows(case, S)
    b = case.batch(device, slice_rows=sr)
    assert eng.slices_of(b) == S
    eng.train_step(b)
    out = dict(m=m, case=case, plan=plan, W=W, state=state, after=eng.pull(case.ukeys),
               stats=eng.read_stats(which=0), overflowed=eng.overflowed(),
               ref=reference(m, case, W, sr))
    _TRAINED[key] = out
    return out


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("c", GRAD_CASES, ids=grad_id)
def test_train_step_counters(device, c):
    t = _train(device, c)
    fails = []
    check_counters(t["stats"], t["ref"], "train counters", fails)
    assert not fails, "\n".join(fails)
    assert not t["overflowed"]


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("c", GRAD_CASES, ids=grad_id)
def test_one_step_gradients(device, c):
    t = _train(device, c)
    opt, sum_slices, layout = c[3], c[6], c[8]
    if layout is not None:
        assert t["plan"]["grad"] == (layout if device.type != "cpu" else "slot_rows"), t["plan"]
    want, tol = expected_update(t["ref"], opt, t["state"], t["W"], sum_slices)
    assert np.isfinite(t["after"]).all()
    err = np.abs(t["after"].astype(np.float64) - want)
    assert np.abs(t["after"] - t["W"]).max() > 0       # (the step moved something)
    ratio = worst_ratio(err, tol)
    note_ratio("grad", _dev(device), t["m"], ratio)
    if not ratio <= 1.0:
        i, q = np.unravel_index(np.argmax(err / tol), err.shape)
        f, width = KEY_CLASS[int(t["case"].ukeys[i])]
        pytest.fail(f"key of field {f} (width class {width}) param {q}: {t['after'][i, q]!r} vs "
                    f"{want[i, q]!r}, error/tolerance {ratio:.3g}")


def test_update_rounding_is_what_was_measured():
    """The plain fp32 update (torch_ref.RefTable.push) against the float64
    update, both fed the same fp32 gradients: the largest deviation relative to
    max(|w before|, |w after|) over GRAD_CASES is UPDATE_ROUNDING_MEASURED."""
    worst = 0.0
    for c in GRAD_CASES:
        opt, S, sum_slices = c[3], c[4], c[6]
        m, case = _model_of(c), CASES[c[7]]
        W = weights(m, case.ukeys)
        P = m.params_per_key
        table = torch_ref.RefTable(P, 0 if m.kind == "mvm" else 1, opt,
                                   init_fn=lambda k, d: np.zeros(len(k), dtype=np.float32))
        table.keys = case.ukeys.copy()
        if opt == "sgd":
            state = (W,)
            table.state = torch.from_numpy(W.copy())
        else:
            state = ftrl_state(W)
            table.state = torch.from_numpy(np.stack(state, axis=2).reshape(len(W), 2 * P).copy())
        table.pushed = torch.ones(len(W), dtype=torch.bool)
        W0 = table.weights(case.ukeys, insert=False).numpy().copy()
        ref = reference(m, case, W0, _slice_rows(case, S))
        g32 = ref.g.astype(np.float32)
        if sum_slices:
            table.push(case.ukeys, torch.from_numpy(np.where(ref.touched[:, :, None], g32, 0).sum(1)))
        else:
            for s in range(g32.shape[1]):
                sel = ref.touched[:, s]
                if sel.any():
                    table.push(case.ukeys[sel], torch.from_numpy(g32[sel, s]))
        got = table.weights(case.ukeys, insert=False).numpy().astype(np.float64)
        exact = ref64.Ref64(**{**ref.__dict__, "g": g32.astype(np.float64), "e_g": np.zeros_like(ref.g)})
        want, _ = expected_update(exact, opt, state, W0, sum_slices)
        rel = np.abs(got - want) / np.maximum(np.abs(want), np.abs(W0))
        worst = max(worst, float(rel.max()))
    print(f"update rounding, measured: {worst:.3e}")
    assert worst <= UPDATE_ROUNDING_MEASURED, worst
    assert worst >= UPDATE_ROUNDING_MEASURED / 2, worst   # (the constant is the measurement)


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("name", ["interleaved65", "hot1025"])
def test_fresh_lr_ftrl_z_is_the_exact_gradient(device, name):
    """A fresh LR-FTRL table: every weight is 0, every p exactly 0.5, every
    gradient sum an exact multiple of 0.5, and the first push leaves z = g:
    the exported z is bit-equal to float32(float64(sum) / rows) -- also for
    the key in all 1025 rows and for the key that is twice in a row."""
    case = CASES[name]
    eng, _ = make_engine(device, ModelConfig(kind="lr"), "ftrl", None, max_rows=case.rows,
                         max_nnz=len(case.keys))
    eng.train_step(case.batch(device))
    sums = {int(k): 0.0 for k in case.ukeys}
    for r in range(case.rows):
        for o in range(case.row_ptr[r], case.row_ptr[r + 1]):
            sums[int(case.keys[o])] += 0.5 - float(case.labels[r])
    keys, words = eng.export_table()
    words = words.reshape(len(keys), eng.state_words)
    assert sorted(int(k) for k in keys) == sorted(sums)
    z = words[:, 1].copy().view(np.float32)
    want = np.array([np.float32(sums[int(k)] / case.rows) for k in keys], dtype=np.float32)
    assert np.array_equal(z.view(np.uint32), want.view(np.uint32)), np.abs(z - want).max()
    st = eng.read_stats(which=0)
    assert st["rows"] == case.rows and st["ln_loss"] == pytest.approx(case.rows * math.log(2), rel=1e-6)


# ---- e. inert rows -------------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("opt", ["sgd", "ftrl"])
@pytest.mark.parametrize("mvm_math", ["compat", "fixed"])
def test_inert_rows_mvm(device, mvm_math, opt):
    """Stated outcomes, not only ref64's: an MVM row with a field missing below
    G predicts sigmoid(0) and moves nothing; the empty product (compat: no
    field below the largest) predicts sigmoid(D); the keys of such rows are
    inserted once."""
    D = 4
    m = ModelConfig(kind="mvm", v_dim=D, mvm_math=mvm_math)
    half = np.float32(0.5)
    sig_d = np.float32(ref64.sigmoid(float(D)))
    rows = ["empty", "missing_mid", "only_last", "single"] * 4
    case = Case("inert", rows)
    expect = {"empty": sig_d if mvm_math == "compat" else half, "missing_mid": half,
              "only_last": half, "single": sig_d if mvm_math == "compat" else None}
    eng, _ = make_engine(device, m, opt, case.ukeys, max_rows=case.rows, max_nnz=len(case.keys))
    p = eng.eval_step(case.batch(device)).cpu().numpy()
    for r, b in enumerate(rows):
        if expect[b] is not None:
            assert p[r] == expect[b], (r, b, p[r])
    # gradients: M = 0 makes every gradient of a missing_mid / only_last row
    # exactly 0, so only the keys of the `single` rows (M = 1 or w) may move
    before = eng.pull(case.ukeys)
    eng.train_step(case.batch(device))
    after = eng.pull(case.ukeys)
    moving = np.array([k for r, b in enumerate(rows) if b == "single" for _, k in ROWS[b](r)],
                      dtype=np.uint64)
    still = ~np.isin(case.ukeys, moving)
    assert still.sum() >= 4
    assert np.array_equal(before[still].view(np.uint32), after[still].view(np.uint32))
    assert not np.array_equal(before[~still], after[~still])
    # a fresh table takes each key of these rows once
    fresh, _ = make_engine(device, m, opt, None, max_rows=case.rows, max_nnz=len(case.keys))
    fresh.train_step(case.batch(device))
    assert fresh.table_size() == len(case.ukeys)


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("m", [ModelConfig(kind="lr"), ModelConfig(kind="fm", v_dim=4),
                               ModelConfig(kind="fm", v_dim=4, fm_math="standard")], ids=cfg_id)
def test_empty_rows_predict_one_half(device, m):
    case = CASES["empty65"]
    eng, _ = make_engine(device, m, "ftrl", None, max_rows=case.rows,
                         max_nnz=len(CASES["interleaved65"].keys))
    p = eng.eval_step(case.batch(device)).cpu().numpy()
    assert (p == np.float32(0.5)).all()
    # an eval of keys the table does not hold, then a training batch without
    # occurrences: nothing of the batch before may be pulled or inserted again
    other = CASES["interleaved65"]
    eng.eval_step(other.batch(device))
    before = eng.pull(other.ukeys)
    eng.train_step(case.batch(device))
    assert eng.table_size() == 0
    assert np.array_equal(eng.pull(other.ukeys).view(np.uint32), before.view(np.uint32))
    st = eng.read_stats(which=0)
    assert st["rows"] == 65 and st["positives"] == float(case.labels.sum())
