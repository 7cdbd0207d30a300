"""Device-side AUC / logloss (Engine.eval_metrics, csrc/hip/kernels_eval.hip:
stable radix sort + rank sums) against a numpy definition written here and
the reference printer semantics (base.h:84-110, native reference_auc).

The definition (EvalMetrics, csrc/include/xflow/backend.h): the sort key of a
prediction is the bit pattern of ``p > 0 ? p : +0.0f``, the order is
descending in that key and stable in prediction order, a label is positive
iff ``> 0.5f``.  n / tp / area are integers and must match exactly; ``auc`` is
one float division of them and must match exactly; the two logloss sums are
held to bounds derived from the number formats (_sum_bound), not to measured
ones."""
import math
import os
import struct

import numpy as np
import pytest
import torch

from conftest import DATA
from xflow_amd import native
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig, TrainConfig
from xflow_amd.engine import Batch, Engine
from xflow_amd.metrics import reference_auc

DEVS = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
TILE = 4096          # rows per radix / scan tile of the kernels (kRsTile)
CHUNK = 256 * TILE   # rows one round of the one-workgroup scans over the tiles covers (kBlock tiles)
CPU_MAX = 300_000    # larger cases run on the GPU only
F32 = np.float32


def _dev(name):
    return torch.device("cuda", 0) if name == "cuda" else torch.device("cpu")


_engines = {}


def _engine(devname):
    if devname not in _engines:
        _engines[devname] = Engine(ModelConfig(), OptimConfig(), EngineConfig(table_log2_cap=8),
                                   device=_dev(devname))
    return _engines[devname]


# ---- the definition, in numpy ---------------------------------------------------
def _key_bits(p):
    """Bits of (p > 0 ? p : +0.0f): NaN, -0.0, 0.0 and negatives are +0.0."""
    with np.errstate(invalid="ignore"):
        k = np.where(p > 0, p, F32(0.0)).astype(F32)
    return k.view(np.uint32)


def _sorted(p, y):
    """(key bits, labels as 0 / 1) in the defined order."""
    bits = _key_bits(p)
    order = np.argsort(~bits, kind="stable")
    with np.errstate(invalid="ignore"):
        lab = (y > F32(0.5)).astype(np.int64)
    return bits[order], lab[order]


def _np_metrics(p, y):
    _, ys = _sorted(p, y)
    tp_before = np.cumsum(ys) - ys  # (exact integer sums)
    area = int(tp_before[ys == 0].sum())
    return area, int(ys.sum())


def _sum_bound(n, abs_sum):
    """Allowed |computed - reference| for a double sum of n logarithm terms
    whose absolute values sum to abs_sum, the reference being math.fsum (one
    rounding at most) of float64 terms: (n + 3) * 2^-53 * abs_sum.

    With u = 2^-53: a floating-point sum of n terms in ANY order (sequential
    on the CPU, per-thread / wave / workgroup partials on the device) is off
    by at most (n - 1) u sum|t_i| to first order; every term is one double
    log of an exactly representable argument (pc is a float; 1 - pc is exact
    in double), allowed 2 ulp = 4 u of itself between the implementation
    under test and numpy's.  (n - 1) u + 4 u = (n + 3) u."""
    return (n + 3) * 2.0 ** -53 * abs_sum


def _ln_reference(p, y):
    """(sum of -ln likelihood with p clipped in float32, allowed difference)."""
    n = len(p)
    pc = np.fmin(np.fmax(p, F32(1e-7)), F32(1) - F32(1e-7))
    assert pc.dtype == F32
    pc = pc.astype(np.float64)
    with np.errstate(invalid="ignore"):
        pos = y > F32(0.5)
    terms = np.where(pos, -np.log(pc), -np.log(1.0 - pc))
    assert (terms > 0).all()
    return math.fsum(terms.tolist()), _sum_bound(n, math.fsum(np.abs(terms).tolist()))


def _log2_reference(p, y):
    """(sum of y*log2(p) + (1-y)*log2(1-p), allowed difference) for p in (0, 1),
    normal.  As in k_logloss / the reference printer a positive row's term is
    a FLOAT log2f(p), allowed 4 float ulp (4 * 2^-24 relative) of error, a
    negative row's a double log2 of the exact 1 - p; the sum as in _sum_bound."""
    n = len(p)
    p64 = p.astype(np.float64)
    pos = y > F32(0.5)
    terms = np.where(pos, np.log2(p64), np.log2(1.0 - p64))
    abs_sum = math.fsum(np.abs(terms).tolist())
    bound = 4 * 2.0 ** -24 * math.fsum(np.abs(terms[pos]).tolist()) + _sum_bound(n, abs_sum)
    return math.fsum(terms.tolist()), bound


def _reference(p, y):
    n = len(p)
    area, tp = _np_metrics(p, y)
    ref = dict(n=n, tp=tp, area=area, ln=None, log2=None)
    if n and not np.isnan(p).any():
        ref["ln"] = _ln_reference(p, y)
    if n and ((p >= np.finfo(F32).tiny) & (p < 1)).all():  # (0, 1), no denormals
        ref["log2"] = _log2_reference(p, y)
    return ref


def _fbits(v):
    return struct.pack("<d", v) if isinstance(v, float) else v


def _run(devname, p, y):
    dev = _dev(devname)
    return _engine(devname).eval_metrics(torch.from_numpy(p.copy()).to(dev),
                                         torch.from_numpy(y.copy()).to(dev))


def _check(r, ref, what=""):
    n, tp, area = ref["n"], ref["tp"], ref["area"]
    assert (r["n"], r["tp"], r["area"]) == (n, tp, area), (what, r["n"], r["tp"], r["area"], ref)
    if 0 < tp < n:
        # eval_result: float area; area /= double(tp * (n - tp))
        auc = float(F32(np.float64(F32(area)) / np.float64(tp * (n - tp))))
        assert r["auc"] == auc, (what, r["auc"], auc)
        assert "auc = " in r["line"] and "tp = %d fp = %d" % (tp, n - tp) in r["line"]
    else:
        assert math.isnan(r["auc"]) and "tp_n = %d" % tp in r["line"], (what, r["auc"], r["line"])
    assert r["ln_logloss"] == (r["ln_sum"] / n if n else 0.0)
    if ref["ln"] is not None:
        s, bound = ref["ln"]
        print(what, "ln_sum", r["ln_sum"], "reference", s, "diff", abs(r["ln_sum"] - s),
              "bound", bound)
        assert math.isfinite(r["ln_sum"]) and abs(r["ln_sum"] - s) <= bound
    if ref["log2"] is not None:
        s, bound = ref["log2"]
        print(what, "log2_sum", r["log2_sum"], "reference", s, "diff", abs(r["log2_sum"] - s),
              "bound", bound)
        assert abs(r["log2_sum"] - s) <= bound
        assert r["logloss_printed"] == float(F32(r["log2_sum"]) / F32(n))


def _check_twice(devname, p, y, ref, what):
    r = _run(devname, p, y)
    _check(r, ref, what)
    r1 = _run(devname, p, y)
    assert set(r) == set(r1)
    for k in r:
        assert _fbits(r[k]) == _fbits(r1[k]), (what, k, r[k], r1[k])  # (floats: bit-identical)
    return r


# ---- the cases -------------------------------------------------------------------
ROWS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 3 * TILE + 1)
OUTSIDE = (-0.0, 0.0, -0.5, -0.2, -np.inf, np.nan, 1.0, 1.5, np.inf)
LABELS = (0.5, 0.5000001, -1.0, 2.0, np.nan, 0.0, 1.0)
SINGLE = ("all_pos", "all_neg", "first_pos", "last_pos")
CHUNKS = (CHUNK, CHUNK + 1, 2 * CHUNK + 1)  # 256, 257 and 513 tiles

CASES = (["rows_%d" % n for n in ROWS] + ["empty", "all_bits", "all_bits_wide"] +
         ["one_byte_%d" % b for b in range(4)] + ["all_equal", "few_values"] +
         ["%s_%d" % (k, n) for k in SINGLE for n in (1, TILE + 1)] +
         ["outside", "outside_nonan", "labels"] + ["chunks_%d" % n for n in CHUNKS])


def _uniform(rng, n):
    return (rng.random(n).astype(F32) * F32(0.999) + F32(1e-6)).astype(F32)


def _labels(rng, n):
    return (rng.random(n) < 0.3).astype(F32)


def _byte_values(bits, b):
    return np.unique((bits >> np.uint32(8 * b)) & np.uint32(0xFF))


def _build(name):
    """(p, y) of a case; what the case claims about its input is asserted here."""
    rng = np.random.default_rng(sum(name.encode()) * 7919 + len(name))
    kind, _, arg = name.rpartition("_")
    if name == "empty":
        return np.zeros(0, F32), np.zeros(0, F32)
    if kind == "rows":
        n = int(arg)
        return _uniform(rng, n), _labels(rng, n)
    if name in ("all_bits", "all_bits_wide"):
        # every bit pattern of (0, 1) -- or of (0, +inf] -- equally likely: every
        # exponent, denormals, and every value a radix byte of a key can take
        # (the top byte of a key's float bits cannot exceed 0x3F below 1, 0x7F at all)
        n, hi = 20_000, 0x3F7FFFFF if name == "all_bits" else 0x7F800000
        bits = rng.integers(1, hi + 1, n, dtype=np.uint32)
        bits[:2] = (1, hi)
        for b in range(3):
            assert len(_byte_values(bits, b)) == 256
        assert np.array_equal(_byte_values(bits, 3), np.arange((hi >> 24) + 1))
        p = bits.view(F32)
        assert (p > 0).all() and (p < np.finfo(F32).tiny).any() and not np.isnan(p).any()
        assert len(np.unique((bits >> np.uint32(23)))) == (hi >> 23) + 1  # every exponent
        return p, _labels(rng, n)
    if kind == "one_byte":
        # three bytes shared, byte b random: pass b alone carries the order and
        # the other three passes must keep it
        b, n = int(arg), 3 * TILE + 1
        lo, hi = (1, 0x40) if b == 3 else (0, 0x100)  # normal, below 1
        base = np.uint32(0x3E5AA53C) & ~np.uint32(0xFF << (8 * b))
        bits = base | (rng.integers(lo, hi, n, dtype=np.uint32) << np.uint32(8 * b))
        assert len(_byte_values(bits, b)) == hi - lo
        assert all(len(_byte_values(bits, o)) == 1 for o in range(4) if o != b)
        return bits.view(F32), _labels(rng, n)
    if name == "all_equal":
        n = 3 * TILE + 1
        return np.full(n, 0.3, F32), _labels(rng, n)
    if name == "few_values":
        n = 20_000
        vals = np.array([1e-30, 0.001, 0.25, 0.25000003, 0.5, 0.75, 0.999], F32)
        p = vals[rng.integers(0, len(vals), n)]
        assert len(np.unique(p)) == 7
        return p, _labels(rng, n)
    if kind in SINGLE:
        n = int(arg)
        y = np.full(n, 1.0 if kind == "all_pos" else 0.0, F32)
        if kind == "first_pos":
            y[0] = 1.0
        if kind == "last_pos":
            y[-1] = 1.0
        return _uniform(rng, n), y
    if name in ("outside", "outside_nonan"):
        n = TILE + 1
        special = np.array([v for v in OUTSIDE if name == "outside" or not np.isnan(v)], F32)
        pick = rng.integers(0, len(special), n)
        p = np.where(rng.random(n) < 0.5, _uniform(rng, n), special[pick]).astype(F32)
        for v in special:  # every value is there, bit for bit (-0.0 is not 0.0)
            assert (p.view(np.uint32) == np.array([v], F32).view(np.uint32)[0]).sum() > 10
        return p, _labels(rng, n)
    if name == "labels":
        n = TILE + 1
        vals = np.array(LABELS, F32)
        assert vals[1] > F32(0.5) and vals[1] < F32(0.5000002)
        y = vals[rng.integers(0, len(vals), n)]
        assert all((y.view(np.uint32) == v.view(np.uint32)).any() for v in vals)
        return _uniform(rng, n), y
    if kind == "chunks":
        n = int(arg)
        p = np.clip(np.round(rng.random(n) * 1000) / 1000, 0.001, 0.999).astype(F32)
        y = _labels(rng, n)
        # the row ranked last is a negative: with 257 tiles it is the only row
        # of the second round, and only a negative adds the carried positives
        y[np.argsort(~_key_bits(p), kind="stable")[-1]] = 0.0
        return p, y
    raise KeyError(name)


_cases = {}


def _case(name):
    """(p, y, reference); computed once, shared, read-only."""
    if name not in _cases:
        p, y = _build(name)
        assert p.dtype == F32 and y.dtype == F32 and len(p) == len(y)
        for a in (p, y):
            a.setflags(write=False)
        _cases[name] = (p, y, _reference(p, y))
    return _cases[name]


def _rows_of(name):
    kind, _, arg = name.rpartition("_")
    return int(arg) if kind == "chunks" else 0


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("name", CASES)
def test_eval_metrics_cases(devname, name):
    if devname == "cpu" and _rows_of(name) > CPU_MAX:
        pytest.skip("large case on the GPU only")
    p, y, ref = _case(name)
    n = len(p)
    r = _check_twice(devname, p, y, ref, name)
    if name == "empty":
        assert r["n"] == r["tp"] == r["area"] == 0 and math.isnan(r["auc"])
        assert r["log2_sum"] == 0.0 and r["ln_sum"] == 0.0 and r["ln_logloss"] == 0.0
    if name.startswith("rows_") or name in ("few_values", "all_equal", "labels") or \
            name.startswith(("one_byte", "chunks")):
        assert ref["log2"] is not None and ref["ln"] is not None
    if name in ("all_bits", "all_bits_wide", "outside_nonan"):
        assert ref["log2"] is None and ref["ln"] is not None
    if name == "outside":
        assert ref["log2"] is None and ref["ln"] is None
        # every row that is not > 0 ranks after every row that is, in input order
        bs, _ = _sorted(p, y)
        with np.errstate(invalid="ignore"):
            k = int((p > 0).sum())
        assert (bs[:k] > 0).all() and (bs[k:] == 0).all() and 0 < k < n
    if name.startswith(("all_pos", "all_neg")) or name in ("first_pos_1", "last_pos_1"):
        assert ref["tp"] in (0, n) and ref["area"] == 0
    if name in ("first_pos_%d" % (TILE + 1), "last_pos_%d" % (TILE + 1)):
        assert ref["tp"] == 1
    if name.startswith("chunks"):
        # from the sorted reference: tie runs lie across tile boundaries and
        # across the boundary between two rounds of the scans over the tiles
        bs, ys = _sorted(p, y)
        assert len(np.unique(bs)) <= 1000
        for c in range(CHUNK, n, CHUNK):  # a lost carry would show: negatives after positives
            assert ys[:c].sum() > 0 and (ys[c:] == 0).any()
        cuts = np.arange(TILE, n, TILE)
        assert (bs[cuts - 1] == bs[cuts]).sum() > 0.9 * len(cuts)
        assert (n + TILE - 1) // TILE in (256, 257, 513)
        if n > CHUNK:
            assert bs[CHUNK - 1] == bs[CHUNK], "no tie run spans rows 256*4096-1 | 256*4096"
        if n > 2 * CHUNK:
            assert bs[2 * CHUNK - 1] == bs[2 * CHUNK]


def test_reference_is_the_definition():
    """The numpy reference on inputs small enough to count by hand."""
    nan, inf = np.nan, np.inf
    # keys: 0.5, 0, 0, 0, inf, 0, 2.0 -> order inf, 2.0, 0.5, then rows 1 2 3 5 as they come
    p = np.array([0.5, -0.0, nan, -3.0, inf, 0.0, 2.0], F32)
    y = np.array([0, 1, 0, 1, 1, 0, 0], F32)
    bs, ys = _sorted(p, y)
    assert ys.tolist() == [1, 0, 0, 1, 0, 1, 0] and (bs[3:] == 0).all()
    assert _np_metrics(p, y) == (1 + 1 + 2 + 3, 3)
    assert _key_bits(np.array([-0.0, nan, -inf, 1e-45], F32)).tolist() == [0, 0, 0, 1]
    # the clip is a float32 clip: 1 - 1e-7 is 1 - 2^-23 there
    s, _ = _ln_reference(np.array([1.0], F32), np.array([1.0], F32))
    assert s == -math.log(1.0 - 2.0 ** -23)


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("n,ties", [(200, False), (5000, True), (1_000_003, False)])
def test_eval_metrics_exact_area(devname, n, ties):
    if devname == "cpu" and n > 100000:
        pytest.skip("large case on the GPU only")
    rng = np.random.default_rng(n)
    p = rng.random(n).astype(np.float32) * 0.999 + 1e-6
    if ties:
        p = (np.round(p * 50) / 50 + 1e-6).astype(np.float32)
    y = (rng.random(n) < 0.3).astype(np.float32)
    ref = _reference(p, y)
    assert ref["ln"] is not None and (ties or ref["log2"] is not None)
    r = _check_twice(devname, p, y, ref, "n=%d" % n)
    if n <= 5000 and not ties:  # the reference printer (float accumulators) agrees exactly
        pr = reference_auc(y.astype(np.int32), p)
        assert r["line"] == pr["line"], (r["line"], pr["line"])


@pytest.mark.parametrize("devname", DEVS)
def test_trainer_eval_on_bundled_data(devname, tmp_path):
    """Bundled data: the trainer prints the reference's line (reference_auc of
    its predictions, pred file written) and logs the device AUC, which equals
    the stable-tie definition of the same predictions."""
    import json

    from xflow_amd.trainer import Trainer

    cfg = TrainConfig(train_prefix=os.path.join(DATA, "small_train"),
                      test_prefix=os.path.join(DATA, "small_test"), epochs=10, threads=8,
                      pred_dir=str(tmp_path), model=ModelConfig(kind="lr"),
                      metrics_file=str(tmp_path / "m.jsonl"),
                      engine=EngineConfig(table_log2_cap=14))
    tr = Trainer(cfg, device=_dev(devname))
    res = tr.train()
    pred = np.loadtxt(tmp_path / "pred_0_0.txt")
    ref = reference_auc(pred[:, 2].astype(np.int32), pred[:, 0].astype(np.float32))
    assert res["line"] == ref["line"] and res["n"] == 200
    ev = [json.loads(l) for l in open(tmp_path / "m.jsonl") if '"eval"' in l][-1]
    p, y = pred[:, 0].astype(np.float32), pred[:, 2].astype(np.float32)
    area, tp = _np_metrics(p, y)
    # (pred file values are %g-rounded: equal up to the rounding's ties)
    assert abs(ev["auc_device"] - area / (tp * (200 - tp))) < 2e-3
    # the unrounded predictions, from the same engine on the same rows (a
    # deterministic forward): the logged device AUC is the definition's, exactly
    dev = _dev(devname)
    blk = native.load().BlockReader(os.path.join(DATA, "small_test-00000"), 4 << 20).next()
    labels = np.asarray(blk["labels"]).astype(np.float32)
    b = Batch(keys=torch.from_numpy(np.asarray(blk["keys"]).astype(np.uint64).view(np.int64)).to(dev),
              labels=torch.from_numpy(labels).to(dev),
              row_ptr=torch.from_numpy(np.asarray(blk["row_ptr"]).astype(np.int32)).to(dev))
    pt = tr.engine.eval_step(b)
    pn = pt.cpu().numpy()
    assert len(pn) == 200 and (np.abs(pn - p) <= 1e-5 * p).all()  # (the file's %g rounding)
    full = _reference(pn, labels)
    r = tr.engine.eval_metrics(pt, b.labels)
    _check(r, full, "bundled")
    assert full["ln"] is not None and full["log2"] is not None and 0 < full["tp"] < 200
    assert ev["auc_device"] == r["auc"]
