"""Grouped evaluation on the device (Engine.eval_grouped / row_group_keys,
csrc/hip/kernels_eval.hip, GroupedEval in csrc/include/xflow/backend.h)
against a numpy definition written here: np.lexsort by (-pctr bits, group),
then integer pair counts per group -- brute force O(n_g^2) for small groups,
a rank formula (searchsorted over the positives) for the rest.  The per-group
integers must match exactly; the two double sums within (G + 2) * 2^-52
relative (each term is one correctly rounded division of exact integers, the
sum has G non-negative terms)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import DATA
from xflow_amd import native
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig, TrainConfig
from xflow_amd.engine import Batch, Engine

DEVS = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
NOGROUP = np.uint64(0xFFFFFFFFFFFFFFFF)
TILE = 4096  # rows per radix / scan tile of the kernels
BRUTE = 64   # groups up to this size are counted pair by pair


def _dev(name):
    return torch.device("cuda", 0) if name == "cuda" else torch.device("cpu")


_engines = {}


def _engine(devname):
    if devname not in _engines:
        _engines[devname] = Engine(ModelConfig(), OptimConfig(), EngineConfig(table_log2_cap=8),
                                   device=_dev(devname))
    return _engines[devname]


def _key(p):
    """p > 0 ? p : +0.0f -- the value both the order and the fixed-point sum use
    (eval_key_bits, backend.h): NaN, -0.0 and negatives are +0.0."""
    with np.errstate(invalid="ignore"):
        return np.where(p > 0, p, np.float32(0)).astype(np.float32)


def _bits(p):
    return _key(p).view(np.uint32).astype(np.int64)


def _sorted_order(p, g):
    return np.lexsort((-_bits(p), g))


def _reference(p, y, g, brute=True):
    """The definitions, in numpy: (scalars, table) with the table in
    ascending key order, integers as Python-exact int64 / uint64 arrays."""
    n = len(p)
    b = _bits(p)
    with np.errstate(invalid="ignore"):
        lab = y > 0.5
    fx = np.rint(_key(p).astype(np.float64) * 2.0 ** 32).astype(np.int64)
    ing = g != NOGROUP
    keys, rank = np.unique(g[ing], return_inverse=True)
    G = len(keys)
    bi, li, fi = b[ing], lab[ing], fx[ing]
    n_g = np.bincount(rank, minlength=G).astype(np.int64)
    pos_g = np.zeros(G, np.int64)
    np.add.at(pos_g, rank[li], 1)
    sump = np.zeros(G, np.int64)
    np.add.at(sump, rank, fi)
    # rank formula: per negative, the positives of its group above it (x2) and tied with it
    comp = rank.astype(np.int64) * (1 << 32) + bi
    pc = np.sort(comp[li])
    cn, rn = comp[~li], rank[~li]
    hi = np.searchsorted(pc, (rn.astype(np.int64) + 1) * (1 << 32), "left")
    right = np.searchsorted(pc, cn, "right")
    left = np.searchsorted(pc, cn, "left")
    area2 = np.zeros(G, np.int64)
    np.add.at(area2, rn, 2 * (hi - right) + (right - left))
    if brute:
        order = np.argsort(rank, kind="stable")
        start = np.concatenate(([0], np.cumsum(n_g)))
        for k in np.flatnonzero(n_g <= BRUTE):
            rows = order[start[k]: start[k + 1]]
            bp, bn = bi[rows][li[rows]], bi[rows][~li[rows]]
            a = int((2 * (bp[:, None] > bn[None, :]) + (bp[:, None] == bn[None, :])).sum())
            assert a == area2[k]  # the two counts of the reference agree
    used = (pos_g > 0) & (pos_g < n_g)
    neg_g = n_g - pos_g
    terms = (n_g[used].astype(np.float64) * area2[used].astype(np.float64)) / (
        2.0 * pos_g[used].astype(np.float64) * neg_g[used].astype(np.float64))
    cal = np.abs(sump.astype(np.float64) * 2.0 ** -32 - pos_g.astype(np.float64))
    sc = dict(n=n, n_nogroup=int(n - ing.sum()), groups=G, groups_used=int(used.sum()),
              rows_used=int(n_g[used].sum()), gauc_num=math.fsum(terms), cal_abs=math.fsum(cal))
    tab = dict(key=keys.astype(np.uint64), n=n_g, pos=pos_g, area2=area2.astype(np.uint64),
               sump=sump)
    return sc, tab


def _run(devname, p, y, g, per_group=True):
    dev = _dev(devname)
    t = [torch.from_numpy(a.copy()).to(dev) for a in (p, y, g.view(np.int64))]  # (shared inputs stay read-only)
    return _engine(devname).eval_grouped(t[0], t[1], t[2], per_group=per_group)


INT_SCALARS = ("n", "n_nogroup", "groups", "groups_used", "rows_used")


def _check(r, sc, tab):
    for k in INT_SCALARS:
        assert r[k] == sc[k], (k, r[k], sc[k])
    t = r["per_group"]
    for k in ("key", "n", "pos", "area2", "sump"):
        assert t[k].dtype == tab[k].dtype, (k, t[k].dtype)
        assert np.array_equal(t[k], tab[k]), k
    tol = (sc["groups"] + 2) * 2.0 ** -52
    print("gauc_num", r["gauc_num"], sc["gauc_num"], "cal_abs", r["cal_abs"], sc["cal_abs"])
    assert abs(r["gauc_num"] - sc["gauc_num"]) <= tol * sc["gauc_num"]
    assert abs(r["cal_abs"] - sc["cal_abs"]) <= tol * sc["cal_abs"]
    if sc["groups_used"] == 0:
        assert r["gauc"] is None and r["coverage"] == 0.0
    else:
        assert r["gauc"] == r["gauc_num"] / r["rows_used"] and 0.0 <= r["gauc"] <= 1.0
        assert r["coverage"] == r["rows_used"] / r["n"]
    if sc["n"] > sc["n_nogroup"]:
        assert r["group_cal_error"] == r["cal_abs"] / (sc["n"] - sc["n_nogroup"])


def _power_law_case(seed=11):
    """n = 2 tiles + 5: power-law group sizes with one group larger than a
    tile, rows of a group interleaved in the input, pctr quantised to 1/50,
    all-positive and all-negative groups, ~3 % rows without a group, and keys
    that make every digit pass matter."""
    rng = np.random.default_rng(seed)
    n = 2 * TILE + 5
    n_no = int(0.03 * n)
    big = TILE + 300
    base = np.uint64(0x4123456789ABCDEF)
    special = [np.uint64(5), base, base ^ np.uint64(0xFF << 56), base ^ np.uint64(0x01),
               np.uint64(0x8000000000000000), np.uint64(0xFFFFFFFFFFFFFFFE),
               np.uint64(0x00000000000000FF), np.uint64(0x01000000000000FF)]
    nk = 160
    keys = np.concatenate((np.array(special, np.uint64),
                           rng.integers(0, 1 << 64, nk - len(special), dtype=np.uint64)))
    assert len(np.unique(keys)) == nk and not (keys == NOGROUP).any()
    assert (keys >= np.uint64(1 << 63)).sum() >= 3
    # group 0 (the smallest key) is the large one; the others follow a power law
    w = 1.0 / np.arange(1, nk) ** 1.2
    rest = n - n_no - big
    sizes = np.maximum(1, np.floor(w / w.sum() * (rest - (nk - 1))).astype(np.int64) + 1)
    sizes[0] += rest - sizes.sum()
    assert sizes.sum() == rest and sizes.min() >= 1
    g = np.concatenate((np.repeat(keys, np.concatenate(([big], sizes))),
                        np.full(n_no, NOGROUP, np.uint64)))
    p = np.clip(np.round(rng.random(n) * 50) / 50, 0.02, 0.98).astype(np.float32)
    y = (rng.random(n) < 0.3).astype(np.float32)
    for k in (keys[1], keys[3], keys[20], keys[100]):  # all positive
        y[g == k] = 1.0
    for k in (keys[2], keys[4], keys[21], keys[101]):  # all negative
        y[g == k] = 0.0
    perm = rng.permutation(n)  # interleave the groups' rows
    return p[perm], y[perm], g[perm]


OUTSIDE = (-0.0, 0.0, -0.5, -0.2, -np.inf, np.nan)
OUTSIDE_KEY = np.uint64(0x7000000000000001)  # a group of such rows only


def _outside_case(seed=13):
    """Predictions that are not > 0 inside the groups: -0.0, 0.0, negatives,
    -inf and NaN next to quantised p in (0, 1], in 40 groups over a tile
    boundary, one group made of such rows only, and rows without a group."""
    rng = np.random.default_rng(seed)
    n = TILE + 500
    keys = rng.integers(0, 1 << 62, 40, dtype=np.uint64)
    assert len(np.unique(keys)) == 40
    g = keys[rng.integers(0, 40, n)]
    g[rng.random(n) < 0.03] = NOGROUP
    special = np.array(OUTSIDE, np.float32)
    p = np.where(rng.random(n) < 0.4, special[rng.integers(0, len(special), n)],
                 np.round(rng.random(n) * 20) / 20).astype(np.float32)
    g[:300] = OUTSIDE_KEY
    p[:300] = special[np.arange(300) % len(special)]
    y = (rng.random(n) < 0.4).astype(np.float32)
    for v in special:  # bit for bit: -0.0 is not 0.0
        assert (p.view(np.uint32) == v.view(np.uint32)).sum() > 50
    perm = rng.permutation(n)
    return p[perm], y[perm], g[perm]


_cases = {}


def _case(name):
    """(p, y, g, reference scalars, reference table); computed once, shared."""
    if name not in _cases:
        rng = np.random.default_rng(3)
        if name == "empty":
            p, y, g = np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint64)
        elif name == "one":
            p, y, g = (np.array([0.25], np.float32), np.array([1.0], np.float32),
                       np.array([1 << 63], np.uint64))
        elif name == "one_group":
            p = (rng.permutation(200) / 211.0 + 0.01).astype(np.float32)  # no ties
            y = (rng.random(200) < 0.3).astype(np.float32)
            g = np.full(200, 0x0123456789ABCDEF, np.uint64)
        elif name == "singletons":
            p = (np.round(rng.random(3000) * 50) / 50).astype(np.float32)
            y = (rng.random(3000) < 0.3).astype(np.float32)
            g = rng.permutation(np.arange(3000, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
        elif name == "power_law":
            p, y, g = _power_law_case()
        elif name == "outside":
            p, y, g = _outside_case()
        else:
            raise KeyError(name)
        for a in (p, y, g):
            a.setflags(write=False)
        _cases[name] = (p, y, g) + _reference(p, y, g)
    return _cases[name]


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("name", ["empty", "one", "one_group", "singletons", "power_law",
                                  "outside"])
def test_grouped_exact_integers_and_sums(devname, name):
    p, y, g, sc, tab = _case(name)
    r = _run(devname, p, y, g)
    _check(r, sc, tab)
    if name == "outside":
        # rows that are not > 0 tie with each other (a pair of them is worth 1
        # in area2, whatever their values) and add 0 to sump
        t = r["per_group"]
        k = int(np.flatnonzero(t["key"] == OUTSIDE_KEY)[0])
        assert t["n"][k] == 300 and 0 < t["pos"][k] < 300
        assert int(t["area2"][k]) == int(t["pos"][k]) * int(300 - t["pos"][k])
        assert t["sump"][k] == 0
        with np.errstate(invalid="ignore"):
            low = ~(p > 0)
        for kk in (0, 7, 39):  # mixed groups: the same from the definition
            rows = g == t["key"][kk] if t["key"][kk] != OUTSIDE_KEY else None
            if rows is None:
                continue
            pos, neg = rows & (y > 0.5), rows & ~(y > 0.5)
            a2 = 0
            for i in np.flatnonzero(pos):
                for j in np.flatnonzero(neg):
                    if low[i] and low[j]:
                        a2 += 1
                    elif low[j] or (not low[i] and p[i] > p[j]):
                        a2 += 2
                    elif not low[i] and p[i] == p[j]:
                        a2 += 1
            assert int(t["area2"][kk]) == a2, kk
            assert int(t["sump"][kk]) == int(np.rint(p[rows & ~low].astype(np.float64)
                                                     * 2.0 ** 32).sum())
    if name == "one_group":
        assert len(np.unique(p)) == len(p) and sc["groups"] == 1
        m = _engine(devname).eval_metrics(torch.from_numpy(p.copy()).to(_dev(devname)),
                                          torch.from_numpy(y.copy()).to(_dev(devname)))
        assert int(r["per_group"]["area2"][0]) == 2 * m["area"]
    if name == "singletons":
        assert r["groups"] == 3000 and r["groups_used"] == 0 and r["gauc"] is None
    if name == "empty":
        assert r["groups"] == 0 and r["gauc"] is None and len(r["per_group"]["key"]) == 0
    # without the table the scalars are the same
    r2 = _run(devname, p, y, g, per_group=False)
    assert "per_group" not in r2
    assert all(r2[k] == r[k] for k in INT_SCALARS + ("gauc_num", "cal_abs"))


def test_power_law_case_is_what_it_claims():
    """From the sorted reference: a group and a tie run straddle a tile
    boundary, a group is larger than a tile, degenerate groups and rows
    without a group exist, and every byte of the keys varies."""
    p, y, g, sc, tab = _case("power_law")
    o = _sorted_order(p, g)
    gs, bs = g[o], _bits(p)[o]
    assert np.array_equal(gs, np.sort(g)) and gs[-1] == NOGROUP
    cuts = [t for t in range(TILE, len(p), TILE)]
    in_groups = [t for t in cuts if gs[t] != NOGROUP and gs[t - 1] == gs[t]]
    assert in_groups, "no group straddles a tile boundary"
    assert any(bs[t - 1] == bs[t] for t in in_groups), "no tie run straddles a tile boundary"
    assert tab["n"].max() > TILE
    assert ((tab["pos"] == tab["n"]) & (tab["n"] > 1)).sum() >= 2
    assert ((tab["pos"] == 0) & (tab["n"] > 1)).sum() >= 2
    assert 0.02 * len(p) < sc["n_nogroup"] < 0.04 * len(p)
    k = tab["key"]
    assert (k >= np.uint64(1 << 63)).any()
    x = k[:, None] ^ k[None, :]
    assert (x == np.uint64(0xFF << 56)).any() and (x == np.uint64(1)).any()
    for byte in range(8):
        assert len(np.unique((k >> np.uint64(8 * byte)) & np.uint64(0xFF))) > 1
    # ties inside groups: the tie-aware count differs from a strict one
    assert len(np.unique(p)) <= 51


@pytest.mark.parametrize("devname", DEVS)
def test_grouped_order_free_and_deterministic(devname):
    p, y, g, sc, tab = _case("power_law")
    r0 = _run(devname, p, y, g)
    r1 = _run(devname, p, y, g)
    perm = np.random.default_rng(5).permutation(len(p))
    r2 = _run(devname, p[perm].copy(), y[perm].copy(), g[perm].copy())
    for r in (r1, r2):
        for k in INT_SCALARS + ("gauc_num", "cal_abs", "gauc", "coverage", "group_cal_error"):
            assert r[k] == r0[k], k  # (floats: bit-identical)
        for k in ("key", "n", "pos", "area2", "sump"):
            assert np.array_equal(r["per_group"][k], r0["per_group"][k]), k


@pytest.mark.gpu
def test_grouped_large_gpu():
    """n = 1 000 003 rows in 50 000 power-law groups with ties: the integers
    against the rank-formula reference."""
    rng = np.random.default_rng(17)
    n, G = 1_000_003, 50_000
    keys = np.unique(rng.integers(0, 1 << 64, G + 16, dtype=np.uint64))
    keys = rng.permutation(keys[keys != NOGROUP])[:G]
    gi = np.minimum((G * rng.random(n) ** 3).astype(np.int64), G - 1)  # power-law sizes
    g = keys[gi]
    g[rng.random(n) < 0.01] = NOGROUP
    p = np.clip(np.round(rng.random(n) * 50) / 50, 0.02, 0.98).astype(np.float32)
    y = (rng.random(n) < 0.3).astype(np.float32)
    sc, tab = _reference(p, y, g, brute=False)
    assert tab["n"].max() > 2 * TILE and sc["groups"] > 40_000
    _check(_run("cuda", p, y, g), sc, tab)


CHUNK = 256 * TILE  # rows (or runs) one round of the one-workgroup scans over the tiles covers


@pytest.mark.gpu
def test_grouped_chunks_gpu():
    """n = 2 097 153 rows (513 tiles) in 120 000 power-law groups with ties:
    past the point where the one-workgroup scans over the tiles (k_rs_scan of
    the sort passes, k_gr_carry, k_gr_carry64) take a second and a third round
    of 256 tiles with a running carry.  The smallest n that reaches each loop:
    the scans over row tiles at n = 256 * 4096 + 1 = 1 048 577; the run-level
    scan (k_gr_runs / k_gr_carry64 / k_gr_runscan tile the RUNS by 4096) needs
    more than 256 * 4096 tie runs -- this case has 1.35 M (0.65 a row); the
    least n with that many runs is 1 048 577 rows, each a run of its own;
    k_gr_groups has no such loop (one lane per group, 4096 groups per
    workgroup, partials summed in order by k_gr_final): more than one
    workgroup of it from 4097 groups on."""
    rng = np.random.default_rng(37)
    n, G = 2 * CHUNK + 1, 120_000
    keys = np.unique(rng.integers(0, 1 << 64, G + 16, dtype=np.uint64))
    keys = rng.permutation(keys[keys != NOGROUP])[:G]
    gi = np.minimum((G * rng.random(n) ** 3).astype(np.int64), G - 1)  # power-law sizes
    g = keys[gi]
    g[rng.random(n) < 0.01] = NOGROUP
    p = np.clip(np.round(rng.random(n) * 50) / 50, 0.02, 0.98).astype(np.float32)
    y = (rng.random(n) < 0.3).astype(np.float32)
    sc, tab = _reference(p, y, g, brute=False)
    o = _sorted_order(p, g)
    gs, bs = g[o], _bits(p)[o]
    runs = 1 + int(((gs[1:] != gs[:-1]) | (bs[1:] != bs[:-1])).sum())
    assert (n + TILE - 1) // TILE > 512
    assert runs / TILE > 256, runs
    assert sc["groups"] / TILE > 1 and 0.005 * n < sc["n_nogroup"] < 0.015 * n
    assert gs[CHUNK - 1] == gs[CHUNK] != NOGROUP, "no group straddles row 256 * 4096"
    assert bs[CHUNK - 1] == bs[CHUNK], "no tie run straddles row 256 * 4096"
    _check(_run("cuda", p, y, g), sc, tab)


@pytest.mark.gpu
def test_one_group_past_a_chunk_gpu():
    """All n = 1 048 577 rows (257 tiles) in one group: area2 is the tie-aware
    pair count of the whole set (rank-formula reference), and with all p
    distinct it is twice eval_metrics' area."""
    rng = np.random.default_rng(41)
    n = CHUNK + 1
    g = np.full(n, 0x0123456789ABCDEF, np.uint64)
    y = (rng.random(n) < 0.3).astype(np.float32)
    tied = np.clip(np.round(rng.random(n) * 50) / 50, 0.02, 0.98).astype(np.float32)
    distinct = ((rng.permutation(n) + 1) / 2.0 ** 21).astype(np.float32)  # exact in float32
    assert len(np.unique(distinct)) == n and distinct.min() > 0 and distinct.max() < 1
    for p in (tied, distinct):
        sc, tab = _reference(p, y, g, brute=False)
        assert sc["groups"] == 1 and tab["n"][0] == n
        r = _run("cuda", p, y, g)
        _check(r, sc, tab)
    dev = _dev("cuda")
    m = _engine("cuda").eval_metrics(torch.from_numpy(distinct).to(dev), torch.from_numpy(y).to(dev))
    assert int(r["per_group"]["area2"][0]) == 2 * m["area"] and m["tp"] == int(tab["pos"][0])


# ---- row_group_keys ---------------------------------------------------------
def _py_group_keys(keys, fgid, rows, field):
    """rows: list of occurrence-index lists; the definition as a Python loop."""
    out = []
    for occ in rows:
        k = int(NOGROUP)
        if fgid is None:
            if 0 <= field < len(occ):
                k = int(keys[occ[field]])
        else:
            for i in occ:
                if fgid[i] == field:
                    k = int(keys[i])
                    break
        out.append(k)
    return np.array(out, dtype=np.uint64)


FIELDS = (0, 1, 2, 3, 5, 7, 70, 71)


@pytest.mark.parametrize("devname", DEVS)
def test_row_group_keys_csr(devname):
    dev = _dev(devname)
    e = _engine(devname)
    rng = np.random.default_rng(2)
    # unsorted field ids, a repeated field (1 in row 0, 3 in row 3), a missing
    # field, field id 70, an empty row (2) and an empty last row
    fg_rows = [[3, 1, 70, 1, 0], [2, 0], [], [70, 3, 3, 5, 1], [7], []]
    fgid = np.array([f for r in fg_rows for f in r], np.int32)
    keys = rng.integers(0, 1 << 64, len(fgid), dtype=np.uint64)
    keys[2] = np.uint64(0xFFFFFFFFFFFFFFFE)  # a key >= 2^63 comes back bit for bit
    row_ptr = np.concatenate(([0], np.cumsum([len(r) for r in fg_rows]))).astype(np.int32)
    rows = [list(range(row_ptr[i], row_ptr[i + 1])) for i in range(len(fg_rows))]
    b = Batch(keys=torch.from_numpy(keys.view(np.int64)).to(dev),
              labels=torch.zeros(len(fg_rows), dtype=torch.float32, device=dev),
              row_ptr=torch.from_numpy(row_ptr).to(dev), fgid=torch.from_numpy(fgid).to(dev))
    for f in FIELDS:
        got = e.row_group_keys(b, f)
        assert got.dtype == torch.int64 and got.device == dev
        assert np.array_equal(got.cpu().numpy().view(np.uint64), _py_group_keys(keys, fgid, rows, f)), f
    assert e.row_group_keys(b, 1).cpu().numpy().view(np.uint64)[0] == keys[1]  # first occurrence
    nofg = Batch(keys=b.keys, labels=b.labels, row_ptr=b.row_ptr)
    with pytest.raises(ValueError):
        e.row_group_keys(nofg, 1)


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("with_fgid", [False, True])
def test_row_group_keys_fixed_width(devname, with_fgid):
    dev = _dev(devname)
    e = _engine(devname)
    rng = np.random.default_rng(4)
    R, F = 37, 3
    keys = rng.integers(0, 1 << 64, R * F, dtype=np.uint64)
    fgid = rng.integers(0, 4, R * F).astype(np.int32) if with_fgid else None
    rows = [list(range(r * F, (r + 1) * F)) for r in range(R)]
    rm = Batch(keys=torch.from_numpy(keys.view(np.int64)).to(dev),
               labels=torch.zeros(R, dtype=torch.float32, device=dev),
               fgid=torch.from_numpy(fgid).to(dev) if with_fgid else None, nnz_per_row=F)
    fm = rm.to_field_major()
    assert fm.field_major and not rm.field_major
    for f in (0, 1, 2, 3, 7):  # (without fgid: inside and >= nnz_per_row)
        want = _py_group_keys(keys, fgid, rows, f)
        if not with_fgid and f >= F:
            assert (want == NOGROUP).all()
        for b in (rm, fm):
            assert np.array_equal(e.row_group_keys(b, f).cpu().numpy().view(np.uint64), want), f


# ---- the trainer on the bundled data ------------------------------------------
def _test_rows():
    """Rows of the bundled test shard as the project's reader hashes them:
    (row_ptr, keys, fgid, labels)."""
    blk = native.load().BlockReader(os.path.join(DATA, "small_test-00000"), 4 << 20).next()
    return (np.asarray(blk["row_ptr"]), np.asarray(blk["keys"]).astype(np.uint64),
            np.asarray(blk["fgid"]), np.asarray(blk["labels"]))


def _label_counts(field):
    """groups, used, rows_used, n_nogroup of grouping the test rows on `field`:
    they depend on the keys and labels only, not on any model."""
    row_ptr, keys, fgid, labels = _test_rows()
    rows = [list(range(row_ptr[i], row_ptr[i + 1])) for i in range(len(labels))]
    g = _py_group_keys(keys, fgid, rows, field)
    ing = g != NOGROUP
    ks, rank = np.unique(g[ing], return_inverse=True)
    n_g = np.bincount(rank, minlength=len(ks))
    pos_g = np.bincount(rank, weights=(labels[ing] > 0.5), minlength=len(ks)).astype(np.int64)
    used = (pos_g > 0) & (pos_g < n_g)
    return dict(groups=len(ks), used=int(used.sum()), rows=int(n_g[used].sum()),
                n_nogroup=int((~ing).sum()), n=len(labels)), g


_trained = {}


def _trainer(devname, tmp_path_factory):
    """One LR trainer per device, trained once; predict() is then called with
    different gauc_field settings."""
    from xflow_amd.trainer import Trainer

    if devname not in _trained:
        d = tmp_path_factory.mktemp("gauc_" + devname)
        cfg = TrainConfig(train_prefix=os.path.join(DATA, "small_train"),
                          test_prefix=os.path.join(DATA, "small_test"), epochs=2, threads=8,
                          pred_dir=str(d), model=ModelConfig(kind="lr"),
                          metrics_file=str(d / "m.jsonl"), engine=EngineConfig(table_log2_cap=14))
        tr = Trainer(cfg, device=_dev(devname))
        tr.train_epochs(cfg.epochs)
        _trained[devname] = (tr, str(d / "m.jsonl"))
    return _trained[devname]


def _predict(devname, tmp_path_factory, field):
    tr, mfile = _trainer(devname, tmp_path_factory)
    tr.cfg.gauc_field = field
    res = tr.predict(0)
    ev = [json.loads(l) for l in open(mfile) if '"eval"' in l][-1]
    return tr, res, ev


GAUC_KEYS = ("gauc", "gauc_field", "gauc_groups", "gauc_groups_used", "gauc_rows_used",
             "group_cal_error")
# groups, used, rows_used, n_nogroup of data/small_test-00000 (label-only facts)
EXPECTED = {7: (70, 23, 126, 0), 16: (53, 9, 134, 5), 11: (1, None, None, 0),
            0: (0, 0, 0, 200)}


@pytest.mark.parametrize("devname", DEVS)
@pytest.mark.parametrize("field", [7, 16, 11, 0])
def test_trainer_gauc_on_bundled_data(devname, field, tmp_path_factory, capsys):
    want, g = _label_counts(field)
    groups, used, rows, nog = EXPECTED[field]
    assert want["n"] == 200 and want["groups"] == groups and want["n_nogroup"] == nog
    if used is not None:
        assert want["used"] == used and want["rows"] == rows
    tr, res, ev = _predict(devname, tmp_path_factory, field)
    out = capsys.readouterr().out
    for src in (res, ev):
        assert src["gauc_field"] == field and src["n"] == 200
        assert src["gauc_groups"] == want["groups"]
        assert src["gauc_groups_used"] == want["used"]
        assert src["gauc_rows_used"] == want["rows"]
    assert res["gauc"] == ev["gauc"] and res["group_cal_error"] == ev["group_cal_error"]
    line = [l for l in out.splitlines() if l.startswith("gauc(")]
    assert len(line) == 1 and line[0].startswith("gauc(field %d): " % field)
    assert line[0].endswith("groups=%d/%d rows=%d/%d" % (want["used"], want["groups"],
                                                         want["rows"], 200))
    # the same engine on the same rows: the same table and a deterministic
    # forward, so the logged figures are equal, not close
    dev = _dev(devname)
    row_ptr, keys, fgid, labels = _test_rows()
    b = Batch(keys=torch.from_numpy(keys.view(np.int64)).to(dev),
              labels=torch.from_numpy(labels.astype(np.float32)).to(dev),
              row_ptr=torch.from_numpy(row_ptr.astype(np.int32)).to(dev),
              fgid=torch.from_numpy(fgid.astype(np.int32)).to(dev))
    gk = tr.engine.row_group_keys(b, field)
    assert np.array_equal(gk.cpu().numpy().view(np.uint64), g)
    p = tr.engine.eval_step(Batch(keys=b.keys, labels=b.labels, row_ptr=b.row_ptr))
    r = tr.engine.eval_grouped(p, b.labels, gk, per_group=True)
    assert r["gauc"] == ev["gauc"] and r["group_cal_error"] == ev["group_cal_error"]
    assert r["n_nogroup"] == want["n_nogroup"] and r["groups"] == want["groups"]
    pn, yn = p.cpu().numpy(), labels.astype(np.float32)
    sc, tab = _reference(pn, yn, g)
    _check(r, sc, tab)
    if field == 0:
        assert ev["gauc"] is None and "none" in line[0]
    if field == 11:
        # one group of all rows: the tie-aware AUC of the 200 predictions
        bp, bn = _bits(pn)[yn > 0.5], _bits(pn)[yn <= 0.5]
        a2 = int((2 * (bp[:, None] > bn[None, :]) + (bp[:, None] == bn[None, :])).sum())
        assert int(r["per_group"]["area2"][0]) == a2 and r["rows_used"] == 200
        assert abs(ev["gauc"] - a2 / (2.0 * len(bp) * len(bn))) <= 4 * 2.0 ** -52


@pytest.mark.parametrize("devname", DEVS)
def test_trainer_gauc_off_changes_nothing(devname, tmp_path_factory, capsys):
    tr, res, ev = _predict(devname, tmp_path_factory, -1)
    out = capsys.readouterr().out
    assert not any(k in ev for k in GAUC_KEYS) and not any(k in res for k in GAUC_KEYS)
    assert set(ev) - {"time", "rank", "ts", "t"} >= {"event", "auc", "auc_device", "ln_logloss",
                                                     "logloss_printed", "n"}
    assert "gauc" not in out
