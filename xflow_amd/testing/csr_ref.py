"""Reference of the CSR gradient entries (CsrOut, csrc/include/xflow/backend.h)
and of their packed wire form, in numpy and plain Python.

A CSR step turns the producers' records into per-key entries (slice, values)
in (key, slice) order: key i of the unique list owns entries
[off[i], off[i] + cnt[i]), one per slice the key occurs in, slice ids
ascending.  ``expected_structure`` says from the batch alone which entries
must exist, ``decode`` reads the device's entry words, ``expected_lr_fresh``
gives the values of LR on a fresh FTRL table bit for bit, and ``fm_ref_bc`` /
``quantisation_*`` give the float64 expectation and the a-priori bound of the
other models on top of ref64.

Entry formats (k_red_csr, k_red_csr_vec, Engine::csr_entry_bytes):

  lr       u64  slice | float bits << 32          (2 words)
  fm_ref   u32 x 3  (slice, B, C)                 (3 words)
  rows     csr_row_words(P) words  (slice, g_0 .. g_{P-1}, pad): standard FM, MVM

Slices: row r is in slice min(r // slice_rows, S - 1) (slice_of,
csrc/hip/model_common.h); a value is divided by the rows of its slice.

LR, fresh FTRL table.  Every weight is 0, every p is exactly 0.5, a record is
a sum of +-0.5 (exact in float32 up to 2^24 terms), the reduction adds records
as integers at 2^36 (exact), and the entry is
float32(float64(sum) / rows_of_slice): one rounding, no tolerance.

The quantisation term (what the fixed-point sums add to ref64's e_g).  u = 2^-24.

  reference FM (k_fm -> k_red_csr<2>).  The producer converts each
  occurrence's loss (B) and loss * vsum (C) with rint(v * 2^32)
  (FxBits<2>::kFx = 32; off by at most 2^-33), a record is the float32 of a
  workgroup's integer sum for one dest, and the reduction converts each
  record the same way: an entry of n occurrences has at most n records, so
     q = 2 n 2^-33 / rows + u |entry|   (the final float32 rounding).

  standard FM (k_fm_std_red -> k_red_csr_vec).  Each row's (loss, loss vs_k)
  is converted to int32 at the workgroup's per-component scale 2^fx, fx = 31 -
  (log2 BLOCK + 1) - e with the workgroup's largest |value| m < 2^e (frexpf):
  rint is off by half a unit, 2^(e - 22 + log2 BLOCK - 9) -- with BLOCK = 512
  (fmstd_block, D <= 10) that is 2^(e - 22) <= m 2^-21 per occurrence.  A
  workgroup's m is at most the batch's largest |value| M_c of the component,
  so with 2^E_c > M_c:  d_c = 2^(E_c - 22) per occurrence.  The record is the
  float32 of the integer sum (u relative), and k_red_csr_vec adds records at
  2^36 (2^-37 each).  The entry is (C_k - v_k B) / rows, w: B / rows:
     q_w = (n (d_0 + 2^-37) + u sum|loss|) / rows + u |g_w|
     q_k = (n (d_k + 2^-37) + u sum|loss vs_k|
            + |v_k| (n (d_0 + 2^-37) + u sum|loss|)) / rows + u |g_k|
  To that the float32 evaluation of the row's latent sums vs_k adds
  |loss| (len + 1) u sum_j |v_jk| per occurrence (ref64's e_g carries the
  loss's error, not the factor's).

  MVM (k_mvm2 -> k_fm_std_red<kScaled> -> k_red_csr_vec<kMvm>, k_mdup_*).  A
  dup-free row leaves T_k = loss M_k per occurrence; the sums run in int64 at
  the step's scale 2^fx, fx = 62 - head - e with the step's largest |T| <
  2^e (fx_scale_bits) and head = max(18, ceil log2 rows) (fx_head_bits).  A
  conversion (rint) is off by 2^-(fx + 1) = 2^(e + head - 63); an occurrence
  is converted as a row value and, inside its record (the float32 of an
  integer sum: u relative), once more by the reduction.  The entry is
  sum T / (1 + v) / rows.  A row with a repeated field leaves its
  occurrences' own gradients c = loss M / (1 + S_f) for the k_mdup_* passes:
  one conversion at the scale of the largest |c| with head' from the batch's
  nnz, a float32 c (u), and a float32 add onto the entry (u).  ref64 does
  not expose M; its condition number A_r = sum_k prod_g sum|v| bounds every
  |M_k| of row r, and |loss| <= 1, so 2^E > max_r A_r bounds both scales'
  2^e.  With non-negative latents |1 + v| >= 1 and |1 + S_f| >= 1 (the
  helper asserts it), so per entry of n occurrences
     q = (n 2^E (2 2^(head - 63) + 2^(head' - 63)) + 2 u sum |loss| A_r) / rows
         + 4 u |g|
  (the last term: the division, the float32 entry, the repeated-field add).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24


def csr_row_words(P: int) -> int:
    return (1 + P + 3) & ~3


def entry_words(kind: str, P: int) -> int:
    return {"lr": 2, "fm_ref": 3}.get(kind) or csr_row_words(P)


def slice_sizes(rows: int, slice_rows: int, S: int) -> np.ndarray:
    """Rows of each of the S slices (the last takes the remainder)."""
    sr = int(slice_rows) if slice_rows and slice_rows > 0 else max(rows, 1)
    s = np.minimum(np.arange(rows, dtype=np.int64) // sr, S - 1)
    return np.bincount(s, minlength=S).astype(np.int64)


def _occurrences(keys, row_ptr, slice_rows, S):
    keys = np.asarray(keys, dtype=np.uint64)
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    rows = len(row_ptr) - 1
    row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(row_ptr))
    sr = int(slice_rows) if slice_rows and slice_rows > 0 else max(rows, 1)
    sl = np.minimum(row_of // sr, S - 1)
    ukeys, inv = np.unique(keys, return_inverse=True)
    return ukeys, inv.astype(np.int64), sl, row_of


@dataclass
class Entries:
    """Per-key entry lists in flat form: key i (of ``ukeys`` when given) owns
    slices[start[i] : start[i] + cnt[i]] and the same rows of ``bits`` (the
    value words as uint32, [N, nv])."""
    cnt: np.ndarray
    start: np.ndarray
    slices: np.ndarray
    bits: np.ndarray | None = None
    ukeys: np.ndarray | None = None

    @property
    def values(self) -> np.ndarray:
        return self.bits.view(np.float32)

    def lists(self):
        """[(slice, values tuple), ...] per key (small cases, messages)."""
        out = []
        for i in range(len(self.cnt)):
            lo, hi = int(self.start[i]), int(self.start[i] + self.cnt[i])
            out.append([(int(self.slices[j]),
                         tuple(self.values[j].tolist()) if self.bits is not None else ())
                        for j in range(lo, hi)])
        return out

    def by_key(self, order: np.ndarray) -> "Entries":
        """The lists of keys order[0], order[1], ... (a permutation or subset)."""
        order = np.asarray(order, dtype=np.int64)
        cnt = self.cnt[order]
        start = np.cumsum(cnt) - cnt
        idx = np.repeat(self.start[order] - start, cnt) + np.arange(int(cnt.sum()), dtype=np.int64)
        return Entries(cnt, start, self.slices[idx], None if self.bits is None else self.bits[idx],
                       None if self.ukeys is None else self.ukeys[order])


def expected_structure(keys, row_ptr, slice_rows: int, S: int) -> Entries:
    """The batch's unique keys (ascending) and, per key, the ascending slices
    it occurs in."""
    ukeys, inv, sl, _ = _occurrences(keys, row_ptr, slice_rows, S)
    pair = np.unique(inv * S + sl)
    cnt = np.bincount(pair // S, minlength=len(ukeys)).astype(np.int64)
    return Entries(cnt, np.cumsum(cnt) - cnt, (pair % S).astype(np.int64), None, ukeys)


def decode(kind: str, P: int, off, cnt, words) -> Entries:
    """The device's entries: off / cnt per key and the entry buffer's words
    (u32).  kind: lr, fm_ref or rows (standard FM, MVM)."""
    ew = entry_words(kind, P)
    nv = {"lr": 1, "fm_ref": 2}.get(kind) or P
    off = np.asarray(off, dtype=np.int64)
    cnt = np.asarray(cnt, dtype=np.int64)
    w = np.asarray(words, dtype=np.uint32).reshape(-1, ew)
    start = np.cumsum(cnt) - cnt
    idx = np.repeat(off - start, cnt) + np.arange(int(cnt.sum()), dtype=np.int64)
    if len(idx) and (idx.min() < 0 or idx.max() >= len(w)):
        raise ValueError("entries outside the entry buffer")
    e = w[idx]
    return Entries(cnt, start, e[:, 0].astype(np.int64), np.ascontiguousarray(e[:, 1:1 + nv]))


def ranges_disjoint(off, cnt, n_entries: int) -> bool:
    """[off, off + cnt) pairwise disjoint and inside [0, n_entries)."""
    off = np.asarray(off, dtype=np.int64)
    cnt = np.asarray(cnt, dtype=np.int64)
    live = cnt > 0
    o, c = off[live], cnt[live]
    order = np.argsort(o, kind="stable")
    o, c = o[order], c[order]
    if len(o) == 0:
        return True
    return bool(o[0] >= 0 and (o[1:] >= o[:-1] + c[:-1]).all() and o[-1] + c[-1] <= n_entries)


def expected_lr_fresh(keys, row_ptr, labels, slice_rows: int, S: int | None = None) -> Entries:
    """LR entries on a fresh FTRL table, exact: float32(float64(sum of
    (0.5 - label)) / rows of the slice)."""
    rows = len(row_ptr) - 1
    if S is None:
        sr = int(slice_rows) if slice_rows and slice_rows > 0 else max(rows, 1)
        S = max(1, -(-rows // sr))
    ukeys, inv, sl, row_of = _occurrences(keys, row_ptr, slice_rows, S)
    pair_all = inv * S + sl
    pair, pinv = np.unique(pair_all, return_inverse=True)
    g = 0.5 - np.asarray(labels, dtype=np.float64)[row_of]
    sums = np.bincount(pinv, weights=g, minlength=len(pair))   # multiples of 0.5: exact
    srows = slice_sizes(rows, slice_rows, S).astype(np.float64)
    slices = (pair % S).astype(np.int64)
    vals = (sums / srows[slices]).astype(np.float32)
    cnt = np.bincount(pair // S, minlength=len(ukeys)).astype(np.int64)
    return Entries(cnt, np.cumsum(cnt) - cnt, slices, vals.view(np.uint32).reshape(-1, 1), ukeys)


def from_ref64(ref):
    """ref64's [U, S, P] gradients of the touched (key, slice) pairs in the
    order of expected_structure: (slices [N], g [N, P], e_g [N, P])."""
    ui, si = np.nonzero(np.asarray(ref.touched))
    return si.astype(np.int64), ref.g[ui, si], ref.e_g[ui, si]


def fm_ref_bc(ref, W, keys, row_ptr, labels, slice_rows: int, S: int):
    """Reference FM's compact entries (B, C) = (sum loss, sum loss * vsum) /
    rows of the slice, vsum the row's sum of every latent (fm_worker form,
    backend.h): float64 expectation [N, 2] and bound [N, 2] in the order of
    expected_structure.  Bound: the loss carries ref64's e_p; vsum is a float32
    sum of len * D latents from the compact value rows (chain len + D); a
    record is a float32 partial sum (count u); plus quantisation(fm_ref)."""
    ukeys, inv, sl, row_of = _occurrences(keys, row_ptr, slice_rows, S)
    W = np.asarray(W, dtype=np.float64)
    lat = W[:, 1:]
    rows = len(row_ptr) - 1
    vsum = np.bincount(row_of, weights=lat.sum(1)[inv], minlength=rows)
    avs = np.bincount(row_of, weights=np.abs(lat).sum(1)[inv], minlength=rows)
    length = np.diff(np.asarray(row_ptr, dtype=np.int64))
    D = lat.shape[1]
    loss = ref.p - np.asarray(labels, dtype=np.float64)
    e_vs = (length + D + 1) * U * avs
    pair, pinv = np.unique(inv * S + sl, return_inverse=True)
    n = np.bincount(pinv, minlength=len(pair)).astype(np.float64)
    srows = slice_sizes(rows, slice_rows, S).astype(np.float64)[pair % S]

    def acc(x):
        return np.bincount(pinv, weights=x[row_of], minlength=len(pair))

    B, C = acc(loss), acc(loss * vsum)
    aB, aC = acc(np.abs(loss)), acc(np.abs(loss * vsum))
    eB = acc(ref.e_p) + n * U * aB
    eC = acc(ref.e_p * np.abs(vsum) + (np.abs(loss) + ref.e_p) * e_vs + U * np.abs(loss * vsum)) + n * U * aC
    want = np.stack([B, C], 1) / srows[:, None]
    q = 2.0 * n[:, None] * 2.0 ** -33 / srows[:, None] + U * np.abs(want)
    return want, np.stack([eB, eC], 1) / srows[:, None] + q


def _pairs(ref, keys, row_ptr, labels, slice_rows, S):
    _, inv, sl, row_of = _occurrences(keys, row_ptr, slice_rows, S)
    rows = len(row_ptr) - 1
    loss = ref.p - np.asarray(labels, dtype=np.float64)
    pair, pinv = np.unique(inv * S + sl, return_inverse=True)
    n = np.bincount(pinv, minlength=len(pair)).astype(np.float64)
    srows = slice_sizes(rows, slice_rows, S).astype(np.float64)[pair % S]
    g = np.abs(ref.g[np.nonzero(np.asarray(ref.touched))])   # [N, P], the same (key, slice) order
    assert len(g) == len(pair)

    def acc(x):
        return np.bincount(pinv, weights=x[row_of], minlength=len(pair))

    return inv, row_of, rows, loss, pair // S, n, srows, g, acc


def _pow2_above(m: float) -> float:
    """2^e with m < 2^e as frexpf gives it, m taken a little larger (the
    device's float32 maximum may sit just above the float64 one)."""
    return 2.0 ** (math.frexp(m * (1.0 + 2.0 ** -10))[1]) if m > 0 else 0.0


def quantisation_fm_std(ref, W, keys, row_ptr, labels, slice_rows: int, S: int,
                        block: int = 512) -> np.ndarray:
    """The quantisation term [N, P] of standard FM entries (module docstring),
    in the order of expected_structure, from float64 quantities only."""
    inv, row_of, rows, loss, ui, n, srows, g, acc = _pairs(ref, keys, row_ptr, labels, slice_rows, S)
    W = np.asarray(W, dtype=np.float64)
    length = np.diff(np.asarray(row_ptr, dtype=np.int64)).astype(np.float64)
    P = W.shape[1]
    q = np.zeros((len(n), P))
    half = 2.0 ** -22 * (block / 512.0)
    d0 = _pow2_above(float(np.abs(loss).max())) * half
    a0 = n * (d0 + 2.0 ** -37) + U * acc(np.abs(loss))
    q[:, 0] = a0 / srows + U * g[:, 0]
    for k in range(1, P):
        vs = np.bincount(row_of, weights=W[inv, k], minlength=rows)
        avs = np.bincount(row_of, weights=np.abs(W[inv, k]), minlength=rows)
        f = loss * vs
        dk = _pow2_above(float(np.abs(f).max())) * half
        ak = n * (dk + 2.0 ** -37) + U * acc(np.abs(f)) + acc(np.abs(loss) * (length + 1) * U * avs)
        q[:, k] = (ak + np.abs(W[ui, k]) * a0) / srows + U * g[:, k]
    return q


def quantisation_mvm(ref, W, keys, row_ptr, labels, slice_rows: int, S: int) -> np.ndarray:
    """The quantisation term [N, P] of MVM entries (module docstring), for
    non-negative latents (every |1 + S| >= 1)."""
    W = np.asarray(W, dtype=np.float64)
    assert (W >= 0).all(), "the bound takes |1 + S| >= 1"
    inv, row_of, rows, loss, ui, n, srows, g, acc = _pairs(ref, keys, row_ptr, labels, slice_rows, S)
    head = max(18, math.ceil(math.log2(max(rows, 1))))
    head2 = max(18, math.ceil(math.log2(max(len(keys), 1))))
    A = np.asarray(ref.A, dtype=np.float64)
    step = _pow2_above(float(A.max())) if len(A) else 0.0      # 2^e >= every |T| and |c|
    conv = step * (2.0 * 2.0 ** (head - 63) + 2.0 ** (head2 - 63))
    q = (n * conv + 2.0 * U * acc(np.abs(loss) * A)) / srows
    return q[:, None] + 4.0 * U * g
