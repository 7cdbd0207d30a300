"""Float64 per-row reference of the forward, the loss counters and the
per-(key, slice) gradients, with an a-priori bound on how far a correct fp32
implementation may be from it.

Written from the model definitions (docs/DESIGN.md, csrc/include/xflow/common.h,
types.h), one row and one occurrence at a time in plain Python loops: nothing
is vectorised over rows (as testing/torch_ref.py is) and nothing follows the
kernels' evaluation order, so a mistake in either shows up as a difference.

Per row (n occurrences, latent width D, u = 2^-24):

  logit y   LR            sum w
            FM reference  wx + ((sum_k sum_j v_jk)^2 - sum v^2)
            FM standard   wx + 1/2 (sum_k (sum_j v_jk)^2 - sum v^2)
            MVM           sum_k prod_{g<G} S_gk, S_gk the sum of the row's
                          occurrences of field g; G = maxf (compat) or
                          maxf + 1 (fixed); an empty row has maxf = 0
  p         the reference sigmoid (base 2.718281828; 1e-6 below -30, 1 above 30)
  A         the logit's expression with every term replaced by its absolute
            value (the condition number of the evaluation)
  N         the longest chain of roundings: LR n, FM 2(n + D) + 4, MVM n + G + D

Any fp32 evaluation of y, in any summation order, is within N u A of y, the
sigmoid's slope is at most 1/4, and rounding p to fp32 (plus the double
evaluation of exp) costs at most 2 u p:

  e_p = 1/4 N u A + 2 u p.

Gradient of an occurrence (loss = p - label):
  LR  loss;  FM  w: loss (standard) or loss D (reference), v_k: loss (ref_k -
  v_k) with ref_k = sum_j v_jk (standard) or sum_k sum_j v_jk (reference);
  MVM  v_k: 0 where S_fk == 0, else loss M_k / (1 + S_fk), f the occurrence's
  field, M_k the row's product.
Its bound is e_p |factor| (the loss carries e_p), for MVM plus (n + G + 2) u
relative for the factor M / (1 + S).  (That holds while 1 + S does not
cancel: a field sum S of several occurrences is itself rounded, and where
|1 + S| is small against sum|v| the factor is ill conditioned beyond this
bound.  Callers keep such sums away from -1.)  A (key, slice) gradient is the
sum of its occurrences divided by the slice's row count; the sum adds count u
relative to the sum of absolute values.

Counter tolerances: sum over rows of e_p / min(p, 1 - p) (over ln 2 for
log2_lik) plus 2 u |term| for logf / log2f.  e_p's 2 u p part is at least
2 u min(p, 1 - p), which also covers the fp32 rounding of 1 - p.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

U = 2.0 ** -24
LN_BASE = math.log(2.718281828)
# the clip of ln_loss as the counters apply it: the fp32 constants 1e-7f and
# 1.0f - 1e-7f (types.h LossStats)
CLIP_LO = float(np.float32(1e-7))
CLIP_HI = float(np.float32(1.0) - np.float32(1e-7))


def sigmoid(y: float) -> float:
    if y < -30.0:
        return 1e-6
    if y > 30.0:
        return 1.0
    ex = math.exp(y * LN_BASE)
    return ex / (1.0 + ex)


def chain_length(kind: str, n: int, D: int, G: int) -> int:
    if kind == "lr":
        return n
    if kind == "fm":
        return 2 * (n + D) + 4
    return n + G + D


def loss_terms(p: float, label: float):
    """(ln_loss term, log2_lik term) of one row."""
    pc = min(max(p, CLIP_LO), CLIP_HI)
    pos = label > 0.5
    ln = -math.log(pc) if pos else -math.log(1.0 - pc)
    q = p if pos else 1.0 - p
    l2 = math.log2(q) if q > 0.0 else -math.inf
    return ln, l2


def counters(p, labels) -> dict:
    """The four loss counters of predictions p (any float sequence)."""
    out = {"ln_loss": 0.0, "log2_lik": 0.0, "rows": 0.0, "positives": 0.0}
    for pr, lab in zip(p, labels):
        ln, l2 = loss_terms(float(pr), float(lab))
        out["ln_loss"] += ln
        out["log2_lik"] += l2
        out["rows"] += 1.0
        out["positives"] += 1.0 if lab > 0.5 else 0.0
    return out


@dataclass
class Ref64:
    y: np.ndarray            # [rows] logits
    p: np.ndarray            # [rows] predictions
    A: np.ndarray            # [rows] condition numbers
    N: np.ndarray            # [rows] chain lengths
    e_p: np.ndarray          # [rows] bound on |p32 - p|
    G: np.ndarray            # [rows] MVM product range (0 otherwise)
    # with labels:
    counters: dict = field(default_factory=dict)
    counter_tol: dict = field(default_factory=dict)   # ln_loss, log2_lik
    ukeys: np.ndarray | None = None
    slice_rows: list | None = None   # rows of each slice
    g: np.ndarray | None = None      # [U, S, P] normalised gradients
    e_g: np.ndarray | None = None    # [U, S, P] their bounds
    touched: np.ndarray | None = None  # [U, S] the key occurs in the slice


def _row_forward(kind, D, fm_math, mvm_math, Wocc, fg):
    """One row: Wocc the [n, P] float64 weights of its occurrences, fg their
    fields.  Returns y, A, G and what the gradient needs."""
    n = len(Wocc)
    if kind == "lr":
        y = A = 0.0
        for j in range(n):
            y += Wocc[j][0]
            A += abs(Wocc[j][0])
        return y, A, 0, None
    if kind == "fm":
        wx = awx = vp = 0.0
        vs = [0.0] * D
        avs = [0.0] * D
        for j in range(n):
            wx += Wocc[j][0]
            awx += abs(Wocc[j][0])
            for k in range(D):
                v = Wocc[j][1 + k]
                vs[k] += v
                avs[k] += abs(v)
                vp += v * v
        if fm_math == "standard":
            y = wx + 0.5 * (sum(s * s for s in vs) - vp)
            A = awx + 0.5 * (sum(s * s for s in avs) + vp)
        else:
            y = wx + (sum(vs) ** 2 - vp)
            A = awx + (sum(avs) ** 2 + vp)
        return y, A, 0, vs
    # MVM
    maxf = 0
    for j in range(n):
        maxf = max(maxf, int(fg[j]))
    G = maxf if mvm_math == "compat" else maxf + 1
    S = [[0.0] * D for _ in range(maxf + 1)]
    aS = [[0.0] * D for _ in range(maxf + 1)]
    for j in range(n):
        for k in range(D):
            S[int(fg[j])][k] += Wocc[j][k]
            aS[int(fg[j])][k] += abs(Wocc[j][k])
    M = [1.0] * D
    aM = [1.0] * D
    for g in range(G):
        for k in range(D):
            M[k] *= S[g][k]
            aM[k] *= aS[g][k]
    return sum(M), sum(aM), G, (S, M)


def reference(kind: str, v_dim: int, ukeys, W, keys, row_ptr, fgid=None, labels=None,
              slice_rows: int = 0, fm_math: str = "reference", mvm_math: str = "compat") -> Ref64:
    """ukeys: the batch's unique keys; W: their float32 weights [U, P] as
    Engine.pull returns them; keys / row_ptr / fgid: the batch in CSR form.
    With labels also the counters and the per-(key, slice) gradients."""
    D = 0 if kind == "lr" else int(v_dim)
    W = np.asarray(W, dtype=np.float64)
    P = W.shape[1]
    index = {int(k): i for i, k in enumerate(np.asarray(ukeys, dtype=np.uint64))}
    rows = len(row_ptr) - 1
    y = np.zeros(rows)
    p = np.zeros(rows)
    A = np.zeros(rows)
    N = np.zeros(rows)
    Gs = np.zeros(rows, dtype=np.int64)
    aux = [None] * rows
    for r in range(rows):
        lo, hi = int(row_ptr[r]), int(row_ptr[r + 1])
        Wocc = [W[index[int(keys[o])]] for o in range(lo, hi)]
        fg = [int(fgid[o]) for o in range(lo, hi)] if kind == "mvm" else None
        y[r], A[r], Gs[r], aux[r] = _row_forward(kind, D, fm_math, mvm_math, Wocc, fg)
        p[r] = sigmoid(y[r])
        N[r] = chain_length(kind, hi - lo, D, int(Gs[r]))
    e_p = 0.25 * N * U * A + 2.0 * U * p
    out = Ref64(y=y, p=p, A=A, N=N, e_p=e_p, G=Gs)
    if labels is None:
        return out

    # ---- counters and their tolerance -------------------------------------
    out.counters = counters(p, labels)
    tol_ln = tol_l2 = 0.0
    for r in range(rows):
        ln, l2 = loss_terms(p[r], float(labels[r]))
        m = min(p[r], 1.0 - p[r])
        # a clamped row (|y| > 30; the caller keeps y off the clamps by more
        # than its fp32 error) has the constant in fp32 too: of e_p only the
        # rounding of p is left, and p = 1 is exact
        e = e_p[r] if abs(y[r]) <= 30.0 else (2.0 * U * p[r] if p[r] < 1.0 else 0.0)
        tol_ln += (e / m if e > 0.0 else 0.0) + 2.0 * U * abs(ln)
        if math.isfinite(l2):  # (-inf for p = 1, label 0: expected exactly)
            tol_l2 += (e / m if e > 0.0 else 0.0) / math.log(2.0) + 2.0 * U * abs(l2)
    out.counter_tol = {"ln_loss": tol_ln, "log2_lik": tol_l2}

    # ---- gradients --------------------------------------------------------
    sr = int(slice_rows) if slice_rows and slice_rows > 0 else rows
    nS = max(1, -(-rows // sr))
    srows = [min(sr, rows - s * sr) for s in range(nS)]
    Uq = len(index)
    gsum = np.zeros((Uq, nS, P))
    gabs = np.zeros((Uq, nS, P))
    gerr = np.zeros((Uq, nS, P))
    count = np.zeros((Uq, nS))
    for r in range(rows):
        lo, hi = int(row_ptr[r]), int(row_ptr[r + 1])
        n = hi - lo
        s = min(r // sr, nS - 1)
        loss = p[r] - float(labels[r])
        for o in range(lo, hi):
            i = index[int(keys[o])]
            w = W[i]
            count[i, s] += 1
            for q in range(P):
                rel = 0.0
                if kind == "lr":
                    fac = 1.0
                elif kind == "fm":
                    vs = aux[r]
                    if q == 0:
                        fac = 1.0 if fm_math == "standard" else float(D)
                    else:
                        ref = vs[q - 1] if fm_math == "standard" else sum(vs)
                        fac = ref - w[q]
                else:
                    S, M = aux[r]
                    sg = S[int(fgid[o])][q]
                    fac = 0.0 if sg == 0.0 else M[q] / (1.0 + sg)
                    rel = (n + int(Gs[r]) + 2) * U
                g = loss * fac
                gsum[i, s, q] += g
                gabs[i, s, q] += abs(g)
                gerr[i, s, q] += e_p[r] * abs(fac) + rel * abs(g)
    norm = np.asarray(srows, dtype=np.float64).reshape(1, nS, 1)
    out.ukeys = np.asarray(ukeys, dtype=np.uint64)
    out.slice_rows = srows
    out.g = gsum / norm
    out.e_g = (gerr + count[:, :, None] * U * gabs) / norm
    out.touched = count > 0
    return out


# ---- float64 optimiser updates (common.h) ------------------------------------
def sgd_update(w, g, lr):
    return w - lr * g


def ftrl_weight(z, n, alpha, beta, l1, l2):
    if abs(z) <= l1:
        return 0.0
    t = z - l1 if z > 0 else z + l1
    return t / (-1.0 * ((beta + math.sqrt(n)) / alpha + l2))


def ftrl_update(n, z, w, g, alpha):
    """One push of g onto (n, z) whose current weight is w; returns (n, z)."""
    nn = n + g * g
    return nn, z + g - (math.sqrt(nn) - math.sqrt(n)) / alpha * w
