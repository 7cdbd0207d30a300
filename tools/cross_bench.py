"""What feature crosses (Engine.cross_batch, csrc/hip/kernels_cross.hip) cost
at the bench shape: one block of 262144 rows x 39 fields of u64 keys, with
C = 1, 4 and 13 pair crosses.

Part 1, fixed width: k_cross_tile (cross + transpose, and with a seed the
shuffle too) against the plain row-major -> field-major pass every block pays
anyway (k_field_major) and against the fused shuffle (k_shuffle_tile), on the
same tensors into preallocated outputs.  Every figure comes with the bytes
the call must move (the keys read, the keys and labels written) and the rate
that makes.

Part 2, field-major input: k_cross_cols in place (the cross columns written
behind the input's columns).

Part 3, CSR: k_cross_csr (with field ids, rows of 19..59 entries) against
device-to-device copies of the bytes it must move.

Part 4, downstream: an LR-FTRL train step on the F = 39 batch against the
same rows with F = 39 + C -- what the extra columns cost the step.

The arms of a part take turns in alternating blocks of calls in one process;
the layout arms cycle through --buffers sets of tensors so that a call's
bytes are not still in the Infinity Cache from the call before.  The outputs
are first checked against cross_keys-equivalent torch code.

    python tools/cross_bench.py [--out profiles/cross.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig  # noqa: E402
from xflow_amd.engine import Batch, Engine, cross_keys  # noqa: E402


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def timed(fn, calls, dev):
    _sync(dev)
    t0 = time.perf_counter()
    for i in range(calls):
        fn(i)
    _sync(dev)
    return 1e6 * (time.perf_counter() - t0) / calls


def alternate(arms, blocks, calls, dev, warm=5):
    """{name: [us per call of each block]}, the arms taking turns."""
    for fn in arms.values():
        timed(fn, warm, dev)
    us = {k: [] for k in arms}
    for _ in range(blocks):
        for k, fn in arms.items():
            us[k].append(timed(fn, calls, dev))
    return us


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--fields", type=int, default=39)
    ap.add_argument("--crosses", default="1,4,13", help="numbers of pair crosses to time")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--blocks", type=int, default=6, help="alternating timed blocks per arm")
    ap.add_argument("--calls", type=int, default=200, help="calls per block")
    ap.add_argument("--step-calls", type=int, default=20, help="train steps per block (part 4)")
    ap.add_argument("--buffers", type=int, default=4,
                    help="source / destination sets a layout arm cycles through")
    ap.add_argument("--out", default="")
    ap.add_argument("--rehearse-cpu", action="store_true",
                    help="run every part on the CPU backend to check the script itself (its "
                         "times say nothing about the GPU; no file is written)")
    a = ap.parse_args()
    dev = torch.device("cpu") if a.rehearse_cpu else torch.device("cuda", 0)
    rows, F = a.rows, a.fields
    nnz = rows * F
    Cs = [int(c) for c in a.crosses.split(",")]
    Cmax = max(Cs)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def report(us, base, nbytes):
        med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
        say("arm us_per_call_median MB_moved GB_per_s vs_%s us_per_call_blocks" % base)
        for k, v in us.items():
            say("%s %.1f %.1f %.0f %.3f %s" % (k, med[k], nbytes[k] / 1e6, nbytes[k] / med[k] / 1e3,
                                             med[k] / med[base], " ".join("%.1f" % x for x in v)))
        return med

    eng = Engine(ModelConfig(kind="lr"), OptimConfig(),
                 EngineConfig(table_log2_cap=10, max_rows=rows, max_nnz=rows * (F + Cmax)),
                 device=dev)
    n = eng.native
    g = torch.Generator(device=dev).manual_seed(a.seed)
    nb = max(1, a.buffers)
    # (per-field vocabularies, so that part 4's step sees realistic repeats)
    base = (torch.arange(F, device=dev, dtype=torch.int64) << 32).repeat(rows)
    srcs = [base + torch.randint(0, 100000, (nnz,), dtype=torch.int64, device=dev, generator=g)
            for _ in range(nb)]
    keys = srcs[0]
    labels = (torch.rand(rows, device=dev, generator=g) < 0.25).float()
    outs = [torch.empty(rows * (F + Cmax), dtype=torch.int64, device=dev) for _ in range(nb)]
    out_y = torch.empty_like(labels)
    say("# tools/cross_bench.py: %d rows x %d fields, u64 keys, %s"
        % (rows, F, "CPU backend (rehearsal)" if a.rehearse_cpu
           else torch.cuda.get_device_name(dev)))
    say("# %d alternating blocks of %d calls per arm over %d buffer sets; host clock around a "
        "synchronise" % (a.blocks, a.calls, nb))

    def pairs(C):
        return [(c, (c + 1) % F) for c in range(C)]

    # the outputs are what the definition says (the first 512 rows, every cross)
    X = pairs(Cmax)
    rm = Batch(keys=keys, labels=labels, nnz_per_row=F)
    got = eng.cross_batch(rm, X, seed=None).keys.view(F + Cmax, rows)
    k_h = keys.view(rows, F)[:512].cpu().numpy()
    assert torch.equal(got[:F], keys.view(rows, F).t())
    for c, x in enumerate(X):
        want = cross_keys(x, k_h[:, list(x)])
        assert np.array_equal(got[F + c, :512].cpu().numpy().view(np.uint64), want), x
    eng._sync_stream()
    views = [Batch(keys=k, labels=labels, nnz_per_row=F).view() for k in srcs]
    rd, lab = nnz * 8, rows * 4

    for C in Cs:
        X = [list(x) for x in pairs(C)]
        wr = (nnz + C * rows) * 8
        # ---- part 1 ------------------------------------------------------------
        arms = {
            "field_major": lambda i: n.field_major(srcs[i % nb].data_ptr(), outs[i % nb].data_ptr(),
                                                   rows, F, 8, False),
            "cross_tile": lambda i: n.cross_rows(views[i % nb], X, 0, None, outs[i % nb].data_ptr(),
                                                 0, out_y.data_ptr(), 0, True, 8),
            "shuffle_field_major": lambda i: n.shuffle_rows(views[i % nb], a.seed,
                                                            outs[i % nb].data_ptr(), 0,
                                                            out_y.data_ptr(), 0, True, 8),
            "cross_tile_shuffle": lambda i: n.cross_rows(views[i % nb], X, 0, a.seed,
                                                         outs[i % nb].data_ptr(), 0,
                                                         out_y.data_ptr(), 0, True, 8),
        }
        nbytes = {"field_major": 2 * rd, "cross_tile": rd + wr + 2 * lab,
                  "shuffle_field_major": 2 * rd + 2 * lab, "cross_tile_shuffle": rd + wr + 2 * lab}
        say("# part 1: C = %d pair crosses, fixed width row-major -> field-major" % C)
        report(alternate(arms, a.blocks, a.calls, dev), "field_major", nbytes)

        # ---- part 2: field-major input, in place ---------------------------------
        fms = []
        for k in srcs:
            buf = torch.empty(rows * (F + C), dtype=torch.int64, device=dev)
            buf[:nnz] = k.view(rows, F).t().reshape(-1)
            v = Batch(keys=buf[:nnz], labels=labels, nnz_per_row=F, field_major=True).view()
            fms.append((buf, v))
        arms = {
            "device_copy": lambda i: outs[i % nb][:3 * C * rows].copy_(
                srcs[i % nb][:3 * C * rows]),
            "cross_cols": lambda i: n.cross_rows(fms[i % nb][1], X, 0, None,
                                                 fms[i % nb][0].data_ptr(), 0, labels.data_ptr(), 0,
                                                 True, 8),
        }
        # (2 operand columns read and 1 column written per cross; the copy moves as much)
        nbytes = {"device_copy": 2 * 3 * C * rows * 8, "cross_cols": 3 * C * rows * 8}
        say("# part 2: C = %d, field-major input crossed in place (k_cross_cols)" % C)
        report(alternate(arms, a.blocks, a.calls, dev), "device_copy", nbytes)
        del fms

    # ---- part 3: CSR ------------------------------------------------------------
    rng = np.random.default_rng(a.seed)
    d = rng.integers(-20, 21, rows // 2)
    lens = np.full(rows, F, np.int64)
    lens[: rows // 2] += d
    lens[rows // 2: 2 * (rows // 2)] -= d
    rp_h = np.zeros(rows + 1, np.int32)
    rp_h[1:] = np.cumsum(lens)
    assert int(rp_h[-1]) == nnz
    rp = torch.from_numpy(rp_h).to(dev)
    # field ids: a row's entries are fields 0, 1, 2, ... in order
    fg = (torch.arange(nnz, device=dev, dtype=torch.int64)
          - torch.repeat_interleave(rp[:-1].long(), torch.from_numpy(lens).to(dev))).int()
    out_rp = torch.empty_like(rp)
    out_fg = torch.empty(rows * (F + Cmax), dtype=torch.int32, device=dev)
    cviews = [Batch(keys=k, labels=labels, row_ptr=rp, fgid=fg).view() for k in srcs]
    for C in Cs:
        X = [list(x) for x in pairs(C)]

        def copies(i):
            outs[i % nb][:nnz].copy_(srcs[i % nb])
            out_fg[:nnz].copy_(fg)
            out_y.copy_(labels)
            out_rp.copy_(rp)

        arms = {
            "device_copy": copies,
            "cross_csr": lambda i: n.cross_rows(cviews[i % nb], X, 100, None,
                                                outs[i % nb].data_ptr(), out_fg.data_ptr(),
                                                out_y.data_ptr(), out_rp.data_ptr(), False, 8),
        }
        cp = 2 * (nnz * 12 + rows * 4 + (rows + 1) * 4)
        nbytes = {"device_copy": cp, "cross_csr": cp + C * rows * 12}
        say("# part 3: C = %d, CSR with field ids, rows of %d..%d entries, %d occurrences"
            % (C, lens.min(), lens.max(), nnz))
        report(alternate(arms, a.blocks, a.calls, dev), "device_copy", nbytes)
    del cviews, outs, out_fg

    # ---- part 4: the LR step downstream -------------------------------------------
    for C in Cs:
        X = pairs(C)

        def engine(width):
            return Engine(ModelConfig(kind="lr"), OptimConfig(),
                          EngineConfig(table_log2_cap=24, max_rows=rows, max_nnz=rows * width),
                          device=dev)

        e0, e1 = engine(F), engine(F + C)
        b0 = [Batch(keys=k, labels=labels, nnz_per_row=F).to_field_major(e0) for k in srcs]
        b1 = [e1.cross_batch(Batch(keys=k, labels=labels, nnz_per_row=F), X) for k in srcs]
        arms = {"lr_step_F%d" % F: lambda i: e0.train_step(b0[i % nb]),
                "lr_step_F%d" % (F + C): lambda i: e1.train_step(b1[i % nb])}
        say("# part 4: C = %d, LR-FTRL train step (1 slice) on %d rows, F = %d against F = %d"
            % (C, rows, F, F + C))
        us = alternate(arms, a.blocks, a.step_calls, dev, warm=10)
        med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
        say("arm us_per_step_median us_per_step_blocks")
        for k, v in us.items():
            say("%s %.1f %s" % (k, med[k], " ".join("%.1f" % x for x in v)))
        k0, k1 = list(us)
        say("# %s / %s: %.3f (columns: %.3f)" % (k1, k0, med[k1] / med[k0], (F + C) / F))
        assert not e0.overflowed() and not e1.overflowed()
        del e0, e1, b0, b1
    if a.out and not a.rehearse_cpu:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
