"""What the per-epoch row shuffle (Engine.shuffle_batch) costs at the bench
shape: one block of 262144 rows x 39 fields of u64 keys, and a CSR block of
the same occurrences (rows of 19..59 entries).

Part 1, fixed width: the fused shuffle + transpose (k_shuffle_tile) against
the plain row-major -> field-major pass it replaces (k_field_major), on the
same tensors into preallocated outputs, timed in alternating blocks of calls
in one process.

Part 2, CSR: the three launches (lengths + labels, scan, gather) against
device-to-device copies of the same bytes (keys, labels, row_ptr).

Every arm cycles through --buffers sets of source and destination tensors,
so that the bytes of a call are not still in the 256 MiB Infinity Cache from
the call before (a block that training shuffles has just arrived from the
host).  --buffers 1 times the cache-resident case.  Both outputs are first
checked against a torch gather by shuffle_permutation.

    python tools/shuffle_bench.py [--out profiles/shuffle.txt]
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
from xflow_amd.engine import Batch, Engine, shuffle_permutation  # noqa: E402


def timed(fn, calls, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(calls):
        fn(i)
    torch.cuda.synchronize(dev)
    return 1e6 * (time.perf_counter() - t0) / calls


def alternate(arms, blocks, calls, dev):
    """{name: [us per call of each block]}, the arms taking turns."""
    for fn in arms.values():
        timed(fn, 10, dev)  # warm-up
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
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--blocks", type=int, default=8, help="alternating timed blocks per arm")
    ap.add_argument("--calls", type=int, default=1000, help="calls per block")
    ap.add_argument("--buffers", type=int, default=4,
                    help="source / destination sets an arm cycles through")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows, F = a.rows, a.fields
    nnz = rows * F
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def report(us, base, arm):
        med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
        say("arm us_per_call_median us_per_call_blocks")
        for k, v in us.items():
            say("%s %.1f %s" % (k, med[k], " ".join("%.1f" % x for x in v)))
        say("# %s / %s: %.3f" % (arm, base, med[arm] / med[base]))

    eng = Engine(ModelConfig(kind="lr"), OptimConfig(),
                 EngineConfig(table_log2_cap=10, max_rows=rows, max_nnz=nnz), device=dev)
    n = eng.native
    g = torch.Generator(device=dev).manual_seed(a.seed)
    keys = torch.randint(0, 2 ** 62, (nnz,), dtype=torch.int64, device=dev, generator=g)
    labels = torch.rand(rows, device=dev, generator=g)
    perm = torch.from_numpy(shuffle_permutation(rows, a.seed)).to(dev)
    say("# tools/shuffle_bench.py: %d rows x %d fields, u64 keys, %s"
        % (rows, F, torch.cuda.get_device_name(dev)))
    say("# %d alternating blocks of %d calls per arm over %d buffer sets; host clock around a "
        "synchronise" % (a.blocks, a.calls, a.buffers))
    nb = max(1, a.buffers)
    srcs = [keys] + [torch.randint(0, 2 ** 62, (nnz,), dtype=torch.int64, device=dev, generator=g)
                     for _ in range(nb - 1)]
    outs = [torch.empty_like(keys) for _ in range(nb)]

    # ---- part 1: fixed width ------------------------------------------------
    rm = Batch(keys=keys, labels=labels, nnz_per_row=F)
    got = eng.shuffle_batch(rm, a.seed)
    assert torch.equal(got.keys.view(F, rows), keys.view(rows, F)[perm].t())
    assert torch.equal(got.labels, labels[perm])
    assert torch.equal(rm.to_field_major(eng).keys.view(F, rows), keys.view(rows, F).t())
    out_y = torch.empty_like(labels)
    eng._sync_stream()
    views = [Batch(keys=k, labels=labels, nnz_per_row=F).view() for k in srcs]
    arms = {
        "field_major": lambda i: n.field_major(srcs[i % nb].data_ptr(), outs[i % nb].data_ptr(),
                                               rows, F, 8, False),
        "shuffle_field_major": lambda i: n.shuffle_rows(views[i % nb], a.seed,
                                                        outs[i % nb].data_ptr(), 0,
                                                        out_y.data_ptr(), 0, True, 8),
    }
    say("# part 1: fixed width, %.1f MB of keys read and written per call" % (nnz * 8 / 1e6))
    report(alternate(arms, a.blocks, a.calls, dev), "field_major", "shuffle_field_major")

    # ---- part 2: CSR ----------------------------------------------------------
    rng = np.random.default_rng(a.seed)
    d = rng.integers(-20, 21, rows // 2)
    lens = np.full(rows, F, np.int64)
    lens[: rows // 2] += d
    lens[rows // 2: 2 * (rows // 2)] -= d
    rp_h = np.zeros(rows + 1, np.int32)
    rp_h[1:] = np.cumsum(lens)
    assert int(rp_h[-1]) == nnz
    rp = torch.from_numpy(rp_h).to(dev)
    csr = Batch(keys=keys, labels=labels, row_ptr=rp)
    got = eng.shuffle_batch(csr, a.seed)
    lens_d = torch.from_numpy(lens).to(dev)
    src_of = torch.repeat_interleave(rp[:-1].long()[perm] - got.row_ptr[:-1].long(), lens_d[perm])
    assert torch.equal(got.row_ptr[1:].long(), torch.cumsum(lens_d[perm], 0))
    assert torch.equal(got.keys, keys[torch.arange(nnz, device=dev) + src_of])
    assert torch.equal(got.labels, labels[perm])
    out_rp = torch.empty_like(rp)
    cviews = [Batch(keys=k, labels=labels, row_ptr=rp).view() for k in srcs]

    def copies(i):
        outs[i % nb].copy_(srcs[i % nb])
        out_y.copy_(labels)
        out_rp.copy_(rp)

    arms = {
        "device_copy": copies,
        "shuffle_csr": lambda i: n.shuffle_rows(cviews[i % nb], a.seed, outs[i % nb].data_ptr(), 0,
                                                out_y.data_ptr(), out_rp.data_ptr(), False, 8),
    }
    say("# part 2: CSR, rows of %d..%d entries, the same %d occurrences"
        % (lens.min(), lens.max(), nnz))
    report(alternate(arms, a.blocks, a.calls, dev), "device_copy", "shuffle_csr")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
