#!/usr/bin/env python3
"""Time the device-side eval metrics (Engine.eval_metrics: stable radix sort
of pctr + exact rank-sum AUC + double logloss, csrc/hip/kernels_eval.hip) on a
synthetic N-row prediction set, against the host path it replaces (D2H copy +
the reference printer's sort, xflow_amd.metrics.reference_auc).

    python tools/eval_bench.py --rows 10000000 --reps 5

With --groups G it also times the grouped evaluation (Engine.eval_grouped:
per-group AUC counts and calibration) on the same predictions in the same
process, the rows spread over G hashed group keys -- uniformly, or with
--group-skew s > 0 group i drawn with probability ~ (i + 1)^-s -- and with
--host the host alternative (D2H of pctr, labels and groups + a numpy lexsort).

    python tools/eval_bench.py --rows 10000000 --groups 1000000 --group-skew 1.1 --host
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig  # noqa: E402
from xflow_amd.engine import Engine  # noqa: E402
from xflow_amd.metrics import reference_auc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host", action="store_true", help="also time the host reference path")
    ap.add_argument("--groups", type=int, default=0,
                    help="also time eval_grouped with the rows spread over this many groups")
    ap.add_argument("--group-skew", type=float, default=0.0,
                    help="--groups: power-law exponent of the group sizes (0: uniform)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    n = args.rows
    # planted signal: labels drawn from the predictions
    p = torch.rand(n, device=dev, generator=g) * 0.98 + 0.01
    y = (torch.rand(n, device=dev, generator=g) < p).float()
    e = Engine(ModelConfig(), OptimConfig(), EngineConfig(table_log2_cap=8), device=dev)
    r = e.eval_metrics(p, y)  # warm (workspace allocation, code load)
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        r = e.eval_metrics(p, y)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    out = {"rows": n, "device_ms_min": 1e3 * min(ts), "device_ms_median": 1e3 * sorted(ts)[len(ts) // 2],
           "auc": r["auc"], "ln_logloss": r["ln_logloss"], "line": r["line"]}
    if args.host:
        t0 = time.perf_counter()
        ph, yh = p.cpu().numpy(), y.cpu().numpy().astype(np.int32)
        ref = reference_auc(yh, ph)
        out["host_ms"] = 1e3 * (time.perf_counter() - t0)
        out["host_line"] = ref["line"]
    if args.groups > 0:
        out.update(grouped(e, p, y, args, g))
    print(json.dumps(out))


def grouped(e, p, y, args, gen):
    """Timings of Engine.eval_grouped next to eval_metrics' (same p, y)."""
    n, G = p.numel(), args.groups
    u = torch.rand(n, device=p.device, generator=gen, dtype=torch.float64)
    if args.group_skew > 0:
        # inverse CDF of the continuous power law on [1, G + 1)
        s = args.group_skew
        if abs(s - 1.0) < 1e-9:
            gi = torch.exp(u * np.log(G + 1.0))
        else:
            gi = (1.0 + u * ((G + 1.0) ** (1.0 - s) - 1.0)) ** (1.0 / (1.0 - s))
        gi = (gi.long() - 1).clamp_(0, G - 1)
    else:
        gi = (u * G).long().clamp_(0, G - 1)
    # hashed keys: an odd multiplier mod 2^64 spreads the ids over all 8 bytes
    keys = (gi + 1) * -7046029254386353131
    r = e.eval_grouped(p, y, keys)  # warm
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        r = e.eval_grouped(p, y, keys)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    out = {"groups_arg": G, "group_skew": args.group_skew, "groups": r["groups"],
           "groups_used": r["groups_used"], "gauc": r["gauc"], "coverage": r["coverage"],
           "group_cal_error": r["group_cal_error"],
           "grouped_ms_min": 1e3 * min(ts), "grouped_ms_median": 1e3 * sorted(ts)[len(ts) // 2]}
    if args.host:
        t0 = time.perf_counter()
        ph, yh, gh = p.cpu().numpy(), y.cpu().numpy(), keys.cpu().numpy().view(np.uint64)
        t1 = time.perf_counter()
        order = np.lexsort((-ph, gh))
        out["grouped_host_d2h_ms"] = 1e3 * (t1 - t0)
        out["grouped_host_lexsort_ms"] = 1e3 * (time.perf_counter() - t1)
        out["grouped_host_ms"] = 1e3 * (time.perf_counter() - t0)
        del order, yh
    return out


if __name__ == "__main__":
    main()
