"""What pruning (Engine.prune) costs and buys.

Part 1, the walk: ms per 2^20-slot segment for LR-FTRL (16-byte slots) and
FM v_dim 8 (96-byte slots) on a table at load 0.47 in which half of the keys
meet the pruning rule (zero state, pushed flag set) and half do not.  The
number to hold it against is the split's, which is the same cluster walk with
a buddy segment to move into: 0.15 ms (LR) and 0.5-0.7 ms (FM-8 / MVM-10) per
segment, profiles/r4_table_segments.txt.  A prune() call is timed whole: the
marks pass, the walk, the counter read-back that ends it.

Part 2, at the bench shape (LR-FTRL, 262144 rows x 39 fields per step,
power-law synthetic Criteo keys over 1e9 features): twin engines train N
steps from an empty table, one prunes, both train M more; the table's keys
before and after, and the progressive logloss (each batch scored before it
trains) of the M steps with and without the prune.

    python tools/prune_bench.py [--out profiles/prune.txt]
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
from xflow_amd.data.synth import SynthConfig, SyntheticCriteo  # noqa: E402
from xflow_amd.engine import Engine  # noqa: E402
from xflow_amd.testing.hashing import fmix64  # noqa: E402


def walk(kind, v_dim, log2_cap, load, dev, reps):
    """ms per prune() of a 2^log2_cap table at `load`, half the keys droppable
    (rebuilt for every repetition: a second prune finds nothing to do)."""
    n = int(load * 2 ** log2_cap)
    keys = fmix64(np.arange(1, n + 1, dtype=np.uint64))
    out = []
    for _ in range(reps):
        eng = Engine(ModelConfig(kind=kind, v_dim=v_dim), OptimConfig(),
                     EngineConfig(table_log2_cap=log2_cap, table_grow=False, max_rows=64,
                                  max_nnz=4096), device=dev)
        P, W = eng.layout["P"], eng.state_words
        words = np.zeros((n, W), dtype=np.uint32)
        st = np.zeros((n, P, 2), dtype=np.float32)
        st[::2, :, 0] = 1.0   # every other key: n = 1, z = 1 on each parameter (weight != 0)
        st[::2, :, 1] = 1.0
        words[:, :2 * P] = st.reshape(n, 2 * P).view(np.uint32)
        if kind != "lr":
            words[:, 2 * P] = 1
        eng.import_table(keys, words.reshape(-1))
        del words, st
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        dropped = eng.prune()
        torch.cuda.synchronize(dev)
        out.append(1000.0 * (time.perf_counter() - t0))
        assert dropped == n // 2 and eng.table_size() == n - dropped, (dropped, n)
        segs = eng.table_geometry["segments"]
        del eng
        torch.cuda.empty_cache()
    return out, segs, n


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2-cap", type=int, default=24, help="part 1: table slots (LR)")
    ap.add_argument("--fm-log2-cap", type=int, default=23, help="part 1: table slots (FM-8)")
    ap.add_argument("--table-load", type=float, default=0.47)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--more-steps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--fields", type=int, default=39)
    ap.add_argument("--features", type=int, default=1_000_000_000)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--empty-log2-cap", type=int, default=24, help="part 2: initial table slots")
    ap.add_argument("--skip-walk", action="store_true")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# tools/prune_bench.py on %s" % torch.cuda.get_device_name(dev))
    if not a.skip_walk:
        say("# part 1: prune() of a table at load %.2f, half of its keys droppable; "
            "ms per 2^20-slot segment" % a.table_load)
        say("# (the split, same walk: LR 0.15, FM-8 / MVM-10 0.5-0.7 ms per segment, "
            "profiles/r4_table_segments.txt)")
        say("model slots keys segments ms_per_segment_median ms_per_prune_reps ratio_to_split")
        for name, kind, vd, lg, split_ms in (("lr", "lr", 10, a.log2_cap, 0.15),
                                             ("fm8", "fm", 8, a.fm_log2_cap, 0.6)):
            ms, segs, n = walk(kind, vd, lg, a.table_load, dev, a.reps)
            per = sorted(ms)[len(ms) // 2] / segs * (2 ** 20 / (2 ** lg / segs))
            say("%s %d %d %d %.3f %s %.2f" % (name, 2 ** lg, n, segs, per,
                                               " ".join("%.3f" % m for m in ms), per / split_ms))
    if not a.skip_train:
        say("# part 2: LR-FTRL, %d rows x %d fields per step, %d features; %d steps from an empty "
            "table of 2^%d slots (grows), then %d more" % (a.batch, a.fields, a.features, a.steps,
                                                            a.empty_log2_cap, a.more_steps))
        say("arm keys_after_%d_steps keys_after_prune nonzero_weights prune_ms logloss_next_%d"
            % (a.steps, a.more_steps))
        for arm in ("plain", "pruned"):
            eng = Engine(ModelConfig(kind="lr"), OptimConfig(),
                         EngineConfig(table_log2_cap=a.empty_log2_cap, max_rows=a.batch,
                                      max_nnz=a.batch * a.fields), device=dev)
            gen = SyntheticCriteo(eng, a.batch, SynthConfig(total_features=a.features,
                                                            hash_space=a.features, seed=a.seed,
                                                            n_fields=a.fields))
            for _ in range(a.steps):
                eng.train_view(gen.next())
            before = eng.table_size()
            nnz = eng.nonzero_weights()
            ms = 0.0
            if arm == "pruned":
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                eng.prune()
                torch.cuda.synchronize(dev)
                ms = 1000.0 * (time.perf_counter() - t0)
            after = eng.table_size()
            eng.read_stats(reset=True)
            for _ in range(a.more_steps):
                eng.train_view(gen.next())
            torch.cuda.synchronize(dev)
            st = eng.read_stats()
            say("%s %d %d %d %.3f %.6f" % (arm, before, after, nnz, ms,
                                          st["ln_loss"] / max(st["rows"], 1.0)))
            del eng, gen
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
