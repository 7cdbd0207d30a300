"""What feature admission (EngineConfig.admit_min_count) buys and costs at the
bench shape (LR-FTRL, 262144 rows x 39 fields per step, power-law synthetic
Criteo keys over 1e9 features).

Part 1, from an EMPTY growing table: N steps with admit_min_count 1, 2 and 4;
per setting the table's keys, the bytes committed to it, the filter's bytes,
ms/step and the progressive logloss (each batch scored before it trains) of
the last quarter of the steps.

Part 2, steady state: two engines with tables prefilled to load 0.47 (2^31
slots, 1e9 keys no batch touches), admission 1 and 2, timed in alternating
blocks of steps in one process.

    python tools/admit_bench.py [--steps N] [--out profiles/admit.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig  # noqa: E402
from xflow_amd.data.synth import SynthConfig, SyntheticCriteo  # noqa: E402
from xflow_amd.engine import Engine  # noqa: E402


def make(a, dev, log2_cap, admit, admit_log2=0):
    eng = Engine(ModelConfig(kind="lr"), OptimConfig(),
                 EngineConfig(table_log2_cap=log2_cap, max_rows=a.batch, max_nnz=a.batch * a.fields,
                              admit_min_count=admit, admit_log2=admit_log2), device=dev)
    synth = SynthConfig(total_features=a.features, hash_space=a.features, seed=a.seed,
                        n_fields=a.fields)
    return eng, SyntheticCriteo(eng, a.batch, synth)


def timed(eng, gen, steps, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.train_view(gen.next())
    torch.cuda.synchronize(dev)
    return 1000.0 * (time.perf_counter() - t0) / steps


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--fields", type=int, default=39)
    ap.add_argument("--features", type=int, default=1_000_000_000)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--empty-log2-cap", type=int, default=24, help="part 1: initial table slots")
    ap.add_argument("--log2-cap", type=int, default=31, help="part 2: table slots")
    ap.add_argument("--table-load", type=float, default=0.47)
    ap.add_argument("--blocks", type=int, default=6, help="part 2: alternating timed blocks")
    ap.add_argument("--block-steps", type=int, default=20)
    ap.add_argument("--skip-steady", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# tools/admit_bench.py: LR-FTRL, %d rows x %d fields per step, %d features, %s"
        % (a.batch, a.fields, a.features, torch.cuda.get_device_name(dev)))
    say("# (ms/step include the on-device batch generator, alike in every arm)")
    say("# part 1: %d steps from an empty table of 2^%d slots (grows)" % (a.steps, a.empty_log2_cap))
    say("admit_min_count table_keys table_bytes_committed filter_bytes ms_per_step "
        "logloss_last_quarter")
    tail = max(1, a.steps // 4)
    for admit in (1, 2, 4):
        eng, gen = make(a, dev, a.empty_log2_cap, admit)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for s in range(a.steps):
            if s == a.steps - tail:
                eng.read_stats(reset=True)
            eng.train_view(gen.next())
        torch.cuda.synchronize(dev)
        ms = 1000.0 * (time.perf_counter() - t0) / a.steps
        st = eng.read_stats()
        say("%d %d %d %d %.3f %.5f" % (admit, eng.table_size(), eng.table_committed,
                                       eng.admit_bytes(), ms, st["ln_loss"] / max(st["rows"], 1.0)))
        del eng, gen
        torch.cuda.empty_cache()
    if not a.skip_steady:
        n_pre = int(a.table_load * 2 ** a.log2_cap)
        say("# part 2: tables of 2^%d slots prefilled with %d keys (load %.2f), %d alternating "
            "blocks of %d steps" % (a.log2_cap, n_pre, a.table_load, a.blocks, a.block_steps))
        pair = []
        for admit in (1, 2):
            eng, gen = make(a, dev, a.log2_cap, admit)
            eng.prefill(n_pre)
            timed(eng, gen, 5, dev)  # warm-up
            pair.append((admit, eng, gen, []))
        for _ in range(a.blocks):
            for admit, eng, gen, ms in pair:
                ms.append(timed(eng, gen, a.block_steps, dev))
        say("admit_min_count ms_per_step_median ms_per_step_blocks")
        med = {}
        for admit, eng, gen, ms in pair:
            med[admit] = sorted(ms)[len(ms) // 2]
            say("%d %.3f %s" % (admit, med[admit], " ".join("%.3f" % m for m in ms)))
        say("# steady-state cost of admission 2 over 1: %+.2f %%" % (100.0 * (med[2] / med[1] - 1.0)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
