"""What delta checkpoints (EngineConfig.delta_track) cost per step and what
they buy per save, at the bench shape (LR-FTRL, 262144 rows x 39 fields per
step, power-law synthetic Criteo keys over 1e9 features).

Part 1, step cost: two engines with tables prefilled to load 0.47 (2^31
slots, 1e9 keys no batch touches), tracking off and on (automatic
delta_log2), timed in alternating blocks of steps in one process.  Every
block starts with delta_clear() and times its first step on its own -- every
key of that step takes the atomic -- then the steady state.

Part 2, what a save costs: a table of 2^--save-log2-cap slots (small enough
that the full export's device buffers fit next to it) prefilled to the same
load, tracking on, 120 steps; then Engine.save against Engine.save_delta:
seconds, file bytes, the peak of extra device memory while each ran (free
memory sampled every few ms), and the delta's false-positive share.

    python tools/delta_bench.py [--out profiles/delta.txt]
"""
from __future__ import annotations

import argparse
import os
import shutil
import sys
import tempfile
import threading
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig  # noqa: E402
from xflow_amd.data.synth import SynthConfig, SyntheticCriteo  # noqa: E402
from xflow_amd.engine import Engine  # noqa: E402


def make(a, dev, log2_cap, track):
    eng = Engine(ModelConfig(kind="lr"), OptimConfig(),
                 EngineConfig(table_log2_cap=log2_cap, max_rows=a.batch, max_nnz=a.batch * a.fields,
                              table_grow=False, delta_track=track), device=dev)
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


def with_peak(dev, fn):
    """(seconds, peak extra device bytes) of fn(): free memory sampled while it runs."""
    torch.cuda.synchronize(dev)
    free0 = torch.cuda.mem_get_info(dev)[0]
    low, stop = [free0], threading.Event()

    def poll():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info(dev)[0])
            time.sleep(0.002)

    th = threading.Thread(target=poll)
    th.start()
    t0 = time.perf_counter()
    try:
        fn()
    finally:
        s = time.perf_counter() - t0
        stop.set()
        th.join()
    return s, free0 - low[0]


def median(v):
    return sorted(v)[len(v) // 2]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--fields", type=int, default=39)
    ap.add_argument("--features", type=int, default=1_000_000_000)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--log2-cap", type=int, default=31, help="part 1: table slots")
    ap.add_argument("--table-load", type=float, default=0.47)
    ap.add_argument("--blocks", type=int, default=6, help="part 1: alternating timed blocks")
    ap.add_argument("--block-steps", type=int, default=20)
    ap.add_argument("--save-log2-cap", type=int, default=28, help="part 2: table slots")
    ap.add_argument("--save-steps", type=int, default=120)
    ap.add_argument("--tmp", default="", help="part 2: directory for the shard files (deleted)")
    ap.add_argument("--skip-steps", action="store_true", help="part 2 only")
    ap.add_argument("--skip-save", action="store_true", help="part 1 only")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# tools/delta_bench.py: LR-FTRL, %d rows x %d fields per step, %d features, %s"
        % (a.batch, a.fields, a.features, torch.cuda.get_device_name(dev)))
    say("# (ms/step include the on-device batch generator, alike in every arm)")
    if not a.skip_steps:
        n_pre = int(a.table_load * 2 ** a.log2_cap)
        say("# part 1: tables of 2^%d slots prefilled with %d keys (load %.2f), %d alternating "
            "blocks: delta_clear(), 1 step timed alone, then %d steps"
            % (a.log2_cap, n_pre, a.table_load, a.blocks, a.block_steps))
        pair = []
        for track in (False, True):
            eng, gen = make(a, dev, a.log2_cap, track)
            eng.prefill(n_pre)
            timed(eng, gen, 5, dev)  # warm-up
            pair.append((track, eng, gen, [], []))
        for _ in range(a.blocks):
            for track, eng, gen, first, steady in pair:
                eng.delta_clear()
                first.append(timed(eng, gen, 1, dev))
                steady.append(timed(eng, gen, a.block_steps, dev))
        say("delta_track delta_log2 first_step_ms_median steady_ms_per_step_median "
            "steady_ms_per_step_blocks | first_step_ms_blocks")
        med = {}
        for track, eng, gen, first, steady in pair:
            med[track] = (median(first), median(steady))
            say("%d %d %.3f %.3f %s | %s" % (track, eng.delta_log2, med[track][0], med[track][1],
                                            " ".join("%.3f" % m for m in steady),
                                            " ".join("%.3f" % m for m in first)))
        say("# cost of tracking, steady state: %+.2f %%; first step after a clear: %+.2f %%"
            % (100.0 * (med[True][1] / med[False][1] - 1.0),
               100.0 * (med[True][0] / med[False][0] - 1.0)))
        st = pair[1][1].delta_stats()
        say("# filter after the last block: %d of 2^%d bits set" % (st["bits_set"], st["log2"]))
        del pair, eng, gen
        torch.cuda.empty_cache()
    if not a.skip_save:
        n_pre = int(a.table_load * 2 ** a.save_log2_cap)
        eng, gen = make(a, dev, a.save_log2_cap, True)
        eng.prefill(n_pre)
        eng.delta_clear()
        for _ in range(a.save_steps):
            eng.train_view(gen.next())
        keys = eng.table_size()
        touched = keys - n_pre  # (prefilled keys have bit 62 set: no batch touches them)
        nd = eng.delta_count()
        st = eng.delta_stats()
        W = eng.state_words
        say("# part 2: a table of 2^%d slots (%d bytes) prefilled with %d keys, %d steps: %d keys, "
            "%d of them touched; filter 2^%d bits (%d bytes), %d set"
            % (a.save_log2_cap, eng.table_committed, n_pre, a.save_steps, keys, touched,
               st["log2"], (1 << st["log2"]) // 8, st["bits_set"]))
        tmp = tempfile.mkdtemp(prefix="delta_bench_", dir=a.tmp or None)
        try:
            say("kind keys file_bytes seconds peak_extra_device_bytes buffers_bytes")
            for kind, fn, n in (("full", eng.save, keys), ("delta", eng.save_delta, nd)):
                p = os.path.join(tmp, kind + ".xftb")
                fn(p)  # (the staging buffers' one allocation, the page cache)
                s, peak = with_peak(dev, lambda: fn(p))
                say("%s %d %d %.3f %d %d" % (kind, n, os.path.getsize(p), s, peak,
                                             n * (8 + 4 * W)))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        say("# delta false positives: %d of %d exported keys (%.4f %%), delta / full keys %.4f"
            % (nd - touched, nd, 100.0 * (nd - touched) / max(nd, 1), nd / max(keys, 1)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
