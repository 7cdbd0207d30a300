"""What a serving delta (docs/DESIGN.md §2 "Serving deltas") costs against the
only other way to serve a new model: export everything, build a new Predictor
from the full snapshot.  tools/serve_bench.py's setup (LR-FTRL, power-law
synthetic Criteo keys over 1e9 features, 39 fields): a table of 2^--log2-cap
slots prefilled to load 0.47 with keys no batch touches, trained --steps steps
with delta tracking on, snapshotted into a Predictor; then --rounds rounds of
--round-steps more steps, each measured on both sides:

  producer   export_weights_delta against a full export_weights
  consumer   Predictor.refresh() through the delta (apply_weights_delta, its
             upsert and sweep steps apart) against building a new Predictor
             from a full snapshot of the same version
  and        the delta's entries, the keys dropped, the segments swept, the
             delta's and the snapshot's file bytes; eval_step at 1 / 4096 /
             --batch rows before the first and after the last applied delta

--model fm --v-dim 8 repeats it for an FM table (2^--fm-log2-cap slots).  No
target is set: the ratios are what the run reports.

    python tools/refresh_bench.py [--model fm] [--out profiles/refresh.txt]
"""
from __future__ import annotations

import argparse
import os
import shutil
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xflow_amd import checkpoint  # noqa: E402
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig  # noqa: E402
from xflow_amd.data.synth import SynthConfig, SyntheticCriteo  # noqa: E402
from xflow_amd.engine import Engine  # noqa: E402
from xflow_amd.serve import Predictor  # noqa: E402


def dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def timed(dev, fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize(dev)
    return r, time.perf_counter() - t0


def eval_ms(pred, gen_batches, dev, reps=50):
    out = []
    for b in gen_batches:
        for _ in range(5):
            pred.engine.eval_step(b)
        _, s = timed(dev, lambda: [pred.engine.eval_step(b) for _ in range(reps)])
        out.append(1000.0 * s / reps)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--fields", type=int, default=39)
    ap.add_argument("--features", type=int, default=1_000_000_000)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--log2-cap", type=int, default=26)
    ap.add_argument("--table-load", type=float, default=0.47)
    ap.add_argument("--fm-log2-cap", type=int, default=25)
    ap.add_argument("--fm-table-load", type=float, default=0.2)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--round-steps", type=int, default=10)
    ap.add_argument("--model", choices=("lr", "fm"), default="lr")
    ap.add_argument("--v-dim", type=int, default=8)
    ap.add_argument("--tmp", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("refresh_bench: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lr = a.model == "lr"
    model = ModelConfig(kind=a.model, v_dim=a.v_dim)
    log2_cap, load = (a.log2_cap, a.table_load) if lr else (a.fm_log2_cap, a.fm_table_load)
    say("# tools/refresh_bench.py: %s-FTRL, %d fields, a table of 2^%d slots prefilled to load "
        "%.2f, %d steps of %d rows, then %d rounds of %d steps, %s"
        % ("LR" if lr else "FM-%d" % a.v_dim, a.fields, log2_cap, load, a.steps, a.batch,
           a.rounds, a.round_steps, torch.cuda.get_device_name(dev)))
    eng = Engine(model, OptimConfig(),
                 EngineConfig(table_log2_cap=log2_cap, max_rows=a.batch, max_nnz=a.batch * a.fields,
                              table_grow=False, delta_track=True), device=dev)
    gen = SyntheticCriteo(eng, a.batch, SynthConfig(total_features=a.features,
                                                    hash_space=a.features, seed=a.seed,
                                                    n_fields=a.fields))
    eng.prefill(int(load * 2 ** log2_cap))
    for _ in range(a.steps):
        eng.train_view(gen.next())
    tmp = tempfile.mkdtemp(prefix="refresh_bench_", dir=a.tmp or None)
    none = lambda: None  # noqa: E731
    try:
        root = os.path.join(tmp, "serving")
        checkpoint.save_serving(eng, checkpoint.version_dir(root, 0), 0, 1, barrier=none)
        checkpoint.publish_serving(root, 0, keep=2)
        pred = Predictor(root, device=dev, max_rows=a.batch, max_nnz_per_row=a.fields)
        say("base snapshot: %d of %d keys, %.1f MB" % (pred.keys, eng.table_size(),
                                                      dir_bytes(pred.ckpt) / 1e6))
        ev = SyntheticCriteo(pred.engine, a.batch, SynthConfig(
            total_features=a.features, hash_space=a.features, seed=a.seed + 1, n_fields=a.fields))
        full = ev.alloc_batch()
        ev.next(out=full)
        sizes = (1, 4096, a.batch)
        from xflow_amd.engine import Batch

        def head(rows):  # (the first rows of the row-major batch)
            return Batch(keys=full.keys[:rows * a.fields].contiguous(), labels=full.labels[:rows],
                         nnz_per_row=a.fields, slice_rows=rows)

        batches = [head(r) for r in sizes]
        say("eval_step ms at %s rows before any delta: %s"
            % (sizes, ["%.4f" % x for x in eval_ms(pred, batches, dev)]))
        for rnd in range(1, a.rounds + 1):
            for _ in range(a.round_steps):
                eng.train_view(gen.next())
            (dk, _dw), t_delta = timed(dev, eng.export_weights_delta)
            (fk, _fw), t_full = timed(dev, eng.export_weights)
            # the version on disk: a delta under the root, a full snapshot aside
            side = os.path.join(tmp, "full-%d" % rnd)
            checkpoint.save_serving(eng, side, 0, 1, barrier=none, clear=False)
            d = checkpoint.version_dir(root, rnd)
            p = checkpoint.save_serving(eng, d, 0, 1, barrier=none,
                                        delta_base=os.path.basename(checkpoint.version_dir(root, rnd - 1)))
            assert p.endswith(".xfwd"), p
            checkpoint.publish_serving(root, rnd, keep=2)
            r, t_refresh = timed(dev, pred.refresh)
            assert r["mode"] == "delta", r
            (dk2, dw2) = checkpoint.read_serving_delta(p)[1:]
            _, t_rebuild = timed(dev, lambda: Predictor(side, device=dev, max_rows=a.batch,
                                                        max_nnz_per_row=a.fields))
            say("round %d: delta %d entries (%.1f MB) of %d kept keys (%.1f MB full)"
                % (rnd, len(dk), dir_bytes(d) / 1e6, len(fk), dir_bytes(side) / 1e6))
            say("  producer  export_weights_delta %.4f s, export_weights %.4f s (x%.1f)"
                % (t_delta, t_full, t_full / max(t_delta, 1e-9)))
            say("  consumer  refresh %.4f s (inserted %d, overwritten %d, dropped %d, segments "
                "swept %d), new Predictor from the full snapshot %.4f s (x%.1f)"
                % (t_refresh, r["inserted"], r["overwritten"], r["dropped"], r["segments_swept"],
                   t_rebuild, t_rebuild / max(t_refresh, 1e-9)))
            # the apply alone, its two steps apart, on a second frozen engine
            # at the previous version would need that engine; the same delta
            # applied again is all overwrites plus the same deletions' sweep
            r2 = pred.engine.apply_weights_delta(dk2, dw2)
            say("  the same delta applied again: upsert %.4f s, sweep %.4f s%s"
                % (r2["upsert_seconds"], r2["sweep_seconds"],
                   "  (the sweep dominates)" if r2["sweep_seconds"] > r2["upsert_seconds"] else ""))
            shutil.rmtree(side)
        say("eval_step ms at %s rows after %d deltas: %s"
            % (sizes, a.rounds, ["%.4f" % x for x in eval_ms(pred, batches, dev)]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
