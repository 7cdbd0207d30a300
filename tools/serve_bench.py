"""What a serving snapshot (checkpoint.save_serving, docs/DESIGN.md §2) buys
over serving the whole training checkpoint, at the bench shape (LR-FTRL,
power-law synthetic Criteo keys over 1e9 features, 39 fields).

A table of 2^--log2-cap slots is prefilled to load 0.47 with keys no batch
touches and trained for --steps steps, as tools/delta_bench.py does; it is
saved as a full checkpoint and as a snapshot.  Then, in one process:

  * checkpoint bytes, load seconds and device bytes of a full ``Predictor``
    against a snapshot ``Predictor``;
  * time per ``eval_step`` at 1, 64, 4096 and 262144 rows x 39 fields on the
    full table, the frozen table with serve_fused off (dedup, pull, forward)
    and the frozen table with serve_fused on (one launch), timed in
    alternating blocks;
  * FM-8: snapshot bytes and keys kept only.

--model fm|mvm [--v-dim D --fm-math M --opt ftrl|sgd --sgd-v-init X] measures
the same three columns for an FM or MVM table instead (2^--fm-log2-cap slots
prefilled to --fm-table-load); the frozen_fused column is then k_serve_fm /
k_serve_mvm.  MVM wants --opt sgd --sgd-v-init 0.9: with the default init of
1e-3 every field product underflows and the table never changes.

    python tools/serve_bench.py [--model fm --v-dim 8] [--out profiles/serve.txt]
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


def trained(a, dev, model, log2_cap, load=None, optim=None):
    eng = Engine(model, optim or OptimConfig(),
                 EngineConfig(table_log2_cap=log2_cap, max_rows=a.batch, max_nnz=a.batch * a.fields,
                              table_grow=False), device=dev)
    synth = SynthConfig(total_features=a.features, hash_space=a.features, seed=a.seed,
                        n_fields=a.fields)
    gen = SyntheticCriteo(eng, a.batch, synth)
    eng.prefill(int((a.table_load if load is None else load) * 2 ** log2_cap))
    for _ in range(a.steps):
        eng.train_view(gen.next())
    torch.cuda.synchronize(dev)
    return eng, synth


def loaded(path, dev, a, **kw):
    torch.cuda.synchronize(dev)
    free0 = torch.cuda.mem_get_info(dev)[0]
    t0 = time.perf_counter()
    p = Predictor(path, device=dev, max_rows=a.batch, max_nnz_per_row=a.fields, **kw)
    torch.cuda.synchronize(dev)
    return p, time.perf_counter() - t0, free0 - torch.cuda.mem_get_info(dev)[0]


def median(v):
    return sorted(v)[len(v) // 2]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--fields", type=int, default=39)
    ap.add_argument("--features", type=int, default=1_000_000_000)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--log2-cap", type=int, default=28)
    ap.add_argument("--table-load", type=float, default=0.47)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--blocks", type=int, default=5, help="alternating timed blocks per batch size")
    ap.add_argument("--fm-log2-cap", type=int, default=25)
    ap.add_argument("--fm-table-load", type=float, default=0.2,
                    help="FM-8 prefill load (the steps' own keys come on top)")
    ap.add_argument("--model", choices=("lr", "fm", "mvm"), default="lr")
    ap.add_argument("--v-dim", type=int, default=8)
    ap.add_argument("--fm-math", choices=("reference", "standard"), default="reference")
    ap.add_argument("--opt", choices=("ftrl", "sgd"), default="ftrl")
    ap.add_argument("--sgd-v-init", type=float, default=1e-3)
    ap.add_argument("--tmp", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lr = a.model == "lr"
    model = ModelConfig(kind=a.model, v_dim=a.v_dim, fm_math=a.fm_math)
    optim = OptimConfig(kind=a.opt, sgd_v_init=a.sgd_v_init)
    log2_cap, load = (a.log2_cap, a.table_load) if lr else (a.fm_log2_cap, a.fm_table_load)
    what = "LR" if lr else ("FM-%d %s" % (a.v_dim, a.fm_math) if a.model == "fm" else "MVM-%d" % a.v_dim)
    say("# tools/serve_bench.py: %s-%s, %d fields, %d features, a table of 2^%d slots prefilled "
        "to load %.2f and trained %d steps of %d rows, %s"
        % (what, a.opt.upper(), a.fields, a.features, log2_cap, load, a.steps, a.batch,
           torch.cuda.get_device_name(dev)))
    tmp = tempfile.mkdtemp(prefix="serve_bench_", dir=a.tmp or None)
    try:
        eng, synth = trained(a, dev, model, log2_cap, load, optim)
        full_dir, snap_dir = os.path.join(tmp, "full"), os.path.join(tmp, "snap")
        checkpoint.save(eng, full_dir, 0, 1, barrier=lambda: None)
        checkpoint.save_serving(eng, snap_dir, 0, 1, barrier=lambda: None)
        m = checkpoint.load_meta(snap_dir)
        del eng
        torch.cuda.empty_cache()
        say("kind keys checkpoint_bytes load_seconds device_bytes")
        arms = []
        for name, path, kw in (("full", full_dir, {}),
                               ("frozen_unfused", snap_dir, {"serve_fused": False}),
                               # ((0, 0): the kernel at every size, not the engine's pick)
                               ("frozen_fused", snap_dir, {"serve_unfused_rows": (0, 0),
                                                           "serve_unfused_rows_latent": (0, 0)})):
            p, s, db = loaded(path, dev, a, **kw)
            arms.append((name, p))
            say("%s %d %d %.3f %d" % (name, p.keys, dir_bytes(path), s, db))
        say("# snapshot: kept %d of %d keys" % (m["keys_kept"], m["keys_total"]))
        say("# ms per eval_step (median of %d alternating blocks; batches generated on the device, "
            "untimed) | the blocks" % a.blocks)
        say("rows " + " ".join(n for n, _ in arms))
        for rows in (1, 8, 16, 32, 64, 128, 256, 512, 1024, 4096, 262144):
            if rows > a.batch:
                continue
            reps = 200 if rows <= 4096 else 20
            gens = [SyntheticCriteo(p.engine, rows, synth) for _, p in arms]
            bats = [[g.alloc_batch() for _ in range(4)] for g in gens]
            for g, bs in zip(gens, bats):
                for b in bs:
                    g.next(out=b)
            times = [[] for _ in arms]
            for blk in range(a.blocks + 1):  # (block 0: warm-up)
                for i, (_, p) in enumerate(arms):
                    out = torch.empty(rows, dtype=torch.float32, device=dev)
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for r in range(reps):
                        p.engine.eval_step(bats[i][r % 4], out)
                    torch.cuda.synchronize(dev)
                    if blk:
                        times[i].append(1000.0 * (time.perf_counter() - t0) / reps)
            say("%d %s | %s" % (rows, " ".join("%.4f" % median(t) for t in times),
                                " ; ".join(" ".join("%.4f" % x for x in t) for t in times)))
        del arms, gens, bats, p
        torch.cuda.empty_cache()
        if lr:  # FM-8: sizes only
            eng, _ = trained(a, dev, ModelConfig(kind="fm", v_dim=8), a.fm_log2_cap,
                             a.fm_table_load)
            ffull, fsnap = os.path.join(tmp, "fm_full"), os.path.join(tmp, "fm_snap")
            checkpoint.save(eng, ffull, 0, 1, barrier=lambda: None)
            checkpoint.save_serving(eng, fsnap, 0, 1, barrier=lambda: None)
            m = checkpoint.load_meta(fsnap)
            say("# FM-8, 2^%d slots prefilled to load %.2f: checkpoint %d bytes, snapshot %d bytes, "
                "kept %d of %d keys" % (a.fm_log2_cap, a.fm_table_load, dir_bytes(ffull),
                                        dir_bytes(fsnap), m["keys_kept"], m["keys_total"]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if a.out:  # (only a run that finished writes its table)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
