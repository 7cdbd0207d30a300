"""``xflow_lr``-compatible command line (multi-rank capable).

    python -m xflow_amd.cli <train_prefix> <test_prefix> <model 0|1|2> <epochs> [flags]

Positional arguments are the reference binary's (src/model/main.cc:15-48).
Process roles follow the reference launch scripts' DMLC_ROLE: scheduler and
server processes exit (the workers' GPUs hold the table shards); workers
train.  World size / rank come from torchrun env (RANK, WORLD_SIZE, ...) or
DMLC_NUM_WORKER / DMLC_WORKER_ID (scripts/local.sh sets both).
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

from xflow_amd.config import (EngineConfig, ModelConfig, OptimConfig, TrainConfig,
                              MODEL_NAMES, model_kind, parse_crosses)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="xflow_lr", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("train_prefix")
    ap.add_argument("test_prefix")
    ap.add_argument("model", help="0 = LR, 1 = FM, 2 = MVM (or lr/fm/mvm)")
    ap.add_argument("epochs", type=int)
    ap.add_argument("--threads", type=int, default=0,
                    help="slices per block (default: os.cpu_count(), like hardware_concurrency)")
    ap.add_argument("--serial-slices", action="store_true",
                    help="one step per slice instead of all slices in one step")
    ap.add_argument("--keep-remainder", action="store_true",
                    help="train rows %% threads too (the reference drops them)")
    ap.add_argument("--optimizer", choices=["ftrl", "sgd"], default="ftrl")
    ap.add_argument("--alpha", type=float, default=5e-2)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--lambda1", type=float, default=5e-5)
    ap.add_argument("--lambda2", type=float, default=10.0)
    ap.add_argument("--lr", type=float, default=1e-3, help="SGD learning rate")
    ap.add_argument("--v-dim", type=int, default=10)
    ap.add_argument("--fm-math", choices=["reference", "standard"], default="reference")
    ap.add_argument("--mvm-math", choices=["compat", "fixed"], default="compat")
    ap.add_argument("--mvm-predict-compat", action="store_true")
    ap.add_argument("--sum-slices", action="store_true",
                    help="one FTRL push of the summed slice gradients per step")
    ap.add_argument("--no-init-push", action="store_true")
    ap.add_argument("--async", dest="async_ps", action="store_true",
                    help="multi-rank: the asynchronous parameter server (BASELINE config 4) -- a "
                         "server thread per rank, workers that never wait for each other")
    ap.add_argument("--async-lockstep", dest="async_p2p", action="store_true",
                    help="multi-rank: lock-step steps whose pushes ride in the next exchange")
    ap.add_argument("--staleness", type=int, default=1,
                    help="--async: own pushes in flight (0..7); --async-lockstep: pulls miss "
                         "the previous N steps' pushes (1..7)")
    ap.add_argument("--log2-cap", type=int, default=22,
                    help="initial table slots per rank = 2^N (the table grows)")
    ap.add_argument("--max-log2-cap", type=int, default=0,
                    help="growth limit 2^N slots per rank (0: 2^31, or what free HBM allows)")
    ap.add_argument("--no-table-grow", action="store_true",
                    help="fixed table capacity: an overflow raises within two steps")
    ap.add_argument("--admit-min-count", type=int, default=1,
                    help="feature admission: a key enters the table only after a counting filter "
                         "has seen it N times in training pulls (1..255; 1: off)")
    ap.add_argument("--admit-log2", type=int, default=0,
                    help="admission filter bytes per rank = 2^N (6..32; 0: min(32, the table's "
                         "largest log2 capacity + 1))")
    ap.add_argument("--prune-every", type=int, default=0,
                    help="every N epochs drop the keys whose weights are all exactly zero "
                         "(what L1 zeroed; 0: never)")
    ap.add_argument("--prune-max-n", type=float, default=-1.0,
                    help="--prune-every, FTRL: drop only keys with every n <= this (0: never "
                         "pushed a non-zero gradient; negative: no bound)")
    ap.add_argument("--gauc-field", type=int, default=-1,
                    help="also report the grouped AUC (GAUC) and per-group calibration of the "
                         "test predictions, grouped by the key of this field id (-1: off)")
    ap.add_argument("--train-block-bytes", type=int, default=2 << 20)
    ap.add_argument("--test-block-bytes", type=int, default=0)
    ap.add_argument("--gpu-parse", action="store_true",
                    help="tokenise libffm text on the GPU (raw blocks uploaded; keys, labels and "
                         "field ids bit-equal to the host parser)")
    ap.add_argument("--resident", action="store_true",
                    help="keep the training shard in HBM after the first epoch (no re-read)")
    ap.add_argument("--shuffle", action="store_true",
                    help="reshuffle each block's rows on the device every epoch (with --resident "
                         "also the block order); not for packed shards or --serial-slices")
    ap.add_argument("--shuffle-seed", type=int, default=0,
                    help="--shuffle: the run's seed (a block's order depends only on it, the "
                         "epoch, the block and the rank)")
    ap.add_argument("--cross", default="",
                    help="feature crosses computed on the device: 3x7,1x2x5 adds to every row one "
                         "key per cross, hashed from its keys of those field ids in that order "
                         "(2..4 fields, at most 16 crosses; a missing field still gives a key); "
                         "not for packed shards or --serial-slices")
    ap.add_argument("--cross-field-base", type=int, default=-1,
                    help="--cross: cross c enters the model as field id N + c (required for MVM, "
                         "whose products run over field ids)")
    ap.add_argument("--csr-only", action="store_true",
                    help="train fixed-width blocks through the CSR path as well")
    ap.add_argument("--block-rows", type=int, default=0,
                    help="rows per block when <prefix>-%%05d.xfb binary shards exist "
                         "(python -m xflow_amd.data.binfmt convert); default 65536")
    ap.add_argument("--cpu", action="store_true", help="use the native CPU backend")
    ap.add_argument("--pred-dir", default=".")
    ap.add_argument("--no-pred-file", action="store_true",
                    help="skip pred_<rank>_<block>.txt (AUC/logloss are computed on the device "
                         "either way; the file is the only reason predictions reach the host)")
    ap.add_argument("--fm-mfma", action="store_true",
                    help="standard-math FM forward on the matrix cores (v_dim <= 8; A/B option)")
    ap.add_argument("--save", default="", help="checkpoint directory to write after training")
    ap.add_argument("--load", default="", help="checkpoint directory to resume from")
    ap.add_argument("--resume", default="",
                    help="versioned checkpoint root: continue from its LATEST checkpoint if one "
                         "exists (epochs = total for the run) and write periodic saves there")
    ap.add_argument("--save-every", type=int, default=0,
                    help="versioned checkpoint every N epochs under --resume (or --save) root")
    ap.add_argument("--save-delta", action="store_true",
                    help="versioned checkpoints (--save-every) write only the keys touched since "
                         "the previous version; loading resolves the chain of deltas")
    ap.add_argument("--delta-full-every", type=int, default=8,
                    help="--save-delta: every K-th version of a chain is a full one (bounds the "
                         "chain's length and the restart time)")
    ap.add_argument("--delta-log2", type=int, default=0,
                    help="--save-delta: bits of the touched-key filter per rank = 2^N (10..34; 0: "
                         "min(34, the table's largest log2 capacity + 2))")
    ap.add_argument("--save-serving", default="",
                    help="after the last epoch every rank writes its shard's serving snapshot "
                         "here: only the keys that differ from an absent key, as resolved fp32 "
                         "weights (xflow_amd.serve loads it; it cannot be resumed from)")
    ap.add_argument("--serving-every", type=int, default=0,
                    help="with --save-serving DIR: at the end of every N-th epoch write a serving "
                         "version DIR/epoch-XXXXXX/ (a delta on the previous one) and point "
                         "DIR/LATEST at it; xflow_amd.serve's refresh follows it (0: off)")
    ap.add_argument("--serving-full-every", type=int, default=8,
                    help="--serving-every: every K-th serving version of a chain is a full snapshot")
    ap.add_argument("--metrics", default="", help="JSON-lines metrics file (rank 0)")
    ap.add_argument("--trace-dir", default="", help="torch.profiler chrome trace directory")
    return ap


def config_from_args(a) -> TrainConfig:
    kind = MODEL_NAMES[model_kind(a.model)]
    return TrainConfig(
        train_prefix=a.train_prefix, test_prefix=a.test_prefix, epochs=a.epochs,
        threads=a.threads, train_block_bytes=a.train_block_bytes, block_rows=a.block_rows,
        resident=a.resident, fixed_width=not a.csr_only, gpu_parse=a.gpu_parse,
        shuffle=a.shuffle, shuffle_seed=a.shuffle_seed,
        crosses=parse_crosses(a.cross), cross_field_base=a.cross_field_base,
        test_block_bytes=a.test_block_bytes, serial_slices=a.serial_slices,
        keep_remainder=a.keep_remainder, mvm_predict_compat=a.mvm_predict_compat,
        init_push=not a.no_init_push, pred_dir=a.pred_dir, write_pred=not a.no_pred_file,
        checkpoint_dir=a.save,
        save_every=a.save_every, resume_dir=a.resume,
        save_delta=a.save_delta, delta_full_every=a.delta_full_every,
        save_serving=a.save_serving,
        serving_every=a.serving_every, serving_full_every=a.serving_full_every,
        prune_every=a.prune_every, prune_max_n=a.prune_max_n, gauc_field=a.gauc_field,
        metrics_file=a.metrics, async_p2p=a.async_p2p, async_ps=a.async_ps,
        staleness=a.staleness,
        model=ModelConfig(kind=kind, v_dim=a.v_dim, fm_math=a.fm_math, mvm_math=a.mvm_math,
                          fm_mfma=a.fm_mfma),
        optim=OptimConfig(kind=a.optimizer, alpha=a.alpha, beta=a.beta, lambda1=a.lambda1,
                          lambda2=a.lambda2, lr=a.lr),
        engine=EngineConfig(table_log2_cap=a.log2_cap, sum_slices=a.sum_slices,
                            max_log2_cap=a.max_log2_cap, table_grow=not a.no_table_grow,
                            admit_min_count=a.admit_min_count, admit_log2=a.admit_log2,
                            delta_track=a.save_delta or a.serving_every > 0, delta_log2=a.delta_log2))


def main(argv=None) -> int:
    from xflow_amd.parallel import dist as xdist

    if xdist.is_scheduler():
        return 0
    if xdist.is_server():
        print("init server success ", flush=True)
        return 0
    a = build_parser().parse_args(argv)
    cfg = config_from_args(a)
    print({0: "start LR ", 1: "start FM ", 2: "start MVM "}[model_kind(a.model)], flush=True)
    device = torch.device("cpu") if a.cpu else xdist.device_for_rank()
    from xflow_amd.trainer import Trainer
    from xflow_amd.utils.trace import torch_profile

    t = Trainer(cfg, device=device)
    try:
        if a.load:
            t.load(a.load)
        if a.resume:
            t.resume(a.resume)
        with torch_profile(a.trace_dir):
            t.train()
        if a.save:
            t.save(a.save)
    finally:
        t.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
