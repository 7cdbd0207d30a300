"""Configuration dataclasses.  Defaults equal the reference's compile-time
constants:

=====================  ==========================  =====================================
knob                   default                     reference
=====================  ==========================  =====================================
FTRL alpha/beta/l1/l2  0.05 / 1.0 / 5e-5 / 10.0    src/optimizer/ftrl.h:17-20
latent dim             10                          fm_worker.h:92, mvm_worker.h:92
SGD lr                 0.001                       src/optimizer/sgd.h:16
SGD v init             0.001                       src/optimizer/sgd.h:69
FTRL v init            N(0,1) * 1e-2               src/optimizer/ftrl.h:117
train block            2 MB                        lr_worker.h:68
test block             4 MB (LR) / 2 MB (FM, MVM)  lr_worker.cc:80, fm_worker.cc:106
epochs                 60                          lr_worker.h:63
slices per block       hardware_concurrency        lr_worker.h:40
=====================  ==========================  =====================================
"""
from __future__ import annotations

import dataclasses
import os
from dataclasses import dataclass, field

MODEL_KINDS = {"lr": 0, "fm": 1, "mvm": 2}
MODEL_NAMES = {v: k for k, v in MODEL_KINDS.items()}
# "frozen": a read-only table of resolved fp32 weights (a serving snapshot,
# docs/DESIGN.md §2), never an optimiser to train with
OPT_KINDS = {"ftrl": 0, "sgd": 1, "frozen": 2}
FM_MATH = {"reference": 0, "standard": 1}
MVM_MATH = {"compat": 0, "fixed": 1}


def model_kind(m) -> int:
    if isinstance(m, int):
        if m not in MODEL_NAMES:
            raise ValueError(f"model index must be 0 (LR), 1 (FM) or 2 (MVM), got {m}")
        return m
    m = str(m).lower()
    if m in ("0", "1", "2"):
        return int(m)
    if m not in MODEL_KINDS:
        raise ValueError(f"unknown model {m!r}; expected lr/fm/mvm")
    return MODEL_KINDS[m]


MAX_CROSSES = 16       # kMaxCrosses, csrc/include/xflow/backend.h
MAX_CROSS_ARITY = 4    # kMaxCrossArity


def check_crosses(crosses) -> list:
    """``crosses`` as a list of tuples of ints, or ValueError: 1..16 crosses of
    2..4 distinct non-negative field ids each, no cross twice (3x7 and 7x3 are
    two crosses: the order is part of the feature)."""
    out = [tuple(int(f) for f in c) for c in crosses]
    if not 1 <= len(out) <= MAX_CROSSES:
        raise ValueError(f"crosses: 1 to {MAX_CROSSES} crosses, got {len(out)}")
    for c in out:
        if not 2 <= len(c) <= MAX_CROSS_ARITY:
            raise ValueError(f"cross {c}: a cross has 2 to {MAX_CROSS_ARITY} fields")
        if min(c) < 0 or max(c) >= 1 << 31:
            raise ValueError(f"cross {c}: field ids are non-negative int32")
        if len(set(c)) != len(c):
            raise ValueError(f"cross {c}: a field is repeated")
    if len(set(out)) != len(out):
        raise ValueError(f"crosses {out}: a cross is given twice")
    return out


def parse_crosses(text: str) -> list:
    """``--cross 3x7,1x2x5`` -> [(3, 7), (1, 2, 5)] (check_crosses' rules; an
    empty string: no crosses)."""
    text = (text or "").strip()
    if not text:
        return []
    try:
        raw = [tuple(int(f) for f in c.split("x")) for c in text.split(",")]
    except ValueError:
        raise ValueError(f"--cross {text!r}: crosses are field ids joined by 'x', separated by "
                         f"commas (3x7,1x2x5)") from None
    return check_crosses(raw)


def format_crosses(crosses) -> str:
    return ",".join("x".join(str(f) for f in c) for c in crosses)


@dataclass
class ModelConfig:
    kind: str = "lr"             # lr | fm | mvm
    v_dim: int = 10
    fm_math: str = "reference"   # reference (fm_worker.cc math) | standard (Rendle FM)
    mvm_math: str = "compat"     # compat (fields [0,max)) | fixed (fields [0,max])
    # standard-math FM forward on the matrix cores (v_mfma_f32_16x16x4_f32,
    # GPU, v_dim <= 8); measured slower than the VALU form, see DESIGN.md 6
    fm_mfma: bool = False

    def native(self) -> dict:
        return {"kind": model_kind(self.kind), "v_dim": int(self.v_dim),
                "fm_math": FM_MATH[self.fm_math], "mvm_math": MVM_MATH[self.mvm_math],
                "fm_mfma": bool(self.fm_mfma)}

    @property
    def params_per_key(self) -> int:
        k = model_kind(self.kind)
        return 1 if k == 0 else (1 + self.v_dim if k == 1 else self.v_dim)


@dataclass
class OptimConfig:
    kind: str = "ftrl"           # ftrl | sgd | frozen (a serving snapshot: read-only)
    alpha: float = 5e-2
    beta: float = 1.0
    lambda1: float = 5e-5
    lambda2: float = 10.0
    lr: float = 1e-3
    sgd_v_init: float = 1e-3
    v_init_scale: float = 1e-2
    seed: int = 0x5EED
    # kind "frozen": the optimiser the snapshot was exported from (ftrl | sgd).
    # It decides what a key that is not in the snapshot reads: latents take
    # that optimiser's init (N(0,1) * v_init_scale under seed, or sgd_v_init)
    frozen_from: str = "ftrl"

    def native(self) -> dict:
        d = dataclasses.asdict(self)
        d["kind"] = OPT_KINDS[self.kind]
        if self.frozen_from not in ("ftrl", "sgd"):
            raise ValueError(f"frozen_from must be ftrl or sgd, got {self.frozen_from!r}")
        d["frozen_from"] = OPT_KINDS[self.frozen_from]
        return d


@dataclass
class EngineConfig:
    table_log2_cap: int = 22
    max_rows: int = 1 << 16
    max_nnz: int = 1 << 22
    max_slices: int = 1
    sum_slices: bool = False      # one push of Σ_s g_s instead of ordered per-slice pushes
    scratch_factor: float = 2.5
    # table capacity management (csrc/include/xflow/engine.h EngineConfig):
    # grow by segment splits (linear hashing) on a schedule that starts when
    # the fullest segments pass grow_start and keeps them <= grow_load, up to
    # 2^max_log2_cap slots (0: 2^31 or what free HBM allows); table_grow=False
    # keeps it fixed and an overflow raises within monitor_lag steps
    table_grow: bool = True
    grow_load: float = 0.8
    grow_start: float = 0.6
    max_log2_cap: int = 0
    monitor_lag: int = 2
    # owner apply of a multi-source sharded step on the GPU: 0 one launch per
    # source (default), 1 one grouped launch (csrc/include/xflow/engine.h)
    owner_group: int = 0
    # several slices on the GPU (LR-FTRL, reference FM): CSR gradients of the
    # touched (key, slice) pairs; False: slice groups of 32 (same pushes)
    csr: bool = True
    # feature admission: a training pull inserts a key only after a counting
    # filter has seen it admit_min_count times (1..255; 1: off, no filter).
    # admit_log2: log2 of the filter's bytes, 0 = min(32, the table's largest
    # log2 capacity + 1).  csrc/include/xflow/engine.h, docs/DESIGN.md §2
    admit_min_count: int = 1
    admit_log2: int = 0
    # LR leader handoff (docs/DESIGN.md §3): the dedup hands its tile leaders
    # to the forward/backward kernel on one-slice field-major batches of a
    # multiple of 1024 rows; False keeps the column-hashing kernel (bit-equal
    # results, the A/B switch)
    lead_handoff: bool = True
    # carry-over rebuilds of the GPU dedup scratch (docs/DESIGN.md §3): a
    # rebuild at an unchanged capacity keeps the batch's own keys; False frees
    # the whole table at every rebuild (bit-equal results, the A/B switch)
    scratch_carry: bool = True
    # one-slice LR / reference FM on the GPU (docs/DESIGN.md §3): the gradient
    # reduction ranks its unique-order outputs from the dedup's stamps, and
    # the compaction writes no slot -> unique map; False keeps the map
    # (bit-equal results, the A/B switch)
    red_rank: bool = True
    # leader-handoff steps (docs/DESIGN.md §3): the forward/backward kernel
    # writes its gradient records sorted by reduction bucket and the sums read
    # them in place, without the reduction's scan and scatter passes; False
    # keeps the passes (bit-equal results, the A/B switch)
    red_local: bool = True
    # bucket-sorted handoff steps with ranked outputs (docs/DESIGN.md §3): the
    # reduction pushes each key's FTRL update itself, so the step has no
    # unique-order gradient array and no apply launch; False keeps both
    # (bit-equal results, the A/B switch)
    red_apply: bool = True
    # delta checkpoints (docs/DESIGN.md §2): mark every key whose state may
    # have changed in a filter of 2^delta_log2 bits indexed by key hash, so
    # that Engine.save_delta writes only those keys.  delta_log2: 10..34,
    # 0 = min(34, the table's largest log2 capacity + 2).  False: no filter,
    # no extra launch.  csrc/include/xflow/engine.h
    delta_track: bool = False
    delta_log2: int = 0
    # a frozen engine (OptimConfig.kind "frozen") scores batches on the GPU
    # with the model's one lookup-and-score launch; False -- or standard FM
    # with fm_mfma -- runs dedup, pull and forward as on a training engine
    # (the A/B switch)
    serve_fused: bool = True
    # ... except for batches of serve_unfused_rows[0] <= rows <
    # serve_unfused_rows[1], which take the three launches (the same bits,
    # tests/test_serving_snapshot.py): profiles/serve.txt has the one-launch
    # kernel ahead up to 32 rows and from 256 rows, 6 % behind at 64 and 128;
    # (0, 0): always one launch
    serve_unfused_rows: tuple = (64, 256)
    # the same window for FM and MVM (serve_unfused_rows is LR's, measured for
    # LR); (0, 0): always one launch.  (-1, -1): the model's own measured
    # window (profiles/serve.txt; csrc/include/xflow/engine.h): reference FM
    # (0, 512), standard FM (0, 0), MVM every size -- its kernel never won
    # and runs only when asked for.  Engine.serve_unfused_rows_latent reports
    # the window in force
    serve_unfused_rows_latent: tuple = (-1, -1)


@dataclass
class TrainConfig:
    train_prefix: str = ""
    test_prefix: str = ""
    epochs: int = 60
    threads: int = 0             # 0 => os.cpu_count() like hardware_concurrency
    train_block_bytes: int = 2 << 20
    block_rows: int = 0          # rows per block of binary (.xfb) shards; 0 => 65536
    fixed_width: bool = True     # blocks whose rows all hold F features train field-major
    resident: bool = False       # keep the first epoch's device batches in HBM for the rest
    # reshuffle every block's used rows on the device each epoch
    # (Engine.shuffle_batch; with resident also the block order): the seed of
    # a block is a pure function of (shuffle_seed, epoch, block, rank), so a
    # resumed run shuffles like an uninterrupted one (docs/DESIGN.md §9)
    shuffle: bool = False
    shuffle_seed: int = 0
    copy_threads: int = 8        # host threads staging a block into pinned memory
    gpu_parse: bool = False      # libffm text shards tokenised on the GPU (data/textstream.py)
    test_block_bytes: int = 0    # 0 => 4 MB LR, 2 MB FM/MVM
    serial_slices: bool = False
    keep_remainder: bool = False
    mvm_predict_compat: bool = False
    init_push: bool = True
    pred_dir: str = "."
    write_pred: bool = True      # the reference's pred_<rank>_<block>.txt (lr_worker.cc:74-77)
    checkpoint_dir: str = ""
    save_every: int = 0          # versioned checkpoint every N epochs (checkpoint.publish)
    resume_dir: str = ""         # versioned checkpoint root: resume from LATEST, save there
    # versioned saves write only the keys touched since the previous version
    # (checkpoint.save delta_base; turns engine.delta_track on); every
    # delta_full_every-th version of a chain is a full one, which bounds the
    # chain's length and the restart time
    save_delta: bool = False
    delta_full_every: int = 8
    # after the last epoch every rank writes its shard's serving snapshot
    # (checkpoint.save_serving: only the keys that differ from an absent key,
    # as resolved fp32 weights) into this directory; "": off
    save_serving: str = ""
    # serving deltas (docs/DESIGN.md §2): at the end of every serving_every-th
    # epoch every rank writes a serving version <save_serving>/epoch-XXXXXX/ and
    # rank 0 points <save_serving>/LATEST at it -- a delta on the previous one
    # (only the keys touched since, deletions included), every
    # serving_full_every-th version of a chain a full snapshot.  Needs
    # save_serving; turns engine.delta_track on.  0: off (one snapshot after
    # the last epoch, in save_serving itself)
    serving_every: int = 0
    serving_full_every: int = 8
    # prune the table (Engine.prune: drop keys whose weights are all exactly
    # zero) at the end of every N-th epoch, 0: never; prune_max_n: with FTRL
    # only keys with every n <= it (negative: no bound)
    prune_every: int = 0
    prune_max_n: float = -1.0
    # also report the grouped AUC (GAUC) and per-group calibration of the
    # predict pass, grouping the test rows by their key of this field id
    # (Engine.eval_grouped); -1: off
    gauc_field: int = -1
    # feature crosses computed on the device (Engine.cross_batch, docs/DESIGN.md
    # §9): tuples of 2..4 field ids; every row gains one key per cross, hashed
    # from its raw keys of those fields (a missing field still gives a key).
    # cross_field_base: cross c enters the model as field id base + c -- MVM
    # needs it (its products run over field ids); -1: LR / FM, which drop the
    # field ids after the cross
    crosses: list = field(default_factory=list)
    cross_field_base: int = -1
    metrics_file: str = ""
    async_p2p: bool = False      # lock-step staleness-k steps, pushes riding the next exchange
    # the asynchronous parameter server (parallel/async_ps.py): per-rank server
    # threads, workers that never lock-step, no collective inside an epoch
    async_ps: bool = False
    staleness: int = 1           # async_ps: own pushes in flight; async_p2p: pushes missed
    model: ModelConfig = field(default_factory=ModelConfig)
    optim: OptimConfig = field(default_factory=OptimConfig)
    engine: EngineConfig = field(default_factory=EngineConfig)

    def resolved_threads(self) -> int:
        if self.threads > 0:
            return self.threads
        # hardware_concurrency (lr_worker.h:40-41); the native trainer's
        # XFLOW_HARDWARE_CONCURRENCY override applies here too
        hc = int(os.environ.get("XFLOW_HARDWARE_CONCURRENCY", "0") or 0)
        return hc if hc > 0 else (os.cpu_count() or 1)

    def resolved_test_block(self) -> int:
        if self.test_block_bytes > 0:
            return self.test_block_bytes
        return (4 << 20) if model_kind(self.model.kind) == 0 else (2 << 20)
