"""Python face of the native Engine: torch-tensor batches, streams, checks.

The native engine (csrc/engine/) owns the HBM hash table and all
per-step buffers; this wrapper only validates tensors and hands device
addresses over.  On a GPU it always runs the gfx950 HIP backend on torch's
current stream (so engine kernels, torch ops and RCCL collectives are ordered
on one queue); on CPU it runs the native C++ backend.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from xflow_amd import native
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig, check_crosses


@dataclass
class Batch:
    """A batch of torch tensors on the engine's device: CSR (row_ptr), or
    fixed-width rows stored row-major or field-major (``field_major``: keys
    and fgid laid out [nnz_per_row][rows], see csrc/include/xflow/types.h)."""

    keys: torch.Tensor                  # int64 [nnz] (u64 bit patterns)
    labels: torch.Tensor                # float32 [rows]
    row_ptr: Optional[torch.Tensor] = None   # int32 [rows+1]; None => fixed nnz/row
    fgid: Optional[torch.Tensor] = None      # int32 [nnz]
    nnz_per_row: int = 0
    slice_rows: int = 0                 # rows per slice (gradient normaliser); 0 => all rows
    field_major: bool = False

    @property
    def rows(self) -> int:
        return int(self.labels.numel())

    @property
    def nnz(self) -> int:
        return int(self.keys.numel())

    def view(self):
        n = native.load()
        v = n.BatchView()
        v.keys = self.keys.data_ptr()
        v.labels = self.labels.data_ptr()
        v.row_ptr = self.row_ptr.data_ptr() if self.row_ptr is not None else 0
        v.fgid = self.fgid.data_ptr() if self.fgid is not None else 0
        v.rows = self.rows
        v.nnz = self.nnz
        v.nnz_per_row = self.nnz_per_row
        v.slice_rows = self.slice_rows
        v.col_stride = self.rows if self.field_major else 0
        return v

    def check(self, device: torch.device, compact_ok: bool = False) -> None:
        """compact_ok: the keys may also be compact u32 keys in an int32 tensor
        (what Engine.shuffle_batch and to_field_major widen)."""
        for name, t, dt in (("keys", self.keys, torch.int64), ("labels", self.labels, torch.float32),
                            ("row_ptr", self.row_ptr, torch.int32), ("fgid", self.fgid, torch.int32)):
            if t is None:
                continue
            if name == "keys" and compact_ok and t.dtype == torch.int32:
                dt = torch.int32
            if t.dtype != dt:
                raise TypeError(f"batch.{name} must be {dt}, got {t.dtype}")
            if t.device != device:
                raise ValueError(f"batch.{name} on {t.device}, engine on {device}")
            if not t.is_contiguous():
                raise ValueError(f"batch.{name} must be contiguous")
        if self.row_ptr is None:
            if self.nnz_per_row <= 0 or self.nnz != self.rows * self.nnz_per_row:
                raise ValueError("fixed-width batch needs nnz == rows * nnz_per_row")
        elif self.row_ptr.numel() != self.rows + 1:
            raise ValueError("row_ptr must have rows+1 entries")
        if self.field_major and self.row_ptr is not None:
            raise ValueError("field-major batches are fixed-width (no row_ptr)")

    def to_field_major(self, engine: "Engine | None" = None) -> "Batch":
        """The same fixed-width batch stored field-major.  With an engine, its
        backend transposes (HIP: an LDS-tiled kernel on the engine's stream,
        csrc/hip/kernels_layout.hip); otherwise torch does."""
        if self.field_major:
            return self
        if self.row_ptr is not None:
            raise ValueError("only fixed-width batches have a field-major form")
        F = self.nnz_per_row
        if engine is not None and F <= 64:
            def t(x, widen=False):
                if x is None:
                    return None
                y = (torch.empty(x.numel(), dtype=torch.int64, device=x.device) if widen
                     else torch.empty_like(x))
                engine._sync_stream()
                engine.native.field_major(x.data_ptr(), y.data_ptr(), self.rows, F,
                                          x.element_size(), widen)
                return y
        else:
            def t(x, widen=False):
                if x is None:
                    return None
                y = x.view(self.rows, F).t().contiguous().view(-1)
                return widen_keys(y) if widen else y
        # compact (u32) keys of an .xfb shard are widened in the same pass
        return Batch(keys=t(self.keys, self.keys.dtype == torch.int32), labels=self.labels,
                     fgid=t(self.fgid), nnz_per_row=F, slice_rows=self.slice_rows,
                     field_major=True)


def widen_keys(keys: torch.Tensor) -> torch.Tensor:
    """Engine keys (int64 u64 bit patterns) from compact u32 keys held in an
    int32 tensor (data/binfmt.py compact shards); int64 keys pass through."""
    if keys.dtype == torch.int64:
        return keys
    if keys.dtype != torch.int32:
        raise TypeError(f"keys must be int64 or compact int32, got {keys.dtype}")
    return keys.to(torch.int64) & 0xFFFFFFFF


def shuffle_permutation(n: int, seed: int) -> np.ndarray:
    """The row-shuffle permutation of ``n`` rows under ``seed`` (int64 [n]):
    element i is the source row of destination row i.  A keyed bijection of
    [0, n) (shuffle_index, csrc/include/xflow/common.h) computed by the
    native host function both backends share; the seed is taken modulo 2^64."""
    return native.load().shuffle_permutation(int(n), int(seed) & 0xFFFFFFFFFFFFFFFF)


CROSS_SALT = 0xC3A5C85C97CB3127
_M64 = (1 << 64) - 1


def _fmix64(h: int) -> int:
    h &= _M64
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & _M64
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & _M64
    h ^= h >> 33
    return h


def cross_keys(fields, ops) -> np.ndarray:
    """The definition of a cross key (cross_key, csrc/include/xflow/common.h)
    in Python ints: ``fields`` the m crossed field ids in order, ``ops`` a
    [rows, m] array (or one row) of the rows' raw u64 keys of those fields,
    all ones (2^64 - 1) where a row has none -- a missing operand is hashed,
    not skipped.  Returns uint64 [rows]; the all-ones key is remapped to
    2^64 - 2 like every key (sanitize_key)."""
    fields = [int(f) for f in fields]
    if isinstance(ops, np.ndarray):  # (int64 bit patterns, as batches hold them, are u64)
        a = ops if ops.dtype == np.uint64 else ops.astype(np.int64).view(np.uint64)
    else:
        flat = np.array(ops, dtype=object).reshape(-1)
        a = np.array([int(v) & _M64 for v in flat], dtype=np.uint64)
    a = a.reshape(-1, len(fields))
    out = np.empty(len(a), dtype=np.uint64)
    h0 = _fmix64(CROSS_SALT + len(fields))
    for r, row in enumerate(a.tolist()):
        h = h0
        for f, v in zip(fields, row):
            h = _fmix64(h ^ (f & 0xFFFFFFFF))
            h = _fmix64(h ^ v)
        out[r] = sanitize_key(h)
    return out


def sanitize_key(k: int) -> int:
    """The all-ones key is the tables' empty-slot mark: it is stored as
    2^64 - 2 (sanitize_key, csrc/include/xflow/common.h)."""
    return _M64 - 1 if k == _M64 else k


def _device_index(device: torch.device) -> int:
    if device.type == "cpu":
        return -1
    if device.type != "cuda":
        raise ValueError(f"unsupported device {device}")
    return device.index if device.index is not None else torch.cuda.current_device()


class Engine:
    """One rank's sparse trainer state (hash-table shard + worker buffers)."""

    def __init__(self, model: ModelConfig | None = None, optim: OptimConfig | None = None,
                 engine: EngineConfig | None = None, device: str | torch.device = "cpu"):
        self.model = model or ModelConfig()
        self.optim = optim or OptimConfig()
        self.cfg = engine or EngineConfig()
        self.device = torch.device(device)
        if self.device.type == "cuda":
            native.require_hip()
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
        n = native.load()
        self._e = n.Engine(self.model.native(), self.optim.native(),
                           table_log2_cap=self.cfg.table_log2_cap, max_rows=self.cfg.max_rows,
                           max_nnz=self.cfg.max_nnz, max_slices=self.cfg.max_slices,
                           sum_slices=self.cfg.sum_slices, scratch_factor=self.cfg.scratch_factor,
                           device=_device_index(self.device), table_grow=self.cfg.table_grow,
                           grow_load=self.cfg.grow_load, max_log2_cap=self.cfg.max_log2_cap,
                           monitor_lag=self.cfg.monitor_lag, owner_group=self.cfg.owner_group,
                           grow_start=self.cfg.grow_start, csr=self.cfg.csr,
                           admit_min_count=self.cfg.admit_min_count,
                           admit_log2=self.cfg.admit_log2,
                           lead_handoff=self.cfg.lead_handoff,
                           scratch_carry=self.cfg.scratch_carry,
                           red_rank=self.cfg.red_rank,
                           red_local=self.cfg.red_local,
                           red_apply=self.cfg.red_apply,
                           delta_track=self.cfg.delta_track,
                           delta_log2=self.cfg.delta_log2,
                           serve_fused=self.cfg.serve_fused,
                           serve_unfused_lo=int(self.cfg.serve_unfused_rows[0]),
                           serve_unfused_hi=int(self.cfg.serve_unfused_rows[1]),
                           serve_unfused_latent_lo=int(self.cfg.serve_unfused_rows_latent[0]),
                           serve_unfused_latent_hi=int(self.cfg.serve_unfused_rows_latent[1]))
        if self.is_gpu != (self.device.type == "cuda"):
            raise RuntimeError("native engine backend does not match the requested device")
        # delta_clear() calls so far: a serving or checkpoint delta is only
        # good on a base the filter was last cleared at (checkpoint.py)
        self.delta_clears = 0

    # ---- properties -------------------------------------------------------
    @property
    def native(self):
        return self._e

    @property
    def is_gpu(self) -> bool:
        return bool(self._e.is_gpu)

    @property
    def backend_name(self) -> str:
        return self._e.backend_name

    @property
    def pstride(self) -> int:
        return int(self._e.pstride)

    @property
    def grad_width(self) -> int:
        """Floats per (key, slice) in the multi-rank gradient exchange."""
        return int(self._e.grad_width)

    @property
    def value_width(self) -> int:
        """Floats per pulled value row (pull outputs / values exchange): pstride,
        or 4 for reference-math FM on the GPU ((w, sum v, sum v^2, 0))."""
        return int(self._e.value_width)

    @property
    def params_per_key(self) -> int:
        return int(self._e.P)

    def _sync_stream(self) -> None:
        if self.is_gpu:
            self._e.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- single rank --------------------------------------------------------
    def train_step(self, batch: Batch) -> None:
        batch.check(self.device)
        self._sync_stream()
        self._e.train_step(batch.view())

    def eval_step(self, batch: Batch, pctr: torch.Tensor | None = None) -> torch.Tensor:
        batch.check(self.device)
        if pctr is None:
            pctr = torch.empty(batch.rows, dtype=torch.float32, device=self.device)
        self._sync_stream()
        self._e.eval_step(batch.view(), pctr.data_ptr())
        return pctr

    def train_view(self, view) -> None:
        """Train on a native BatchView (e.g. engine-staged synthetic batch)."""
        self._sync_stream()
        self._e.train_step(view)

    def synth_batch(self, rows: int, vocab, zipf_s, hash_space: int, seed: int, step: int,
                    planted_scale: float = 0.3, planted_bias: float = -1.2, slice_rows: int = 0,
                    out: Batch | None = None, field_major: bool = False):
        """Generate a synthetic batch on the engine's device.

        Without ``out`` the batch lives in engine-owned staging memory and a
        native BatchView is returned; with ``out`` (a Batch of preallocated
        tensors) the generator writes into those tensors and ``out`` is returned.
        ``field_major`` stores keys/fgid [field][row] (same rows, same values).
        """
        self._sync_stream()
        kw = {}
        if out is not None:
            kw = dict(keys=out.keys.data_ptr(), labels=out.labels.data_ptr(),
                      fgid=out.fgid.data_ptr() if out.fgid is not None else 0)
        v = self._e.synth_batch(int(rows), [int(x) for x in vocab], [float(s) for s in zipf_s],
                                int(hash_space), int(seed), int(step), float(planted_scale),
                                float(planted_bias), int(slice_rows), field_major=bool(field_major),
                                **kw)
        if out is None:
            return v
        out.nnz_per_row = len(vocab)
        out.slice_rows = int(slice_rows)
        out.field_major = bool(field_major)
        return out

    def push(self, keys, grads) -> None:
        self._e.push_host(np.asarray(keys, dtype=np.uint64),
                          np.asarray(grads, dtype=np.float32).reshape(-1))

    def prefill(self, n: int, seed: int = 0x5eed) -> None:
        """Insert n synthetic keys that no batch touches (bit 62 set): a table
        at the occupancy a long run reaches (untimed benchmark setup)."""
        self._sync_stream()
        self._e.prefill(int(n), int(seed))

    # ---- feature admission (EngineConfig.admit_min_count) -------------------
    def admit_bytes(self) -> int:
        """Bytes of the admission filter (0: admission off)."""
        return int(self._e.admit_bytes)

    @property
    def admit_log2(self) -> int:
        """log2 of the filter's bytes as allocated (0: admission off)."""
        return int(self._e.admit_log2)

    def admit_counts(self, keys) -> np.ndarray:
        """The filter's estimate of each key's sightings, min of its two
        counters (uint8, saturating at 255; zeros with admission off).  A
        small synchronising call for tests and diagnostics."""
        self._sync_stream()
        return self._e.admit_counts(np.ascontiguousarray(keys, dtype=np.uint64))

    def admit_export(self) -> np.ndarray:
        """A host copy of the whole filter (uint8 [admit_bytes()])."""
        self._sync_stream()
        return self._e.admit_export()

    def admit_import(self, counters: np.ndarray) -> None:
        self._sync_stream()
        self._e.admit_import(np.ascontiguousarray(counters, dtype=np.uint8))

    # ---- delta checkpoints (EngineConfig.delta_track) ------------------------
    def delta_stats(self) -> dict:
        """{log2, bits_set, needs_full}: log2 of the touched-key filter's bits
        (0: tracking off), its popcount (synchronises), and whether the table
        changed in a way a delta cannot carry (a prune that dropped a key,
        import_table / load, prefill) so that the next save must be full."""
        self._sync_stream()
        d = self._e.delta_stats()
        return {"log2": int(d["log2"]), "bits_set": int(d["bits_set"]),
                "needs_full": bool(d["needs_full"])}

    @property
    def delta_log2(self) -> int:
        """log2 of the touched-key filter's bits as allocated (0: tracking off)."""
        return int(self._e.delta_log2)

    @property
    def delta_needs_full(self) -> bool:
        """delta_stats()["needs_full"] without the popcount pass (no sync)."""
        return bool(self._e.delta_needs_full)

    def delta_count(self) -> int:
        """Keys of the table whose filter bit is set (a count pass; syncs)."""
        self._sync_stream()
        return int(self._e.delta_count())

    def delta_export(self):
        """(keys u64 [n], words u32 [n * state_words]) of the table's keys
        whose filter bit is set: every key touched since the last
        delta_clear(), plus the untouched keys that share a bit with one."""
        self._sync_stream()
        return self._e.delta_export()

    def save_delta(self, path: str) -> None:
        """delta_export() as a shard file (Engine.save's format, header word
        7 = 1)."""
        self._sync_stream()
        self._e.save_delta(path)

    def delta_clear(self) -> None:
        """Zero the filter and reset needs_full (no-op with tracking off)."""
        self._sync_stream()
        self._e.delta_clear()
        self.delta_clears += 1

    def server_slots(self, buf: int = 0) -> np.ndarray:
        """Table slots the last s_pull into server buffer ``buf`` recorded
        (0xFFFFFFFF: no slot); synchronising, for tests."""
        self._sync_stream()
        return self._e.server_slots(int(buf))

    def pull(self, keys) -> np.ndarray:
        k = np.asarray(keys, dtype=np.uint64)
        return self._e.pull_host(k).reshape(len(k), self.params_per_key)

    # ---- multi-rank phases (driven by parallel.sparse_a2a) ----------------------
    # wb: worker buffer set (0/1) holding a prepared batch's dedup state, so the
    # next batch can be prepared while the current one is still in flight.
    def w_prepare(self, batch: Batch, world: int, counts: torch.Tensor, send_keys: torch.Tensor,
                  wb: int = 0, seq: int = -1):
        """seq >= 0 (world > 1): counts are written encoded with the prepare
        sequence number (csrc/include/xflow/backend.h encode_count)."""
        batch.check(self.device)
        self._sync_stream()
        self._e.w_prepare(batch.view(), world, counts.data_ptr(), send_keys.data_ptr(), int(wb),
                          int(seq))

    def s_pull(self, recv_keys: torch.Tensor, n: int, out_vals: torch.Tensor,
               insert: bool = True, buf: int = 0, offsets=None, keep_weights: bool = False) -> None:
        """Owner pull of n received keys into out_vals ([n, value_width]);
        ``offsets`` (world+1 source boundaries) lets the GPU backend group the
        sources for a one-launch apply; ``keep_weights`` keeps the pulled
        per-parameter weights for an apply after other updates (async step)."""
        self._sync_stream()
        self._e.s_pull(recv_keys.data_ptr(), int(n), out_vals.data_ptr(), insert, int(buf),
                       [int(o) for o in offsets] if offsets is not None else [],
                       bool(keep_weights))

    def w_forward(self, batch: Batch, pulled: torch.Tensor, n_send: int,
                  pctr: torch.Tensor | None, wb: int = 0) -> None:
        self._sync_stream()
        self._e.w_forward(batch.view(), pulled.data_ptr(), int(n_send),
                          pctr.data_ptr() if pctr is not None else 0, int(wb))

    def w_forward_backward(self, batch: Batch, pulled: torch.Tensor, n_send: int,
                           grads_out: torch.Tensor, masks_out: torch.Tensor | None,
                           S: int = 0, wb: int = 0, group: int = 0) -> None:
        """S > SLICE_GROUP: slice group ``group`` of the step only (its rows;
        grads_out holds group_slices(S, group) slices per key)."""
        self._sync_stream()
        self._e.w_forward_backward(batch.view(), pulled.data_ptr(), int(n_send),
                                   grads_out.data_ptr(),
                                   masks_out.data_ptr() if masks_out is not None else 0, int(S),
                                   int(wb), int(group))

    def s_apply(self, recv_keys: torch.Tensor, recv_grads: torch.Tensor,
                recv_masks: torch.Tensor | None, offsets, S: int, buf: int = 0) -> None:
        self._sync_stream()
        self._e.s_apply(recv_keys.data_ptr(), recv_grads.data_ptr(),
                        recv_masks.data_ptr() if recv_masks is not None else 0,
                        [int(o) for o in offsets], int(S), int(buf))

    def w_finish(self) -> None:
        self._sync_stream()
        self._e.w_finish()

    # ---- stats / checkpoint -------------------------------------------------
    def slices_of(self, batch: Batch) -> int:
        return int(self._e.slices_of(batch.view()))

    @staticmethod
    def slice_groups(S: int) -> list[int]:
        """Slices of each slice group of an S-slice step (Engine::slice_groups:
        more than 32 slices run in groups of 32, each group >= 2 slices)."""
        from xflow_amd import native

        n = native.load()
        return [int(n.Engine.group_slices(int(S), g)) for g in range(int(n.Engine.slice_groups(int(S))))]

    def read_stats(self, reset: bool = False, which: int = 0) -> dict:
        self._sync_stream()
        return self._e.read_stats(reset, which)

    def table_size(self) -> int:
        self._sync_stream()
        return int(self._e.table_size())

    @property
    def layout(self) -> dict:
        """Table slot layout (model kind, params per key, optimizer, words per slot)."""
        return dict(self._e.layout)

    @property
    def table_capacity(self) -> int:
        """Slots of this rank's table shard (grows, see EngineConfig.table_grow)."""
        return int(self._e.table_capacity)

    @property
    def table_growths(self) -> int:
        """Times the table grew (each: one or more segment splits)."""
        return int(self._e.table_growths)

    @property
    def csr_steps(self) -> int:
        """Steps of several slices that ran on the CSR path (one reduction and
        one apply of only the touched (key, slice) pairs, Engine::train_step_csr)."""
        return int(self._e.csr_steps)

    @property
    def table_splits(self) -> int:
        """Segments split so far (each added one segment of memory)."""
        return int(self._e.table_splits)

    @property
    def table_geometry(self) -> dict:
        """{seg_log2, level, split, segments} (TableView, csrc/include/xflow/backend.h)."""
        g, lv, sp, ns = self._e.table_geometry
        return {"seg_log2": int(g), "level": int(lv), "split": int(sp), "segments": int(ns)}

    @property
    def table_committed(self) -> int:
        """Device bytes committed to the table's address range."""
        return int(self._e.table_committed)

    @property
    def grow_seconds(self) -> float:
        """Host seconds spent in growth calls (memory mapping + split launches)."""
        return float(self._e.grow_seconds)

    @property
    def monitor_waits(self) -> int:
        """Host waits of the capacity monitor (bounded run-ahead, exact-size reads)."""
        return int(self._e.monitor_waits)

    def parse_text(self, text: torch.Tensor, n: int, out: dict, row_mod: int = 1):
        """libffm bytes text[:n] (uint8, engine device, 16-byte aligned,
        allocated >= n + 32 bytes) ->
        out["keys"/"fgid"/"row_ptr"/"labels"] on the device (kernels_parse.hip;
        reader.cpp's rules).  Returns (rows, occurrences, shortest row,
        longest row, occurrences of the first rows - rows % row_mod rows)."""
        self._sync_stream()
        if text.numel() < n + 32 and text.is_cuda:
            raise ValueError("parse_text: the text tensor needs >= n + 32 bytes")
        return tuple(int(x) for x in self._e.parse_text(
            text.data_ptr(), int(n), out["keys"].data_ptr(), out["fgid"].data_ptr(),
            out["row_ptr"].data_ptr(), out["labels"].data_ptr(), int(out["labels"].numel()),
            int(out["keys"].numel()), int(row_mod)))

    def unpack_packed(self, block: torch.Tensor, rows: int, shard, slice_rows: int = 0,
                      with_fgid: bool = False, used: int = -1) -> Batch:
        """A packed (version 3) .xfb block -- its raw bytes as a uint8 tensor
        on this engine's device -- as a field-major Batch (keys expanded from
        the per-field codes / dictionaries on the device, Backend::unpack_block).
        used >= 0: only the first `used` rows (the slicing rule's remainder drop)."""
        if block.device != self.device or block.dtype != torch.uint8:
            raise ValueError("unpack_packed: uint8 block bytes on the engine's device")
        F = shard.F
        dd = shard.device_dicts(self.device)
        keys = torch.empty(F * rows, dtype=torch.int64, device=self.device)
        labels = torch.empty(rows, dtype=torch.float32, device=self.device)
        fgid = torch.empty(F * rows, dtype=torch.int32, device=self.device) if with_fgid else None
        cols = shard.columns(rows)
        if block.numel() < cols[-1] + rows * shard.widths[-1]:
            raise ValueError("unpack_packed: block shorter than its columns")
        self._sync_stream()
        self._e.unpack_block(block.data_ptr(), int(rows), list(shard.widths), [int(c) for c in cols],
                             [dd[f] for f in range(F)], list(shard.fgid_cols), keys.data_ptr(),
                             labels.data_ptr(), fgid.data_ptr() if fgid is not None else 0)
        if 0 <= used < rows:  # (field-major: each field's first `used` rows)
            keys = keys.view(F, rows)[:, :used].contiguous().view(-1)
            labels = labels[:used]
            if fgid is not None:
                fgid = fgid.view(F, rows)[:, :used].contiguous().view(-1)
        return Batch(keys=keys, labels=labels, fgid=fgid, nnz_per_row=F, slice_rows=slice_rows,
                     field_major=True)

    def count_records(self, on: bool = True) -> None:
        """Count the gradient-reduction records the producers write."""
        self._e.count_records(bool(on))

    def take_records(self) -> int:
        """Records written since the last call (-1: never counted)."""
        self._sync_stream()
        return int(self._e.take_records())

    @property
    def monitor_wait_seconds(self) -> float:
        """Host seconds blocked by the monitor's run-ahead bound."""
        return float(self._e.monitor_wait_seconds)

    def grow_table(self, log2_cap: int) -> None:
        """Grow the table to >= 2^log2_cap slots now by segment splits (normally
        automatic)."""
        self._sync_stream()
        self._e.grow_table(int(log2_cap))

    def prune(self, max_n: float | None = None) -> int:
        """Drop every key whose weights are all exactly zero -- with FTRL and
        max_n given, only those with every n <= max_n (0: keys never pushed a
        non-zero gradient) -- and re-pack the keys that stay; returns the number
        dropped.  Call it between steps.  For LR a zero-weight key predicts
        like an absent one, so no prediction changes; a dropped FM / MVM key
        reads as never seen again (its latents take the lazy init).  Capacity
        is not given back: the load falls and growth comes later."""
        self._sync_stream()
        return int(self._e.prune(-1.0 if max_n is None else float(max_n)))

    @property
    def pruned_keys(self) -> int:
        """Keys dropped by prune() so far."""
        return int(self._e.pruned_keys)

    def end_step(self) -> None:
        """Queue the step's capacity snapshot (the sharded steps call it via
        w_finish; raises if an earlier step overflowed)."""
        self._sync_stream()
        self._e.end_step()

    def n_unique(self) -> int:
        self._sync_stream()
        return int(self._e.n_unique())

    def scratch_capacity(self) -> int:
        """Active dedup scratch capacity (device-adaptive on the GPU)."""
        self._sync_stream()
        return int(self._e.scratch_capacity())

    def batch_capacity(self) -> int:
        """Scratch slots the last batch's compaction and gradient reduction
        covered: the capacity it was deduplicated with, or the whole
        allocation when the batch spilled past it.  Synchronises."""
        self._sync_stream()
        return int(self._e.batch_capacity())

    def scratch_stats(self) -> dict:
        """The dedup scratch's counters: ``capacity`` (active), ``occupancy``
        (the rebuild counter: occupied slots with scratch_carry, else the keys
        claimed since the last rebuild), ``rebuilds`` decided by the compaction
        so far and the keys ``carried`` by the last of them (0: a full clear).
        Synchronises: for tests and tools.  The CPU backend reports its fixed
        capacity and its claims, and no rebuilds."""
        self._sync_stream()
        return {k: int(v) for k, v in self._e.scratch_stats().items()}

    def overflowed(self) -> bool:
        self._sync_stream()
        return bool(self._e.overflowed())

    def nonzero_weights(self) -> int:
        """Exactly non-zero (key, param) weights in this shard (L1 sparsity)."""
        self._sync_stream()
        return int(self._e.nonzero_weights())

    def download_small(self, dst: torch.Tensor, src: torch.Tensor) -> None:
        """Queue a copy of a small device tensor into pinned host memory on the
        current stream without the copy engine (read it after an event
        recorded behind this call)."""
        if self.is_gpu and not dst.is_pinned():
            raise ValueError("download_small: dst must be pinned host memory")
        if dst.numel() * dst.element_size() < src.numel() * src.element_size():
            raise ValueError("download_small: dst too small")
        self._sync_stream()
        self._e.download_small(dst.data_ptr(), src.contiguous().data_ptr(),
                               src.numel() * src.element_size())

    def eval_metrics(self, pctr: torch.Tensor, labels: torch.Tensor) -> dict:
        """AUC / logloss of predictions on this engine's device, computed there
        (GPU: radix sort + rank sums; only scalars come back).  Returns the
        reference's printed line (base.h:84-110) with auc / logloss_printed /
        ln_logloss / n / tp, and the exact sums area / log2_sum / ln_sum.  The
        predictions are ranked by the bits of ``p > 0 ? p : +0`` (descending,
        stable): NaN, zeros and negative values tie and rank last."""
        if pctr.device != self.device or labels.device != self.device:
            raise ValueError("eval_metrics: tensors must be on the engine's device")
        p = pctr.contiguous().float()
        y = labels.contiguous().float()
        if p.numel() != y.numel():
            raise ValueError("eval_metrics: pctr and labels differ in length")
        self._sync_stream()
        return dict(self._e.eval_metrics(p.data_ptr(), y.data_ptr(), int(p.numel())))

    def eval_grouped(self, pctr: torch.Tensor, labels: torch.Tensor, groups: torch.Tensor,
                     per_group: bool = False) -> dict:
        """Grouped AUC (GAUC) and per-group calibration of predictions on this
        engine's device, computed there (GroupedEval, csrc/include/xflow/backend.h).
        ``groups`` is int64 holding u64 bit patterns, like batch keys; a row
        whose group is all ones (-1) belongs to no group.  Returns the exact
        counts n / n_nogroup / groups / groups_used / rows_used, the sums
        gauc_num / cal_abs, and gauc (None when no group has both a positive
        and a negative row), coverage and group_cal_error derived from them.
        ``per_group``: also ``per_group`` = numpy arrays key / n / pos / area2 /
        sump in ascending key order."""
        if pctr.device != self.device or labels.device != self.device or \
                groups.device != self.device:
            raise ValueError("eval_grouped: tensors must be on the engine's device")
        if groups.dtype != torch.int64:
            raise TypeError(f"eval_grouped: groups must be int64, got {groups.dtype}")
        p = pctr.contiguous().float()
        y = labels.contiguous().float()
        g = groups.contiguous()
        if p.numel() != y.numel() or p.numel() != g.numel():
            raise ValueError("eval_grouped: pctr, labels and groups differ in length")
        self._sync_stream()
        r = dict(self._e.eval_grouped(p.data_ptr(), y.data_ptr(), g.data_ptr(), int(p.numel()),
                                      bool(per_group)))
        in_groups = r["n"] - r["n_nogroup"]
        r["gauc"] = r["gauc_num"] / r["rows_used"] if r["groups_used"] > 0 else None
        r["coverage"] = r["rows_used"] / r["n"] if r["n"] > 0 else 0.0
        r["group_cal_error"] = r["cal_abs"] / in_groups if in_groups > 0 else 0.0
        if per_group:
            r["per_group"] = dict(r["per_group"])
        return r

    def row_group_keys(self, batch: Batch, field: int) -> torch.Tensor:
        """The key each row of ``batch`` is grouped by for ``field`` (int64
        holding u64 bit patterns, on the device): with fgid, the key of the
        row's first occurrence of that field id; without fgid, on a fixed-width
        batch, occurrence ``field`` of the row; all ones (no group) when the
        row has none.  A CSR batch without fgid is an error."""
        batch.check(self.device)
        if batch.fgid is None and batch.row_ptr is not None:
            raise ValueError("row_group_keys: a CSR batch needs its field ids (fgid)")
        out = torch.empty(batch.rows, dtype=torch.int64, device=self.device)
        self._sync_stream()
        self._e.row_group_keys(batch.view(), int(field), out.data_ptr())
        return out

    def shuffle_batch(self, batch: Batch, seed: int, field_major: bool | None = None) -> Batch:
        """``batch`` with its rows permuted on the device, as new tensors: row
        i of the result is row ``shuffle_permutation(rows, seed)[i]`` of
        ``batch`` (keys, field ids, label; a row's entries keep their order).
        The source is CSR or fixed-width row-major -- a field-major one is
        refused: its rows are not contiguous -- and is left unchanged.  A
        fixed-width result is field-major unless ``field_major`` is False (the
        fused shuffle + transpose: the one pass the step's layout costs
        anyway); a CSR batch stays CSR.  Compact u32 keys (int32) come out as
        u64.  Above 64 fields torch gathers, as in ``to_field_major``."""
        batch.check(self.device, compact_ok=True)
        fixed = batch.row_ptr is None
        if batch.field_major:
            raise ValueError("shuffle_batch: a field-major source (row-major or CSR only)")
        fm = fixed if field_major is None else bool(field_major)
        if fm and not fixed:
            raise ValueError("shuffle_batch: only fixed-width batches have a field-major form")
        if batch.rows > self.cfg.max_rows or batch.nnz > self.cfg.max_nnz:
            raise ValueError("shuffle_batch: the batch exceeds max_rows / max_nnz")
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        rows, F, dev = batch.rows, batch.nnz_per_row, self.device
        if not fixed and batch.keys.dtype == torch.int32:
            batch = Batch(keys=widen_keys(batch.keys), labels=batch.labels, row_ptr=batch.row_ptr,
                          fgid=batch.fgid, slice_rows=batch.slice_rows)
        if fixed and F > 64:
            perm = torch.from_numpy(shuffle_permutation(rows, seed)).to(dev)

            def g(x):
                if x is None:
                    return None
                y = x.view(rows, F)[perm]
                return (y.t() if fm else y).contiguous().view(-1)
            return Batch(keys=g(widen_keys(batch.keys)), labels=batch.labels[perm],
                         fgid=g(batch.fgid), nnz_per_row=F, slice_rows=batch.slice_rows,
                         field_major=fm)
        keys = torch.empty(batch.nnz, dtype=torch.int64, device=dev)
        labels = torch.empty(rows, dtype=torch.float32, device=dev)
        fgid = torch.empty_like(batch.fgid) if batch.fgid is not None else None
        row_ptr = None if fixed else torch.empty(rows + 1, dtype=torch.int32, device=dev)
        self._sync_stream()
        self._e.shuffle_rows(batch.view(), seed, keys.data_ptr(),
                             fgid.data_ptr() if fgid is not None else 0, labels.data_ptr(),
                             row_ptr.data_ptr() if row_ptr is not None else 0, fm,
                             batch.keys.element_size())
        return Batch(keys=keys, labels=labels, row_ptr=row_ptr, fgid=fgid,
                     nnz_per_row=batch.nnz_per_row, slice_rows=batch.slice_rows, field_major=fm)

    def cross_batch(self, batch: Batch, crosses, seed: int | None = None,
                    field_major: bool | None = None, fgid_base: int | None = None) -> Batch:
        """``batch`` with one cross key per cross appended to every row, as new
        tensors, computed on the device (Backend::cross_rows,
        csrc/hip/kernels_cross.hip).  ``crosses``: tuples of 2..4 field ids
        (check_crosses).  Cross c of a row is ``cross_keys(crosses[c], ops)``
        with ops the row's raw keys of those fields by the rule of
        ``row_group_keys`` -- with fgid the first occurrence of the field id,
        without it (fixed width) the occurrence's index, all ones when the row
        has none: a missing field still gives a key.  A fixed-width batch of
        width F comes out with width F + C (at most 64 from a row-major
        source), field-major unless ``field_major`` is False; a field-major
        source (no fgid) stays field-major; a CSR batch (needs fgid) stays CSR.
        ``seed``: the rows are also permuted as ``shuffle_batch(batch, seed)``
        does, in the same pass for fixed-width batches.  The result carries
        field ids only when ``fgid_base`` is given (the batch needs them
        then): cross c gets ``fgid_base + c``.  Compact u32 keys come out as
        u64; labels and slice_rows carry over."""
        batch.check(self.device, compact_ok=True)
        X = check_crosses(crosses)
        C = len(X)
        fixed = batch.row_ptr is None
        fm = fixed if field_major is None else bool(field_major)
        if fm and not fixed:
            raise ValueError("cross_batch: only fixed-width batches have a field-major form")
        if fgid_base is not None and batch.fgid is None:
            raise ValueError("cross_batch: fgid_base needs a batch with field ids")
        if not fixed and batch.fgid is None:
            raise ValueError("cross_batch: a CSR batch needs its field ids (fgid)")
        rows, F, dev = batch.rows, batch.nnz_per_row, self.device
        if rows > self.cfg.max_rows or batch.nnz + C * rows > self.cfg.max_nnz:
            raise ValueError("cross_batch: the crossed batch exceeds max_rows / max_nnz")
        if batch.field_major:
            if batch.fgid is not None or seed is not None or not fm:
                raise ValueError("cross_batch: a field-major source has no fgid, takes no seed "
                                 "and stays field-major")
        elif fixed and F + C > 64:
            raise ValueError(f"cross_batch: fields + crosses exceed 64 ({F} + {C})")
        if seed is not None:
            seed = int(seed) & 0xFFFFFFFFFFFFFFFF
            if not fixed:  # CSR: the shuffle's three launches, then the cross
                batch, seed = self.shuffle_batch(batch, seed), None
        if not fixed and batch.keys.dtype == torch.int32:
            batch = Batch(keys=widen_keys(batch.keys), labels=batch.labels, row_ptr=batch.row_ptr,
                          fgid=batch.fgid, slice_rows=batch.slice_rows)
        keys = torch.empty(batch.nnz + C * rows, dtype=torch.int64, device=dev)
        labels = torch.empty(rows, dtype=torch.float32, device=dev)
        fgid = (torch.empty(batch.nnz + C * rows, dtype=torch.int32, device=dev)
                if fgid_base is not None else None)
        row_ptr = None if fixed else torch.empty(rows + 1, dtype=torch.int32, device=dev)
        self._sync_stream()
        self._e.cross_rows(batch.view(), [list(c) for c in X],
                           int(fgid_base) if fgid_base is not None else 0, seed, keys.data_ptr(),
                           fgid.data_ptr() if fgid is not None else 0, labels.data_ptr(),
                           row_ptr.data_ptr() if row_ptr is not None else 0, fm,
                           batch.keys.element_size())
        return Batch(keys=keys, labels=labels, row_ptr=row_ptr, fgid=fgid,
                     nnz_per_row=F + C if fixed else 0, slice_rows=batch.slice_rows,
                     field_major=fm)

    def export_table(self):
        self._sync_stream()
        return self._e.export_table()

    def import_table(self, keys: np.ndarray, words: np.ndarray) -> None:
        self._sync_stream()
        self._e.import_table(np.ascontiguousarray(keys, dtype=np.uint64),
                             np.ascontiguousarray(words, dtype=np.uint32))

    @property
    def state_words(self) -> int:
        return int(self._e.state_words)

    # ---- serving snapshots (docs/DESIGN.md §2) --------------------------------
    @property
    def frozen(self) -> bool:
        """This engine holds a serving snapshot (OptimConfig.kind "frozen"):
        read-only; training, prune and the training checkpoints raise."""
        return bool(self._e.frozen)

    @property
    def serve_fused(self) -> bool:
        """The model's one-launch kernel is available and switched on
        (EngineConfig.serve_fused on a frozen engine on the GPU; not standard
        FM with fm_mfma).  Which batch sizes eval_step gives it is the
        window's business: serve_unfused_rows for LR, serve_unfused_rows_latent
        (this engine's property: the window in force) for FM and MVM -- by
        default MVM never takes the kernel and reference FM from 512 rows."""
        return bool(self._e.serve_fused)

    @property
    def serve_unfused_rows_latent(self) -> tuple:
        """The FM / MVM batch sizes [lo, hi) that take the unfused path on this
        engine (EngineConfig.serve_unfused_rows_latent, resolved per model)."""
        lo, hi = self._e.serve_unfused_latent
        return int(lo), int(hi)

    def export_weights_count(self) -> int:
        """Keys export_weights() would write (a count pass; syncs)."""
        self._sync_stream()
        return int(self._e.export_weights_count())

    def export_weights(self):
        """(keys u64 [n], weights f32 [n, P]) of the keys whose weights differ
        -- as bit patterns -- from what an absent key reads (slot_exported,
        csrc/include/xflow/types.h), each with its P resolved weights.  LR
        drops every zero-weight key; FM / MVM drop the keys never pushed and
        keep a pushed key even when L1 zeroed its latents.  A pull of any key
        returns the same bits from ``import_weights`` of this as from here."""
        self._sync_stream()
        k, w = self._e.export_weights()
        return k, w.reshape(len(k), self.params_per_key)

    def save_serving(self, path: str) -> int:
        """export_weights() as one ``.xfw`` file (checkpoint.save_serving's
        per-rank file); returns the keys written."""
        self._sync_stream()
        return int(self._e.save_serving(path))

    def import_weights(self, keys, weights) -> None:
        """Insert (key, P weights) pairs into this frozen engine."""
        self._sync_stream()
        self._e.import_weights(np.ascontiguousarray(keys, dtype=np.uint64),
                               np.ascontiguousarray(weights, dtype=np.float32).reshape(-1))

    # ---- serving deltas (docs/DESIGN.md §2) -----------------------------------
    def serving_delta_count(self) -> int:
        """Entries export_weights_delta() would write (a count pass; syncs)."""
        self._sync_stream()
        return int(self._e.serving_delta_count())

    def export_weights_delta(self):
        """(keys u64 [n], weights f32 [n, P]) of every key of the table whose
        touched-key bit is set (EngineConfig.delta_track), each with its P
        resolved weights -- a key that now reads exactly as an absent key
        included: that entry is a deletion, and nothing else marks it.  The
        filter is not cleared.  Raises with tracking off and on a frozen
        engine."""
        self._sync_stream()
        k, w = self._e.export_weights_delta()
        return k, w.reshape(len(k), self.params_per_key)

    def save_serving_delta(self, path: str) -> int:
        """export_weights_delta() as one ``.xfwd`` file (magic "XFLOWSD1", then
        the ``.xfw`` layout); returns the entries written."""
        self._sync_stream()
        return int(self._e.save_serving_delta(path))

    def apply_weights_delta(self, keys, weights) -> dict:
        """Apply a serving delta to this frozen engine: upsert every (key, P
        weights) entry, then sweep out every slot that now reads as an absent
        key.  Keys must be unique within one call.  Queued on the engine's
        stream: an eval_step before it scores with the old model, one after it
        with the new one.  Raises -- the table untouched -- when size + n would
        pass grow_load of the slots the table may grow to.  Returns
        {inserted, overwritten, dropped, segments_swept, upsert_seconds,
        sweep_seconds}."""
        self._sync_stream()
        d = self._e.apply_weights_delta(
            np.ascontiguousarray(keys, dtype=np.uint64),
            np.ascontiguousarray(weights, dtype=np.float32).reshape(-1))
        return {k: (float(v) if k.endswith("seconds") else int(v)) for k, v in d.items()}

    def save(self, path: str) -> None:
        self._sync_stream()
        self._e.save(path)

    def load(self, path: str) -> None:
        self._sync_stream()
        self._e.load(path)

    def synchronize(self) -> None:
        self._e.synchronize()
