"""Inference from a trained model: ``Predictor`` (batch / online scoring from a
checkpoint) and a small HTTP service around it.

The reference only predicts inside its training job: rank 0 scores the test
file after the last epoch (lr_worker.cc:40-98, fm_worker.cc:40-122) and the
weights die with the servers (ftrl.h:84,151).  Here a checkpoint
(xflow_amd/checkpoint.py, any world size) is loaded into ONE engine -- its
HBM table holds every shard -- and rows are scored by the same forward
kernels the trainer's evaluation uses (keys looked up, never inserted; an
unseen key scores with the weight its pull would have: 0 for w, the lazy
N(0,1)*scale init for latent factors, ftrl.h:110-122).

    p = Predictor("ckpt/")                     # or a versioned root (LATEST)
    p.predict_libffm(open("test-00000", "rb").read())   -> np.float32 [rows]
    p.predict_csr(keys_u64, row_ptr)                      -> np.float32 [rows]
    p.rank_keys([context], [[cand, ...]])   -> [np.float32 [candidates]] (one
        context scored against many candidates: Predictor.rank_csr)

    python -m xflow_amd.serve --checkpoint ckpt/ --port 8080
        POST /predict {"libffm": "1 1:123:1 2:456:1\\n..."}
                   or {"keys": [[k, ...], ...]}  -> {"pctr": [...]}
        POST /rank    {"context": [k, ...], "candidates": [[k, ...], ...]}
                      (+ "context_fields", "candidate_fields")  -> {"pctr": [...]}
                      with "top_k": K, the best K selected on the device
                                                -> {"index": [...], "pctr": [...]}
        POST /pool    {"name": "ads", "candidates": [[k, ...], ...]}  -> {"name", "candidates"}
                      registers or replaces a resident candidate pool; then
        POST /rank    {"context": [k, ...], "pool": "ads"}  (or "contexts": [[k, ...], ...];
                      optional "top_k")     -> as above, one entry per context with "contexts"
                      with "pool_index": [i, ...] (under "contexts": [[i, ...], ...]) the
                      context's own list of pool indices is scored, not the whole pool
                      a model with feature crosses: "fields": [[f, ...], ...] with
                      POST /pool and "context_fields" (a list, or lists under
                      "contexts") with POST /rank
        GET  /health

A candidate catalogue that many requests share is uploaded and probed once,
as a ``Pool`` (docs/DESIGN.md §2, candidate pools): ``build_pool`` turns every
candidate into 1 + Dk floats, and ``rank_pool`` scores R contexts against all
of them as one matrix product on the device, touching the table for the
contexts' keys alone.

    pool = p.build_pool([[k, ...], ...])         # once per catalogue
    p.rank_pool([context, ...], pool)         -> [np.float32 [len(pool)]] per context
    p.rank_pool([context, ...], pool, top_k=K) -> [(index, pctr)] per context

A serving snapshot (checkpoint.save_serving, ``--save-serving``, or the offline
conversion below) is loaded the same way: ``Predictor(dir)`` sees "kind":
"serving" in its meta.json and builds a frozen engine that holds only the keys
whose weights differ from an absent key's, as resolved fp32 weights -- the
same predictions, bit for bit, from a fraction of the memory.

    python -m xflow_amd.serve export --checkpoint ckpt/ --out snap/ [--parts N]

converts any checkpoint (a delta tip included) part by part: part r of N loads
only the keys it owns (checkpoint.load's resharding) into a table sized for
them and writes serving-r-of-N.xfw, so the peak memory is 1/N of the model.

A Predictor opened on a versioned root of serving versions (the trainer's
``--serving-every``) follows the training job: ``refresh()`` resolves LATEST
again and, when the new version's chain of serving deltas contains the loaded
one, applies the missing deltas to the live frozen table (inserts, overwrites
and deletions on the device, Engine.apply_weights_delta) -- otherwise it builds
a new engine off to the side and swaps it in.

        POST /refresh                                -> refresh()'s dict
    python -m xflow_amd.serve --checkpoint serving/ --refresh-seconds 30

Rows are scored in batches of ``max_rows``; one engine serves requests one
at a time (a lock around the device work).
"""
from __future__ import annotations

import argparse
import math
import os
import threading
import time
from typing import Optional, Sequence, Union

import numpy as np
import torch

from xflow_amd import checkpoint
from xflow_amd import native as _native
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig
from xflow_amd.engine import Batch, Engine


def _resolve(path: str) -> str:
    """A checkpoint directory, or a versioned root whose LATEST names one."""
    if os.path.exists(os.path.join(path, "meta.json")):
        return path
    d = checkpoint.latest(path)
    if d is None:
        raise FileNotFoundError(f"{path}: no checkpoint (meta.json or LATEST)")
    return d


def _fields(cls, d: dict):
    names = {f.name for f in cls.__dataclass_fields__.values()}
    return cls(**{k: v for k, v in d.items() if k in names})


class Pool:
    """A resident candidate pool (Predictor.build_pool): the candidates' rows on
    the device as CSR chunks, their pool vectors [n, W] and the model version
    of the Predictor the vectors were computed from."""

    def __init__(self, chunks, n: int):
        self.chunks, self.n = chunks, int(n)
        self.vecs, self.version = None, None
        self.ops = None  # a crossed model: the candidates' operand rows [n, 1 + nu]

    def __len__(self) -> int:
        return self.n


class Predictor:
    """Scores rows with a model loaded from a checkpoint (see module doc)."""

    def __init__(self, ckpt: str, device: Optional[torch.device] = None, max_rows: int = 65536,
                 max_nnz_per_row: int = 64, serve_fused: bool = True,
                 serve_unfused_rows=None, serve_unfused_rows_latent=None, rank_cross: bool = True,
                 pool_max_scores: int = 1 << 26, pool_topk_fused: bool = True,
                 pool_topk_strip: int = 0, pool_topk_fused_min: Optional[int] = None):
        self.root = ckpt  # (refresh() resolves it again)
        self.pool_max_scores = int(pool_max_scores)  # floats of one rank_pool chunk's scores
        self._version = 0  # bumped whenever the model this Predictor scores with changes
        if device is None:
            device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
        self.device = device
        self.max_rows = int(max_rows)
        self._max_nnz_per_row = int(max_nnz_per_row)
        self._serve_cfg = dict(serve_fused=serve_fused, rank_cross=bool(rank_cross),
                               pool_topk_fused=bool(pool_topk_fused),
                               pool_topk_strip=int(pool_topk_strip),
                               **({} if pool_topk_fused_min is None else
                                  {"pool_topk_fused_min": int(pool_topk_fused_min)}),
                               **({} if serve_unfused_rows is None else
                                  {"serve_unfused_rows": tuple(serve_unfused_rows)}),
                               **({} if serve_unfused_rows_latent is None else
                                  {"serve_unfused_rows_latent": tuple(serve_unfused_rows_latent)}))
        self._lock = threading.Lock()
        self._refreshing = threading.Lock()  # (one refresh at a time)
        self._adopt(self._load(_resolve(ckpt)))

    def _load(self, ckpt_dir: str) -> dict:
        """A new engine holding the version ``ckpt_dir``, and what describes it."""
        meta = checkpoint.load_meta(ckpt_dir)
        snapshot = checkpoint.is_serving(meta)
        model = _fields(ModelConfig, meta["model"])
        optim = _fields(OptimConfig, checkpoint.frozen_optim(meta) if snapshot else meta["optim"])
        # the feature crosses the model was trained with (absent: none): every
        # request is crossed the same way before it is scored
        crosses, cross_field_base = checkpoint.crosses_of(meta)
        # (key counts from the file headers: nothing else is read twice; a
        # delta version: its full base's keys plus every delta's of its
        # chain, an upper bound -- a delta repeats keys its bases hold)
        if snapshot:
            n_keys = checkpoint.serving_chain_keys(ckpt_dir)
        else:
            n_keys = sum(checkpoint.shard_keys(p) for p in checkpoint.chain_files(ckpt_dir))
        # every shard's keys in one table at load <= 0.5.  A training
        # checkpoint's table never grows while serving; a snapshot's may, by
        # segment splits, when serving deltas bring more keys (refresh)
        lg = max(16, int(math.ceil(math.log2(max(2 * n_keys, 1)))))
        engine = Engine(model, optim,
                        EngineConfig(table_log2_cap=lg, max_rows=self.max_rows,
                                     max_nnz=self.max_rows * (self._max_nnz_per_row + len(crosses)),
                                     table_grow=snapshot, **self._serve_cfg),
                        device=self.device)
        if snapshot:
            checkpoint.load_serving(engine, ckpt_dir)
        else:
            checkpoint.load(engine, ckpt_dir, 0, 1)
        return dict(ckpt=ckpt_dir, meta=meta, snapshot=snapshot, model=model, optim=optim,
                    crosses=crosses, cross_field_base=cross_field_base, engine=engine,
                    keys=engine.table_size())  # (a snapshot: the keys it kept)

    def _adopt(self, v: dict) -> None:
        for k, x in v.items():
            setattr(self, k, x)
        self._version += 1

    # ---------------------------------------------------------------- refresh
    def refresh(self) -> dict:
        """Follow the root this Predictor was opened on to its LATEST version.
        Returns {version, mode, inserted, overwritten, dropped, segments_swept,
        seconds}; mode "delta": the missing serving deltas were applied to the
        live table under the lock (their files read before it is taken);
        "full": a new engine was built off to the side and swapped in under
        the lock -- the new version's chain does not contain the loaded one,
        its model, crosses or source optimiser differ, this Predictor holds a
        training checkpoint, or the table refused a delta for capacity;
        "none": nothing is new.  A request sees one version or the other
        whole, never a mix."""
        t0 = time.perf_counter()
        counts = {"inserted": 0, "overwritten": 0, "dropped": 0, "segments_swept": 0}
        with self._refreshing:
            tip = _resolve(self.root)
            mode = "none"
            if os.path.abspath(tip) != os.path.abspath(self.ckpt):
                mode = "full"
                missing = self._missing_deltas(tip)
                if missing is not None:
                    try:
                        # (host reads outside the lock: requests go on meanwhile)
                        deltas = [(d, checkpoint.read_serving_deltas(self.engine, d))
                                  for d in missing]
                        for d, files in deltas:
                            with self._lock:  # a version lands whole
                                r = checkpoint.apply_serving_deltas(self.engine, files)
                                self.ckpt, self.meta = d, checkpoint.load_meta(d)
                                self.keys = self.engine.table_size()
                                self._version += 1
                            for k in counts:
                                counts[k] += r[k]
                        mode = "delta"
                    except RuntimeError:  # (no room for a delta: the table is at a whole version)
                        mode = "full"
                if mode == "full":
                    v = self._load(tip)
                    with self._lock:
                        self._adopt(v)
            return dict(version=os.path.basename(os.path.abspath(self.ckpt)), mode=mode, **counts,
                        seconds=time.perf_counter() - t0)

    def _missing_deltas(self, tip: str):
        """The serving delta versions between the loaded version and ``tip``,
        oldest first; None when the live table cannot be brought there by
        deltas."""
        if not self.snapshot:
            return None
        try:
            meta = checkpoint.load_meta(tip)
            if not checkpoint.is_serving(meta):
                return None
            links = [os.path.abspath(d) for d in checkpoint.serving_chain(tip)]
        except (OSError, ValueError):
            return None
        cur = os.path.abspath(self.ckpt)
        same = all(meta.get(k) == self.meta.get(k) for k in ("model", "optim")) and \
            checkpoint.crosses_of(meta) == checkpoint.crosses_of(self.meta)
        if cur not in links or not same:
            return None
        return links[links.index(cur) + 1:]

    # ---------------------------------------------------------------- scoring
    def predict_csr(self, keys: np.ndarray, row_ptr: np.ndarray,
                    fgid: Optional[np.ndarray] = None) -> np.ndarray:
        """pctr of every row of a CSR batch (keys u64, row_ptr rows+1 offsets;
        fgid: the field ids MVM groups by -- required for an MVM model, whose
        field products would be wrong with every feature in one field)."""
        keys = np.ascontiguousarray(keys).view(np.uint64)
        row_ptr = np.asarray(row_ptr, dtype=np.int64)
        rows = len(row_ptr) - 1
        if rows < 0 or row_ptr[0] != 0 or row_ptr[-1] != len(keys):
            raise ValueError("row_ptr must hold rows+1 offsets from 0 to len(keys)")
        if fgid is None:
            if self.crosses:
                raise ValueError("this model was trained with feature crosses "
                                 f"{self.crosses}: their operands are looked up by field id, so "
                                 "give the field ids (fgid / 'fields') with the keys")
            if self.model.kind == "mvm":
                raise ValueError("an MVM model groups features by field: give the field ids "
                                 "(fgid / 'fields') with the keys")
            fgid = np.zeros(len(keys), np.int32)
        elif len(fgid) != len(keys):
            raise ValueError("fgid must hold one field id per key")
        out = np.empty(rows, np.float32)
        # (the engine's max_nnz also holds the rows' cross keys)
        cap_nnz = self.engine.cfg.max_nnz - len(self.crosses) * self.max_rows
        r = 0
        with self._lock:
            while r < rows:
                r1 = min(rows, r + self.max_rows)
                while r1 > r + 1 and row_ptr[r1] - row_ptr[r] > cap_nnz:
                    r1 = r + (r1 - r) // 2
                k0, k1 = int(row_ptr[r]), int(row_ptr[r1])
                if k1 - k0 > cap_nnz:
                    raise ValueError(f"row {r} has more than {cap_nnz} features")
                dev = self.device
                b = Batch(keys=torch.from_numpy(keys[k0:k1].view(np.int64)).to(dev),
                          labels=torch.zeros(r1 - r, dtype=torch.float32, device=dev),
                          row_ptr=torch.from_numpy((row_ptr[r:r1 + 1] - k0).astype(np.int32)).to(dev),
                          fgid=torch.from_numpy(np.ascontiguousarray(fgid[k0:k1], np.int32)).to(dev),
                          slice_rows=r1 - r)
                if self.crosses:
                    b = self.engine.cross_batch(b, self.crosses, fgid_base=self.cross_field_base)
                out[r:r1] = self.engine.eval_step(b).cpu().numpy()
                r = r1
        return out

    def predict_libffm(self, text: bytes) -> np.ndarray:
        """pctr of every line of libffm text (``label fgid:fid:val ...``; the
        features hashed like the training reader, csrc/io/reader.cpp)."""
        if isinstance(text, str):
            text = text.encode()
        if text and not text.endswith(b"\n"):
            text += b"\n"
        blk = _native.load().parse_libffm(text)
        return self.predict_csr(np.asarray(blk["keys"]).view(np.uint64),
                                np.asarray(blk["row_ptr"], np.int64), np.asarray(blk["fgid"]))

    def predict_keys(self, rows: Sequence[Sequence[int]],
                     fields: Optional[Sequence[Sequence[int]]] = None) -> np.ndarray:
        """pctr of rows given as lists of (already hashed) u64 keys, with the
        keys' field ids (same shape; required for MVM and for a model trained
        with feature crosses)."""
        lens = np.array([len(r) for r in rows], np.int64)
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        keys = (np.array([k for r in rows for k in r], dtype=np.uint64) if len(rp) > 1 and rp[-1]
                else np.zeros(0, np.uint64))
        fg = None
        if fields is not None:
            if [len(f) for f in fields] != lens.tolist():
                raise ValueError("'fields' must give one field id per key of every row")
            fg = np.array([g for f in fields for g in f], dtype=np.int32)
        return self.predict_csr(keys, rp, fg)


    # ---------------------------------------------------------------- ranking
    def rank_csr(self, ctx_keys: np.ndarray, ctx_ptr: np.ndarray, cand_keys: np.ndarray,
                 cand_ptr: np.ndarray, req_ptr: np.ndarray,
                 ctx_fgid: Optional[np.ndarray] = None,
                 cand_fgid: Optional[np.ndarray] = None, top_k: Optional[int] = None) -> list:
        """R ranking requests: request q is the context ctx_keys[ctx_ptr[q]:
        ctx_ptr[q + 1]] scored against the candidate rows req_ptr[q] ..
        req_ptr[q + 1] - 1 of the CSR batch (cand_keys, cand_ptr).  Returns one
        float32 array per request: the model's prediction for the context's
        keys followed by the candidate's.  A frozen LR or FM snapshot on the
        GPU scores a request's context once per 64 candidates
        (Engine.rank_step), a model with feature crosses too: given the field
        ids, its cross keys are built inside the kernel.  Every other model, a
        full checkpoint, the CPU and a crossed model with ``rank_cross=False``
        expand the rows on the host and score them with predict_csr (which
        needs the field ids where it would).

        With ``top_k`` (1 .. 1024) the selection happens on the device too
        (Engine.topk_step) and request q comes back as (index int32[n], pctr
        float32[n]), n = min(top_k, its candidates): the best candidates'
        positions in the request, best first, and their scores.  The order is
        total -- descending pctr with NaN and values <= 0 equal and last, equal
        scores by ascending position -- so chunking cannot change it."""
        if top_k is not None and not (isinstance(top_k, (int, np.integer)) and 1 <= top_k <= 1024):
            raise ValueError("top_k must be an integer from 1 to 1024")
        ctx_keys = np.ascontiguousarray(ctx_keys).view(np.uint64)
        cand_keys = np.ascontiguousarray(cand_keys).view(np.uint64)
        ctx_ptr, cand_ptr, req_ptr = (np.asarray(p, dtype=np.int64)
                                      for p in (ctx_ptr, cand_ptr, req_ptr))
        R, rows = len(req_ptr) - 1, len(cand_ptr) - 1
        for name, p, n, end in (("req_ptr", req_ptr, R, rows), ("ctx_ptr", ctx_ptr, R, len(ctx_keys)),
                                ("cand_ptr", cand_ptr, rows, len(cand_keys))):
            if p.ndim != 1 or n < 0 or len(p) != n + 1 or p[0] != 0 or p[-1] != end or \
                    (np.diff(p) < 0).any():
                raise ValueError(f"{name} must hold {max(n, 0) + 1} non-decreasing offsets "
                                 f"from 0 to {end}")
        if (ctx_fgid is None) != (cand_fgid is None):
            raise ValueError("give the field ids of both the contexts and the candidates, or neither")
        if ctx_fgid is not None and (len(ctx_fgid) != len(ctx_keys) or len(cand_fgid) != len(cand_keys)):
            raise ValueError("field ids must hold one id per key")
        crossed = bool(self.crosses)
        # (a crossed model without field ids: predict_csr below raises)
        if self.engine.ranks and (not crossed or
                                  (self.engine.cfg.rank_cross and ctx_fgid is not None)):
            fg = (np.asarray(ctx_fgid, np.int32), np.asarray(cand_fgid, np.int32)) if crossed else None
            out = self._rank_device(ctx_keys, ctx_ptr, cand_keys, cand_ptr, req_ptr, top_k, fg)
            if top_k is not None:
                return out
        else:
            # row = context then candidate, as the kernel sums them
            req = np.repeat(np.arange(R), np.diff(req_ptr))
            cat = lambda c, x: np.concatenate(
                [np.concatenate([c[ctx_ptr[q]:ctx_ptr[q + 1]], x[cand_ptr[r]:cand_ptr[r + 1]]])
                 for r, q in enumerate(req)]) if rows else x[:0]
            rp = np.concatenate([[0], np.cumsum(np.diff(ctx_ptr)[req] + np.diff(cand_ptr))])
            out = self.predict_csr(cat(ctx_keys, cand_keys), rp,
                                   None if ctx_fgid is None else
                                   cat(np.asarray(ctx_fgid, np.int32), np.asarray(cand_fgid, np.int32)))
            if top_k is not None:
                parts = [[] for _ in range(R)]
                with self._lock:
                    self._topk_parts(torch.from_numpy(out).to(self.device), req_ptr, int(top_k),
                                     np.zeros(R, np.int64), parts)
                return self._topk_merge(parts, int(top_k))
        return [out[req_ptr[q]:req_ptr[q + 1]] for q in range(R)]

    def _topk_parts(self, p, rp, k, first, parts) -> None:
        """Engine.topk_step on the device scores ``p`` of the requests with
        offsets ``rp`` into them; request j's pairs are appended to parts[j],
        its indices moved by first[j] (the rows of it that came before p)."""
        idx, sc = self.engine.topk_step(
            p, torch.from_numpy(np.ascontiguousarray(rp, np.int32)).to(self.device), k)
        idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
        n = np.minimum(np.diff(rp), k).tolist()
        idx += np.asarray(first, np.int32)[:, None]  # (the padding is cut off below)
        for j in np.flatnonzero(n).tolist():
            parts[j].append((idx[j, :n[j]], sc[j, :n[j]]))

    @staticmethod
    def _topk_merge(parts, k) -> list:
        """One (index, pctr) pair of arrays per request from its chunks' best
        k: a request cut by the chunking is selected again from those pairs,
        in topk_step's order."""
        out = []
        none = (np.zeros(0, np.int32), np.zeros(0, np.float32))
        for ps in parts:
            if len(ps) > 1:
                i, s = (np.concatenate(x) for x in zip(*ps))
                key = np.where(s > 0, s, 0).astype(np.float32).view(np.uint32).astype(np.int64)
                o = np.lexsort((i, -key))[:k]
                ps = [(i[o], s[o])]
            out.append(ps[0] if ps else none)
        return out

    def _rank_device(self, ctx_keys, ctx_ptr, cand_keys, cand_ptr, req_ptr, top_k=None, fgid=None):
        """Engine.rank_step over chunks of at most max_rows candidate rows and
        the engine's max_nnz keys.  A chunk takes the contexts of the requests
        it meets; a context's sums do not depend on which rows share its
        launch, so the chunking cannot change a score.  With ``top_k`` only
        each chunk's best pairs are downloaded (rank_csr's second form).
        ``fgid``: the (context, candidate) field ids of a model with crosses,
        uploaded per chunk like the keys; nothing is appended to the rows."""
        rows, dev = len(cand_ptr) - 1, self.device
        out = np.empty(rows, np.float32)
        parts = [[] for _ in range(len(req_ptr) - 1)]
        cap_nnz = self.engine.cfg.max_nnz
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt, copy=False)).to(dev)
        r = 0
        with self._lock:
            while r < rows:
                r1 = min(rows, r + self.max_rows)
                while r1 > r + 1 and cand_ptr[r1] - cand_ptr[r] > cap_nnz:
                    r1 = r + (r1 - r) // 2
                k0, k1 = int(cand_ptr[r]), int(cand_ptr[r1])
                if k1 - k0 > cap_nnz:
                    raise ValueError(f"candidate {r} has more than {cap_nnz} features")
                # requests q0 .. q1 - 1 have rows in [r, r1)
                q0 = int(np.searchsorted(req_ptr, r, side="right")) - 1
                q1 = int(np.searchsorted(req_ptr, r1, side="left"))
                c0, c1 = int(ctx_ptr[q0]), int(ctx_ptr[q1])
                b = Batch(keys=up(cand_keys[k0:k1].view(np.int64), np.int64),
                          labels=torch.zeros(r1 - r, dtype=torch.float32, device=dev),
                          row_ptr=up(cand_ptr[r:r1 + 1] - k0, np.int32),
                          fgid=None if fgid is None else up(fgid[1][k0:k1], np.int32))
                rp = np.clip(req_ptr[q0:q1 + 1], r, r1) - r
                p = self.engine.rank_step(up(ctx_keys[c0:c1].view(np.int64), np.int64),
                                          up(ctx_ptr[q0:q1 + 1] - c0, np.int32),
                                          up(rp, np.int32), b,
                                          ctx_fgid=None if fgid is None else up(fgid[0][c0:c1], np.int32),
                                          crosses=self.crosses if fgid is not None else None)
                if top_k is None:
                    out[r:r1] = p.cpu().numpy()
                else:
                    self._topk_parts(p, rp, int(top_k), rp[:-1] + r - req_ptr[q0:q1], parts[q0:q1])
                r = r1
        return out if top_k is None else self._topk_merge(parts, int(top_k))

    def rank_keys(self, contexts: Sequence[Sequence[int]],
                  candidates: Sequence[Sequence[Sequence[int]]],
                  context_fields: Optional[Sequence[Sequence[int]]] = None,
                  candidate_fields: Optional[Sequence[Sequence[Sequence[int]]]] = None,
                  top_k: Optional[int] = None) -> list:
        """rank_csr from lists: contexts[q] the (already hashed) u64 keys of
        request q's context, candidates[q] its candidates' key lists; the
        fields mirror their shapes (required where predict_keys requires
        them).  One float32 array per request, or with ``top_k`` one (index,
        pctr) pair of its best candidates (rank_csr)."""
        if len(contexts) != len(candidates):
            raise ValueError("give one list of candidates per context")
        flat = [c for cs in candidates for c in cs]
        ptr = lambda ls: np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.int64)
        arr = lambda ls, dt: np.array([k for x in ls for k in x], dtype=dt)
        fg = [None, None]
        if (context_fields is None) != (candidate_fields is None):
            raise ValueError("give 'context_fields' and 'candidate_fields' together")
        if context_fields is not None:
            ff = [f for fs in candidate_fields for f in fs]
            if [len(f) for f in context_fields] != [len(c) for c in contexts] or \
                    [len(fs) for fs in candidate_fields] != [len(cs) for cs in candidates] or \
                    [len(f) for f in ff] != [len(c) for c in flat]:
                raise ValueError("the fields must give one field id per key")
            fg = [arr(context_fields, np.int32), arr(ff, np.int32)]
        return self.rank_csr(arr(contexts, np.uint64), ptr(contexts), arr(flat, np.uint64), ptr(flat),
                             ptr(candidates), fg[0], fg[1], top_k)

    def rank_libffm(self, context_line: bytes, candidate_lines: bytes,
                    top_k: Optional[int] = None):
        """One request from libffm text (``label fgid:fid:val ...``, the label
        ignored): the context's features on one line, a candidate's on each
        line of ``candidate_lines``.  pctr of every candidate, or with
        ``top_k`` the (index, pctr) of the best (rank_csr)."""
        def parse(text):
            if isinstance(text, str):
                text = text.encode()
            if text and not text.endswith(b"\n"):
                text += b"\n"
            blk = _native.load().parse_libffm(text)
            return (np.asarray(blk["keys"]).view(np.uint64), np.asarray(blk["row_ptr"], np.int64),
                    np.asarray(blk["fgid"]))
        ck, cp, cf = parse(context_line)
        if len(cp) != 2:
            raise ValueError("the context is one libffm line")
        k, p, f = parse(candidate_lines)
        return self.rank_csr(ck, cp, k, p, np.array([0, len(p) - 1]), cf, f, top_k)[0]

    # ---------------------------------------------------------------- pools
    def build_pool_csr(self, keys: np.ndarray, row_ptr: np.ndarray,
                       fgid: Optional[np.ndarray] = None) -> Pool:
        """A Pool of the candidates of a CSR batch (keys u64, row_ptr n + 1
        offsets): their rows go to the device once, in chunks of at most
        ``max_rows`` rows, and Engine.pool_rows turns them into vectors.  A
        frozen LR or FM snapshot only, on either device; there is no host
        fallback -- the expanded rows are what a pool exists to avoid.

        A model trained with feature crosses needs ``fgid`` (int32, one field
        id per key): the pool then keeps every candidate's cross operands next
        to its vector, and rank_pool builds the pairs' cross keys on the
        device (Engine.pool_subset with crosses)."""
        if self.crosses and (fgid is None or not self.engine.cfg.rank_cross):
            raise ValueError("this model was trained with feature crosses: a cross key depends on "
                             "both the context and the candidate, so a candidate has no vector of "
                             "its own -- rank with rank_keys / rank_csr, or give the candidates' "
                             "field ids (fields= / fgid=, with rank_cross on) for a pool that keeps "
                             "their cross operands")
        if not self.crosses:
            fgid = None
        elif len(fgid) != len(np.ascontiguousarray(keys).reshape(-1)):
            raise ValueError("fgid must hold one field id per key")
        if not self.engine.pools:
            raise ValueError("candidate pools need a frozen LR or FM serving snapshot "
                             "(not MVM, not a full checkpoint, not fm_mfma)")
        keys = np.ascontiguousarray(keys).view(np.uint64)
        row_ptr = np.asarray(row_ptr, dtype=np.int64)
        n = len(row_ptr) - 1
        if row_ptr.ndim != 1 or n < 0 or row_ptr[0] != 0 or row_ptr[-1] != len(keys) or \
                (np.diff(row_ptr) < 0).any():
            raise ValueError("row_ptr must hold candidates + 1 non-decreasing offsets from 0 to len(keys)")
        chunks = []
        for r in range(0, n, self.max_rows):
            r1 = min(n, r + self.max_rows)
            k0, k1 = int(row_ptr[r]), int(row_ptr[r1])
            chunks.append(self._csr_batch(keys[k0:k1], row_ptr[r:r1 + 1] - k0,
                                          None if fgid is None else fgid[k0:k1]))
        pool = Pool(chunks, n)
        with self._lock:
            self._pool_vectors(pool)
        return pool

    def build_pool(self, rows: Sequence[Sequence[int]],
                   fields: Optional[Sequence[Sequence[int]]] = None) -> Pool:
        """build_pool_csr from lists of (already hashed) u64 keys; ``fields``:
        the field id of every key (a model with feature crosses)."""
        rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        fg = None
        if fields is not None:
            if [len(f) for f in fields] != [len(r) for r in rows]:
                raise ValueError("fields must hold one field id per key")
            fg = np.array([g for f in fields for g in f], dtype=np.int32)
        return self.build_pool_csr(np.array([k for r in rows for k in r], dtype=np.uint64), rp, fg)

    def build_pool_libffm(self, text: bytes) -> Pool:
        """build_pool_csr from libffm text, a candidate per line (predict_libffm)."""
        if isinstance(text, str):
            text = text.encode()
        if text and not text.endswith(b"\n"):
            text += b"\n"
        blk = _native.load().parse_libffm(text)
        return self.build_pool_csr(np.asarray(blk["keys"]).view(np.uint64),
                                   np.asarray(blk["row_ptr"], np.int64), np.asarray(blk["fgid"]))

    def _csr_batch(self, keys, row_ptr, fgid=None) -> Batch:
        dev = self.device
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        return Batch(keys=torch.from_numpy(np.ascontiguousarray(keys).view(np.int64)).to(dev),
                     labels=torch.zeros(len(row_ptr) - 1, dtype=torch.float32, device=dev),
                     row_ptr=up(row_ptr, np.int32), fgid=None if fgid is None else up(fgid, np.int32))

    def _pool_vectors(self, pool: Pool) -> torch.Tensor:
        """The pool's vectors under this Predictor's current model (lock held):
        rebuilt from the stored rows when the version has changed -- a
        refresh() or an engine swap -- so a pool never serves a stale model."""
        if pool.version != self._version:
            X = self.crosses
            if not self.engine.pools or \
                    (X and not (self.engine.cfg.rank_cross and all(b.fgid is not None for b in pool.chunks))):
                raise ValueError("the model this Predictor now holds has no candidate pools")
            vecs = torch.empty((pool.n, self.engine.pool_width), dtype=torch.float32,
                               device=self.device)
            ops, r = [], 0
            for b in pool.chunks:  # (a crossed model: the operand rows too)
                got = self.engine.pool_rows(b, out=vecs[r:r + b.rows], crosses=X or None)
                if X:
                    ops.append(got[1])
                r += b.rows
            pool.ops = torch.cat(ops) if ops else (
                torch.empty((0, self.engine.pool_ops_width(X)), dtype=torch.int64,
                            device=self.device) if X else None)
            pool.vecs, pool.version = vecs, self._version
        return pool.vecs

    def _rank_pool_subsets(self, ctx_keys, ctx_ptr, pool: Pool, top_k, index, ptr,
                           ctx_fgid=None) -> list:
        """rank_pool_csr with subsets (arguments checked there but for these).
        ctx_fgid: a crossed model -- the contexts are folded and every pair's
        cross keys are built inside Engine.pool_subset."""
        index = np.asarray(index, dtype=np.int64)
        ptr = np.asarray(ptr, dtype=np.int64)
        R, N = len(ctx_ptr) - 1, pool.n
        if index.ndim != 1 or ptr.ndim != 1 or len(ptr) != R + 1 or ptr[0] != 0 or \
                ptr[-1] != len(index) or (np.diff(ptr) < 0).any():
            raise ValueError("subset_ptr must hold requests + 1 non-decreasing offsets from 0 to "
                             "len(subset_index)")
        if len(index) and (index.min() < 0 or index.max() >= N):
            raise ValueError(f"a subset index is outside [0, {N}), the pool's candidates")
        out = []
        with self._lock:
            vecs = self._pool_vectors(pool)
            q = 0
            while q < R:
                # whole requests while their entries stay under pool_max_scores (one at least)
                q1 = int(np.searchsorted(ptr, ptr[q] + min(self.pool_max_scores, 0x7fffffff),
                                         side="right")) - 1
                q1 = min(R, max(q1, q + 1))
                c0, c1, m0, m1 = int(ctx_ptr[q]), int(ctx_ptr[q1]), int(ptr[q]), int(ptr[q1])
                if m1 - m0 > 0x7fffffff:
                    raise ValueError("one request's subset must stay below 2^31 candidates")
                xkw = {}
                if ctx_fgid is None:
                    cv = self.engine.pool_rows(self._csr_batch(ctx_keys[c0:c1], ctx_ptr[q:q1 + 1] - c0))
                else:
                    cv, co = self.engine.pool_rows(
                        self._csr_batch(ctx_keys[c0:c1], ctx_ptr[q:q1 + 1] - c0, ctx_fgid[c0:c1]),
                        crosses=self.crosses, fold=True)
                    xkw = dict(crosses=self.crosses, ctx_ops=co, pool_ops=pool.ops)
                rp = ptr[q:q1 + 1] - m0
                up = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(self.device)
                idx_d, rp_d = up(index[m0:m1]), up(rp)
                if top_k is None:
                    p = self.engine.pool_subset(cv, vecs, idx_d, rp_d, **xkw).cpu().numpy()
                    out += [p[rp[j]:rp[j + 1]] for j in range(q1 - q)]
                elif m1 == m0:
                    out += [(np.zeros(0, np.int32), np.zeros(0, np.float32))] * (q1 - q)
                else:
                    # scored and selected on the device, as pool indices
                    pi, sc = (t.cpu().numpy() for t in self.engine.pool_subset_topk(
                        cv, vecs, idx_d, rp_d, int(top_k), **xkw))
                    n = np.minimum(int(top_k), np.diff(rp))
                    out += [(pi[j, :n[j]], sc[j, :n[j]]) for j in range(q1 - q)]
                q = q1
        return out

    def rank_pool_csr(self, ctx_keys: np.ndarray, ctx_ptr: np.ndarray, pool: Pool,
                      top_k: Optional[int] = None, subset_index: Optional[np.ndarray] = None,
                      subset_ptr: Optional[np.ndarray] = None,
                      ctx_fgid: Optional[np.ndarray] = None) -> list:
        """R contexts (CSR: ctx_keys u64, ctx_ptr R + 1 offsets) against every
        candidate of ``pool``.  Returns one float32 array of len(pool) scores
        per context -- the model's prediction for the context's keys followed
        by the candidate's -- or with ``top_k`` (1 .. 1024) one (index int32[n],
        pctr float32[n]) pair, n = min(top_k, len(pool)), in rank_csr's order.
        The contexts are scored in chunks of whole requests whose scores stay
        under ``pool_max_scores`` floats; with ``top_k`` on an engine whose
        pool_topk is fused no scores are stored, and a chunk is bounded by the
        kernel's scratch instead (at most 4 * pool_max_scores bytes).

        ``subset_index`` / ``subset_ptr`` (together): request q is scored
        against its own list of pool indices subset_index[subset_ptr[q]:
        subset_ptr[q + 1]] only (Engine.pool_subset) and gets one score per
        entry of its list, in the list's order; with ``top_k`` the pair holds
        the pool indices of the best n = min(top_k, len(list)) entries, equal
        scores in ascending position in the list.  An index outside [0,
        len(pool)) raises ValueError before anything is uploaded.  A chunk is
        whole requests whose entries stay under ``pool_max_scores``.

        A model with feature crosses (a pool built with field ids) needs
        ``ctx_fgid``, one field id per context key, and raises ValueError
        without it.  Its scores are those of the row context + candidate +
        cross keys; without subsets every request's list is the whole pool,
        through the same kernel."""
        if top_k is not None and not (isinstance(top_k, (int, np.integer)) and 1 <= top_k <= 1024):
            raise ValueError("top_k must be an integer from 1 to 1024")
        ctx_keys = np.ascontiguousarray(ctx_keys).view(np.uint64)
        ctx_ptr = np.asarray(ctx_ptr, dtype=np.int64)
        R, N = len(ctx_ptr) - 1, pool.n
        if ctx_ptr.ndim != 1 or R < 0 or ctx_ptr[0] != 0 or ctx_ptr[-1] != len(ctx_keys) or \
                (np.diff(ctx_ptr) < 0).any():
            raise ValueError("ctx_ptr must hold requests + 1 non-decreasing offsets from 0 to len(ctx_keys)")
        if (subset_index is None) != (subset_ptr is None):
            raise ValueError("give 'subset_index' and 'subset_ptr' together")
        if self.crosses:
            if ctx_fgid is None:
                raise ValueError("this model was trained with feature crosses: give the contexts' "
                                 "field ids (context_fields= / ctx_fgid=)")
            ctx_fgid = np.asarray(ctx_fgid, dtype=np.int32)
            if ctx_fgid.shape != ctx_keys.shape:
                raise ValueError("ctx_fgid must hold one field id per context key")
        else:
            ctx_fgid = None
        if subset_index is not None:
            return self._rank_pool_subsets(ctx_keys, ctx_ptr, pool, top_k, subset_index, subset_ptr,
                                           ctx_fgid)
        per = max(1, min(self.pool_max_scores, 0x7fffffff) // max(N, 1))
        if self.crosses:
            # the whole pool as every request's list (the matrix-core kernels
            # take no crosses): chunks of whole requests, built as they go
            out = []
            for q in range(0, R, per):
                q1 = min(R, q + per)
                c0, c1 = int(ctx_ptr[q]), int(ctx_ptr[q1])
                out += self._rank_pool_subsets(ctx_keys[c0:c1], ctx_ptr[q:q1 + 1] - c0, pool, top_k,
                                               np.tile(np.arange(N), q1 - q),
                                               np.arange(q1 - q + 1) * N, ctx_fgid[c0:c1])
            return out
        if top_k is not None and self.engine.pool_topk_fused:
            words = self.engine.pool_topk_words(N, int(top_k))
            per = max(1, min(4 * self.pool_max_scores // (8 * max(words, 1)), 0x7fffffff))
        out = []
        with self._lock:
            vecs = self._pool_vectors(pool)
            for q in range(0, R, per):
                q1 = min(R, q + per)
                c0, c1 = int(ctx_ptr[q]), int(ctx_ptr[q1])
                cv = self.engine.pool_rows(self._csr_batch(ctx_keys[c0:c1], ctx_ptr[q:q1 + 1] - c0))
                if N == 0:
                    none = (np.zeros(0, np.int32), np.zeros(0, np.float32))
                    out += [none if top_k is not None else none[1]] * (q1 - q)
                elif top_k is None:
                    out += list(self.engine.pool_score(cv, vecs).cpu().numpy())
                else:
                    idx, sc = (t.cpu().numpy() for t in self.engine.pool_topk(cv, vecs, int(top_k)))
                    n = min(int(top_k), N)
                    out += [(idx[j, :n], sc[j, :n]) for j in range(q1 - q)]
        return out

    def rank_pool(self, contexts: Sequence[Sequence[int]], pool: Pool,
                  top_k: Optional[int] = None,
                  subsets: Optional[Sequence[Sequence[int]]] = None,
                  context_fields: Optional[Sequence[Sequence[int]]] = None) -> list:
        """rank_pool_csr from lists: contexts[q] the (already hashed) u64 keys
        of request q's context, ``subsets[q]`` its own list of pool indices,
        ``context_fields[q]`` the field id of every key (a crossed model)."""
        ptr = lambda ls: np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.int64)
        sub = {}
        if context_fields is not None:
            if [len(f) for f in context_fields] != [len(c) for c in contexts]:
                raise ValueError("context_fields must hold one field id per context key")
            sub["ctx_fgid"] = np.array([g for f in context_fields for g in f], dtype=np.int32)
        if subsets is not None:
            if len(subsets) != len(contexts):
                raise ValueError("give one list of pool indices per context")
            sub.update(subset_index=np.array([i for s in subsets for i in s], dtype=np.int64),
                       subset_ptr=ptr(subsets))
        return self.rank_pool_csr(np.array([k for c in contexts for k in c], dtype=np.uint64),
                                  ptr(contexts), pool, top_k, **sub)


# -------------------------------------------------------------------- service
def make_app(pred: Predictor):
    """FastAPI app: POST /predict, POST /rank, POST /refresh, GET /health."""
    from fastapi import FastAPI, HTTPException
    from pydantic import create_model

    # (built with explicit types: this module's postponed annotations would
    # leave FastAPI a string to resolve in a function scope)
    Req = create_model("PredictRequest", libffm=(Optional[str], None),
                       keys=(Optional[list[list[int]]], None),
                       fields=(Optional[list[list[int]]], None))

    app = FastAPI(title="xflow-amd predictor")

    @app.get("/health")
    def health():
        return {"status": "ok", "model": pred.model.kind, "keys": int(pred.keys),
                "device": str(pred.device), "checkpoint": pred.ckpt,
                "snapshot": bool(pred.snapshot),
                "version": os.path.basename(os.path.abspath(pred.ckpt))}

    @app.post("/refresh")
    def refresh():
        return pred.refresh()

    def predict(req):
        if (req.libffm is None) == (req.keys is None):
            raise HTTPException(400, "give exactly one of 'libffm' or 'keys'")
        try:
            p = (pred.predict_libffm(req.libffm) if req.libffm is not None
                 else pred.predict_keys(req.keys, req.fields))
        except ValueError as e:
            raise HTTPException(400, str(e))
        return {"pctr": [float(x) for x in p]}

    predict.__annotations__ = {"req": Req}
    app.post("/predict")(predict)

    PoolReq = create_model("PoolRequest", name=(str, ...), candidates=(list[list[int]], ...),
                           fields=(Optional[list[list[int]]], None))
    pools = {}  # name -> Pool, registered by POST /pool

    def pool(req):
        try:
            pools[req.name] = pred.build_pool(req.candidates, req.fields)
        except ValueError as e:
            raise HTTPException(400, str(e))
        return {"name": req.name, "candidates": len(pools[req.name])}

    pool.__annotations__ = {"req": PoolReq}
    app.post("/pool")(pool)

    RankReq = create_model("RankRequest", context=(Optional[list[int]], None),
                           candidates=(Optional[list[list[int]]], None),
                           context_fields=(Optional[Union[list[int], list[list[int]]]], None),
                           candidate_fields=(Optional[list[list[int]]], None),
                           top_k=(Optional[int], None), pool=(Optional[str], None),
                           contexts=(Optional[list[list[int]]], None),
                           pool_index=(Optional[Union[list[int], list[list[int]]]], None))

    def rank_pool(req):
        """"pool": a registered pool in place of "candidates", under one
        "context" or many "contexts" (then one entry per context).
        "pool_index": the context's own list of pool indices (one list per
        context under "contexts"); the scores, or with "top_k" the best, are
        of that list alone."""
        if req.candidates is not None or (req.context is None) == (req.contexts is None):
            raise HTTPException(400, "with 'pool' give 'context' or 'contexts', and no 'candidates'")
        if req.pool not in pools:
            raise HTTPException(404, f"no pool named {req.pool!r}: POST /pool first")
        subsets = req.pool_index
        if subsets is not None:
            nested = any(isinstance(s, list) for s in subsets)
            if req.context is not None and not nested:
                subsets = [subsets]
            elif req.context is not None or not all(isinstance(s, list) for s in subsets):
                raise HTTPException(400, "'pool_index' is a list under 'context' and a list of "
                                         "lists under 'contexts'")
        fields = req.context_fields  # (a crossed model: a list under 'context', lists under 'contexts')
        if fields is not None:
            nested = all(isinstance(f, list) for f in fields)
            if req.context is not None and not any(isinstance(f, list) for f in fields):
                fields = [fields]
            elif req.context is not None or not nested:
                raise HTTPException(400, "'context_fields' is a list under 'context' and a list of "
                                         "lists under 'contexts'")
        try:
            got = pred.rank_pool(req.contexts if req.context is None else [req.context],
                                 pools[req.pool], req.top_k, subsets, fields)
        except ValueError as e:
            raise HTTPException(400, str(e))
        if req.top_k is not None:
            got = [{"index": [int(i) for i in g[0]], "pctr": [float(x) for x in g[1]]} for g in got]
            return got[0] if req.context is not None else {"results": got}
        got = [[float(x) for x in g] for g in got]
        return {"pctr": got[0] if req.context is not None else got}

    def rank(req):
        if req.pool is not None:
            return rank_pool(req)
        if req.context is None or req.candidates is None or req.contexts is not None:
            raise HTTPException(400, "give 'context' and 'candidates' (or 'pool')")
        try:
            p = pred.rank_keys([req.context], [req.candidates],
                               None if req.context_fields is None else [req.context_fields],
                               None if req.candidate_fields is None else [req.candidate_fields],
                               req.top_k)[0]
        except ValueError as e:
            raise HTTPException(400, str(e))
        if req.top_k is not None:
            return {"index": [int(i) for i in p[0]], "pctr": [float(x) for x in p[1]]}
        return {"pctr": [float(x) for x in p]}

    rank.__annotations__ = {"req": RankReq}
    app.post("/rank")(rank)
    return app


def poll_refresh(pred: Predictor, seconds: float, stop: Optional[threading.Event] = None):
    """A daemon thread that calls ``pred.refresh()`` every ``seconds`` until
    ``stop`` is set; a failed refresh is logged and the loaded version stays."""
    import logging

    stop = stop or threading.Event()

    def loop():
        while not stop.wait(seconds):
            try:
                r = pred.refresh()
                if r["mode"] != "none":
                    logging.getLogger(__name__).info("refreshed: %s", r)
            except Exception:  # noqa: BLE001 - keep serving the loaded version
                logging.getLogger(__name__).exception("refresh failed")

    t = threading.Thread(target=loop, name="xflow-refresh", daemon=True)
    t.start()
    return t, stop


def export_snapshot(ckpt: str, out: str, parts: int = 1,
                    device: Optional[torch.device] = None) -> dict:
    """Offline conversion of a checkpoint (a delta tip included) into a
    serving snapshot of ``parts`` files.  Part r loads the keys it owns under
    a ``parts``-way sharding into a table sized for them, exports, and frees
    the engine before the next part.  Returns the snapshot's meta."""
    src = _resolve(ckpt)
    meta = checkpoint.load_meta(src)
    if checkpoint.is_serving(meta):
        raise ValueError(f"{src}: already a serving snapshot")
    if parts < 1:
        raise ValueError("--parts must be >= 1")
    model = _fields(ModelConfig, meta["model"])
    optim = _fields(OptimConfig, meta["optim"])
    n_keys = sum(checkpoint.shard_keys(p) for p in checkpoint.chain_files(src))
    # (hash sharding is even: a part holds about 1/parts of the keys; the table
    # still grows if a part turns out fuller)
    lg = max(16, int(math.ceil(math.log2(max(2 * n_keys / parts, 1)))))
    if device is None:
        device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    keep = {k: meta[k] for k in ("epoch", "steps", "crosses", "cross_field_base") if k in meta}
    for r in reversed(range(parts)):
        eng = Engine(model, optim, EngineConfig(table_log2_cap=min(lg, 31), max_rows=1024,
                                                max_nnz=1 << 16), device=device)
        checkpoint.load(eng, src, r, parts)
        # (one process writes every part in turn, part 0 last: its meta.json
        # is written once every file exists)
        checkpoint.save_serving(eng, out, r, parts, meta=keep, barrier=lambda: None)
        del eng
    return checkpoint.load_meta(out)


def main(argv=None) -> int:
    import sys

    argv = list(sys.argv[1:] if argv is None else argv)
    if argv and argv[0] == "export":
        ap = argparse.ArgumentParser(prog="python -m xflow_amd.serve export",
                                     description="convert a checkpoint into a serving snapshot")
        ap.add_argument("--checkpoint", required=True, help="checkpoint directory or versioned root")
        ap.add_argument("--out", required=True, help="directory of the snapshot")
        ap.add_argument("--parts", type=int, default=1,
                        help="files to write; each part loads 1/N of the model at a time")
        ap.add_argument("--cpu", action="store_true")
        a = ap.parse_args(argv[1:])
        m = export_snapshot(a.checkpoint, a.out, a.parts,
                            device=torch.device("cpu") if a.cpu else None)
        print(f"serving snapshot {a.out}: kept {m['keys_kept']} of {m['keys_total']} keys "
              f"in {a.parts} part(s)", flush=True)
        return 0
    ap = argparse.ArgumentParser(prog="python -m xflow_amd.serve", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=8080)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--max-rows", type=int, default=65536)
    ap.add_argument("--refresh-seconds", type=float, default=0.0,
                    help="poll the root's LATEST this often and refresh() (0: only POST /refresh)")
    a = ap.parse_args(argv)
    pred = Predictor(a.checkpoint, device=torch.device("cpu") if a.cpu else None,
                     max_rows=a.max_rows)
    if a.refresh_seconds > 0:
        poll_refresh(pred, a.refresh_seconds)
    import uvicorn

    uvicorn.run(make_app(pred), host=a.host, port=a.port, log_level="warning")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
