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

    python -m xflow_amd.serve --checkpoint ckpt/ --port 8080
        POST /predict {"libffm": "1 1:123:1 2:456:1\\n..."}
                   or {"keys": [[k, ...], ...]}  -> {"pctr": [...]}
        GET  /health

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
from typing import Optional, Sequence

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


class Predictor:
    """Scores rows with a model loaded from a checkpoint (see module doc)."""

    def __init__(self, ckpt: str, device: Optional[torch.device] = None, max_rows: int = 65536,
                 max_nnz_per_row: int = 64, serve_fused: bool = True,
                 serve_unfused_rows=None, serve_unfused_rows_latent=None):
        self.root = ckpt  # (refresh() resolves it again)
        if device is None:
            device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
        self.device = device
        self.max_rows = int(max_rows)
        self._max_nnz_per_row = int(max_nnz_per_row)
        self._serve_cfg = dict(serve_fused=serve_fused,
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


# -------------------------------------------------------------------- service
def make_app(pred: Predictor):
    """FastAPI app: POST /predict, POST /refresh, GET /health."""
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
