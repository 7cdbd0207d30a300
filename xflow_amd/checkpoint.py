"""Sharded checkpoint / resume of the HBM parameter table (an extension: the
reference keeps weights only in server RAM and loses them at exit,
src/optimizer/ftrl.h:84,151).

Layout of ``<dir>/``:
  meta.json                      model/optimizer config, world size, epoch, step;
                                 "crosses" / "cross_field_base" when the table
                                 was trained with feature crosses (cross_meta;
                                 absent: none)
  shard-<rank>-of-<world>.xftb   native binary shard (csrc/engine/engine_io.cpp
                                 Engine::save): header + keys + state words
  admit-<rank>-of-<world>.xfad   only with feature admission on
                                 (EngineConfig.admit_min_count > 1): the rank's
                                 counting filter, its raw bytes; meta.json then
                                 also records admit_min_count and admit_log2

  delta-<rank>-of-<world>.xftb   instead of the shard, in a delta version
                                 (meta.json "delta_base": "<version dir name>"):
                                 only the keys touched since that version was
                                 saved (Engine.save_delta, the shard format with
                                 header word 7 = 1)

A delta version (``save(..., delta_base=...)``, EngineConfig.delta_track) is
loaded by resolving its chain of bases back to a full version, loading that
one and importing each delta on top, oldest first -- an import overwrites the
state of a key that is present.  ``publish`` never deletes a version that a
kept version's chain needs.

A serving snapshot (``save_serving``; meta.json "kind": "serving") is not a
checkpoint to resume from: it holds only the keys whose weights differ from
what an absent key reads, as resolved fp32 weights without optimiser state,
  serving-<rank>-of-<world>.xfw  magic "XFLOWSW1", int32 {model kind, v_dim,
                                 fm_math, mvm_math, P, source optimiser kind},
                                 u64 keys of the source table, u64 n,
                                 keys u64[n], weights f32[n, P]
  meta.json                      "kind": "serving", model, optim (the source's),
                                 the crosses record, keys_total, keys_kept
``load_serving`` imports every rank's file into one frozen engine
(OptimConfig.kind "frozen"); ``load`` / ``check_compatible`` refuse it, and
``publish`` neither counts nor deletes such a directory.

A serving delta version (``save_serving(..., delta_base=...)``; meta.json still
"kind": "serving", plus "delta_base") holds, instead of the .xfw files,
  serving-delta-<rank>-of-<world>.xfwd   magic "XFLOWSD1", then the .xfw header
                                 fields and arrays: (key, P resolved weights) of
                                 every key touched since the base version --
                                 a key that now reads as an absent key included,
                                 which is how a deletion is written
``serving_chain`` resolves it to its full base; ``load_serving`` loads the
base and applies the deltas in order (Engine.apply_weights_delta);
``publish_serving`` keeps every version a kept one needs.

Resume is world-size agnostic: with the same world size each rank loads its
own shard; otherwise every rank scans all shards and imports exactly the keys
it owns under the new hash sharding (owner = fmix64(key) >> 32 mod world).

Periodic checkpoints (``--save-every``, the tracker's recovery) are versioned:
``<root>/epoch-NNNNNN/`` holds one complete checkpoint in the layout above and
``<root>/LATEST`` names the newest complete one.  LATEST is replaced
atomically by rank 0 only after every rank has written its shard, so a job
killed mid-save resumes from the previous version.
"""
from __future__ import annotations

import dataclasses
import glob
import json
import logging
import os
import shutil
import struct
import warnings
from typing import Callable, Optional

import numpy as np

from xflow_amd.testing.hashing import owner_of

MAGIC = b"XFLOWTB1"

log = logging.getLogger(__name__)


def shard_name(rank: int, world: int) -> str:
    return f"shard-{rank:05d}-of-{world:05d}.xftb"


def admit_name(rank: int, world: int) -> str:
    return f"admit-{rank:05d}-of-{world:05d}.xfad"


def delta_name(rank: int, world: int) -> str:
    return f"delta-{rank:05d}-of-{world:05d}.xftb"


SERVING_MAGIC = b"XFLOWSW1"


def serving_name(rank: int, world: int) -> str:
    return f"serving-{rank:05d}-of-{world:05d}.xfw"


SERVING_DELTA_MAGIC = b"XFLOWSD1"


def serving_delta_name(rank: int, world: int) -> str:
    return f"serving-delta-{rank:05d}-of-{world:05d}.xfwd"


def is_serving(meta: dict) -> bool:
    return meta.get("kind") == "serving"


def _refuse_serving(meta: dict, where: str) -> None:
    if is_serving(meta):
        raise ValueError(f"{where}: a serving snapshot (resolved weights only, no optimiser "
                         f"state): it cannot be resumed from; load it with "
                         f"xflow_amd.serve.Predictor or checkpoint.load_serving")


def shard_keys(path: str) -> int:
    """Number of keys in a native shard file, from its header only (48 bytes
    read, not the keys and state words)."""
    with open(path, "rb") as f:
        if f.read(8) != MAGIC:
            raise ValueError(f"{path}: not an xflow table shard")
        f.seek(32, os.SEEK_CUR)
        (n,) = struct.unpack("<Q", f.read(8))
    return int(n)


def read_shard(path: str):
    """(header ints, keys u64, words u32 [n, W]) of a native shard file."""
    with open(path, "rb") as f:
        magic = f.read(8)
        if magic != MAGIC:
            raise ValueError(f"{path}: not an xflow table shard")
        hdr = struct.unpack("<8i", f.read(32))
        (n,) = struct.unpack("<Q", f.read(8))
        keys = np.frombuffer(f.read(8 * n), dtype=np.uint64)
        W = hdr[6] - 2
        words = np.frombuffer(f.read(4 * n * W), dtype=np.uint32).reshape(n, W)
    return hdr, keys, words


def _fsync_file(path: str) -> None:
    fd = os.open(path, os.O_RDONLY)
    try:
        os.fsync(fd)
    finally:
        os.close(fd)


def _fsync_dir(path: str) -> None:
    try:
        _fsync_file(path)
    except OSError:  # pragma: no cover - directories cannot be opened on some filesystems
        pass


def _default_barrier() -> None:
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        dist.barrier()


def _tip(ckpt_dir: str) -> str:
    return os.path.abspath(ckpt_dir)


def _can_delta(engine, ckpt_dir: str, world: int, delta_base: Optional[str]) -> bool:
    """Whether this save may be a delta on ``delta_base``: tracking on, nothing
    happened that a delta cannot carry, the base is a complete version under
    the same root, written with the same world size -- and it is the version
    the engine's filter was last cleared at (its last save or load)."""
    if not delta_base or engine.delta_log2 == 0 or engine.delta_needs_full:
        return False
    base = os.path.join(os.path.dirname(_tip(ckpt_dir)), delta_base)
    if getattr(engine, "_delta_tip", None) != _tip(base):
        return False
    try:
        return int(load_meta(base)["world"]) == world
    except (OSError, ValueError, KeyError):
        return False


def save(engine, ckpt_dir: str, rank: int, world: int, meta: Optional[dict] = None,
         barrier: Optional[Callable[[], None]] = None, delta_base: Optional[str] = None) -> str:
    """Write this rank's shard (fsync'd), wait for every rank (``barrier``,
    default: the torch.distributed group when one is initialised), then rank 0
    writes meta.json -- so a valid meta.json only ever sits next to a complete
    set of shards of one save.  Returns the shard's path.

    ``delta_base``: the name of the previous version's directory under the
    same root.  The rank then writes only the keys touched since that version
    (``delta-*.xftb``) and meta.json names the base -- when the engine tracks
    deltas, its ``needs_full`` is unset, and the base exists with this world
    size; otherwise the version is a full one.  Ranks of one job must decide
    alike: ``needs_full`` is per rank, so a multi-rank caller passes a base
    only when no rank needs a full save (Trainer.save_versioned).  Once its
    file is durable the rank clears its filter (delta_clear), after a full
    save too: the next delta holds what changes from here on."""
    os.makedirs(ckpt_dir, exist_ok=True)
    delta = _can_delta(engine, ckpt_dir, world, delta_base)
    name, other = delta_name(rank, world), shard_name(rank, world)
    if not delta:
        name, other = other, name
    path = os.path.join(ckpt_dir, name)
    tmp = path + ".tmp"
    (engine.save_delta if delta else engine.save)(tmp)
    _fsync_file(tmp)
    os.replace(tmp, path)
    stale = os.path.join(ckpt_dir, other)  # (an interrupted save of the other kind)
    if os.path.exists(stale):
        os.remove(stale)
    engine.delta_clear()
    engine._delta_tip = _tip(ckpt_dir)
    admit = engine.admit_bytes() > 0
    if admit:  # the admission filter next to the shard
        apath = os.path.join(ckpt_dir, admit_name(rank, world))
        with open(apath + ".tmp", "wb") as f:
            engine.admit_export().tofile(f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(apath + ".tmp", apath)
    (barrier or _default_barrier)()
    if rank == 0:
        m = dict(meta or {})
        m.update(world=world, model=dataclasses.asdict(engine.model),
                 optim=dataclasses.asdict(engine.optim))
        m.pop("delta_base", None)
        if delta:
            m["delta_base"] = delta_base
        kinds = [len(glob.glob(os.path.join(ckpt_dir, pat % world)))
                 for pat in ("delta-*-of-%05d.xftb", "shard-*-of-%05d.xftb")]
        if kinds[0] and kinds[1]:
            raise RuntimeError(f"{ckpt_dir}: the ranks did not agree on a full or a delta save "
                               f"(delta, full files: {kinds}, world {world})")
        if admit:
            m.update(admit_min_count=int(engine.cfg.admit_min_count),
                     admit_log2=int(engine.admit_log2))
        mtmp = os.path.join(ckpt_dir, "meta.json.tmp")
        with open(mtmp, "w") as f:
            json.dump(m, f, indent=1)
            f.flush()
            os.fsync(f.fileno())
        os.replace(mtmp, os.path.join(ckpt_dir, "meta.json"))
        _fsync_dir(ckpt_dir)
    return path


# Fields that define what the table's state means: a resume must match them.
# Everything else (fm_mfma picks a kernel; lr/alpha/beta/lambda1/lambda2 are
# a schedule the user may change on resume) only warns.
_LAYOUT_FIELDS = {"model": ("kind", "v_dim", "fm_math", "mvm_math"),
                  "optim": ("kind", "v_init_scale", "sgd_v_init", "seed")}


def check_compatible(engine, meta: dict) -> None:
    """The checkpoint's layout-defining model/optimizer fields must equal the
    running ones; other differences (hyperparameters, kernel choices) are
    reported as warnings."""
    _refuse_serving(meta, "checkpoint")
    want = {"model": dataclasses.asdict(engine.model), "optim": dataclasses.asdict(engine.optim)}
    for k, cur in want.items():
        saved = meta.get(k)
        if saved is None:
            continue
        diff = {f: (saved.get(f), v) for f, v in cur.items() if f in saved and saved[f] != v}
        hard = {f: d for f, d in diff.items() if f in _LAYOUT_FIELDS[k]}
        if hard:
            raise ValueError(f"checkpoint {k} config differs from the running one: {hard}")
        if diff:
            warnings.warn(f"resuming with a changed {k} config (saved, now): {diff}")


def _check_header(engine, path: str, hdr) -> None:
    """Shard header (csrc/engine/engine_io.cpp Engine::save: version, kind, v_dim,
    P, p_w, opt, stride) against the engine's table layout."""
    if hdr[0] != 1:
        raise ValueError(f"{path}: unsupported shard version {hdr[0]}")
    lay = engine.layout
    got = {"kind": hdr[1], "P": hdr[3], "opt": hdr[5], "stride": hdr[6]}
    exp = {"kind": lay["kind"], "P": lay["P"], "opt": lay["opt"], "stride": lay["stride"]}
    if got != exp:
        raise ValueError(f"{path}: shard layout {got} does not match this engine {exp}")


def load_meta(ckpt_dir: str) -> dict:
    with open(os.path.join(ckpt_dir, "meta.json")) as f:
        return json.load(f)


def cross_meta(crosses, field_base) -> dict:
    """meta.json's record of the feature crosses a table was trained with
    (TrainConfig.crosses): ``crosses`` (lists of field ids) and
    ``cross_field_base`` (-1: the crosses carry no field id).  Nothing when
    there are none -- the file of an uncrossed model is what it always was."""
    if not crosses:
        return {}
    return {"crosses": [[int(f) for f in c] for c in crosses],
            "cross_field_base": -1 if field_base is None else int(field_base)}


def crosses_of(meta: dict):
    """(crosses as a list of tuples, field base or None) of a checkpoint's
    meta.json; absent keys (every checkpoint written before crosses existed):
    no crosses."""
    crosses = [tuple(int(f) for f in c) for c in meta.get("crosses") or []]
    base = int(meta.get("cross_field_base", -1))
    return crosses, (base if crosses and base >= 0 else None)


def check_crosses_match(meta: dict, crosses, field_base, where: str = "checkpoint") -> None:
    """A table holds the keys of the crosses it was trained with: continuing
    or serving it under another spec would look up keys it never saw."""
    saved, sbase = crosses_of(meta)
    now = [tuple(int(f) for f in c) for c in crosses or []]
    nbase = field_base if now else None
    if saved != now or sbase != nbase:
        raise ValueError(f"{where}: trained with crosses {saved} (field base {sbase}), the "
                         f"running configuration has {now} (field base {nbase})")


def _load_admit(engine, ckpt_dir: str, rank: int, world: int, meta: dict) -> None:
    """Restore the admission filter when the checkpoint holds one of this
    world size and filter size; otherwise the filter starts empty (a filter is
    not resharded or resized) and the log says what that costs."""
    if engine.admit_bytes() == 0:
        return
    path = os.path.join(ckpt_dir, admit_name(rank, world))
    if (int(meta["world"]) == world and int(meta.get("admit_log2", 0)) == engine.admit_log2
            and os.path.exists(path)):
        engine.admit_import(np.fromfile(path, dtype=np.uint8))
        return
    log.warning("checkpoint %s: no admission filter for world %d / admit_log2 %d (saved: world "
                "%s, admit_log2 %s); the filter starts empty, so keys not yet admitted need "
                "their sightings again", ckpt_dir, world, engine.admit_log2, meta.get("world"),
                meta.get("admit_log2"))


def chain(ckpt_dir: str) -> list:
    """The version directories ``ckpt_dir`` is made of, oldest first: the full
    version its chain of ``delta_base`` links ends at, then every delta up to
    ``ckpt_dir`` itself ([ckpt_dir] for a full version).  A link that is
    missing raises FileNotFoundError naming it."""
    tip = _tip(ckpt_dir)
    out, d = [], tip
    while True:
        if not os.path.exists(os.path.join(d, "meta.json")):
            raise FileNotFoundError(
                f"{d}: no meta.json" if d == tip else
                f"{tip}: its delta chain needs the version {d}, which is missing")
        if d in out:
            raise ValueError(f"{tip}: delta chain loops at {d}")
        out.append(d)
        base = load_meta(d).get("delta_base")
        if not base:
            return out[::-1]
        d = os.path.join(os.path.dirname(d), base)


def chain_files(ckpt_dir: str) -> list:
    """Every table file of the chain, in loading order: the full version's
    shards, then each delta version's.  Raises FileNotFoundError when a
    version does not hold one file per saved rank."""
    files = []
    for i, d in enumerate(chain(ckpt_dir)):
        w = int(load_meta(d)["world"])
        pat = ("shard-*-of-%05d.xftb" if i == 0 else "delta-*-of-%05d.xftb") % w
        got = sorted(glob.glob(os.path.join(d, pat)))
        if len(got) != w:
            raise FileNotFoundError(f"{d}: expected {w} files {pat}, found {len(got)}")
        files += got
    return files


def _load_version(engine, d: str, rank: int, world: int, delta: bool) -> None:
    """One version's table files into the engine: this rank's own file when
    the world size is the saved one, else the keys it now owns of every file.
    An import overwrites the state of a present key, so a delta lands on top
    of what its bases loaded."""
    saved_world = int(load_meta(d)["world"])
    name = delta_name if delta else shard_name
    if saved_world == world:
        p = os.path.join(d, name(rank, world))
        if not os.path.exists(p):
            raise FileNotFoundError(f"{p}: missing")
        engine.load(p)
        return
    pat = ("delta-*-of-%05d.xftb" if delta else "shard-*-of-%05d.xftb") % saved_world
    shards = sorted(glob.glob(os.path.join(d, pat)))
    if len(shards) != saved_world:
        raise FileNotFoundError(f"{d}: expected {saved_world} shards, found {len(shards)}")
    for p in shards:
        hdr, keys, words = read_shard(p)
        _check_header(engine, p, hdr)
        mine = owner_of(keys, world) == rank
        if mine.any():
            engine.import_table(keys[mine], words[mine].reshape(-1))


def load(engine, ckpt_dir: str, rank: int, world: int) -> dict:
    """Load the version (resolving a delta's chain, see ``chain``) and leave
    the engine's touched-key filter clean: its state equals the chain's tip,
    so the next save may be a delta on ``ckpt_dir``."""
    _refuse_serving(load_meta(ckpt_dir), ckpt_dir)
    links = chain(ckpt_dir)
    meta = load_meta(ckpt_dir)
    check_compatible(engine, meta)
    _load_admit(engine, ckpt_dir, rank, world, meta)
    for i, d in enumerate(links):
        _load_version(engine, d, rank, world, delta=i > 0)
    engine.delta_clear()
    engine._delta_tip = _tip(ckpt_dir)
    return meta


# ---------------------------------------------------------------- serving
def _read_serving_file(path: str, magic: bytes, what: str):
    with open(path, "rb") as f:
        if f.read(8) != magic:
            raise ValueError(f"{path}: not an xflow {what}")
        head = f.read(40)
        if len(head) != 40:
            raise ValueError(f"{path}: truncated {what}")
        hdr = struct.unpack("<6i", head[:24])
        _total, n = struct.unpack("<QQ", head[24:])
        P = hdr[4]
        if P < 1 or n > (1 << 40):
            raise ValueError(f"{path}: bad {what} header")
        kb, wb = f.read(8 * n), f.read(4 * n * P)
    if len(kb) != 8 * n or len(wb) != 4 * n * P:
        raise ValueError(f"{path}: truncated {what}")
    return hdr, np.frombuffer(kb, dtype=np.uint64), \
        np.frombuffer(wb, dtype=np.float32).reshape(n, P)


def read_serving(path: str):
    """(header ints, keys u64 [n], weights f32 [n, P]) of a serving file."""
    return _read_serving_file(path, SERVING_MAGIC, "serving snapshot")


def read_serving_delta(path: str):
    """The same of a serving delta file (``.xfwd``)."""
    return _read_serving_file(path, SERVING_DELTA_MAGIC, "serving delta")


def serving_counts(path: str):
    """(keys of the source table, keys kept) of a serving file, from its
    header only."""
    with open(path, "rb") as f:
        if f.read(8) not in (SERVING_MAGIC, SERVING_DELTA_MAGIC):
            raise ValueError(f"{path}: not an xflow serving snapshot or delta")
        f.seek(24, os.SEEK_CUR)
        total, n = struct.unpack("<QQ", f.read(16))
    return int(total), int(n)


def serving_files(ckpt_dir: str) -> list:
    """Every rank's file of a serving directory, by rank (the ``.xfwd`` files
    of a delta version)."""
    meta = load_meta(ckpt_dir)
    w = int(meta["world"])
    pat = ("serving-delta-*-of-%05d.xfwd" if meta.get("delta_base") else "serving-*-of-%05d.xfw") % w
    got = sorted(glob.glob(os.path.join(ckpt_dir, pat)))
    if len(got) != w:
        raise FileNotFoundError(f"{ckpt_dir}: expected {w} files {pat}, found {len(got)}")
    return got


def serving_chain(ckpt_dir: str) -> list:
    """The serving versions ``ckpt_dir`` is made of, oldest first: the full
    snapshot its ``delta_base`` links end at, then every delta up to
    ``ckpt_dir`` itself.  A missing link raises FileNotFoundError naming it."""
    links = chain(ckpt_dir)
    for d in links:
        if not is_serving(load_meta(d)):
            raise ValueError(f"{_tip(ckpt_dir)}: its chain holds {d}, which is not a serving version")
    return links


def _serving_record(meta: dict):
    """What two serving versions of one chain must share."""
    return meta.get("model"), meta.get("optim"), crosses_of(meta)


def _can_serving_delta(engine, out_dir: str, world: int, delta_base: Optional[str],
                       record) -> bool:
    """``_can_delta`` for a serving version: tracking on, nothing happened
    that a delta cannot carry, the filter was last cleared when the base was
    written, and the base is a complete serving version under the same root
    with the same world size, model, source optimiser and crosses record."""
    if not delta_base or engine.frozen or engine.delta_log2 == 0 or engine.delta_needs_full:
        return False
    base = os.path.join(os.path.dirname(_tip(out_dir)), delta_base)
    if getattr(engine, "_serving_tip", None) != (_tip(base), engine.delta_clears):
        return False
    try:
        bm = load_meta(base)
        serving_files(base)
    except (OSError, ValueError, KeyError):
        return False
    return is_serving(bm) and int(bm["world"]) == world and _serving_record(bm) == record


def mark_serving_tip(engine, out_dir: str) -> None:
    """The engine's touched-key filter was cleared with ``out_dir`` durable on
    every rank: the next serving version may be a delta on it -- until the
    filter is cleared again."""
    engine._serving_tip = (_tip(out_dir), engine.delta_clears)


def _serving_dir(d: str) -> bool:
    try:
        return is_serving(load_meta(d))
    except (OSError, ValueError):
        return False


def save_serving(engine, out_dir: str, rank: int, world: int, meta: Optional[dict] = None,
                 barrier: Optional[Callable[[], None]] = None, delta_base: Optional[str] = None,
                 clear: bool = True) -> str:
    """Write this rank's serving file (Engine.save_serving: the keys that
    differ from an absent key, as resolved weights; fsync'd), wait for every
    rank, then rank 0 writes meta.json -- ``save``'s protocol.  keys_total /
    keys_kept are summed from the files' headers, which carry both counts.

    ``delta_base``: the name of the previous serving version's directory under
    the same root.  The rank then writes a serving delta (``.xfwd``:
    Engine.save_serving_delta) and meta.json names the base -- under
    ``save``'s conditions for a checkpoint delta (``_can_serving_delta``);
    otherwise the version is a full snapshot.  As there, the ranks of one job
    must decide alike.

    The touched-key filter has one clear per version point.  ``clear`` (the
    default): once every rank's file is durable the rank clears its filter and
    the next serving version may be a delta on this one; a checkpoint chain
    loses its base by that (its next version is full).  ``clear=False``: the
    filter stays as it is, and so does the base of the next serving delta (a
    snapshot written aside); or a checkpoint version is written from the same
    filter at this point -- the caller saves it next (its save clears) and
    then calls ``mark_serving_tip``."""
    os.makedirs(out_dir, exist_ok=True)
    optim = dataclasses.asdict(engine.optim)
    if optim.get("kind") == "frozen":  # (a snapshot of a snapshot: the source's source)
        optim["kind"] = optim["frozen_from"]
    m = dict(meta or {})
    m.pop("delta_base", None)
    m.update(kind="serving", world=world, model=dataclasses.asdict(engine.model), optim=optim)
    m = json.loads(json.dumps(m))  # (as a reader sees it: tuples are lists)
    delta = _can_serving_delta(engine, out_dir, world, delta_base, _serving_record(m))
    name, other = serving_delta_name(rank, world), serving_name(rank, world)
    if not delta:
        name, other = other, name
    path = os.path.join(out_dir, name)
    (engine.save_serving_delta if delta else engine.save_serving)(path + ".tmp")
    _fsync_file(path + ".tmp")
    os.replace(path + ".tmp", path)
    stale = os.path.join(out_dir, other)  # (an interrupted save of the other kind)
    if os.path.exists(stale):
        os.remove(stale)
    (barrier or _default_barrier)()
    if clear and not engine.frozen and engine.delta_log2:
        engine.delta_clear()
        engine._delta_tip = None  # (a checkpoint delta would miss what was marked before)
        mark_serving_tip(engine, out_dir)
    if rank == 0:
        counts = [serving_counts(os.path.join(out_dir, (serving_delta_name if delta else
                                                        serving_name)(r, world)))
                  for r in range(world)]
        kinds = [len(glob.glob(os.path.join(out_dir, pat % world)))
                 for pat in ("serving-delta-*-of-%05d.xfwd", "serving-*-of-%05d.xfw")]
        if kinds[0] and kinds[1]:
            raise RuntimeError(f"{out_dir}: the ranks did not agree on a full or a delta serving "
                               f"version (delta, full files: {kinds}, world {world})")
        if delta:
            m.update(delta_base=delta_base, keys_total=sum(c[0] for c in counts),
                     keys_delta=sum(c[1] for c in counts))
        else:
            m.update(keys_total=sum(c[0] for c in counts), keys_kept=sum(c[1] for c in counts))
        mtmp = os.path.join(out_dir, "meta.json.tmp")
        with open(mtmp, "w") as f:
            json.dump(m, f, indent=1)
            f.flush()
            os.fsync(f.fileno())
        os.replace(mtmp, os.path.join(out_dir, "meta.json"))
        _fsync_dir(out_dir)
    return path


def frozen_optim(meta: dict) -> dict:
    """The OptimConfig fields of the frozen engine that serves ``meta``'s
    snapshot: the source optimiser's, with kind "frozen"."""
    o = dict(meta["optim"])
    o["frozen_from"] = o.get("kind", "ftrl")
    o["kind"] = "frozen"
    return o


def check_serving_header(engine, path: str, hdr) -> None:
    """A serving file's header (a snapshot's or a delta's) against the frozen
    engine that is to take it."""
    lay = engine.layout
    from xflow_amd.config import FM_MATH, MVM_MATH, OPT_KINDS

    exp = (lay["kind"], int(engine.model.v_dim), FM_MATH[engine.model.fm_math],
           MVM_MATH[engine.model.mvm_math], lay["P"], OPT_KINDS[engine.optim.frozen_from])
    got = tuple(hdr[:6])
    # (v_dim, fm_math and mvm_math only mean something to their own model)
    same = got[0] == exp[0] and got[4] == exp[4] and got[5] == exp[5] and \
        (exp[0] == 0 or got[1] == exp[1]) and (exp[0] != 1 or got[2] == exp[2]) and \
        (exp[0] != 2 or got[3] == exp[3])
    if not same:
        raise ValueError(f"{path}: snapshot header {got} does not match this engine {exp}")


def read_serving_deltas(engine, version_dir_: str) -> list:
    """[(keys, weights)] of one serving delta version, every rank's file read
    into host memory and its header checked against ``engine``."""
    out = []
    for p in serving_files(version_dir_):
        hdr, keys, weights = read_serving_delta(p)
        check_serving_header(engine, p, hdr)
        out.append((keys, weights))
    return out


def apply_serving_deltas(engine, deltas: list) -> dict:
    """Apply what ``read_serving_deltas`` read; the counts of every file summed."""
    tot = {"inserted": 0, "overwritten": 0, "dropped": 0, "segments_swept": 0}
    for keys, weights in deltas:
        if len(keys):
            r = engine.apply_weights_delta(keys, weights)
            for k in tot:
                tot[k] += r[k]
    return tot


def load_serving(engine, ckpt_dir: str) -> dict:
    """Import every rank's serving file into one frozen engine; a delta tip:
    its chain's full snapshot first, then each delta version applied in order.
    Any world size per version: every rank's file goes into the one engine."""
    meta = load_meta(ckpt_dir)
    if not is_serving(meta):
        raise ValueError(f"{ckpt_dir}: not a serving snapshot (use checkpoint.load)")
    if not engine.frozen:
        raise ValueError("load_serving: the engine must be frozen (OptimConfig.kind 'frozen')")
    links = serving_chain(ckpt_dir)
    for p in serving_files(links[0]):
        hdr, keys, weights = read_serving(p)
        check_serving_header(engine, p, hdr)
        if len(keys):
            engine.import_weights(keys, weights)
    for d in links[1:]:
        apply_serving_deltas(engine, read_serving_deltas(engine, d))
    return meta


def serving_chain_keys(ckpt_dir: str) -> int:
    """An upper bound of the keys a frozen engine holds after loading the
    version: the full base's kept keys plus every delta's entries."""
    return sum(serving_counts(p)[1] for d in serving_chain(ckpt_dir) for p in serving_files(d))


LATEST = "LATEST"


def version_dir(root: str, epoch: int) -> str:
    return os.path.join(root, "epoch-%06d" % epoch)


def publish(root: str, epoch: int, keep: int = 2) -> None:
    """Rank 0, after every rank saved the epoch's shards: point LATEST at the
    version atomically and drop all but the newest ``keep`` versions -- and
    the versions those are deltas on (``chain``)."""
    tmp = os.path.join(root, LATEST + ".tmp")
    with open(tmp, "w") as f:
        f.write(os.path.basename(version_dir(root, epoch)) + "\n")
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, os.path.join(root, LATEST))
    _fsync_dir(root)
    vers = [d for d in sorted(glob.glob(os.path.join(root, "epoch-*"))) if not _serving_dir(d)]
    needed = set()
    for d in vers[-keep:]:  # the kept versions and every link of their chains
        try:
            needed.update(chain(d))
        except (OSError, ValueError):
            needed.add(_tip(d))
    for d in vers[:-keep]:
        if _tip(d) not in needed:
            shutil.rmtree(d, ignore_errors=True)


def publish_serving(root: str, epoch: int, keep: int = 2) -> None:
    """``publish`` for a root of serving versions: point LATEST at the
    version and drop all but the newest ``keep`` serving versions -- and the
    versions those are deltas on (``serving_chain``)."""
    tmp = os.path.join(root, LATEST + ".tmp")
    with open(tmp, "w") as f:
        f.write(os.path.basename(version_dir(root, epoch)) + "\n")
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, os.path.join(root, LATEST))
    _fsync_dir(root)
    vers = [d for d in sorted(glob.glob(os.path.join(root, "epoch-*"))) if _serving_dir(d)]
    needed = set()
    for d in vers[-keep:]:
        try:
            needed.update(serving_chain(d))
        except (OSError, ValueError):
            needed.add(_tip(d))
    for d in vers[:-keep]:
        if _tip(d) not in needed:
            shutil.rmtree(d, ignore_errors=True)


def latest(root: str) -> Optional[str]:
    """Directory of the newest complete versioned checkpoint under root, or None."""
    p = os.path.join(root, LATEST)
    if not os.path.exists(p):
        return None
    with open(p) as f:
        d = os.path.join(root, f.read().strip())
    return d if os.path.exists(os.path.join(d, "meta.json")) else None
