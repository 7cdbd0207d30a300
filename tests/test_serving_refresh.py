"""Serving deltas on disk and in service (docs/DESIGN.md §2): the trainer's
--serving-every chain (full / delta pattern, retention, a missing link), the
chain next to a --save-delta checkpoint chain written from the same filter,
and Predictor.refresh() -- against predictors opened fresh, and racing a
request."""
import json
import os
import shutil
import threading

import numpy as np
import pytest
import torch

from conftest import DATA

from xflow_amd import checkpoint
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig, TrainConfig
from xflow_amd.engine import Engine
from xflow_amd.serve import Predictor

CPU = torch.device("cpu")
TRAIN, TEST = os.path.join(DATA, "small_train"), os.path.join(DATA, "small_test")
TEXT = open(TEST + "-00000", "rb").read()


def _trainer(tmp_path, sroot, ck=None, metrics="", serving_every=1, full_every=3, save_every=1,
             **kw):
    from xflow_amd.trainer import Trainer

    cfg = TrainConfig(train_prefix=TRAIN, test_prefix=TEST, epochs=5, threads=8,
                      pred_dir=str(tmp_path), write_pred=False, init_push=False,
                      save_serving=str(sroot), serving_every=serving_every,
                      serving_full_every=full_every, metrics_file=metrics,
                      resume_dir=str(ck) if ck else "", save_every=save_every if ck else 0,
                      model=ModelConfig(kind="lr"), optim=OptimConfig(lambda1=2e-3),
                      engine=EngineConfig(table_log2_cap=14, delta_log2=20), **kw)
    return Trainer(cfg, device=CPU)


def _ver(root, ep):
    return checkpoint.version_dir(str(root), ep)


def _sorted(k, w):
    o = np.argsort(k)
    return k[o], np.ascontiguousarray(w, np.float32).view(np.uint32).reshape(len(k), -1)[o]


def _weights_of(eng):
    return _sorted(*eng.export_weights())


def _frozen_table(eng):
    k, w = eng.export_table()
    return _sorted(k, w.view(np.float32).reshape(len(k), -1)[:, :eng.params_per_key])


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _bits(p):
    return np.ascontiguousarray(p, np.float32).view(np.uint32)


def test_trainer_chain_and_refresh(tmp_path):
    sroot, mf = tmp_path / "serving", str(tmp_path / "m.jsonl")
    t = _trainer(tmp_path, sroot, metrics=mf)
    kinds, modes, pred = [], [], None
    try:
        for ep in range(1, 6):
            t.train_epochs(1)
            tip = checkpoint.latest(str(sroot))
            assert os.path.abspath(tip) == os.path.abspath(_ver(sroot, ep))
            meta = checkpoint.load_meta(tip)
            assert checkpoint.is_serving(meta) and meta["epoch"] == ep
            kinds.append("delta" if "delta_base" in meta else "full")
            # the tip loads to what the training table exports at this epoch
            fresh = Predictor(tip, device=CPU, max_rows=256)
            assert fresh.engine.table_size() == fresh.keys
            _same(_frozen_table(fresh.engine), _weights_of(t.table))
            if pred is None:
                pred = Predictor(str(sroot), device=CPU, max_rows=256)
                assert pred.refresh()["mode"] == "none"
                continue
            r = pred.refresh()
            modes.append(r["mode"])
            assert r["version"] == os.path.basename(tip) and r["seconds"] > 0
            assert pred.keys == fresh.keys and os.path.abspath(pred.ckpt) == os.path.abspath(tip)
            if r["mode"] == "delta":
                assert r["inserted"] + r["overwritten"] == meta["keys_delta"] > 0
            _same(_frozen_table(pred.engine), _frozen_table(fresh.engine))
            a, b = pred.predict_libffm(TEXT), fresh.predict_libffm(TEXT)
            assert len(a) > 0 and np.array_equal(_bits(a), _bits(b))
            again = pred.refresh()
            assert again["mode"] == "none" and again["version"] == r["version"]
    finally:
        t.close()
    assert kinds == ["full", "delta", "delta", "full", "delta"]
    assert modes == ["delta", "delta", "full", "delta"]
    eps = [json.loads(x) for x in open(mf)]
    assert [r["serving_kind"] for r in eps if r.get("event") == "epoch"] == kinds
    # retention kept tips 4 and 5: a full version and its delta
    assert sorted(os.listdir(sroot)) == ["LATEST", "epoch-000004", "epoch-000005"]
    assert os.path.exists(os.path.join(_ver(sroot, 4), checkpoint.serving_name(0, 1)))
    assert os.path.exists(os.path.join(_ver(sroot, 5), checkpoint.serving_delta_name(0, 1)))
    assert [os.path.basename(d) for d in checkpoint.serving_chain(_ver(sroot, 5))] == \
        ["epoch-000004", "epoch-000005"]
    shutil.rmtree(_ver(sroot, 4))
    with pytest.raises(FileNotFoundError, match="epoch-000004"):
        checkpoint.serving_chain(_ver(sroot, 5))
    with pytest.raises(FileNotFoundError, match="epoch-000004"):
        Predictor(str(sroot), device=CPU, max_rows=256)


def test_retention_keeps_needed_bases(tmp_path):
    """keep=2 of a chain full, delta, delta: the full base stays while a kept
    version needs it."""
    sroot = tmp_path / "serving"
    t = _trainer(tmp_path, sroot, full_every=8)
    try:
        t.train_epochs(3)
    finally:
        t.close()
    assert sorted(os.listdir(sroot)) == ["LATEST", "epoch-000001", "epoch-000002", "epoch-000003"]
    assert len(checkpoint.serving_chain(_ver(sroot, 3))) == 3


CHAIN = ["full", "delta", "delta", "full", "delta"]


@pytest.mark.parametrize("serving_every,save_every,sv_want,ck_want", [
    (1, 1, CHAIN, CHAIN),
    # a checkpoint's clear at epoch 3 passed the serving base: full again
    (2, 1, ["full", "full"], CHAIN),
    # the serving writer clears alone at the odd epochs: the checkpoint is full
    (1, 2, CHAIN, ["full", "full"])])
def test_two_chains_share_the_filter(tmp_path, serving_every, save_every, sv_want, ck_want):
    """--save-delta and --serving-every together: both chains load to the
    training table at every version -- neither lost keys to the other's clear
    (written at the same point they share one clear; a version whose base the
    other chain's clear has passed is written in full)."""
    sroot, ck = tmp_path / "serving", tmp_path / "ck"
    t = _trainer(tmp_path, sroot, ck=ck, save_delta=True, delta_full_every=3,
                 serving_every=serving_every, full_every=3, save_every=save_every)
    ck_kinds, sv_kinds = [], []
    try:
        for ep in range(1, 6):
            t.train_epochs(1)
            if ep % save_every == 0:
                tip = checkpoint.latest(str(ck))
                assert os.path.basename(tip) == "epoch-%06d" % ep
                ck_kinds.append("delta" if "delta_base" in checkpoint.load_meta(tip) else "full")
                e = Engine(t.table.model, t.table.optim, EngineConfig(table_log2_cap=14))
                checkpoint.load(e, tip, 0, 1)
                _same(_sorted(*e.export_table()), _sorted(*t.table.export_table()))
            if ep % serving_every == 0:
                tip = checkpoint.latest(str(sroot))
                assert os.path.basename(tip) == "epoch-%06d" % ep
                sv_kinds.append("delta" if "delta_base" in checkpoint.load_meta(tip) else "full")
                p = Predictor(tip, device=CPU, max_rows=256)
                _same(_frozen_table(p.engine), _weights_of(t.table))
    finally:
        t.close()
    assert (sv_kinds, ck_kinds) == (sv_want, ck_want)


def test_refresh_races_a_request(tmp_path):
    sroot = tmp_path / "serving"
    t = _trainer(tmp_path, sroot, full_every=8)
    try:
        t.train_epochs(3)
    finally:
        t.close()
    old, new = Predictor(_ver(sroot, 1), device=CPU, max_rows=64), \
        Predictor(_ver(sroot, 3), device=CPU, max_rows=64)
    a, b = _bits(old.predict_libffm(TEXT)), _bits(new.predict_libffm(TEXT))
    assert not np.array_equal(a, b)
    checkpoint.publish_serving(str(sroot), 1, keep=99)
    pred = Predictor(str(sroot), device=CPU, max_rows=64)
    assert os.path.basename(pred.ckpt) == "epoch-000001"
    checkpoint.publish_serving(str(sroot), 3, keep=99)
    got, started, stop = [], threading.Event(), threading.Event()

    def requests():
        while not stop.is_set():
            got.append(_bits(pred.predict_libffm(TEXT)))
            started.set()

    th = threading.Thread(target=requests)
    th.start()
    try:
        started.wait()
        r = pred.refresh()  # (two delta versions, each applied under the lock)
        n = len(got)
        while len(got) < n + 2 and th.is_alive():
            pass
    finally:
        stop.set()
        th.join()
    assert r["mode"] == "delta" and r["version"] == "epoch-000003"
    mid = _bits(Predictor(_ver(sroot, 2), device=CPU, max_rows=64).predict_libffm(TEXT))
    # one version or another whole, never a mix -- max_rows=64 scores the
    # file in several batches, all under one hold of the lock
    assert all(any(np.array_equal(g, v) for v in (a, mid, b)) for g in got)
    assert np.array_equal(got[0], a) and np.array_equal(got[-1], b)


def test_cli_flags():
    from xflow_amd.cli import build_parser, config_from_args

    args = [TRAIN, TEST, "0", "3", "--cpu"]
    cfg = config_from_args(build_parser().parse_args(
        args + ["--save-serving", "s", "--serving-every", "2", "--serving-full-every", "4"]))
    assert cfg.serving_every == 2 and cfg.serving_full_every == 4 and cfg.engine.delta_track
    off = config_from_args(build_parser().parse_args(args))
    assert off.serving_every == 0 and not off.engine.delta_track
    from xflow_amd.trainer import Trainer

    with pytest.raises(ValueError, match="--save-serving"):
        Trainer(TrainConfig(train_prefix=TRAIN, test_prefix=TEST, serving_every=1), device=CPU)
