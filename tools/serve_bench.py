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

--rank measures candidate ranking instead of the three columns (docs/DESIGN.md
§2): on the snapshot's engine (default windows) ``rank_step`` -- contexts of
--rank-ctx fields, candidates of the remaining ones -- against ``eval_step`` on
the same rows expanded to --fields keys, timed with device events in
alternating blocks; then ``Predictor.rank_keys`` against ``predict_keys`` from
host lists, wall clock with the upload.  --rank --top-k K[,K..] measures the
selection of the best K instead: ``rank_topk`` on the device against
``rank_step``, the download of every score and a vectorised selection on the
host in the same order (what a caller does without ``topk_step``), from device
batches and from host lists, in alternating blocks.  --rank --cross SPEC
(3x30,1x2) trains and exports with those feature crosses and measures crossed
ranking: ``rank_step(crosses=...)`` against ``cross_batch`` + ``eval_step`` on
the expanded rows of the same engine, with the uncrossed ``rank_step`` as the
floor, then ``Predictor.rank_keys`` with ``rank_cross`` on and off.

--pool measures candidate pools (docs/DESIGN.md §2): R contexts of --rank-ctx
fields against a resident pool of N candidates of the remaining fields --
``pool_rows`` on the pool (once per model version), then per call ``pool_rows``
on the contexts + ``pool_score``, the top K (--top-k, 100) by the fused
``pool_topk`` kernel and by ``pool_score`` + ``topk_step`` (a line for 2048
requests on a million candidates, fused alone, and one for a pool sorted
ascending, its worst case), and
``pool_score`` alone with its store bandwidth -- against the only other way to
serve the shape, ``rank_step`` on the pool's rows repeated once per request
(where those R x N rows stay under --pool-expand-rows).  --pool --pool-subset
L[,L..] measures ``pool_subset`` instead: R requests with L random pool indices
each, against ``rank_step`` on the gathered rows, ``pool_score`` over the whole
pool, and itself with the staged gather off.  With --top-k K[,K..] a second
table follows (--topk-ab-only: it alone): ``pool_subset_topk`` at every K, the
fused kernel / the composed path of an engine pair that differs in
``pool_subset_topk_fused`` alone, and the composition with torch ops it replaced.

    python tools/serve_bench.py [--model fm --v-dim 8] [--out profiles/serve.txt]
    python tools/serve_bench.py --pool [--model fm --v-dim 32 --fm-math standard]
    python tools/serve_bench.py --rank [--model fm --fm-math standard] [--out profiles/rank.txt]
    python tools/serve_bench.py --rank --top-k 10,100 [--out profiles/rank_topk.txt]
    python tools/serve_bench.py --rank --cross 3x30,5x7 [--out profiles/rank_cross.txt]
"""
from __future__ import annotations

import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xflow_amd import checkpoint  # noqa: E402
from xflow_amd.config import EngineConfig, ModelConfig, OptimConfig, parse_crosses  # noqa: E402
from xflow_amd.data.synth import SynthConfig, SyntheticCriteo  # noqa: E402
from xflow_amd.engine import Batch, Engine  # noqa: E402
from xflow_amd.serve import Predictor  # noqa: E402


def dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def trained(a, dev, model, log2_cap, load=None, optim=None, crosses=()):
    eng = Engine(model, optim or OptimConfig(),
                 EngineConfig(table_log2_cap=log2_cap, max_rows=a.batch,
                              max_nnz=a.batch * (a.fields + len(crosses)), table_grow=False),
                 device=dev)
    synth = SynthConfig(total_features=a.features, hash_space=a.features, seed=a.seed,
                        n_fields=a.fields)
    gen = SyntheticCriteo(eng, a.batch, synth)
    eng.prefill(int((a.table_load if load is None else load) * 2 ** log2_cap))
    b = gen.alloc_batch() if crosses else None
    for _ in range(a.steps):
        if crosses:  # (a field's id is its position in the row)
            eng.train_step(eng.cross_batch(gen.next(out=b), crosses))
        else:
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


def rank_section(a, dev, snap_dir, synth, say):
    """rank_step against eval_step on the expanded rows, one engine."""
    p, _, _ = loaded(snap_dir, dev, a)
    e, C, F = p.engine, a.rank_ctx, a.fields
    assert e.ranks and 0 < C < F
    say("# ms per call, median of %d alternating blocks of device-event time (batches on the "
        "device) | the blocks; then host lists to scores, wall clock" % a.blocks)
    say("requests candidates rank_step eval_step_expanded ratio | blocks | "
        "rank_keys_ms predict_keys_ms")
    for R, per in ((1, 64), (1, 256), (1, 4096), (1, 65536), (256, 16)):
        rows = R * per
        if rows > a.batch:
            continue
        gen = SyntheticCriteo(e, rows, synth)
        b = gen.alloc_batch()
        gen.next(out=b)
        keys = (b.keys.view(F, rows).t() if b.field_major else b.keys.view(rows, F)).contiguous()
        first = torch.arange(R, device=dev) * per  # a request's context: its first row's
        ctx = keys[first, :C].contiguous()
        # (both batches field-major, the layout the one-lane-per-row kernels favour)
        fm = lambda k: Batch(keys=k.t().contiguous().view(-1), labels=b.labels,
                             nnz_per_row=k.shape[1], field_major=True)
        full = fm(torch.cat([ctx.repeat_interleave(per, 0), keys[:, C:]], 1))
        cand = fm(keys[:, C:])
        cptr = (torch.arange(R + 1, device=dev) * C).to(torch.int32)
        rptr = (torch.arange(R + 1, device=dev) * per).to(torch.int32)
        out = torch.empty(rows, dtype=torch.float32, device=dev)
        calls = (lambda: e.rank_step(ctx.view(-1), cptr, rptr, cand, out),
                 lambda: e.eval_step(full, out))
        reps = 200 if rows <= 4096 else 50
        times = [[], []]
        for blk in range(a.blocks + 1):  # (block 0: warm-up)
            for i, f in enumerate(calls):
                t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                t0.record()
                for _ in range(reps):
                    f()
                t1.record()
                torch.cuda.synchronize(dev)
                if blk:
                    times[i].append(t0.elapsed_time(t1) / reps)
        lc, lk = ctx.cpu().tolist(), keys[:, C:].cpu().tolist()
        host = (lambda: p.rank_keys(lc, [lk[q * per:(q + 1) * per] for q in range(R)]),
                lambda: p.predict_keys([lc[r // per] + lk[r] for r in range(rows)]))
        wall = [[], []]
        for blk in range(4):
            for i, f in enumerate(host):
                t0 = time.perf_counter()
                f()
                if blk:
                    wall[i].append(1000.0 * (time.perf_counter() - t0))
        m = [median(t) for t in times]
        say("%d %d %.4f %.4f %.2f | %s | %.2f %.2f"
            % (R, per, m[0], m[1], m[1] / m[0],
               " ; ".join(" ".join("%.4f" % x for x in t) for t in times),
               median(wall[0]), median(wall[1])))


def timed_blocks(calls, reps, blocks, dev):
    """ms per call of each of `calls`, device-event time, in alternating
    blocks of `reps` calls (block 0: warm-up)."""
    times = [[] for _ in calls]
    for blk in range(blocks + 1):
        for i, f in enumerate(calls):
            t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            t0.record()
            for _ in range(reps):
                f()
            t1.record()
            torch.cuda.synchronize(dev)
            if blk:
                times[i].append(t0.elapsed_time(t1) / reps)
    return times


def rank_cross_section(a, dev, snap_dir, synth, say):
    """Crossed ranking: the crosses built inside the rank kernel against the
    rows expanded on the device, crossed by cross_batch and scored by
    eval_step, one engine; then from host lists with rank_cross on and off
    (off: the rows are expanded on the host and uploaded)."""
    p, _, _ = loaded(snap_dir, dev, a)
    off, _, _ = loaded(snap_dir, dev, a, rank_cross=False)
    e, C, F, X = p.engine, a.rank_ctx, a.fields, p.crosses
    assert e.ranks and 0 < C < F and X == a.cross
    say("# crosses %s: %d of %d take every field from the context"
        % (a.cross, sum(max(c) < C for c in X), len(X)))
    say("# ms per call, median of %d alternating blocks of device-event time (batches on the "
        "device): rank_step with crosses, cross_batch + eval_step on the expanded rows, "
        "rank_step without crosses (the floor: other scores) | the blocks; then host lists to "
        "scores, wall clock, Predictor.rank_keys with rank_cross on and off" % a.blocks)
    say("requests candidates rank_cross expand_cross_eval ratio rank_uncrossed | blocks | "
        "rank_keys_on_ms rank_keys_off_ms")
    for R, per in ((1, 64), (1, 256), (1, 4096), (1, 65536), (256, 16)):
        rows = R * per
        if rows > a.batch:
            continue
        gen = SyntheticCriteo(e, rows, synth)
        b = gen.alloc_batch()
        gen.next(out=b)
        keys = (b.keys.view(F, rows).t() if b.field_major else b.keys.view(rows, F)).contiguous()
        ctx = keys[torch.arange(R, device=dev) * per, :C].contiguous()
        fm = lambda k, **kw: Batch(keys=k.t().contiguous().view(-1), labels=b.labels,
                                   nnz_per_row=k.shape[1], field_major=True, **kw)
        full = fm(torch.cat([ctx.repeat_interleave(per, 0), keys[:, C:]], 1))
        ids = torch.arange(F, dtype=torch.int32, device=dev)
        cand = fm(keys[:, C:], fgid=ids[C:].repeat_interleave(rows))
        cfg = ids[:C].repeat(R)
        cptr = (torch.arange(R + 1, device=dev) * C).to(torch.int32)
        rptr = (torch.arange(R + 1, device=dev) * per).to(torch.int32)
        out = torch.empty(rows, dtype=torch.float32, device=dev)
        calls = (lambda: e.rank_step(ctx.view(-1), cptr, rptr, cand, out, ctx_fgid=cfg, crosses=X),
                 lambda: e.eval_step(e.cross_batch(full, X), out),
                 lambda: e.rank_step(ctx.view(-1), cptr, rptr, cand, out))
        want = calls[1]().clone()  # (the two routes score the same rows)
        assert (calls[0]() - want).abs().max().item() < 1e-5
        times = timed_blocks(calls, 200 if rows <= 4096 else 50, a.blocks, dev)
        lc, lk = ctx.cpu().tolist(), keys[:, C:].cpu().tolist()
        lists = (lc, [lk[q * per:(q + 1) * per] for q in range(R)],
                 [list(range(C))] * R, [[list(range(C, F))] * per] * R)
        wall = [[], []]
        for blk in range(4):
            for i, q in enumerate((p, off)):
                t0 = time.perf_counter()
                q.rank_keys(*lists)
                if blk:
                    wall[i].append(1000.0 * (time.perf_counter() - t0))
        m = [median(t) for t in times]
        say("%d %d %.4f %.4f %.2f %.4f | %s | %.2f %.2f"
            % (R, per, m[0], m[1], m[1] / m[0], m[2],
               " ; ".join(" ".join("%.4f" % x for x in t) for t in times),
               median(wall[0]), median(wall[1])))


def host_select(p, R, per, k):
    """The best k of R requests of `per` scores each on the host, in
    topk_step's order: what a caller of rank_step does without it (one
    vectorised partition and sort of sort key << 32 | ~index)."""
    skey = np.where(p > 0, p, 0).astype(np.float32).view(np.uint32).astype(np.uint64)
    key = (skey.reshape(R, per) << np.uint64(32)) | (~np.arange(per, dtype=np.uint32)).astype(np.uint64)
    n = min(k, per)
    if n < per:
        key = np.partition(key, per - n, axis=1)[:, per - n:]
    idx = (~np.sort(key, axis=1)[:, ::-1].astype(np.uint32)).astype(np.int32)  # (the low words)
    return idx, np.take_along_axis(p.reshape(R, per), idx, 1)


def topk_section(a, dev, snap_dir, synth, say):
    """rank_topk (selection on the device) against rank_step, download and
    host_select -- the same answer, as a caller gets it without topk_step."""
    p, _, _ = loaded(snap_dir, dev, a)
    e, C, F = p.engine, a.rank_ctx, a.fields
    say("# top-k: ms per call, medians of %d alternating blocks.  device: event time of rank_step "
        "alone and of rank_topk (rank_step + topk_step), batches on the device.  to_host: wall "
        "clock from the same device batches to numpy results, rank_topk + download of the pairs "
        "against rank_step + download of the scores + host_select.  lists: wall clock from host "
        "lists, Predictor.rank_keys(top_k=k) against rank_keys() + host_select" % a.blocks)
    say("requests candidates k | device: rank_step rank_topk | to_host: topk download_select ratio "
        "| lists: rank_keys_topk rank_keys_select")
    for R, per in ((1, 64), (1, 256), (1, 4096), (1, 65536), (256, 16)):
        rows = R * per
        if rows > a.batch:
            continue
        gen = SyntheticCriteo(e, rows, synth)
        b = gen.alloc_batch()
        gen.next(out=b)
        keys = (b.keys.view(F, rows).t() if b.field_major else b.keys.view(rows, F)).contiguous()
        ctx = keys[torch.arange(R, device=dev) * per, :C].contiguous()
        cand = Batch(keys=keys[:, C:].t().contiguous().view(-1), labels=b.labels,
                     nnz_per_row=F - C, field_major=True)
        cptr = (torch.arange(R + 1, device=dev) * C).to(torch.int32)
        rptr = (torch.arange(R + 1, device=dev) * per).to(torch.int32)
        lc, lk = ctx.cpu().tolist(), keys[:, C:].cpu().tolist()
        lcand = [lk[q * per:(q + 1) * per] for q in range(R)]
        reps = 200 if rows <= 4096 else 50
        for k in a.top_k:
            def to_host_topk():
                i, s = e.rank_topk(ctx.view(-1), cptr, rptr, cand, k)
                return i.cpu().numpy(), s.cpu().numpy()

            def to_host_select():
                return host_select(e.rank_step(ctx.view(-1), cptr, rptr, cand).cpu().numpy(), R, per, k)

            def lists_select():
                return host_select(np.concatenate(p.rank_keys(lc, lcand)), R, per, k)

            got, want = to_host_topk(), to_host_select()  # (the two ways agree, bit for bit)
            n = min(k, per)
            assert np.array_equal(got[0][:, :n], want[0]) and \
                np.array_equal(got[1][:, :n].view(np.uint32), want[1].view(np.uint32))
            dev_calls = (lambda: e.rank_step(ctx.view(-1), cptr, rptr, cand),
                         lambda: e.rank_topk(ctx.view(-1), cptr, rptr, cand, k))
            wall_calls = (to_host_topk, to_host_select, lambda: p.rank_keys(lc, lcand, top_k=k),
                          lists_select)
            times, wall = [[], []], [[], [], [], []]
            for blk in range(a.blocks + 1):  # (block 0: warm-up)
                for i, f in enumerate(dev_calls):
                    t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                    t0.record()
                    for _ in range(reps):
                        f()
                    t1.record()
                    torch.cuda.synchronize(dev)
                    if blk:
                        times[i].append(t0.elapsed_time(t1) / reps)
                for i, f in enumerate(wall_calls):
                    n_rep = max(1, reps // 10) if i < 2 else 1
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for _ in range(n_rep):
                        f()
                    if blk:
                        wall[i].append(1000.0 * (time.perf_counter() - t0) / n_rep)
            m, w = [median(t) for t in times], [median(t) for t in wall]
            say("%d %d %d | %.4f %.4f | %.4f %.4f %.2f | %.2f %.2f"
                % (R, per, k, m[0], m[1], w[0], w[1], w[1] / w[0], w[2], w[3]))


def pool_section(a, dev, snap_dir, synth, say):
    """Candidate pools against rank_step on the repeated rows, one engine."""
    p, _, _ = loaded(snap_dir, dev, a, pool_topk_fused_min=0)  # (the kernel at every size)
    e, C, F = p.engine, a.rank_ctx, a.fields
    K = a.top_k[0] if a.top_k else 100
    assert e.pools and e.ranks and 0 < C < F and e.pool_topk_fused
    say("# ms per call, medians of %d alternating blocks of device-event time, everything on the "
        "device.  pool_build: pool_rows on the N candidates (once per model version).  score: "
        "pool_rows on the R contexts + pool_score.  topk_fused: pool_rows on the contexts + "
        "pool_topk on the fused kernel; topk_composed: score + topk_step; both K = %d, the same "
        "arrays.  gemm: pool_score alone, and its R*N*4 bytes of stores per second.  rank_step: "
        "the pool's rows repeated once per request (R*N rows of %d keys; 'does not fit': more "
        "than %d rows)" % (a.blocks, K, F - C, a.pool_expand_rows))
    say("requests candidates pool_build score topk_fused topk_composed gemm gemm_GB/s "
        "rank_step_repeated rank_step/score")
    gen = SyntheticCriteo(e, a.batch, synth)
    b = gen.alloc_batch()

    def rows_of(n):  # n rows of F keys, a batch at a time
        parts = []
        while sum(len(x) for x in parts) < n:
            gen.next(out=b)
            parts.append((b.keys.view(F, a.batch).t() if b.field_major
                          else b.keys.view(a.batch, F)).clone())
        return torch.cat(parts)[:n]

    fm = lambda k: Batch(keys=k.t().contiguous().view(-1),
                         labels=torch.zeros(k.shape[0], device=dev), nnz_per_row=k.shape[1],
                         field_major=True)
    for N in (4096, 65536, 1048576):
        cand_keys = rows_of(N)[:, C:].contiguous()
        pool = fm(cand_keys)
        pv = e.pool_rows(pool)
        build = median(timed_blocks((lambda: e.pool_rows(pool, out=pv),), 20, a.blocks, dev)[0])
        for R in (1, 32, 256):
            ctx_keys = rows_of(R)[:, :C].contiguous()
            ctx = Batch(keys=ctx_keys.view(-1), labels=torch.zeros(R, device=dev), nnz_per_row=C)
            cv, out = e.pool_rows(ctx), torch.empty((R, N), dtype=torch.float32, device=dev)
            rptr = (torch.arange(R + 1, device=dev) * N).to(torch.int32)

            def score():
                e.pool_rows(ctx, out=cv)
                return e.pool_score(cv, pv, out)

            def fused(vecs=pv):
                e.pool_rows(ctx, out=cv)
                return e.pool_topk(cv, vecs, K)

            calls = [score, lambda: e.topk_step(score().view(-1), rptr, K),
                     lambda: e.pool_score(cv, pv, out), fused]
            for x, y in zip(calls[1](), fused()):  # (the two paths agree, bit for bit)
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))
            fits = R * N <= a.pool_expand_rows
            if fits:
                rep = fm(cand_keys.repeat(R, 1))
                cptr = (torch.arange(R + 1, device=dev) * C).to(torch.int32)
                flat = out.view(-1)
                calls.append(lambda: e.rank_step(ctx_keys.view(-1), cptr, rptr, rep, flat))
                want = calls[4]().clone()  # (the two routes score the same rows)
                assert (score().view(-1) - want).abs().max().item() < 1e-5
            reps = 200 if R * N <= 1 << 20 else (20 if R * N <= 1 << 25 else 5)
            m = [median(t) for t in timed_blocks(calls, reps, a.blocks, dev)]
            say("%d %d %.4f %.4f %.4f %.4f %.4f %.0f %s"
                % (R, N, build, m[0], m[3], m[1], m[2], R * N * 4 / m[2] / 1e6,
                   "%.4f %.2f" % (m[4], m[4] / m[0]) if fits else "does not fit -"))
            del calls, out
            if fits:
                del rep, flat, want
            torch.cuda.empty_cache()
            if (R, N) == (32, 1048576):  # every score survives its filter: the fused path's worst case
                asc = pv[pv[:, 0].argsort()].contiguous()
                t = median(timed_blocks((lambda: fused(asc),), reps, a.blocks, dev)[0])
                say("# %d %d, the pool sorted ascending by c (LR: by score), fused: %.4f" % (R, N, t))
                del asc
        if N == 1048576:  # R * N >= 2^31: the fused path alone
            R = 2048
            ctx_keys = rows_of(R)[:, :C].contiguous()
            ctx = Batch(keys=ctx_keys.view(-1), labels=torch.zeros(R, device=dev), nnz_per_row=C)
            cv = e.pool_rows(ctx)
            t = median(timed_blocks((lambda: e.pool_topk(e.pool_rows(ctx, out=cv), pv, K),), 5,
                                    a.blocks, dev)[0])
            say("%d %d %.4f - %.4f - - - does not fit -" % (R, N, build, t))


def pool_subset_section(a, dev, snap_dir, synth, say):
    """Every request against its own --pool-subset candidates of a resident
    pool: pool_subset against rank_step on the gathered rows and against
    pool_score over the whole pool, one engine."""
    p, _, _ = loaded(snap_dir, dev, a)
    e, C, F, K = p.engine, a.rank_ctx, a.fields, (a.top_k[0] if a.top_k else 100)
    assert e.pools and e.ranks and 0 < C < F
    wide = e.pool_width > 4
    # (pool_subset never reads the table: empty engines serve the two forced settings)
    st, d = (Engine(p.model, p.optim, EngineConfig(table_log2_cap=16, max_rows=16, max_nnz=1024,
                                                   pool_subset_stage=on), device=dev)
             for on in (True, False))
    say("# ms per call, medians of %d alternating blocks of device-event time, everything on the "
        "device; every request has its own L random pool indices.  subset: pool_rows on the R "
        "contexts + pool_subset.  rank_step: the R*L gathered candidate rows of %d keys, the "
        "gather untimed.  whole_pool: pool_rows on the contexts + pool_score over all N (R*N < "
        "2^31).  kernel_staged / kernel_direct: pool_subset alone with pool_subset_stage True and "
        "False (the same kernel twice when a vector is one float4; subset runs the default).  subset_topk: subset + "
        "topk_step, K = %d" % (a.blocks, F - C, K))
    say("candidates L requests subset rank_step whole_pool kernel_staged kernel_direct "
        "subset_topk rank_step/subset whole_pool/subset")
    gen = SyntheticCriteo(e, a.batch, synth)
    b = gen.alloc_batch()

    def rows_of(n):  # n rows of F keys, a batch at a time
        parts = []
        while sum(len(x) for x in parts) < n:
            gen.next(out=b)
            parts.append((b.keys.view(F, a.batch).t() if b.field_major
                          else b.keys.view(a.batch, F)).clone())
        return torch.cat(parts)[:n]

    fm = lambda k: Batch(keys=k.t().contiguous().view(-1),
                         labels=torch.zeros(k.shape[0], device=dev), nnz_per_row=k.shape[1],
                         field_major=True)
    for N in (65536, 1048576):
        cand_keys = rows_of(N)[:, C:].contiguous()
        pv = e.pool_rows(fm(cand_keys))
        for L in a.pool_subset:
            for R in (1, 32, 256):
                ctx_keys = rows_of(R)[:, :C].contiguous()
                ctx = Batch(keys=ctx_keys.view(-1), labels=torch.zeros(R, device=dev), nnz_per_row=C)
                cv = e.pool_rows(ctx)
                index = torch.randint(0, N, (R * L,), device=dev, dtype=torch.int32)
                rptr = (torch.arange(R + 1, device=dev) * L).to(torch.int32)
                cptr = (torch.arange(R + 1, device=dev) * C).to(torch.int32)
                out, out2 = (torch.empty(R * L, dtype=torch.float32, device=dev) for _ in range(2))
                rep = fm(cand_keys[index.long()])
                whole = torch.empty((R, N), dtype=torch.float32, device=dev)

                def subset():
                    e.pool_rows(ctx, out=cv)
                    return e.pool_subset(cv, pv, index, rptr, out)

                def whole_pool():
                    e.pool_rows(ctx, out=cv)
                    return e.pool_score(cv, pv, whole)

                calls = [subset, lambda: e.rank_step(ctx_keys.view(-1), cptr, rptr, rep, out2),
                         whole_pool, lambda: st.pool_subset(cv, pv, index, rptr, out),
                         lambda: d.pool_subset(cv, pv, index, rptr, out2),
                         lambda: e.topk_step(subset(), rptr, K)]
                # (the routes score the same rows; the two gathers leave the same bits)
                assert (subset() - calls[1]()).abs().max().item() < 1e-5
                assert torch.equal(calls[4]().view(torch.int32), subset().view(torch.int32))
                rows = whole_pool().view(-1)[index.long() + (torch.arange(R * L, device=dev) // L) * N]
                assert (subset() - rows).abs().max().item() < 1e-5
                reps = 200 if R * L <= 1 << 16 else 50
                m = [median(t) for t in timed_blocks(calls, reps, a.blocks, dev)]
                say("%d %d %d %.4f %.4f %.4f %.4f %s %.4f %.2f %.2f"
                    % (N, L, R, m[0], m[1], m[2], m[3], "%.4f" % m[4] if wide else "-", m[5],
                       m[1] / m[0], m[2] / m[0]))
                del calls, rep, whole, rows
                torch.cuda.empty_cache()
        if wide:  # the two gathers at a size that is throughput, not launch latency
            R, L = 1024, 4096
            cv = pv[:R].contiguous()  # (any vectors do)
            index = torch.randint(0, N, (R * L,), device=dev, dtype=torch.int32)
            rptr = (torch.arange(R + 1, device=dev) * L).to(torch.int32)
            out = torch.empty(R * L, dtype=torch.float32, device=dev)
            m = [median(t) for t in timed_blocks(
                [lambda: st.pool_subset(cv, pv, index, rptr, out),
                 lambda: d.pool_subset(cv, pv, index, rptr, out)], 50, a.blocks, dev)]
            say("# %d %d %d, pool_subset alone, staged / direct: %.4f / %.4f, %.0f / %.0f GB/s of "
                "gathered rows" % (N, L, R, m[0], m[1], R * L * e.pool_width * 4 / m[0] / 1e6,
                                   R * L * e.pool_width * 4 / m[1] / 1e6))


def pool_subset_topk_section(a, dev, snap_dir, synth, say):
    """The best K of every request's own --pool-subset candidates: the fused
    pool_subset_topk kernel against the composed path of the same build, an
    engine pair that differs in EngineConfig.pool_subset_topk_fused alone."""
    p, _, _ = loaded(snap_dir, dev, a)
    e, C, F = p.engine, a.rank_ctx, a.fields
    assert e.pools and 0 < C < F
    # (neither path reads the table: empty engines serve the two settings)
    f, c = (Engine(p.model, p.optim, EngineConfig(table_log2_cap=16, max_rows=16, max_nnz=1024,
                                                  pool_subset_topk_fused=on,
                                                  pool_subset_topk_fused_max=0), device=dev)
            for on in (True, False))
    assert f.pool_subset_topk_fused and not c.pool_subset_topk_fused
    say("# ms per call of Engine.pool_subset_topk alone (the vectors resident), medians of %d "
        "alternating blocks of device-event time; every request has its own L random pool "
        "indices.  fused: one kernel scores a tile of the list into the registers it sorts.  "
        "composed: pool_subset into a score array, topk_step, positions -> pool indices by one "
        "kernel (pool_subset_topk_fused=False).  torch_map: pool_subset, topk_step and the "
        "positions mapped by torch ops, the path before the fused kernel" % a.blocks)
    say("candidates L requests K fused composed torch_map composed/fused torch_map/fused")
    gen = SyntheticCriteo(e, a.batch, synth)
    b = gen.alloc_batch()
    keys = []
    while sum(len(x) for x in keys) < 65536 + 256:
        gen.next(out=b)
        keys.append((b.keys.view(F, a.batch).t() if b.field_major else b.keys.view(a.batch, F)).clone())
    keys = torch.cat(keys)
    N = 65536
    cand = keys[:N, C:].contiguous()
    pv = e.pool_rows(Batch(keys=cand.t().contiguous().view(-1), labels=torch.zeros(N, device=dev),
                           nnz_per_row=F - C, field_major=True))
    for L in a.pool_subset:
        for R in (1, 32, 256):
            cv = e.pool_rows(Batch(keys=keys[N:N + R, :C].contiguous().view(-1),
                                   labels=torch.zeros(R, device=dev), nnz_per_row=C))
            index = torch.randint(0, N, (R * L,), device=dev, dtype=torch.int32)
            rptr = (torch.arange(R + 1, device=dev) * L).to(torch.int32)
            for K in a.top_k:
                def torch_map():
                    pos, sc = c.topk_step(c.pool_subset(cv, pv, index, rptr), rptr, K)
                    at = (pos.clamp(min=0).long() + rptr[:-1, None].long()).clamp(max=R * L - 1)
                    return index[at], sc

                calls = [lambda: f.pool_subset_topk(cv, pv, index, rptr, K),
                         lambda: c.pool_subset_topk(cv, pv, index, rptr, K), torch_map]
                got = [x() for x in calls]
                n = min(K, L)  # (past a request's entries torch_map holds no padding)
                assert all(torch.equal(g[0][:, :n], got[0][0][:, :n]) and
                           torch.equal(g[1].view(torch.int32), got[0][1].view(torch.int32))
                           for g in got[1:])
                reps = 200 if R * L <= 1 << 16 else 50
                m = [median(t) for t in timed_blocks(calls, reps, a.blocks, dev)]
                say("%d %d %d %d %.4f %.4f %.4f %.2f %.2f"
                    % (N, L, R, K, m[0], m[1], m[2], m[1] / m[0], m[2] / m[0]))


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
    ap.add_argument("--rank", action="store_true", help="the candidate ranking section only")
    ap.add_argument("--rank-ctx", type=int, default=26, help="context fields of --fields")
    ap.add_argument("--top-k", type=lambda s: [int(x) for x in s.split(",")], default=[],
                    metavar="K[,K..]", help="with --rank: the top-k section instead, at these k")
    ap.add_argument("--cross", type=parse_crosses, default=[], metavar="SPEC",
                    help="with --rank: train with these feature crosses (3x30,5x7) and measure "
                         "crossed ranking")
    ap.add_argument("--pool", action="store_true", help="the candidate pool section only")
    ap.add_argument("--pool-expand-rows", type=int, default=1 << 25,
                    help="with --pool: rank_step on the repeated rows runs up to this many rows")
    ap.add_argument("--pool-subset", type=lambda s: [int(x) for x in s.split(",")], default=[],
                    metavar="L[,L..]", help="with --pool: every request scores its own L random "
                                            "pool indices (pool_subset) instead")
    ap.add_argument("--topk-ab-only", action="store_true",
                    help="with --pool --pool-subset --top-k: only the fused / composed table")
    ap.add_argument("--tmp", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def done():
        if a.out:  # (only a run that finished writes its table)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return 0

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
        eng, synth = trained(a, dev, model, log2_cap, load, optim, a.cross)
        full_dir, snap_dir = os.path.join(tmp, "full"), os.path.join(tmp, "snap")
        checkpoint.save(eng, full_dir, 0, 1, barrier=lambda: None)
        checkpoint.save_serving(eng, snap_dir, 0, 1, barrier=lambda: None,
                                meta=checkpoint.cross_meta(a.cross, None) or None)
        m = checkpoint.load_meta(snap_dir)
        del eng
        torch.cuda.empty_cache()
        if a.pool:
            if not (a.pool_subset and a.top_k and a.topk_ab_only):
                (pool_subset_section if a.pool_subset else pool_section)(a, dev, snap_dir, synth, say)
            if a.pool_subset and a.top_k:
                pool_subset_topk_section(a, dev, snap_dir, synth, say)
            return done()
        if a.rank:
            section = rank_cross_section if a.cross else (topk_section if a.top_k else rank_section)
            section(a, dev, snap_dir, synth, say)
            return done()
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
    return done()


if __name__ == "__main__":
    sys.exit(main())
