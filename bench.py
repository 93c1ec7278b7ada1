"""bench.py - BASELINE.json metric on MI355X:
   queries/s (embed+top-k, k=5, b=256) over 1M x 768 corpus; p50 single-query ms

One step = one batch of 256 synthetic queries (L = 32 token ids, resident in HBM)
through the 12-layer HIP BERT encoder (K1..K7) and the exact fp32 flat search (K9+K10)
over the corpus (BASELINE config 3; config 2/4 via --corpus-rows / --batch).

Multi-GPU (python -m torch.distributed.run --nproc-per-node N bench.py --gpus N):
the 1M-row corpus is row-sharded over the N ranks; each rank embeds its
own 256 queries (DP), the ranks all-gather query embeddings (RCCL), every rank scans its
shard for all 256*N queries, one RCCL all-gather of per-shard (score, id) candidates,
then a device merge of each rank's own queries.  Per-GPU work is fixed as N grows
(256 encodes + 256 x 1M scored rows): "scaling": "weak"; value = 256*N*steps / time.

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times --steps steps of the
headline arithmetic and prints that figure with the per-kernel times and rooflines read
from those same steps.  --full adds everything else to the line, each a run of its own:
the planted-query parity guard, the other arithmetics, BASELINE configs 2 / 4 / 5, the
single-query latencies, the clustered corpus, the LangChain leg and the CPU baseline (the
oracle restatement timed on this host's cores on a bounded sample).  --dump-outputs DIR
writes what the last timed step returned as DIR/<name>.npy.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(ROOT, "mediquery-rag_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from mediquery_hip import synth  # noqa: E402
from mediquery_hip.config import DMETA_BASE  # noqa: E402
from mediquery_hip.distributed import ShardedSearcher, shard_bounds  # noqa: E402
from mediquery_hip.native import Encoder, FlatIndex  # noqa: E402
from mediquery_hip import _lib  # noqa: E402

# run name -> (encoder arithmetic, search mode).  The headline "f32x6_screen" computes
# fp32-class results: the encoder on the split-f32 GEMMs (every fp32 operand split exactly
# into three bf16 planes, six bf16 MFMAs per product, fp32 accumulation: 24-bit
# significands, the same parity tolerances as fp32; K2p on the pre-split weights), the
# top-k exact fp32 by certified screens (bf16-shadow scan for 64 candidates, fp32 re-rank,
# proven bound per query; uncertified queries re-run on the split-f32 screen or the direct
# exact scan).  Beside it, in the same line: "f32" (the same with the encoder on the exact
# f32 MFMA), the direct exact scan ("f32_direct_search") and the all-split-f32 variant.
PRECISIONS = {"f32": (_lib.MQ_DTYPE_F32, _lib.MQ_DTYPE_F32_SCREEN),
              "f32_direct_search": (_lib.MQ_DTYPE_F32, _lib.MQ_DTYPE_F32),
              "f32x6": (_lib.MQ_DTYPE_F32X6, _lib.MQ_DTYPE_F32X6),
              "f32x6_screen": (_lib.MQ_DTYPE_F32X6, _lib.MQ_DTYPE_F32_SCREEN)}

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP32_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: FP32 matrix (= vector) peak
BF16_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: BF16 dense MFMA peak (spec)


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--corpus-rows", type=int, default=1_000_000)
    p.add_argument("--batch", type=int, default=256, help="queries per GPU per step")
    p.add_argument("--seq-len", type=int, default=32)
    p.add_argument("--k", type=int, default=5)
    p.add_argument("--layers", type=int, default=DMETA_BASE.layers)
    p.add_argument("--single-iters", type=int, default=50, help="single-query latency samples")
    p.add_argument("--secondary-seq-len", type=int, default=128,
                   help="also time the headline step at this L (0 = skip)")
    p.add_argument("--config4-steps", type=int, default=10,
                   help="BASELINE config 4 line (10M x 768 as 8 row shards, batch 1024): timed steps (0 = skip)")
    p.add_argument("--enc-opt", action="append", default=[],
                   help="NAME=VALUE encoder option (Encoder.OPTIONS) for A/B runs; repeatable")
    p.add_argument("--no-extras", action="store_true",
                   help="skip the config-2, clustered-corpus, long-query and k=50 extras")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--cpu-threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "0") or 0))
    p.add_argument("--full", action="store_true",
                   help="also run everything beside the headline: the parity guard, the other arithmetics, "
                        "configs 2 / 4 / 5, single-query latencies, the extras and the CPU baseline")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's outputs (scores, ids, embeddings) as DIR/<name>.npy")
    args = p.parse_args()
    if args.steps < 1 or args.warmup < 0:
        p.error("--steps must be >= 1 and --warmup >= 0")
    return args


def dump_outputs(path, arrays):
    """DIR/<name>.npy of the last timed step's outputs: float32 as computed, the int64 row
    ids as float64 (exact below 2^53).  A few hundred KB at the bench's sizes."""
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        a = a.detach().cpu().numpy()
        np.save(os.path.join(path, name + ".npy"),
                a.astype(np.float32 if a.dtype == np.float32 else np.float64))


def encoder_flops(cfg, B, L):
    return B * cfg.flops_per_sequence(L)


def cpu_baseline(args, cfg, corpus_host_fn):
    """Oracle (torch-CPU restatement) timed on this host: q/s = batch /
    (median of 5 encoder batches + median of 5 fp32 mm/topk batches over the full
    corpus), after one warm-up batch each; p50 single query = median over 100 single
    queries of encoder + search.  BASELINE.md §3's other configs as bounded legs beside
    it (`configs`): config 2 (100k rows) measured whole; config 4 (10M rows, batch 1024)
    and config 5 (1M bf16 rows, k = 50 re-rank) timed on a stated sample and scaled
    linearly in rows / queries (~40 s of CPU work in all)."""
    from oracle.encoder import OracleEncoder
    from oracle.flat import search_fp32_torch
    from mediquery_hip.weights import synthetic_state_dict
    threads = args.cpu_threads or os.cpu_count()
    torch.set_num_threads(threads)
    enc = OracleEncoder(cfg, synthetic_state_dict(cfg, 0))
    ids, mask = synth.token_batch(args.batch, args.seq_len)
    reps, singles = 5, 100
    q = enc.embed(ids, mask)  # warm-up batch
    t_enc = []
    for _ in range(reps):
        t0 = time.perf_counter()
        q = enc.embed(ids, mask)
        t_enc.append(time.perf_counter() - t0)
    c = corpus_host_fn()

    def med_search(qq, cc, k, n):
        search_fp32_torch(qq, cc, k, threads)  # warm-up
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            search_fp32_torch(qq, cc, k, threads)
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    ts = med_search(q, c, args.k, reps)
    lat = []
    for j in range(singles + 2):
        jj = j % args.batch
        t0 = time.perf_counter()
        q1 = enc.embed(ids[jj:jj + 1], mask[jj:jj + 1])
        search_fp32_torch(q1, c, args.k, threads)
        if j >= 2:
            lat.append((time.perf_counter() - t0) * 1e3)
    te = statistics.median(t_enc)
    configs = {}
    # config 2: 100k x 768, batch 256 embed + search (the first 100k rows of the same slab)
    ts2 = med_search(q, c[:100_000], args.k, reps)
    configs["config2"] = {"value": round(args.batch / (te + ts2), 2), "unit": "queries/s",
                          "sample": "whole config: encoder median (above) + median of %d searches of %d "
                                    "queries over 100000 rows (%.4f s)" % (reps, args.batch, ts2)}
    # config 4: 10M rows, batch 1024 - 1024 queries over the slab, scaled in rows; encoder x4
    q4 = np.concatenate([q] * 4)
    ts4 = med_search(q4, c, args.k, 1)
    scale4 = 10_000_000 / c.shape[0]
    configs["config4"] = {"value": round(1024 / (4 * te + scale4 * ts4), 2), "unit": "queries/s",
                          "sample": "1024 queries over the %d-row slab (%.3f s, one timed after a warm-up) "
                                    "scaled x%.0f to 10M rows; encoder = 4 x the 256-query batch median"
                                    % (c.shape[0], ts4, scale4)}
    # config 5: bf16 coarse scan (torch bf16 mm) for 64 candidates + fp32 re-rank -> k = 50,
    # search only (as the GPU line) - on the first 100k rows, scaled x10 to 1M
    c5 = torch.as_tensor(np.asarray(c[:100_000], dtype=np.float32))
    c5b = c5.to(torch.bfloat16)
    qt = torch.as_tensor(np.asarray(q, dtype=np.float32))

    def c5_search():
        _, cand = torch.topk((qt.to(torch.bfloat16) @ c5b.T).float(), 64, dim=1)
        ex = torch.einsum("qd,qkd->qk", qt, c5[cand])
        v, o = torch.topk(ex, 50, dim=1)
        return v, torch.gather(cand, 1, o)

    c5_search()
    t5 = []
    for _ in range(3):
        t0 = time.perf_counter()
        c5_search()
        t5.append(time.perf_counter() - t0)
    ts5 = statistics.median(t5)
    configs["config5"] = {"value": round(args.batch / (10 * ts5), 2), "unit": "queries/s (search only)",
                          "sample": "median of 3: %d queries, torch bf16 mm over 100000 bf16 rows -> top-64 "
                                    "-> fp32 re-rank -> k=50 (%.4f s), scaled x10 to 1M rows"
                                    % (args.batch, ts5)}
    return {"value": round(args.batch / (te + ts), 2), "unit": "queries/s",
            "cores": threads, "kind": "port",
            "p50_single_query_ms": round(statistics.median(lat), 2),
            "configs": configs,
            "sample": ("oracle torch-CPU fp32 on %d threads: median of %d %d-layer BERT encodes of %d "
                       "queries (L=%d) + median of %d fp32 mm+topk batches of %d queries over %d x 768 "
                       "rows (enc %.3f s/batch, search %.3f s/batch); p50 of %d single queries "
                       "(encode + search)" % (threads, reps, cfg.layers, args.batch, args.seq_len, reps,
                                              args.batch, c.shape[0], te, ts, singles))}


C4_ROWS, C4_SHARDS, C4_BATCH = 10_000_000, 8, 1024


def config4(args, enc, world, rank, dev, backend):
    """BASELINE config 4: a 10M x 768 fp32 corpus in 8 row shards of 1.25M, batch 1024
    (global), k = 5.  Rank r of N owns shards [r*8/N, (r+1)*8/N) as `LocalShards` (all 8 on
    one GPU at N = 1), embeds 1024/N of the queries (DP), and the ranks exchange query
    embeddings and the packed per-shard candidates with one all-gather each.  Total work
    is fixed as N grows ("strong").  Returns the rank's record (rank 0's is printed)."""
    from mediquery_hip.distributed import LocalShards
    if C4_SHARDS % world or C4_BATCH % world:
        return None
    spr, per = C4_SHARDS // world, C4_ROWS // C4_SHARDS
    first = rank * spr
    block = torch.empty((spr * per, 768), dtype=torch.float32, device=dev)
    for j in range(spr):
        block[j * per:(j + 1) * per] = synth.corpus_shard_device(per, first + j, 768, dev)
    shards = LocalShards(spr, 768, device=dev.index)
    shards.add_device(block)
    del block
    shards.set_precision(_lib.MQ_DTYPE_F32_SCREEN)
    B = C4_BATCH // world
    K = args.k
    ids_np, mask_np = synth.token_batch(B, args.seq_len, seed=synth.TOKEN_SEED + 100 + rank)
    ids, mask = torch.from_numpy(ids_np).to(dev), torch.from_numpy(mask_np).to(dev)
    q = torch.empty((B, 768), dtype=torch.float32, device=dev)
    s_loc = torch.empty((C4_BATCH, K), dtype=torch.float32, device=dev)
    i_loc = torch.empty((C4_BATCH, K), dtype=torch.int64, device=dev)

    def local(qq, k):
        n = qq.shape[0]
        shards.search_device(qq, k, s_loc[:n], i_loc[:n])
        return s_loc[:n], i_loc[:n]

    searcher = ShardedSearcher(local, first * per)
    # property check at full size: queries planted on shard 0's rows (regenerated on every
    # rank, so the query set is identical everywhere) find their global row ids
    sh0 = synth.corpus_shard_device(per, 0, 768, dev)
    pq, planted = synth.queries_device(64, sh0)
    del sh0
    torch.cuda.empty_cache()
    _, pi = searcher.search(pq, K) if world > 1 else local(pq, K)
    ok = bool((pi[:32, 0] == planted[:32]).all())

    def step(ev=None):
        if ev:
            ev[0].record()
        enc.embed_device(ids, mask, q)
        if ev:
            ev[1].record()
        if world > 1:
            searcher.search_local_batch(q, K, sizes=[B] * world)
        else:
            local(q, K)
        if ev:
            ev[2].record()

    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.config4_steps)]
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    if world > 1:
        searcher.timings = []
    t0 = time.perf_counter()
    for it in range(args.config4_steps):
        step(evs[it])
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    coll = None
    if world > 1:
        coll = {}
        for tag, nbytes, ms in searcher.resolve_timings():
            c = coll.setdefault(tag, {"ms_per_step": 0.0, "bytes_per_rank": nbytes})
            c["ms_per_step"] = round(c["ms_per_step"] + ms / args.config4_steps, 4)
    if world > 1:
        t = torch.tensor([elapsed], device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    fb = sum(ix.screen_fallbacks for ix in shards.shards)
    del shards
    torch.cuda.empty_cache()
    return {"workload": "BASELINE config 4: %d x 768 fp32 corpus as %d row shards of %d (%d per GPU x %d GPU), "
                        "batch %d (global, %d per GPU, L=%d) embed + exact top-%d, one packed candidate "
                        "all-gather%s" % (C4_ROWS, C4_SHARDS, per, spr, world, C4_BATCH, B, args.seq_len, K,
                                          "" if world > 1 else " (none needed: device merge of the 8 shards)"),
            "queries_per_s": round(C4_BATCH * args.config4_steps / elapsed, 1),
            "ms_per_step": round(elapsed / args.config4_steps * 1e3, 3),
            "steps": args.config4_steps, "n_gpus": world, "scaling": "strong",
            "encoder_ms": round(statistics.mean(e[0].elapsed_time(e[1]) for e in evs), 3),
            "search_ms": round(statistics.mean(e[1].elapsed_time(e[2]) for e in evs), 3),
            "planted_top1_ok": ok, "screen_fallbacks": fb, "allgather_rank0": coll}


def _timed_steps(fn, steps, warmup):
    """Wall time of `steps` calls of fn after `warmup` (device synchronised both sides)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def _counters(ix):
    out = {"batch_fallbacks": ix.screen_fallbacks, "passdowns": ix.screen_passdowns}
    try:
        out.update(bf16_tier_skips=ix.screen_skips, int8_tier_skips=ix.int8_skips)
    except AttributeError:  # an older library under A/B (MQ_LIB_ALLOW_MISSING=1)
        out.update(bf16_tier_skips=0, int8_tier_skips=0)
    return out


def config2(args, enc, dev, ids, mask, q):
    """BASELINE config 2: 100k x 768 fp32 corpus, batch 256 (L = 32) embed + exact top-k
    on one GPU, timed like the headline (exact fp32 via the certified screen)."""
    n = 100_000
    ix = FlatIndex(dim=768, capacity=n, device=dev.index)
    ix.add_device(synth.corpus_device(n, 768, dev, seed=synth.CORPUS_SEED + 2))
    ix.set_precision(_lib.MQ_DTYPE_F32_SCREEN)
    B, K = q.shape[0], args.k
    s = torch.empty((B, K), dtype=torch.float32, device=dev)
    i = torch.empty((B, K), dtype=torch.int64, device=dev)

    def step():
        enc.embed_device(ids, mask, q)
        ix.search_device(q, K, s, i)

    t = _timed_steps(step, args.steps, args.warmup)
    t_s = _timed_steps(lambda: ix.search_device(q, K, s, i), args.steps, 2)
    ix.set_precision(_lib.MQ_DTYPE_F32)
    s2, i2 = torch.empty_like(s), torch.empty_like(i)
    ix.search_device(q, K, s2, i2)
    ix.set_precision(_lib.MQ_DTYPE_F32_SCREEN)
    ix.search_device(q, K, s, i)
    torch.cuda.synchronize()
    out = {"workload": "BASELINE config 2: %d x 768 fp32 corpus, batch %d (L=%d) embed + exact top-%d" % (n, B, args.seq_len, K),
           "queries_per_s": round(B / t, 1), "ms_per_step": round(t * 1e3, 3), "steps": args.steps,
           "search_ms": round(t_s * 1e3, 4),
           "ids_equal_direct_exact": bool((i == i2).all()), "counters": _counters(ix)}
    ix.close()
    return out


def exact_k50(index, q, dev):
    """The exact top-50 batch (screened) beside the direct exact scan: the large-k path
    that skips the bf16 tier (r3 paid a 157 ms device fallback here)."""
    B, k = q.shape[0], 50
    s = torch.empty((B, k), dtype=torch.float32, device=dev)
    i = torch.empty((B, k), dtype=torch.int64, device=dev)
    s2, i2 = torch.empty_like(s), torch.empty_like(i)
    c0 = _counters(index)
    index.set_precision(_lib.MQ_DTYPE_F32_SCREEN)
    t_scr = _timed_steps(lambda: index.search_device(q, k, s, i), 10, 2)
    index.set_precision(_lib.MQ_DTYPE_F32)
    t_dir = _timed_steps(lambda: index.search_device(q, k, s2, i2), 10, 2)
    index.set_precision(_lib.MQ_DTYPE_F32_SCREEN)
    c1 = _counters(index)
    return {"batch": B, "k": k, "screened_ms": round(t_scr * 1e3, 3), "direct_ms": round(t_dir * 1e3, 3),
            "ratio": round(t_scr / t_dir, 3), "ids_equal_frac": round(float((i == i2).float().mean()), 6),
            "counters": {kk: c1[kk] - c0[kk] for kk in c1}}


def long_queries(args, enc, index, dev, K):
    """Single-query p50 (embed + screened search) at the advisor path's query lengths
    (200-500 chars, src/ui/interface.py:437-479): L = 128 / 256 / 512 tokens."""
    out = {}
    s = torch.empty((1, K), dtype=torch.float32, device=dev)
    i = torch.empty((1, K), dtype=torch.int64, device=dev)
    q1 = torch.empty((1, 768), dtype=torch.float32, device=dev)
    for L in (128, 256, 512):
        ids_np, mask_np = synth.token_batch(1, L, seed=synth.TOKEN_SEED + L)
        ids1, mask1 = torch.from_numpy(ids_np).to(dev), torch.from_numpy(mask_np).to(dev)
        lat, enc_l = [], []
        for it in range(35):
            torch.cuda.synchronize()
            a = time.perf_counter()
            enc.embed_device(ids1, mask1, q1)
            torch.cuda.synchronize()
            b = time.perf_counter()
            index.search_device(q1, K, s, i)
            torch.cuda.synchronize()
            if it >= 5:
                lat.append((time.perf_counter() - a) * 1e3)
                enc_l.append((b - a) * 1e3)
        out["L%d" % L] = {"p50_ms": round(statistics.median(lat), 3),
                          "encoder_p50_ms": round(statistics.median(enc_l), 3)}
    return out


def clustered(args, enc, dev, ids, mask, q):
    """The headline step where the certificate is stressed (SURVEY.md §8d clustered
    variant: 4096 centroids, sigma 0.35, the reference corpus's duplicate-row pattern):
    (a) the config-3 step (encoder queries), (b) search-only batches of in-distribution
    queries (each a corpus row + noise: its cluster-mates crowd the top scores), (c)
    single in-distribution queries; certificate counters for each, and the direct exact
    scan beside (b) for ids and time."""
    n = args.corpus_rows
    rows, _ = synth.clustered_corpus_device(n, 768, dev)
    ix = FlatIndex(dim=768, capacity=n, device=dev.index)
    ix.add_device(rows)
    B, K = q.shape[0], args.k
    pq, _ = synth.queries_device(B, rows, seed=synth.QUERY_SEED + 11, planted_frac=1.0)
    del rows
    torch.cuda.empty_cache()
    ix.set_precision(_lib.MQ_DTYPE_F32_SCREEN)
    s = torch.empty((B, K), dtype=torch.float32, device=dev)
    i = torch.empty((B, K), dtype=torch.int64, device=dev)

    def step():
        enc.embed_device(ids, mask, q)
        ix.search_device(q, K, s, i)

    c0 = _counters(ix)
    t_step = _timed_steps(step, args.steps, args.warmup)
    c1 = _counters(ix)
    t_pq = _timed_steps(lambda: ix.search_device(pq, K, s, i), args.steps, 2)
    c2 = _counters(ix)
    ix.set_precision(_lib.MQ_DTYPE_F32)
    s2, i2 = torch.empty_like(s), torch.empty_like(i)
    t_dir = _timed_steps(lambda: ix.search_device(pq, K, s2, i2), args.steps, 2)
    ix.set_precision(_lib.MQ_DTYPE_F32_SCREEN)
    ix.search_device(pq, K, s, i)
    torch.cuda.synchronize()
    same = float((i == i2).float().mean())
    lat, lat_e2e = [], []
    s1, i1 = s[:1], i[:1]
    c3 = _counters(ix)
    for j in range(min(B, 100)):
        torch.cuda.synchronize()
        a = time.perf_counter()
        ix.search_device(pq[j:j + 1], K, s1, i1)
        torch.cuda.synchronize()
        lat.append((time.perf_counter() - a) * 1e3)
    # end to end: one query's forward (few-row path) + the in-distribution search
    q1 = q[:1]
    for j in range(min(B, 100)):
        torch.cuda.synchronize()
        a = time.perf_counter()
        enc.embed_device(ids[j:j + 1], mask[j:j + 1], q1)
        ix.search_device(pq[j:j + 1], K, s1, i1)
        torch.cuda.synchronize()
        lat_e2e.append((time.perf_counter() - a) * 1e3)
    c4 = _counters(ix)
    d = lambda x, y: {kk: y[kk] - x[kk] for kk in y}
    ix.close()
    return {"workload": "%d x 768 clustered corpus (4096 centroids, sigma 0.35, reference duplicate-row "
                        "pattern), batch %d, k=%d" % (n, B, K),
            "step_queries_per_s": round(B / t_step, 1), "step_ms": round(t_step * 1e3, 3),
            "step_counters": d(c0, c1),
            "in_distribution_search_ms": round(t_pq * 1e3, 4),
            "in_distribution_direct_search_ms": round(t_dir * 1e3, 4),
            "in_distribution_ids_equal_direct": round(same, 6),
            "in_distribution_counters": d(c1, c2),
            "single_query_search_p50_ms": round(statistics.median(lat), 4),
            "single_query_p50_ms": round(statistics.median(lat_e2e), 4),
            "single_query_counters": d(c3, c4),
            "single_query_note": "%d in-distribution single queries searched alone, then %d more times each "
                                 "after one query's forward (encode + search, end to end); counters over both"
                                 % (min(B, 100), min(B, 100))}


def langchain_embed_documents(args, dev):
    """LangChain-level `embed_documents` (the call `Chroma.from_documents` makes at
    src/ingest_medical.py:106-110) through the drop-in at both arithmetics
    (`HipBertEmbeddings(precision=)`): host strings in (char tokenizer, 30 CJK chars = 32
    tokens), Python float lists out - tokenisation, H2D / D2H and list building included."""
    from mediquery_hip import HipBertEmbeddings
    rng = np.random.default_rng(17)
    texts = ["".join(chr(c) for c in rng.integers(0x4E00, 0x9FA5, 30)) for _ in range(2048)]
    out = {}
    for prec in ("f32", "f32x6"):
        emb = HipBertEmbeddings(synthetic=True, precision=prec, device=dev.index, batch_size=args.batch)
        emb.embed_documents(texts[:args.batch])  # warm-up
        t0 = time.perf_counter()
        vecs = emb.embed_documents(texts)
        dt = time.perf_counter() - t0
        assert len(vecs) == len(texts) and len(vecs[0]) == 768
        out[prec] = {"docs_per_s": round(len(texts) / dt, 1), "ms_per_batch": round(dt / (len(texts) / args.batch) * 1e3, 3)}
        del emb
    torch.cuda.empty_cache()
    out["note"] = ("%d texts of 30 CJK chars (L = 32 with [CLS]/[SEP]), batches of %d, host strings -> "
                   "List[List[float]]" % (len(texts), args.batch))
    return out


def workload_name(rows, batch, world):
    """Which BASELINE.json config the sizes are (config 4 = its per-GPU shard at N=1)."""
    if rows == 1_000_000 and batch == 256:
        return "BASELINE config 3"
    if rows == 100_000 and batch == 256:
        return "BASELINE config 2"
    if rows == 10_000_000 or (rows == 1_250_000 and batch == 1024):
        return "BASELINE config 4" + (" (one GPU's 1.25M-row shard)" if world == 1 and rows < 10_000_000 else "")
    return "custom"


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # MQ_DIST_BACKEND=gloo rehearses the N-rank path with several ranks on one GPU
    backend = os.environ.get("MQ_DIST_BACKEND", "nccl")
    local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    cfg = DMETA_BASE if args.layers == DMETA_BASE.layers else \
        type(DMETA_BASE)(layers=args.layers)
    B, L, K = args.batch, args.seq_len, args.k

    # ---- resident inputs: corpus shard, token ids, encoder weights ------------------
    off, cnt = shard_bounds(args.corpus_rows, world, rank)
    full = synth.corpus_device(args.corpus_rows, 768, dev)  # same seed on every rank
    index = FlatIndex(dim=768, capacity=cnt, device=local)
    index.add_device(full[off:off + cnt].contiguous())
    enc = Encoder(cfg, device=local)
    for kv in args.enc_opt:
        name, val = kv.split("=")
        enc.set_option(name, int(val))
    ids_np, mask_np = synth.token_batch(B, L, seed=synth.TOKEN_SEED + rank)
    ids = torch.from_numpy(ids_np).to(dev)
    mask = torch.from_numpy(mask_np).to(dev)
    q = torch.empty((B, 768), dtype=torch.float32, device=dev)
    nq_all = B * world
    s_loc = torch.empty((nq_all, K), dtype=torch.float32, device=dev)
    i_loc = torch.empty((nq_all, K), dtype=torch.int64, device=dev)

    def local_search(queries, k):
        index.search_device(queries, k, s_loc[:queries.shape[0]], i_loc[:queries.shape[0]])
        return s_loc[:queries.shape[0]], i_loc[:queries.shape[0]]

    searcher = ShardedSearcher(local_search, off)

    def step(ev=None):
        if ev:
            ev[0].record()
        enc.embed_device(ids, mask, q)
        if ev:
            ev[1].record()
        if world > 1:
            s, i = searcher.search_local_batch(q, K, sizes=[B] * world)  # equal batches: no size exchange
        else:
            s, i = local_search(q, K)
        if ev:
            ev[2].record()
        return s, i

    # parity guard at full size: planted queries find their rows (property check)
    ok_planted = {}
    if args.full:
        pq, planted = synth.queries_device(64, full)
        for name, (_, prec) in PRECISIONS.items():
            index.set_precision(prec)
            _, pq_i = searcher.search(pq, K) if world > 1 else local_search(pq, K)
            ok_planted[name] = bool((pq_i[:32, 0] == planted[:32]).all())
    del full
    torch.cuda.empty_cache()

    def measure(precs):
        """Warm up, then time exactly args.steps steps (barrier + sync on both sides,
        max over ranks); per-kernel-class device time from HIP events."""
        enc.set_precision(precs[0])
        index.set_precision(precs[1])
        fb0, pd0 = index.screen_fallbacks, index.screen_passdowns
        evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        enc.read_timing()
        index.read_timing()
        enc.set_timing(True)
        index.set_timing(True)
        if world > 1:
            searcher.timings = []  # HIP events around each collective (host time for gloo)
        t0 = time.perf_counter()
        for it in range(args.steps):
            s_last, i_last = step(evs[it])
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        # what the last timed step handed back (later runs reuse the buffers)
        last = {"scores": s_last[:B].clone(), "ids": i_last[:B].clone(), "embeddings": q.clone()}
        coll = None
        if world > 1:
            coll = {}
            for tag, nbytes, ms in searcher.resolve_timings():
                c = coll.setdefault(tag, {"ms_per_step": 0.0, "bytes_per_rank": nbytes, "calls": 0})
                c["ms_per_step"] += ms / args.steps
                c["calls"] += 1
            searcher.timings = None
        if world > 1:
            t = torch.tensor([elapsed], device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        stage_ms = {k: v / args.steps for k, v in enc.read_timing().items()}
        stage_ms.update({k: v / args.steps for k, v in index.read_timing().items()})
        enc.set_timing(False)
        index.set_timing(False)
        return {"elapsed": elapsed, "stage_ms": stage_ms, "collectives": coll, "last": last,
                "screen_fallbacks": index.screen_fallbacks - fb0,
                "screen_passdowns": index.screen_passdowns - pd0,
                "enc_ms": statistics.mean(e[0].elapsed_time(e[1]) for e in evs),
                "srch_ms": statistics.mean(e[1].elapsed_time(e[2]) for e in evs)}

    HEAD = "f32x6_screen"
    if args.full:
        runs = {name: measure(precs) for name, precs in PRECISIONS.items()}
    else:
        # set-up the other runs otherwise do: untimed steps build the index's shadow slabs
        # and the encoder's pre-split weights, whatever --warmup is, the last ones on the
        # per-kernel timeline the timed steps run with
        enc.set_precision(PRECISIONS[HEAD][0])
        index.set_precision(PRECISIONS[HEAD][1])
        step()
        enc.set_timing(True)
        index.set_timing(True)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        enc.set_timing(False)
        index.set_timing(False)
        runs = {HEAD: measure(PRECISIONS[HEAD])}
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, runs[HEAD]["last"])
    for r in runs.values():
        del r["last"]
    # the headline configuration for everything after (the few-row single-query forward is
    # fp32 whatever the precision)
    enc.set_precision(_lib.MQ_DTYPE_F32X6)
    index.set_precision(_lib.MQ_DTYPE_F32_SCREEN)

    # ---- BASELINE config 5 beside it: bf16 index scanned as an MFMA GEMM for the top 64
    # (k=50 -> max(2k,50) capped at 64) + exact fp32 re-rank; search only, same queries,
    # recall@50 against the exact fp32 scan ---------------------------------------------
    cfg5 = None
    if world == 1 and args.full:
        k5 = 50
        s5 = torch.empty((B, k5), dtype=torch.float32, device=dev)
        i5 = torch.empty((B, k5), dtype=torch.int64, device=dev)
        index.search_device(q, k5, s5, i5)
        exact = i5.clone()
        index.set_precision(_lib.MQ_DTYPE_BF16)
        index.search_device(q, k5, s5, i5)  # builds the bf16 shadow slab (untimed)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            index.search_device(q, k5, s5, i5)
        e1.record()
        torch.cuda.synchronize()
        ms5 = e0.elapsed_time(e1) / 10
        hits = sum(len(set(a) & set(b)) for a, b in zip(i5.cpu().tolist(), exact.cpu().tolist()))
        cfg5 = {"workload": "BASELINE config 5 (search only): %d x 768 bf16 shadow slab, batch %d, "
                            "bf16 MFMA coarse top-64 + exact fp32 re-rank to k=%d" % (cnt, B, k5),
                "queries_per_s": round(B / ms5 * 1e3, 1), "ms_per_batch": round(ms5, 3),
                "recall_at_k_vs_exact_f32": round(hits / (B * k5), 5),
                "hbm_gbs_algorithmic": round(cnt * 768 * 2 / (ms5 * 1e-3) / 1e9, 1)}
        index.set_precision(_lib.MQ_DTYPE_F32_SCREEN)

    # ---- SURVEY.md §8d secondary run: the same step at L = 128 (headline arithmetic) ----
    sec = None
    if world == 1 and args.full and args.secondary_seq_len > 0:
        L2 = args.secondary_seq_len
        ids2_np, mask2_np = synth.token_batch(B, L2, seed=synth.TOKEN_SEED)
        ids2, mask2 = torch.from_numpy(ids2_np).to(dev), torch.from_numpy(mask2_np).to(dev)
        n2 = max(3, args.steps // 4)
        for it in range(2 + n2):
            if it == 2:
                torch.cuda.synchronize()
                a = time.perf_counter()
            enc.embed_device(ids2, mask2, q)
            local_search(q, K)
        torch.cuda.synchronize()
        t2 = (time.perf_counter() - a) / n2
        sec = {"seq_len": L2, "steps": n2, "queries_per_s": round(B / t2, 1),
               "ms_per_step": round(t2 * 1e3, 3),
               "encoder_tflops_effective": round(encoder_flops(cfg, B, L2) / t2 / 1e12, 2)}

    traffic_db_early = {}
    pmc = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(pmc):
        try:
            traffic_db_early = json.load(open(pmc))
        except Exception:
            traffic_db_early = {}

    # ---- single-query latency (embed 1 query + search the shard), exact f32 ----------
    lat, lat_parts, single_roof = [], None, None
    if world == 1 and args.full and args.single_iters > 0:
        ids1, mask1, q1 = ids[:1].contiguous(), mask[:1].contiguous(), q[:1]
        pd0 = index.screen_passdowns
        for it in range(args.single_iters + 5):
            torch.cuda.synchronize()
            a = time.perf_counter()
            enc.embed_device(ids1, mask1, q1)
            local_search(q1, K)
            torch.cuda.synchronize()
            if it >= 5:
                lat.append((time.perf_counter() - a) * 1e3)
        enc_l, srch_l = [], []  # the two halves alone (a host sync between them)
        for it in range(args.single_iters):
            torch.cuda.synchronize()
            a = time.perf_counter()
            enc.embed_device(ids1, mask1, q1)
            torch.cuda.synchronize()
            b = time.perf_counter()
            local_search(q1, K)
            torch.cuda.synchronize()
            enc_l.append((b - a) * 1e3)
            srch_l.append((time.perf_counter() - b) * 1e3)
        lat_parts = {"encoder_ms": round(statistics.median(enc_l), 3),
                     "search_ms": round(statistics.median(srch_l), 3),
                     "search_tier": "int8 screen (K9q) -> fp32 re-rank + certificate",
                     "passdowns": index.screen_passdowns - pd0}
        # one query's forward streams every fp32 weight matrix once (few-row path, 61
        # launches): its HBM roofline is weights / 8 TB/s; the gap is per-launch latency
        wbytes = 4 * cfg.layers * (4 * cfg.hidden * cfg.hidden + 2 * cfg.hidden * cfg.ffn)
        enc_ms = lat_parts["encoder_ms"]
        lat_parts["encoder_roofline"] = {
            "bound": "hbm (weight streaming)", "weight_bytes": wbytes,
            "achieved_gbs": round(wbytes / (enc_ms * 1e-3) / 1e9, 1), "peak_gbs": HBM_PEAK_GBS,
            "frac": round(wbytes / (enc_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "t_min_ms": round(wbytes / (HBM_PEAK_GBS * 1e9) * 1e3, 4)}
        # the single query's scan: K9q sample + appending pass over the int8 shadow (HBM-bound)
        index.read_timing()
        index.set_timing(True)
        for _ in range(20):
            local_search(q1, K)
        scan_ms = index.read_timing()["flat_search_kernel"] / 20
        index.set_timing(False)
        i8_bytes = cnt * (768 + 4) * (1 + 1 / 16)  # appending pass + 1/16 sample pass
        single_roof = {"kernel": "i8_thresh_kernel (K9q: sample + appending pass)", "bound": "hbm",
                       "achieved": round(i8_bytes / (scan_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS,
                       "unit": "GB/s", "frac": round(i8_bytes / (scan_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                       "bytes_per_search": int(i8_bytes), "ms_per_search": round(scan_ms, 4),
                       "traffic": (traffic_db_early.get("i8_thresh_kernel", 0) + traffic_db_early.get("i8_thresh_sample", 0))
                       or None}

    c4 = config4(args, enc, world, rank, dev, backend) if args.full and args.config4_steps > 0 else None

    extras = {}
    if world == 1 and args.full and not args.no_extras:
        extras["exact_k50_batch"] = exact_k50(index, q, dev)
        extras["long_query_p50"] = long_queries(args, enc, index, dev, K)
        extras["config2"] = config2(args, enc, dev, ids, mask, q)
        extras["clustered_corpus"] = clustered(args, enc, dev, ids, mask, q)
        extras["langchain_embed_documents"] = langchain_embed_documents(args, dev)
    run_counters = _counters(index)  # every search of the run, timed or not

    dist_info = None
    if world > 1:
        # what the collectives ran on, for the driver's SCALE run: the backend, the world
        # size the process group saw, each rank's bound device, and the headline step's
        # per-collective time on every rank
        props = torch.cuda.get_device_properties(local)
        mine = {"rank": rank, "local_rank": int(os.environ.get("LOCAL_RANK", "0")), "device": local,
                "device_name": props.name, "pci_bus_id": getattr(props, "pci_bus_id", None),
                "rows": cnt, "row_offset": off,
                "collectives_ms_per_step": {t: round(c["ms_per_step"], 4)
                                            for t, c in (runs["f32x6_screen"]["collectives"] or {}).items()}}
        everyone = [None] * world
        dist.all_gather_object(everyone, mine)
        dist_info = {"backend": dist.get_backend(), "world_size": dist.get_world_size(),
                     "ranks": everyone,
                     "allgather": {t: {"ms_per_step_rank0": round(c["ms_per_step"], 4),
                                       "ms_per_step_max": round(max(r["collectives_ms_per_step"].get(t, 0.0)
                                                                    for r in everyone), 4),
                                       "bytes_per_rank": c["bytes_per_rank"], "calls_per_step": c["calls"] / args.steps,
                                       "timer": "HIP events on the launch stream" if dist.get_backend() == "nccl"
                                       else "host wall time (gloo gathers host copies)"}
                                   for t, c in (runs["f32x6_screen"]["collectives"] or {}).items()}}

    if rank != 0:
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    H, F, NL = cfg.hidden, cfg.ffn, cfg.layers
    M = B * L
    full_l, last = NL - 1, 1  # the CLS-pooled last layer runs out-proj/FFN on B rows only
    flops = {  # algorithmic FLOPs per step actually issued by each kernel class
        # the CLS-pooled last layer projects K and V for every token, Q for the CLS rows only
        "qkv_gemm": full_l * 2.0 * M * 3 * H * H + last * (2.0 * M * 2 * H * H + 2.0 * B * H * H),
        "attention": NL * 4.0 * B * L * L * H,
        "out_proj_gemm": (full_l * M + last * B) * 2.0 * H * H,
        "ffn_up_gemm": (full_l * M + last * B) * 2.0 * H * F,
        "ffn_down_gemm": (full_l * M + last * B) * 2.0 * H * F,
        "flat_search_kernel": 2.0 * nq_all * cnt * 768,
    }
    traffic_db = traffic_db_early
    srch_bytes = cnt * 768 * 4 + nq_all * 768 * 4 + nq_all * K * 12

    X6_PEAK = BF16_PEAK_TFLOPS / 6.0  # six bf16 MFMAs per fp32 product: 417 TFLOP/s fp32-equiv.

    def summarize(name, r):
        enc_x6 = PRECISIONS[name][0] == _lib.MQ_DTYPE_F32X6
        # arithmetic of the timed scan kernel: the screen's first tier scans the bf16 shadow
        scan = {_lib.MQ_DTYPE_F32X6: "x6", _lib.MQ_DTYPE_F32_SCREEN: "bf16"}.get(PRECISIONS[name][1], "f32")
        scan_peak = {"x6": X6_PEAK, "bf16": BF16_PEAK_TFLOPS, "f32": FP32_PEAK_TFLOPS}[scan]
        kernels = {}
        for kname, ms in r["stage_ms"].items():
            d = {"ms_per_step": round(ms, 4)}
            if kname in flops and ms > 0:
                pk = scan_peak if kname == "flat_search_kernel" else (X6_PEAK if enc_x6 else FP32_PEAK_TFLOPS)
                tf = flops[kname] / (ms * 1e-3) / 1e12
                d.update(tflops=round(tf, 2), frac_peak=round(tf / pk, 4))
            kernels[kname] = d
        dom = max((n for n in flops if r["stage_ms"].get(n, 0) > 0), key=lambda n: r["stage_ms"][n])
        dom_x6 = (scan == "x6") if dom == "flat_search_kernel" else enc_x6
        peak = (scan_peak if dom == "flat_search_kernel" else X6_PEAK if enc_x6 else FP32_PEAK_TFLOPS)
        dom_tf = flops[dom] / (r["stage_ms"][dom] * 1e-3) / 1e12
        roof = {"kernel": dom + (" (K2p split-f32)" if dom_x6 and dom != "flat_search_kernel" else ""),
                "bound": "mfma", "achieved": round(dom_tf, 2), "peak": round(peak, 1),
                "unit": "TFLOP/s (fp32-equivalent)" if dom_x6 else "TFLOP/s",
                "frac": round(dom_tf / peak, 4),
                "traffic": traffic_db.get(dom + "_x6p") if dom_x6 else traffic_db.get(dom)}
        sk = r["stage_ms"].get("flat_search_kernel", r["srch_ms"])
        # bf16 screen (K9t threshold scan, sample + main pass): 1.5 GB of shadow rows at
        # 256 FLOP/B - under the spec bf16 ridge (~312), but measured MFMA-bound: the main
        # pass multiplying only takes 346 us, streaming only 255 us
        sbytes = srch_bytes if scan != "bf16" else cnt * 768 * 2 + nq_all * 768 * 2 + nq_all * K * 8
        search_roof = {"kernel": {"x6": "flat_search_kernel (split-f32)",
                                  "bf16": "bf16_thresh_kernel (K9t screen: sample + main pass)",
                                  "f32": "flat_search_kernel (exact f32)"}[scan],
                       "bound": "mfma",
                       "achieved_tflops": kernels.get("flat_search_kernel", {}).get("tflops"),
                       "peak_tflops": round(scan_peak, 1),
                       "hbm_gbs_algorithmic": round(sbytes / (sk * 1e-3) / 1e9, 1),
                       "hbm_frac": round(sbytes / (sk * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                       "bytes_per_launch": sbytes, "flops_per_launch": flops["flat_search_kernel"],
                       "traffic": (traffic_db.get("bf16_thresh_kernel") + traffic_db.get("bf16_thresh_sample")
                                   if scan == "bf16" and "bf16_thresh_kernel" in traffic_db
                                   and "bf16_thresh_sample" in traffic_db else
                                   traffic_db.get({"x6": "flat_search_kernel_x6", "bf16": "-",
                                                   "f32": "flat_search_kernel"}[scan]))}
        return {"value": round(nq_all * args.steps / r["elapsed"], 2),
                "ms_per_step": round(r["elapsed"] / args.steps * 1e3, 3),
                "roofline": roof, "search_roofline": search_roof,
                "encoder_ms": round(r["enc_ms"], 3), "search_ms": round(r["srch_ms"], 3),
                "kernels": kernels, "planted_top1_ok": ok_planted.get(name),
                "screen_fallbacks": r["screen_fallbacks"], "screen_passdowns": r["screen_passdowns"]}

    main_r = summarize(HEAD, runs[HEAD])
    out = {
        "metric": "queries/s (embed+top-k, k=5, b=256) over 1M×768 corpus; p50 single-query ms",
        "value": main_r["value"], "unit": "queries/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": main_r["ms_per_step"],
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32 (exact 3-way bf16 split, fp32 accumulate; exact fp32 top-k)",
        "data": "synthetic (seeded corpus on device, seeded token ids, seeded BERT-base weights)",
        "config": {"workload": "%s: %d x 768 fp32 corpus, batch %d/GPU (L=%d) "
                               "embed + exact top-%d" % (workload_name(args.corpus_rows, B, world),
                                                          args.corpus_rows, B, L, K),
                   "corpus_rows": args.corpus_rows, "rows_per_gpu": cnt, "batch_per_gpu": B,
                   "global_batch": nq_all, "seq_len": L, "k": K,
                   "encoder": "BERT-base %dL (dmeta-embedding-zh shape)" % cfg.layers,
                   "parallelism": "row-shard x%d + DP encoder" % world if world > 1 else "single GPU"},
        "p50_single_query_ms": round(statistics.median(lat), 3) if lat else None,
        "p50_single_query_parts": lat_parts,
        "single_query_search_roofline": single_roof,
        "planted_top1_ok": main_r["planted_top1_ok"],
        "roofline": main_r["roofline"],
        "search_roofline": main_r["search_roofline"],
        "encoder_ms": main_r["encoder_ms"], "search_ms": main_r["search_ms"],
        "kernels": main_r["kernels"],
        "search_mode": "exact fp32 top-k: bf16-shadow MFMA threshold scan (K9t) for 64 candidates, fp32 "
                       "re-rank, certified bound per query; uncertified queries re-run on the split-f32 "
                       "screen (%d in the timed steps) or the direct exact scan (%d)"
                       % (main_r["screen_passdowns"], main_r["screen_fallbacks"]),
        "full": args.full,  # False: the keys --full measures in runs of their own are null
        "exact_f32_encoder": None, "f32_direct_search": None, "split_f32": None,
    }
    if args.full:
        exact_r = summarize("f32", runs["f32"])
        direct_r = summarize("f32_direct_search", runs["f32_direct_search"])
        alt_r = summarize("f32x6", runs["f32x6"])
        out["exact_f32_encoder"] = dict(
            {kk: exact_r[kk] for kk in ("value", "ms_per_step", "encoder_ms", "search_ms", "roofline",
                                        "kernels", "planted_top1_ok", "screen_fallbacks", "screen_passdowns")},
            dtype="f32 (encoder on the exact f32 MFMA, v_mfma_f32_32x32x2_f32; exact fp32 top-k)")
        out["f32_direct_search"] = {kk: direct_r[kk] for kk in ("value", "ms_per_step", "search_ms",
                                                                "search_roofline", "planted_top1_ok")}
        out["split_f32"] = dict(alt_r, dtype="f32 via exact 3-way bf16 split (6 bf16 MFMAs / product, "
                                             "fp32 accumulate) for the encoder and the direct scan")
    out["distributed"] = dist_info
    # which library ran: the source hash compiled into it, and whether it is this tree's
    built = _lib.built_source_hash()
    try:
        tree = _lib.tree_source_hash()
    except OSError:
        tree = None
    out["library"] = {"path": os.path.relpath(_lib.LIB_PATH, ROOT), "source_hash": built,
                      "built_from_this_tree": built == tree if tree else None}
    out["config4_sharded"] = c4
    out["config5_bf16_rerank"] = cfg5
    out["secondary_long_queries"] = sec
    out["screen_counters_whole_run"] = run_counters
    out.update(extras)
    if world == 1 and args.full and not args.no_cpu_baseline:
        def corpus_host():
            return torch.nn.functional.normalize(
                synth.corpus_device(args.corpus_rows, 768, dev), dim=1).cpu().numpy()
        out["cpu_baseline"] = cpu_baseline(args, cfg, corpus_host)
    else:
        out["cpu_baseline"] = None
    print(json.dumps(out, ensure_ascii=False), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
