"""Range search (K17), one run on tools/grouped_latency.py's corpus: N rows x 768 (rows = one of
N / 64 standard-normal centroids + 0.35 noise), queries a corpus row plus noise.

Single query, device buffers, HIP events (the variants alternate inside every repetition):
  mq_index_search_range   max_hits 64 / 256 / 1024 / 4096 at min_score -inf, and max_hits 4096 at
                          two thresholds that leave about 100 and about 10k hits
  mq_index_search_grouped one query over a group per row: the same row walk with atomic maxima
                          where the range scan stores keys
  _index.search(q, 64)    the list search every k <= 64 method uses
  16 x search_masked(64)  the only route to 1024 rows without the range search: each round
                          masks out the rows the earlier rounds returned (wall clock, host I/O)
then one 16-query pass and 256 queries (max_hits 1024), the range and grouped single query on an
N x 64 index (64 B of keys per 256 B read, where the 4-byte stores weigh most), and at the store:
similarity_search_range_by_vector_with_score(limit=200) beside similarity_search_by_vector(k=5).
Every figure is the p50 and [min, max] of --reps repetitions in ms.

--kernels: only a few range calls (max_hits 64 and 4096, one query, then 16), for a
`rocprofv3 --kernel-trace --stats -- python tools/range_latency.py --kernels` run of its own,
which splits the call into its scan, histogram, pick, collect and sort kernels.

  timeout -k 10 900 python tools/range_latency.py [--rows 1000000] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mediquery-rag_amd"), ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mediquery_hip import _lib  # noqa: E402
from mediquery_hip.native import FlatIndex, group_scratch_bytes, range_scratch_bytes  # noqa: E402
from mediquery_hip.vectorstore import HipChroma  # noqa: E402

INF = float("inf")


def note(msg):
    print("[range_latency] " + msg, file=sys.stderr, flush=True)


def stats(ms):
    return {"p50": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def corpus(n, dim, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    cents = torch.randn(((n + 63) // 64, dim), generator=g, device=dev)
    rows = torch.randn((n, dim), generator=g, device=dev).mul_(0.35)
    rows.add_(cents[torch.arange(n, device=dev) // 64])
    return torch.nn.functional.normalize(rows, dim=1)


def noisy_queries(rows, nq, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(99)
    picks = torch.randint(0, rows.shape[0], (nq,), generator=g, device=dev)
    noise = torch.randn((nq, rows.shape[1]), generator=g, device=dev) / rows.shape[1] ** 0.5
    return torch.nn.functional.normalize(rows[picks] + 0.05 * noise, dim=1).contiguous()


def alternate(variants, reps, warm=1, device=True):
    """{name: fn} -> {name: stats}: every repetition runs each variant once, in turn."""
    out = {name: [] for name in variants}
    for it in range(reps + warm):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            if device:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms = a.elapsed_time(b)
            else:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
            if it >= warm:
                out[name].append(ms)
    return {name: stats(ms) for name, ms in out.items()}


class RangeCall:
    """mq_index_search_range on device buffers kept across calls."""

    def __init__(self, ix, nq, max_hits, dev):
        self.ix, self.max_hits = ix, max_hits
        self.scratch = torch.empty(range_scratch_bytes(len(ix), nq, max_hits), dtype=torch.uint8, device=dev)
        self.counts = torch.empty(nq, dtype=torch.int64, device=dev)
        self.scores = torch.empty((nq, max_hits), dtype=torch.float32, device=dev)
        self.ids = torch.empty((nq, max_hits), dtype=torch.int64, device=dev)

    def __call__(self, q, min_score=-INF):
        self.ix.search_range_device(q, self.max_hits, self.counts, self.scores, self.ids, min_score, None,
                                    self.scratch)


def grouped_call(ix, q, dev):
    n = len(ix)
    codes = torch.arange(n, dtype=torch.int32, device=dev)
    scratch = torch.empty(group_scratch_bytes(n, q.shape[0], 64), dtype=torch.uint8, device=dev)
    os_ = torch.empty((q.shape[0], 64), dtype=torch.float32, device=dev)
    oi = torch.empty((q.shape[0], 64), dtype=torch.int64, device=dev)
    return lambda: ix.search_grouped_device(q, 64, codes, n, os_, oi, None, scratch)


def masked_rounds(ix, q_host, dev, rounds=16):
    """1024 rows the parent's way: `rounds` masked top-64 searches, each excluding the rows the
    earlier ones returned -> the ids, in order."""
    n = len(ix)
    words = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev)
    got = []
    for _ in range(rounds):
        _, ids = ix.search_masked(q_host, 64, words)
        rows = torch.from_numpy(ids[0][ids[0] >= 0]).to(dev)
        clear = torch.zeros_like(words)
        clear.index_put_((rows >> 5,), (1 << (rows & 31)).to(torch.int32), accumulate=True)  # distinct rows: an OR
        words &= ~clear
        got += ids[0].tolist()
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON line to this file too")
    ap.add_argument("--kernels", action="store_true", help="a few range calls only, for a kernel trace")
    ap.add_argument("--no-store", action="store_true", help="skip the store-level figures")
    args = ap.parse_args()
    n, dim = args.rows, 768
    dev = torch.device("cuda", 0)
    rows_dev = corpus(n, dim, dev)
    q_dev = noisy_queries(rows_dev, 256, dev)
    if args.kernels:
        ix = FlatIndex(dim=dim, device=0)
        ix.add_device(rows_dev)
        del rows_dev
        for nq in (1, 16):
            for mh in (64, 4096):
                call = RangeCall(ix, nq, mh, dev)
                for _ in range(6):
                    call(q_dev[:nq])
        torch.cuda.synchronize()
        return
    out = {"rows": n, "dim": dim, "reps": args.reps, "slab_GB": round(n * dim * 4 / 1e9, 3),
           "lib": os.path.basename(_lib.LIB_PATH)}
    if args.no_store:
        store = None
        ix = FlatIndex(dim=dim, device=0)
        ix.add_device(rows_dev)
    else:
        store = HipChroma(dim=dim, auto_persist=False)
        store.add_embeddings(rows_dev.cpu().numpy(), [""] * n, [{"s": 0}] * n, ["id%d" % r for r in range(n)])
        ix = store._index
    note("%d rows indexed" % n)
    q1 = q_dev[:1].contiguous()
    s1 = torch.sort(rows_dev @ q1[0], descending=True).values  # the tool's own scoring, to place the thresholds
    del rows_dev
    t100, t10k = float(s1[99]), float(s1[min(9999, n - 1)])
    calls = {mh: RangeCall(ix, 1, mh, dev) for mh in (64, 256, 1024, 4096)}
    variants = {"range_max_hits_%d" % mh: (lambda c=c: c(q1)) for mh, c in calls.items()}
    variants["range_4096_about_100_hits"] = lambda: calls[4096](q1, t100)
    variants["range_4096_about_10k_hits"] = lambda: calls[4096](q1, t10k)
    variants["grouped_scan_one_group_per_row_k64"] = grouped_call(ix, q1, dev)
    ks = torch.empty((1, 64), dtype=torch.float32, device=dev)
    ki = torch.empty((1, 64), dtype=torch.int64, device=dev)
    variants["index_search_k64"] = lambda: ix.search_device(q1, 64, ks, ki)
    out["single_query_device_ms"] = alternate(variants, args.reps)
    calls[4096](q1, t100)
    torch.cuda.synchronize()
    out["hits_at_thresholds"] = {"about_100": int(calls[4096].counts[0]), "min_score_100": t100}
    calls[4096](q1, t10k)
    torch.cuda.synchronize()
    out["hits_at_thresholds"].update({"about_10k": int(calls[4096].counts[0]), "min_score_10k": t10k})
    note("single query: %s" % json.dumps(out["single_query_device_ms"]))
    # 1024 rows: one range call against 16 masked rounds, host I/O both, and the same ids
    q1_host = q1.cpu().numpy()
    room = torch.empty(range_scratch_bytes(n, 1, 1024), dtype=torch.uint8, device=dev)
    want = ix.search_range(q1_host, 1024, -INF, None, room)[2][0].tolist()
    got = masked_rounds(ix, q1_host, dev)
    out["masked_rounds_same_rows_as_range"] = sorted(got) == sorted(want)
    out["masked_rounds_same_order_as_range"] = got == want
    out["to_1024_rows_host_io_wall_ms"] = alternate(
        {"range_max_hits_1024": lambda: ix.search_range(q1_host, 1024, -INF, None, room),
         "16_masked_rounds_k64": lambda: masked_rounds(ix, q1_host, dev)}, args.reps, device=False)
    note("to 1024 rows: %s" % json.dumps(out["to_1024_rows_host_io_wall_ms"]))
    batch = {}
    for nq in (16, 256):
        call = RangeCall(ix, nq, 1024, dev)
        batch["range_q%d_max_hits_1024" % nq] = (lambda c=call, nq=nq: c(q_dev[:nq]))
        batch["grouped_q%d_k64" % nq] = grouped_call(ix, q_dev[:nq].contiguous(), dev)
    out["batch_device_ms"] = alternate(batch, args.reps)
    note("batches: %s" % json.dumps(out["batch_device_ms"]))
    if store is not None:
        qs = q_dev[:16].cpu().numpy()
        res = alternate(
            {"similarity_search_range_by_vector_limit200": lambda: [
                store.similarity_search_range_by_vector_with_score(q, None, 200) for q in qs],
             "similarity_search_by_vector_k5": lambda: [store.similarity_search_by_vector(q, k=5) for q in qs]},
            args.reps, device=False)
        out["store_ms_per_query"] = {k: {a: round(b / len(qs), 3) for a, b in v.items()} for k, v in res.items()}
        note("store: %s" % json.dumps(out["store_ms_per_query"]))
        del store
    del ix, calls, variants, batch
    # dim 64: 64 B of keys written per 256 B of rows read
    rows64 = corpus(n, 64, dev)
    ix64 = FlatIndex(dim=64, device=0)
    ix64.add_device(rows64)
    q64 = noisy_queries(rows64, 16, dev)
    del rows64
    c1, c16 = RangeCall(ix64, 1, 1024, dev), RangeCall(ix64, 16, 1024, dev)
    out["dim64_device_ms"] = alternate(
        {"range_q1_max_hits_1024": lambda: c1(q64[:1]), "grouped_q1_k64": grouped_call(ix64, q64[:1].contiguous(), dev),
         "range_q16_max_hits_1024": lambda: c16(q64), "grouped_q16_k64": grouped_call(ix64, q64, dev)}, args.reps)
    note("dim 64: %s" % json.dumps(out["dim64_device_ms"]))
    line = json.dumps(out, ensure_ascii=False)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
