"""Grouped search at the VectorStore surface, one run: N rows x 768 of a synthetic parent-child
corpus (rows = one of N / 64 standard-normal centroids + 0.35 noise, 64 consecutive rows per
centroid, so the children of a parent are each other's nearest rows) with three parent keys in
every row's metadata: "p1" (a parent per row), "p8" (8 children) and "p64" (64 children: one
parent owns a query's whole top 64).  Queries are a corpus row plus noise.  Per family size:

  similarity_search_by_vector(k=5)              the plain dense search
  grouped, certificate first                    similarity_search_grouped_by_vector_with_score
  grouped, forced onto the scan                 the same with _force_scan=True
  a batch of 256: _index.search, the grouped rows with the certificate, and forced onto the scan
  mq_index_search_grouped alone (device in, device out, HIP events): 1, 16 and 256 queries

Every figure is the p50 and [min, max] of --reps repetitions in ms.  `scan_GBps` is the fp32
slab's bytes times the passes (16 queries a pass) over the device time of the whole call - table
zeroing, scan, select and merge - and `certified` the share of the queries the top 64 answered.
`mismatched` counts the queries whose certified and forced answers name different rows (the two
stages take their fp32 dots from different kernels, so a near-tie may order differently).

  timeout -k 10 900 python tools/grouped_latency.py [--rows 1000000] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mediquery-rag_amd"), ROOT]
import torch  # noqa: E402
from mediquery_hip import _lib  # noqa: E402
from mediquery_hip.native import group_scratch_bytes  # noqa: E402
from mediquery_hip.vectorstore import HipChroma  # noqa: E402

FAMILIES = (1, 8, 64)
DIM = 768


def note(msg):
    print("[grouped_latency] " + msg, file=sys.stderr, flush=True)


def stats(ms):
    return {"p50": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def wall(fn, reps, warm=1):
    out = []
    for it in range(reps + warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def device_ms(fn, reps, warm=1):
    out = []
    for it in range(reps + warm):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if it >= warm:
            out.append(a.elapsed_time(b))
    return out


def corpus(n, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    cents = torch.randn(((n + 63) // 64, DIM), generator=g, device=dev)
    rows = torch.randn((n, DIM), generator=g, device=dev).mul_(0.35)
    rows.add_(cents[torch.arange(n, device=dev) // 64])
    return torch.nn.functional.normalize(rows, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--singles", type=int, default=16, help="single queries timed per repetition")
    ap.add_argument("--out", default=None, help="append the JSON line to this file too")
    args = ap.parse_args()
    n = args.rows
    dev = torch.device("cuda", 0)
    rows_dev = corpus(n, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(99)
    picks = torch.randint(0, n, (256,), generator=g, device=dev)
    q_dev = torch.nn.functional.normalize(
        rows_dev[picks] + 0.05 * torch.randn((256, DIM), generator=g, device=dev) / DIM ** 0.5, dim=1).contiguous()
    queries = q_dev.cpu().numpy()
    store = HipChroma(dim=DIM, auto_persist=False)
    store.add_embeddings(rows_dev.cpu().numpy(), [""] * n,
                         [{"p1": r, "p8": r >> 3, "p64": r >> 6} for r in range(n)], ["id%d" % r for r in range(n)])
    del rows_dev
    torch.cuda.synchronize()
    slab_bytes = n * DIM * 4
    out = {"rows": n, "dim": DIM, "k": 5, "reps": args.reps, "slab_GB": round(slab_bytes / 1e9, 3),
           "lib": os.path.basename(_lib.LIB_PATH), "families": {}}
    note("store of %d rows built" % n)
    ns = args.singles
    plain = lambda: [store.similarity_search_by_vector(q, k=5) for q in queries[:ns]]  # noqa: E731
    out["similarity_search_k5_ms_per_query"] = stats([t / ns for t in wall(plain, args.reps)])
    out["index_search_batch256_k5_ms"] = stats(wall(lambda: store._index.search(queries, 5), args.reps))
    ix = store._index
    for fam in FAMILIES:
        key = "p%d" % fam
        case = {"n_groups": len(store._cols.cols[key][1])}
        grouped = lambda force: [store.similarity_search_grouped_by_vector_with_score(  # noqa: E731
            q, 5, group_by=key, _force_scan=force) for q in queries[:ns]]
        before = store.group_scans
        a = grouped(False)
        case["certified_singles"] = round(1.0 - (store.group_scans - before) / ns, 3)
        b = grouped(True)
        case["mismatched_singles"] = sum([d.id for d, _ in x] != [d.id for d, _ in y] for x, y in zip(a, b))
        case["grouped_ms_per_query"] = stats([t / ns for t in wall(lambda: grouped(False), args.reps)])
        case["grouped_forced_scan_ms_per_query"] = stats([t / ns for t in wall(lambda: grouped(True), args.reps)])
        before = store.group_scans
        a = store._grouped_rows(queries, 5, key)
        case["certified_batch256"] = round(1.0 - (store.group_scans - before) / 256, 3)
        b = store._grouped_rows(queries, 5, key, force_scan=True)
        case["mismatched_batch256"] = sum([r for r, _ in x] != [r for r, _ in y] for x, y in zip(a, b))
        case["grouped_batch256_ms"] = stats(wall(lambda: store._grouped_rows(queries, 5, key), args.reps))
        case["grouped_batch256_forced_scan_ms"] = stats(
            wall(lambda: store._grouped_rows(queries, 5, key, force_scan=True), args.reps))
        # the C call alone on device buffers
        codes = store._cols.dev_codes(key, dev)
        n_groups = case["n_groups"]
        for nq in (1, 16, 256):
            scratch = torch.empty(group_scratch_bytes(n_groups, nq, 5), dtype=torch.uint8, device=dev)
            os_ = torch.empty((nq, 5), dtype=torch.float32, device=dev)
            oi = torch.empty((nq, 5), dtype=torch.int64, device=dev)
            ms = device_ms(lambda: ix.search_grouped_device(q_dev[:nq], 5, codes, n_groups, os_, oi, None, scratch),
                           args.reps)
            passes = (nq + 15) // 16
            case["scan_call_q%d" % nq] = dict(stats(ms), passes=passes, table_MB=round(min(nq, 16) * n_groups * 8 / 1e6, 1),
                                              scan_GBps=round(slab_bytes * passes / statistics.median(ms) / 1e6, 1))
        out["families"][key] = case
        note("%s: %d groups, single %.3f ms certified (%.0f%%) / %.3f ms scan, batch %.2f / %.2f ms, scan call q256 %.2f ms"
             % (key, n_groups, case["grouped_ms_per_query"]["p50"], 100 * case["certified_singles"],
                case["grouped_forced_scan_ms_per_query"]["p50"], case["grouped_batch256_ms"]["p50"],
                case["grouped_batch256_forced_scan_ms"]["p50"], case["scan_call_q256"]["p50"]))
    line = json.dumps(out, ensure_ascii=False)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
