"""What maximal marginal relevance costs on top of the search it starts from, at 1M x 768 on
the default "screen" precision:

  * FlatIndex.search_mmr(q, k=5, fetch_k) against FlatIndex.search(q, fetch_k), for one query
    and for a batch of 256, fetch_k 20 and 64.  The two legs of a pair alternate call by call
    in one process (same clocks, same cache state), after warm-up calls of both; each leg is
    reported as median and range over the repeats, the pair also as the median of the
    per-repeat differences.
  * the selection kernel alone (mq_index_mmr_select on device lists), timed with HIP events
    on the stream: single launches (median / range) and a back-to-back run of 50.

  python tools/mmr_latency.py [--rows 1000000] [--reps 40] [--out profiles/mmr/latency.json]
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
from mediquery_hip import _lib, synth  # noqa: E402
from mediquery_hip.native import FlatIndex  # noqa: E402


def spread(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits),
            "max": round(max(xs), digits), "n": len(xs)}


def pair(leg_a, leg_b, reps, warmup=5):
    """Alternate the two legs; -> (ms of a, ms of b, b - a per repeat)."""
    a, b = [], []
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        leg_a(it)
        t1 = time.perf_counter()
        leg_b(it)
        t2 = time.perf_counter()
        if it >= warmup:
            a.append((t1 - t0) * 1e3)
            b.append((t2 - t1) * 1e3)
    return a, b, [y - x for x, y in zip(a, b)]


def kernel_ms(ix, cs, ci, k, lam, reps):
    """HIP-event time of mmr_select launches on device lists: singles, and 50 back to back."""
    nq = cs.shape[0]
    os_ = torch.empty((nq, k), dtype=torch.float32, device=cs.device)
    oi = torch.empty((nq, k), dtype=torch.int64, device=cs.device)
    for _ in range(5):
        ix.mmr_select_device(cs, ci, k, lam, os_, oi)
    torch.cuda.synchronize()
    singles = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ix.mmr_select_device(cs, ci, k, lam, os_, oi)
        e1.record()
        e1.synchronize()
        singles.append(e0.elapsed_time(e1) * 1e3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        ix.mmr_select_device(cs, ci, k, lam, os_, oi)
    e1.record()
    e1.synchronize()
    return {"single_launch_us": spread(singles, 2), "back_to_back_us": round(e0.elapsed_time(e1) * 1e3 / 50, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmr", "latency.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows, _ = synth.clustered_corpus_device(args.rows, 768, dev)
    ix = FlatIndex(dim=768, capacity=args.rows, device=0)
    for r0 in range(0, args.rows, 1 << 18):
        ix.add_device(rows[r0:r0 + (1 << 18)].contiguous())
    torch.cuda.synchronize()
    ix.set_precision(_lib.MQ_DTYPE_F32_SCREEN)
    qd, _ = synth.queries_device(256, rows)
    del rows
    q = qd.cpu().numpy()
    out = {"rows": args.rows, "dim": 768, "precision": "screen", "k": 5, "lambda": 0.5,
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "unit": "ms unless named"}
    for fetch_k in (20, 64):
        for nq in (1, 256):
            reps = args.reps if nq == 1 else max(10, args.reps // 2)
            sel = (lambda it: q[it % 256:it % 256 + 1]) if nq == 1 else (lambda it: q)
            a, b, d = pair(lambda it: ix.search(sel(it), fetch_k),
                           lambda it: ix.search_mmr(sel(it), 5, fetch_k, 0.5), reps)
            # the kernel alone, on this search's own lists
            cs = torch.empty((nq, fetch_k), dtype=torch.float32, device=dev)
            ci = torch.empty((nq, fetch_k), dtype=torch.int64, device=dev)
            ix.search_device(qd[:nq].contiguous(), fetch_k, cs, ci)
            torch.cuda.synchronize()
            out["fetch_k=%d nq=%d" % (fetch_k, nq)] = {
                "search": spread(a), "search_mmr": spread(b), "mmr_minus_search": spread(d),
                "select_kernel": kernel_ms(ix, cs, ci, 5, 0.5, args.reps)}
            print(fetch_k, nq, json.dumps(out["fetch_k=%d nq=%d" % (fetch_k, nq)]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
