"""K-means (K19), one run on a clustered corpus: N rows x 768 around 256 unit Gaussian bases,
member = normalise(base + sigma z), sigma uniform in [0.3, 0.9], z ~ N(0, I / dim), drawn on the
device; the initial centres are n_clusters stored rows.

Device buffers, HIP events around each call; the variants alternate inside every repetition.
For n_clusters 8 / 64 / 256: the predict call (n_iter = 0: ceil(n_clusters / 16) assign passes),
the one- and the ten-iteration call; derived from their p50s: the time per assign pass
(predict / passes), per iteration ((ten - one) / 9) and per update (iteration - predict: the
update is what an iteration runs beside an assign).  In the same run:
  (a) the range search at nq = 16, max_hits = 1, min_score above every score - its score pass is
      the same walk; the call's selection passes come on top (the kernel trace separates them);
  (b) a host baseline: float32 Lloyd iterations in numpy on the read-back slab (sgemm for the
      dots, argmax, a sort and np.add.reduceat for the sums), at the thread count the
      environment sets.
Every figure is the p50 and [min, max] of --reps repetitions in ms.

--kernels: a few calls only, for a
`rocprofv3 --kernel-trace --stats -- python tools/kmeans_latency.py --kernels` run of its own.

  timeout -k 10 900 python tools/kmeans_latency.py [--rows 1000000] [--reps 5] [--out FILE]
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
from mediquery_hip.native import FlatIndex, kmeans_scratch_bytes, range_scratch_bytes  # noqa: E402

CLUSTERS = (8, 64, 256)


def note(msg):
    print("[kmeans_latency] " + msg, file=sys.stderr, flush=True)


def stats(ms):
    return {"p50": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def clustered(n, dim, dev, bases=256, seed=1234):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    base = torch.nn.functional.normalize(torch.randn((bases, dim), generator=g, device=dev), dim=1)
    which = torch.randint(0, bases, (n,), generator=g, device=dev)
    sigma = torch.rand((n, 1), generator=g, device=dev) * 0.6 + 0.3
    rows = torch.randn((n, dim), generator=g, device=dev).mul_(sigma / dim ** 0.5).add_(base[which])
    return torch.nn.functional.normalize(rows, dim=1).contiguous()


def alternate(variants, reps, warm=1):
    """{name: fn} -> {name: stats}: every repetition runs each variant once, in turn."""
    out = {name: [] for name in variants}
    for it in range(reps + warm):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= warm:
                out[name].append(a.elapsed_time(b))
    return {name: stats(ms) for name, ms in out.items()}


class KmeansCall:
    """mq_index_kmeans on device buffers kept across calls; every call starts from the same centres."""

    def __init__(self, ix, init, dev):
        n, c = len(ix), init.shape[0]
        self.ix, self.init, self.cent = ix, init, init.clone()
        self.scratch = torch.empty(kmeans_scratch_bytes(n, c), dtype=torch.uint8, device=dev)
        self.outs = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
                     torch.empty(c, dtype=torch.int64, device=dev), torch.empty(4, dtype=torch.int64, device=dev))

    def __call__(self, n_iter):
        self.cent.copy_(self.init)
        self.ix.kmeans_device(self.cent, n_iter, *self.outs, scratch=self.scratch)
        return self.outs[3]


class RangeCall:
    """(a): the range search's walk over the same index, 16 queries, no hit."""

    def __init__(self, ix, queries, dev):
        nq = queries.shape[0]
        self.ix, self.q = ix, queries
        self.scratch = torch.empty(range_scratch_bytes(len(ix), nq, 1), dtype=torch.uint8, device=dev)
        self.counts = torch.empty(nq, dtype=torch.int64, device=dev)
        self.scores = torch.empty((nq, 1), dtype=torch.float32, device=dev)
        self.ids = torch.empty((nq, 1), dtype=torch.int64, device=dev)

    def __call__(self):
        self.ix.search_range_device(self.q, 1, self.counts, self.scores, self.ids, 2.0, None, self.scratch)


def host_lloyd(rows, cents, n_iter):
    """float32 Lloyd in numpy -> seconds per iteration (assign + update)."""
    t0 = time.perf_counter()
    for _ in range(n_iter):
        d = rows @ cents.T
        d -= 0.5 * (cents * cents).sum(1)[None, :]
        lab = d.argmax(1)
        order = np.argsort(lab, kind="stable")
        sl = lab[order]
        starts = np.flatnonzero(np.r_[True, sl[1:] != sl[:-1]])
        sums = np.add.reduceat(rows[order], starts, axis=0)
        cents = cents.copy()
        cents[sl[starts]] = sums / np.diff(np.r_[starts, len(sl)])[:, None].astype(np.float32)
    return (time.perf_counter() - t0) / n_iter


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON line to this file too")
    ap.add_argument("--kernels", action="store_true", help="a few calls only, for a kernel trace")
    ap.add_argument("--host-iters", type=int, default=2, help="iterations of the host baseline (0: skip it)")
    args = ap.parse_args()
    n, dim = args.rows, 768
    dev = torch.device("cuda", 0)
    rows = clustered(n, dim, dev)
    ix = FlatIndex(dim=dim, device=0)
    ix.add_device(rows)
    note("%d rows indexed" % n)
    pick = (torch.arange(max(CLUSTERS), dtype=torch.int64, device=dev) * (n // max(CLUSTERS))).contiguous()
    seeds = rows[pick].contiguous()
    del rows
    if args.kernels:
        RangeCall(ix, seeds[:16].contiguous(), dev)()
        for c in CLUSTERS:
            KmeansCall(ix, seeds[:c].contiguous(), dev)(3)
        torch.cuda.synchronize()
        return
    out = {"rows": n, "dim": dim, "reps": args.reps, "slab_GB": round(n * dim * 4 / 1e9, 3),
           "lib": os.path.basename(_lib.LIB_PATH)}
    rng = RangeCall(ix, seeds[:16].contiguous(), dev)
    for c in CLUSTERS:
        call = KmeansCall(ix, seeds[:c].contiguous(), dev)
        res = alternate({"predict": lambda: call(0), "one_iteration": lambda: call(1),
                         "ten_iterations": lambda: call(10), "range_nq16_call": rng}, args.reps)
        info = call(10).cpu().tolist()
        passes = (c + 15) // 16
        res["derived_ms"] = {"assign_passes": passes, "per_assign_pass": round(res["predict"]["p50"] / passes, 3)}
        if info[0] == 10:  # converged earlier: the skipped launches would spoil the difference
            it = (res["ten_iterations"]["p50"] - res["one_iteration"]["p50"]) / 9
            res["derived_ms"].update(per_iteration=round(it, 3), per_update=round(it - res["predict"]["p50"], 3))
        res["info_after_ten"] = info
        res["scratch_MB"] = round(kmeans_scratch_bytes(n, c) / 1e6, 1)
        out["clusters_%d_device_ms" % c] = res
        note("%d clusters: %s" % (c, json.dumps(res)))
        del call
    if args.host_iters > 0:
        t0 = time.perf_counter()
        host = ix.get()
        read_back = time.perf_counter() - t0
        base = {"threads": os.environ.get("OMP_NUM_THREADS"), "read_back_s": round(read_back, 2)}
        for c in CLUSTERS:
            base["clusters_%d_s_per_iteration" % c] = round(host_lloyd(host, host[pick[:c].cpu().numpy()].copy(),
                                                                       args.host_iters), 3)
        out["host_numpy_float32"] = base
        note("host: %s" % json.dumps(base))
    line = json.dumps(out, ensure_ascii=False)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
