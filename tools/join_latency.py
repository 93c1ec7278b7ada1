"""Self-join (K18), one run on a corpus with planted near-copies: N rows x 768 in families of
about 8 around a unit Gaussian base, member = normalise(base + sigma z), sigma uniform in
[0.1, 0.6], z ~ N(0, I / dim) (tests/join_cases.py's neardup_corpus, drawn on the device).

Device buffers, HIP events around the call (which synchronises itself); the variants alternate
inside every repetition.  One panel of 256 left rows and 4096 left rows, each three ways:
  MQ_JOIN_SCREEN, MQ_JOIN_EXACT, and the route without the self-join: search_range_device with
  the same stored rows as the queries (max_hits 64).
Then the whole corpus once in MQ_JOIN_SCREEN, the survivors per left row and the bound E of
csrc/join.hip evaluated on this corpus, and, for MQ_JOIN_AUTO's crossover, SCREEN against EXACT
for 16 and 256 left rows on the first 1024 ... 262144 rows at dims 256 and 768.
Every figure is the p50 and [min, max] of --reps repetitions in ms.

--kernels: a few SCREEN and EXACT calls only, for a
`rocprofv3 --kernel-trace --stats -- python tools/join_latency.py --kernels` run of its own.

  timeout -k 10 900 python tools/join_latency.py [--rows 1000000] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mediquery-rag_amd"), ROOT]
import torch  # noqa: E402
from mediquery_hip import _lib  # noqa: E402
from mediquery_hip.native import FlatIndex, join_scratch_bytes, range_scratch_bytes  # noqa: E402

TAU = 0.9


def note(msg):
    print("[join_latency] " + msg, file=sys.stderr, flush=True)


def stats(ms):
    return {"p50": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def neardup(n, dim, dev, seed=1234):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    n_fam = (n + 7) // 8
    base = torch.nn.functional.normalize(torch.randn((n_fam, dim), generator=g, device=dev), dim=1)
    fam = torch.randint(0, n_fam, (n,), generator=g, device=dev)
    sigma = torch.rand((n, 1), generator=g, device=dev) * 0.5 + 0.1
    rows = torch.randn((n, dim), generator=g, device=dev).mul_(sigma / dim ** 0.5).add_(base[fam])
    return torch.nn.functional.normalize(rows, dim=1).contiguous()


def bound(rows):
    """E of csrc/join.hip from the corpus's own maxima (d = max ||c - bf16(c)||, c = max ||c||)."""
    dim = rows.shape[1]
    d = float((rows - rows.to(torch.bfloat16).float()).norm(dim=1).max()) * 1.001
    c = float(rows.norm(dim=1).max()) * 1.001
    g = 2 * dim * 2.0 ** -24
    return {"dmax": d / 1.001, "cmax": c / 1.001, "E": (2 * d * c + d * d + g * (c + d) ** 2 + g * c * c) * 1.001 + 1e-7}


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


class JoinCall:
    """mq_index_self_join on device buffers kept across calls."""

    def __init__(self, ix, left, dev):
        n_left = len(ix) if left is None else left.numel()
        self.ix, self.left = ix, left
        self.scratch = torch.empty(join_scratch_bytes(len(ix), n_left), dtype=torch.uint8, device=dev)
        self.outs = [torch.empty(n_left, dtype=torch.int64, device=dev) for _ in range(3)]
        self.outs += [torch.empty(n_left, dtype=torch.float32, device=dev), torch.empty(4, dtype=torch.int64, device=dev)]

    def __call__(self, mode, tau=TAU):
        self.ix.self_join_device(tau, *self.outs, left_rows=self.left, mode=mode, scratch=self.scratch)
        return self.outs[4]


class RangeCall:
    """The route without the self-join: the stored rows as the queries of the range search."""

    def __init__(self, ix, queries, dev, max_hits=64):
        nq = queries.shape[0]
        self.ix, self.q, self.max_hits = ix, queries, max_hits
        self.scratch = torch.empty(range_scratch_bytes(len(ix), nq, max_hits), dtype=torch.uint8, device=dev)
        self.counts = torch.empty(nq, dtype=torch.int64, device=dev)
        self.scores = torch.empty((nq, max_hits), dtype=torch.float32, device=dev)
        self.ids = torch.empty((nq, max_hits), dtype=torch.int64, device=dev)

    def __call__(self, tau=TAU):
        self.ix.search_range_device(self.q, self.max_hits, self.counts, self.scores, self.ids, tau, None, self.scratch)


def left_list(n, n_left, dev):
    return (torch.arange(n_left, dtype=torch.int64, device=dev) * (n // n_left)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON line to this file too")
    ap.add_argument("--kernels", action="store_true", help="a few calls only, for a kernel trace")
    ap.add_argument("--no-sweep", action="store_true", help="skip the crossover sweep")
    args = ap.parse_args()
    n, dim = args.rows, 768
    dev = torch.device("cuda", 0)
    rows = neardup(n, dim, dev)
    ix = FlatIndex(dim=dim, device=0)
    ix.add_device(rows)
    note("%d rows indexed" % n)
    if args.kernels:
        for n_left in (256, 4096):
            call = JoinCall(ix, left_list(n, n_left, dev), dev)
            for _ in range(3):
                call(_lib.MQ_JOIN_SCREEN)
        call = JoinCall(ix, left_list(n, 256, dev), dev)
        call(_lib.MQ_JOIN_EXACT)
        torch.cuda.synchronize()
        return
    out = {"rows": n, "dim": dim, "reps": args.reps, "min_score": TAU, "slab_GB": round(n * dim * 4 / 1e9, 3),
           "lib": os.path.basename(_lib.LIB_PATH), "bound": bound(rows)}
    for n_left in (256, 4096):
        left = left_list(n, n_left, dev)
        call = JoinCall(ix, left, dev)
        rng = RangeCall(ix, rows[left].contiguous(), dev)
        res = alternate({"screen": lambda: call(_lib.MQ_JOIN_SCREEN), "exact": lambda: call(_lib.MQ_JOIN_EXACT),
                         "search_range_device_max_hits_64": rng}, args.reps)
        info = call(_lib.MQ_JOIN_SCREEN).cpu().tolist()
        same = [a.clone() for a in call.outs[:4]]
        call(_lib.MQ_JOIN_EXACT)
        res["screen_equals_exact"] = all(torch.equal(a, b) for a, b in zip(same, call.outs[:4]))
        res["info_screen"] = info
        res["survivors_per_left_row"] = round(info[2] / n_left, 2)
        out["left_%d_device_ms" % n_left] = res
        note("%d left rows: %s" % (n_left, json.dumps(res)))
        del call, rng
    call = JoinCall(ix, None, dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    info = call(_lib.MQ_JOIN_SCREEN).cpu().tolist()
    b.record()
    b.synchronize()
    out["whole_corpus_screen"] = {"ms": round(a.elapsed_time(b), 1), "info": info,
                                  "survivors_per_left_row": round(info[2] / n, 2),
                                  "rows_with_a_partner": int((call.outs[0] > 0).sum())}
    note("whole corpus: %s" % json.dumps(out["whole_corpus_screen"]))
    del call, ix
    if not args.no_sweep:
        sweep = {}
        for d in (256, 768):
            src = rows if d == dim else neardup(262144, d, dev)
            for m in (1024, 4096, 16384, 65536, 262144):
                if m > n:
                    continue
                sub = FlatIndex(dim=d, device=0)
                sub.add_device(src[:m].contiguous())
                for n_left in (16, 256):
                    call = JoinCall(sub, left_list(m, n_left, dev), dev)
                    sweep["dim%d_rows%d_left%d" % (d, m, n_left)] = alternate(
                        {"screen": lambda: call(_lib.MQ_JOIN_SCREEN), "exact": lambda: call(_lib.MQ_JOIN_EXACT)},
                        args.reps)
                del sub
        out["crossover_device_ms"] = sweep
        note("sweep: %s" % json.dumps(sweep))
    line = json.dumps(out, ensure_ascii=False)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
