"""The device MMR selection against float64 on the random class of tests/mmr_cases.py, over
more queries than the test takes: per configuration the share of steps at which the device's
pick is not the float64 argmax of its own prefix, and the largest float64 deficit (best
unpicked score minus the pick's) among them.  The test's bound is 1e-5.

  python tools/mmr_accuracy.py [--queries 256] [--out profiles/mmr/accuracy.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mediquery-rag_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import mmr_cases as mc  # noqa: E402
from mediquery_hip import _lib  # noqa: E402
from mediquery_hip.native import FlatIndex  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmr", "accuracy.txt"))
    args = ap.parse_args()
    lines = ["device MMR selection vs float64 along the device's own path (tests/mmr_cases.py random class,",
             "%d queries per line; deficit = best unpicked float64 score - the pick's; bound 1e-5)" % args.queries,
             "%-5s %-8s %-3s %-7s %-10s %-12s %-12s %s" % ("dim", "fetch_k", "k", "lambda", "steps", "off-argmax",
                                                         "max deficit", "path == float64 sequence")]
    worst = 0.0
    for dim in (32, 96, 768):
        ix = FlatIndex(dim=dim, device=0)
        ix.add(mc.random_corpus(dim))
        stored = ix.get()
        queries = mc.random_queries(stored, args.queries, seed=2)
        for fetch_k in (20, 64):
            cands = [mc.top_candidates(stored, q, fetch_k) for q in queries]
            ci = np.stack([c[0] for c in cands])
            s64 = np.stack([c[1] for c in cands])
            G64 = [mc.gram64(stored, ids) for ids in ci]
            for k in (5, 16):
                for lam in (0.25, 0.5, 0.9):
                    _, gi = ix.mmr_select(s64.astype(np.float32), ci, k, lam)
                    lam32 = float(np.float32(lam))
                    steps = off = same = 0
                    dmax = 0.0
                    for q in range(len(queries)):
                        picks = mc.positions(gi[q], ci[q])
                        assert mc.check_path(picks, s64[q], G64[q], lam32, np.inf, k) == [], (dim, fetch_k, k, lam, q)
                        d = mc.path_deficits(picks, s64[q], G64[q], lam32)
                        steps += len(d)
                        off += sum(x > 0 for x in d)
                        dmax = max([dmax] + d)
                        same += picks == mc.mmr_reference(s64[q], G64[q], lam32, k)
                    worst = max(worst, dmax)
                    lines.append("%-5d %-8d %-3d %-7g %-10d %-12d %-12.3g %d / %d"
                                 % (dim, fetch_k, k, lam, steps, off, dmax, same, len(queries)))
    lines.append("largest deficit over all lines: %.3g" % worst)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
