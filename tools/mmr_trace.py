"""Per-dispatch durations of mmr_select_kernel from a rocprofv3 kernel trace:
the 1M x 768 index (fetch_k 20 / 64, one query / 256) and 20k-row indexes of dim 128, 256, 768
and 1024 (1, 2, 6 and 8 K-slices), which split the kernel's fixed time from its time per slice.

  rocprofv3 --kernel-trace --output-format csv -d OUT -o mmr -- python tools/mmr_trace.py > OUT/run.log
  python tools/mmr_trace.py --summarize OUT      # -> the table of profiles/mmr/kernel_trace.txt
"""
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mediquery-rag_amd"), ROOT]
REPS = 12


def summarize(out_dir):
    trace = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)[0]
    with open(trace) as f:
        rows = [r for r in csv.DictReader(f) if "mmr_select_kernel" in r["Kernel_Name"]]
    with open(os.path.join(out_dir, "run.log")) as f:
        order = [line.split()[1:] for line in f if line.startswith("ORDER")]
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    assert len(us) == REPS * len(order), (len(us), len(order))
    print("mmr_select_kernel, %d dispatches each (k = 5, lambda 0.5), us" % REPS)
    print("%-6s %-5s %-8s %-4s %-8s %-8s %-8s" % ("rows", "dim", "fetch_k", "nq", "median", "min", "max"))
    for i, o in enumerate(order):
        x = us[REPS * i:REPS * (i + 1)]
        print("%-6s %-5s %-8s %-4s %-8.2f %-8.2f %-8.2f" % (*o, statistics.median(x), min(x), max(x)))


def main():
    import torch
    from mediquery_hip import _lib, synth
    from mediquery_hip.native import FlatIndex
    dev = torch.device("cuda", 0)

    def run(ix, qd, fetch_k, nq, k=5):
        cs = torch.empty((nq, fetch_k), dtype=torch.float32, device=dev)
        ci = torch.empty((nq, fetch_k), dtype=torch.int64, device=dev)
        ix.search_device(qd[:nq].contiguous(), fetch_k, cs, ci)
        os_ = torch.empty((nq, k), dtype=torch.float32, device=dev)
        oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        for _ in range(REPS):
            ix.mmr_select_device(cs, ci, k, 0.5, os_, oi)
            torch.cuda.synchronize()

    order = []
    for dim in (128, 256, 768, 1024):
        rows = torch.randn((20000, dim), device=dev)
        ix = FlatIndex(dim=dim, device=0)
        ix.add_device(rows)
        qd = torch.nn.functional.normalize(rows[:256] + 0.05 * torch.randn((256, dim), device=dev), dim=1)
        for fetch_k in (20, 64):
            for nq in (1, 256):
                run(ix, qd, fetch_k, nq)
                order.append(("20k", dim, fetch_k, nq))
    rows, _ = synth.clustered_corpus_device(1_000_000, 768, dev)
    ix = FlatIndex(dim=768, capacity=1_000_000, device=0)
    for r0 in range(0, 1_000_000, 1 << 18):
        ix.add_device(rows[r0:r0 + (1 << 18)].contiguous())
    ix.set_precision(_lib.MQ_DTYPE_F32_SCREEN)
    qd, _ = synth.queries_device(256, rows)
    for fetch_k in (20, 64):
        for nq in (1, 256):
            run(ix, qd, fetch_k, nq)
            order.append(("1M", 768, fetch_k, nq))
    for o in order:  # the dispatch groups, in trace order
        print("ORDER", *o)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        main()
