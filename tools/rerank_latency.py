"""What cross-encoder reranking costs: one query x {5, 20, 64} documents at pair
lengths 128 and 512, BERT-base with the seeded weights and head, both precisions.

Per case, the p50 (and range) of warmed calls:
  * tokenize  - NativeTokenizer.pairs on (query, document) strings of that length (host only);
  * score     - Encoder.score on the token arrays, host pointers (the call synchronises);
  * device    - Encoder.score_device on device tensors, timed with HIP events on the stream;
  * head      - cls_head_kernel alone (mq_debug_cls_head on [n, 768] rows), HIP events.

  python tools/rerank_latency.py [--reps 30] [--out profiles/rerank/latency.json]
  python tools/rerank_latency.py --trace   # a few scoring calls only (for a kernel trace)
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
from mediquery_hip.config import DMETA_BASE  # noqa: E402
from mediquery_hip.native import Encoder  # noqa: E402
from mediquery_hip.tokenizer import NativeTokenizer  # noqa: E402
from mediquery_hip.weights import HEAD_NAMES, synthetic_head_state_dict  # noqa: E402

PRECS = {"f32": _lib.MQ_DTYPE_F32, "f32x6": _lib.MQ_DTYPE_F32X6}
QUERY = "2型糖尿病患者的饮食应该注意什么？"
DOC = "糖尿病患者应控制总热量摄入，均衡饮食，定时定量进餐，少吃高糖高脂食物，多吃蔬菜和全谷物，并遵医嘱监测血糖。"


def spread(xs, digits=4):
    return {"p50": round(statistics.median(xs), digits), "min": round(min(xs), digits),
            "max": round(max(xs), digits), "n": len(xs)}


def wall_ms(fn, reps, warmup=3):
    out = []
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if it >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def event_ms(fn, reps, warmup=3):
    out = []
    for it in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--trace", action="store_true", help="three scoring calls of 20 x 128 per precision, no report")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerank", "latency.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = DMETA_BASE
    enc = Encoder(cfg)
    head = synthetic_head_state_dict(cfg, 0)
    enc.load_head(head)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = {"model": "BERT-base (seeded weights + head), 1 label", "device": torch.cuda.get_device_name(0),
           "reps": args.reps, "unit": "ms", "cases": {}}
    for pname, prec in PRECS.items():
        enc.set_precision(prec)
        for L in (128, 512):
            tok = NativeTokenizer.char(cfg.vocab_size, max_length=L)
            doc = DOC * (L // len(DOC) + 3)  # longer than L + 64: every pair is truncated to exactly L tokens
            for n in (5, 20, 64):
                if args.trace and (n, L) != (20, 128):
                    continue
                firsts, seconds = [QUERY] * n, [doc[i:] for i in range(n)]
                ids, types, mask = tok.pairs(firsts, seconds)
                assert ids.shape == (n, L) and mask.all()
                if args.trace:
                    for _ in range(3):
                        enc.score(ids, types, mask)
                    continue
                dids, dtypes, dmask = t(ids), t(types), t(mask)
                dout = torch.empty((n, 1), device=dev)
                rows = torch.randn((n, cfg.hidden), device=dev)
                dw = [t(head[k]) for k in HEAD_NAMES]
                dlog = torch.empty((n, 1), device=dev)
                case = {
                    "tokenize": spread(wall_ms(lambda: tok.pairs(firsts, seconds), args.reps)),
                    "score": spread(wall_ms(lambda: enc.score(ids, types, mask), args.reps)),
                    "device": spread(event_ms(lambda: enc.score_device(dids, dtypes, dmask, dout), args.reps)),
                    "head": spread(event_ms(lambda: _lib.call(
                        "mq_debug_cls_head", _lib.ptr(rows), n, cfg.hidden, *[_lib.ptr(w) for w in dw], 1,
                        _lib.ptr(dlog), _lib.stream_handle()), args.reps)),
                }
                out["cases"]["%s docs=%d L=%d" % (pname, n, L)] = case
                print(pname, n, L, json.dumps(case), flush=True)
    if args.trace:
        torch.cuda.synchronize()
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
