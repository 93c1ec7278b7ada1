"""Time the encoder's batched GEMM shapes (M = 8192 = 256 queries x 32 tokens, BERT-base)
on the exact-f32 tiles, the split-f32 (x6) tiles of gemm_f32.hpp and the pre-split K2p
tiles (gemm_x6p.hip).  Prints one JSON line per (shape, kernel): us per launch and
fp32-equivalent TFLOP/s (2 M N K / t).  Run on the GPU box from the repo root."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mediquery-rag_amd"))

import torch  # noqa: E402

from mediquery_hip import _lib  # noqa: E402

SHAPES = {"qkv": (8192, 2304, 768, 0), "out_proj": (8192, 768, 768, 3), "ffn_up": (8192, 3072, 768, 1),
          "ffn_down": (8192, 768, 3072, 3), "kv_last": (8192, 1536, 768, 0)}


REPS = 3


def timed(fn, iters):
    """Median over REPS runs of `iters` back-to-back launches (us per launch)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    runs = []
    for _ in range(REPS):
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) * 1000.0 / iters)
    return sorted(runs)[len(runs) // 2]


def ab(a, dev, st):
    """--ab OLD:NEW[,OLD:NEW...]: per shape, time the two K2p tile codes of each pair in one
    process, alternating (old, new, old, new, ...) `--reps` times on the same random
    operands; one JSON line per (shape, pair) with every round's us per launch and each arm's
    round-to-round spread (max - min over its median).  With --ln-fold the launches carry the
    LayerNorm-fold epilogues (mq_debug_gemm_x6p_ln: the producer, epi 5 with stats_in, for the
    residual shapes, the consumers 6 / 7 / 8 for the others), e.g. --ab 20:0 for the producer's
    former epilogue against the loader-wave hand-off on tile 0.  Codes 20 / 21 differ from 0 / 1
    on the producer shapes (out_proj, ffn_down; --ln-fold only) and on the GELU kinds (ffn_up, or
    --epi 1 / 2: the split epilogue, with and without --ln-fold): a pair that names them skips the
    others (it would time one kernel twice).  --epi overrides the kind of the non-residual
    shapes (0 bias, 1 GELU erf, 2 GELU tanh; with --ln-fold 6 / 7 / 8)."""
    pairs = [tuple(int(t) for t in p.split(":")) for p in a.ab.split(",")]
    out_f = open(a.out, "a") if a.out else None
    for name in a.shapes.split(","):
        M, N, K, epi = SHAPES[name]
        if a.epi >= 0 and epi != 3:
            epi = a.epi
        g = torch.Generator(device=dev).manual_seed(1)
        A = torch.randn(M, K, device=dev, generator=g)
        W = torch.randn(N, K, device=dev, generator=g) * 0.05
        b = torch.randn(N, device=dev, generator=g)
        R = torch.randn(M, N, device=dev, generator=g)
        out = torch.empty(M, N, device=dev)
        w3 = torch.empty(_lib.lib().mq_debug_w3_bytes(N, K), dtype=torch.uint8, device=dev)
        _lib.call("mq_debug_split_w3", _lib.ptr(W), N, K, _lib.ptr(w3), st)
        ref = A.double() @ W.double().T + b.double() if a.check else None
        fepi = 5 if epi == 3 else 6 + epi
        has_former = epi in (1, 2) and not a.check or (a.ln_fold and fepi == 5) or a.split_bias
        if not has_former:
            pairs_here = [p for p in pairs if not {20, 21} & set(p)]
        else:
            pairs_here = pairs
        if a.ln_fold:
            gam = torch.ones(max(N, K), device=dev)
            bet = torch.zeros(max(N, K), device=dev)
            s_fold = torch.zeros(N, device=dev)
            stats_in = torch.zeros(M, 8, 2, device=dev)
            stats_in[:, :, 1] = 96.0
            stats_out = torch.empty(M, 8, 2, device=dev)

        def run(t):
            if a.ln_fold:
                _lib.call("mq_debug_gemm_x6p_ln", _lib.ptr(A), _lib.ptr(w3), _lib.ptr(b), _lib.ptr(R), _lib.ptr(out),
                          M, N, K, fepi, t, _lib.ptr(stats_in), _lib.ptr(stats_out), _lib.ptr(gam), _lib.ptr(bet),
                          _lib.ptr(s_fold), 1e-12, st)
                return
            _lib.call("mq_debug_gemm_x6p", _lib.ptr(A), _lib.ptr(w3), _lib.ptr(b), _lib.ptr(R), _lib.ptr(out),
                      M, N, K, 0 if a.check else epi, t, st)

        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for old, new in pairs_here:
            rounds = {old: [], new: []}
            err = {}
            for t in (old, new):
                for _ in range(a.iters if a.ln_fold else 3):  # (a whole untimed round: the clock settles)
                    run(t)
                if ref is not None:
                    torch.cuda.synchronize()
                    err[t] = float((out.double() - ref).abs().max())
            for _ in range(a.reps):
                for t in (old, new):
                    e0.record()
                    for _ in range(a.iters):
                        run(t)
                    e1.record()
                    torch.cuda.synchronize()
                    rounds[t].append(round(e0.elapsed_time(e1) * 1000.0 / a.iters, 2))
            med = {t: sorted(v)[len(v) // 2] for t, v in rounds.items()}
            spread = {t: round((max(v) - min(v)) / med[t], 4) for t, v in rounds.items()}
            line = json.dumps({"shape": name, "M": M, "N": N, "K": K, "epi": fepi if a.ln_fold else epi,
                               "old_tile": old, "new_tile": new, "old_spread": spread[old],
                               "new_spread": spread[new],
                               "old_us": rounds[old], "new_us": rounds[new], "old_med": med[old],
                               "new_med": med[new], "old_over_new": round(med[old] / med[new], 4),
                               "old_tflops": round(2.0 * M * N * K / med[old] / 1e6, 1),
                               "new_tflops": round(2.0 * M * N * K / med[new] / 1e6, 1),
                               "max_abs_err_f64": err or None})
            print(line, flush=True)
            if out_f:
                out_f.write(line + "\n")
                out_f.flush()


def ln_fold(a, dev, st):
    """--ln-fold: per shape, the plain K2p launch against the same launch with its LayerNorm-fold
    epilogue (mq_debug_gemm_x6p_ln: the producer, epi 5, for the residual shapes, the
    consumers, epi 6 / 7 / 8, for the others), alternating `--reps` times on the default
    tile; one JSON line per shape with every round's us per launch."""
    out_f = open(a.out, "a") if a.out else None
    for name in a.shapes.split(","):
        M, N, K, epi = SHAPES[name]
        g = torch.Generator(device=dev).manual_seed(1)
        A = torch.randn(M, K, device=dev, generator=g)
        W = torch.randn(N, K, device=dev, generator=g) * 0.05
        b = torch.randn(N, device=dev, generator=g)
        R = torch.randn(M, N, device=dev, generator=g)
        out = torch.empty(M, N, device=dev)
        gam = torch.ones(max(N, K), device=dev)
        bet = torch.zeros(max(N, K), device=dev)
        s_fold = torch.zeros(N, device=dev)
        stats_in = torch.zeros(M, 8, 2, device=dev)
        stats_in[:, :, 1] = 96.0
        stats_out = torch.empty(M, 8, 2, device=dev)
        w3 = torch.empty(_lib.lib().mq_debug_w3_bytes(N, K), dtype=torch.uint8, device=dev)
        _lib.call("mq_debug_split_w3", _lib.ptr(W), N, K, _lib.ptr(w3), st)
        fepi = 5 if epi == 3 else 6 + epi

        def plain():
            _lib.call("mq_debug_gemm_x6p", _lib.ptr(A), _lib.ptr(w3), _lib.ptr(b), _lib.ptr(R), _lib.ptr(out),
                      M, N, K, epi, -1, st)

        def fold():
            _lib.call("mq_debug_gemm_x6p_ln", _lib.ptr(A), _lib.ptr(w3), _lib.ptr(b), _lib.ptr(R), _lib.ptr(out),
                      M, N, K, fepi, -1, _lib.ptr(stats_in), _lib.ptr(stats_out), _lib.ptr(gam), _lib.ptr(bet),
                      _lib.ptr(s_fold), 1e-12, st)

        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        rounds = {"plain": [], "fold": []}
        for fn in (plain, fold):
            for _ in range(3):
                fn()
        for _ in range(a.reps):
            for key, fn in (("plain", plain), ("fold", fold)):
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                rounds[key].append(round(e0.elapsed_time(e1) * 1000.0 / a.iters, 2))
        med = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
        line = json.dumps({"shape": name, "M": M, "N": N, "K": K, "epi": epi, "fold_epi": fepi,
                           "plain_us": rounds["plain"], "fold_us": rounds["fold"], "plain_med": med["plain"],
                           "fold_med": med["fold"], "fold_minus_plain_us": round(med["fold"] - med["plain"], 2)})
        print(line, flush=True)
        if out_f:
            out_f.write(line + "\n")
            out_f.flush()


def attn(a, dev, st):
    """--attn: at M = 8192 (256 sequences of 32), K = 768, heads = 12, the QKV launch whose
    epilogue is the attention (mq_debug_gemm_x6p_attn) against the QKV launch + the attention
    launch (mq_debug_gemm_x6p or, with --ln-fold, _ln epi 6; then mq_debug_attention variant
    12), alternating `--reps` times; one JSON line with every round's us and the medians."""
    M, K, heads, L = 8192, 768, 12, 32
    H, N = 64 * heads, 3 * 64 * heads
    g = torch.Generator(device=dev).manual_seed(1)
    A = torch.randn(M, K, device=dev, generator=g)
    W = torch.randn(N, K, device=dev, generator=g) * 0.05
    b = torch.randn(N, device=dev, generator=g)
    mask = torch.ones(M, dtype=torch.int32, device=dev)
    mask.view(-1, L)[::3, 20:] = 0
    qkv = torch.empty(M, N, device=dev)
    ctx_two = torch.empty(M, H, device=dev)
    ctx_fused = torch.empty(M, H, device=dev)
    s_fold = torch.randn(N, device=dev, generator=g) * 0.1
    stats_in = torch.zeros(M, 8, 2, device=dev)
    stats_in[:, :, 1] = 96.0
    w3 = torch.empty(_lib.lib().mq_debug_w3_bytes(N, K), dtype=torch.uint8, device=dev)
    _lib.call("mq_debug_split_w3", _lib.ptr(W), N, K, _lib.ptr(w3), st)
    epi = 10 if a.ln_fold else 9

    def two():
        if a.ln_fold:
            _lib.call("mq_debug_gemm_x6p_ln", _lib.ptr(A), _lib.ptr(w3), _lib.ptr(b), None, _lib.ptr(qkv), M, N, K, 6,
                      0, _lib.ptr(stats_in), None, None, None, _lib.ptr(s_fold), 1e-12, st)
        else:
            _lib.call("mq_debug_gemm_x6p", _lib.ptr(A), _lib.ptr(w3), _lib.ptr(b), None, _lib.ptr(qkv), M, N, K, 0, 0,
                      st)
        _lib.call("mq_debug_attention", _lib.ptr(qkv), _lib.ptr(mask), M // L, L, H, heads, 0.125, 12,
                  _lib.ptr(ctx_two), st)

    def fused():
        _lib.call("mq_debug_gemm_x6p_attn", _lib.ptr(A), _lib.ptr(w3), _lib.ptr(b), _lib.ptr(mask),
                  _lib.ptr(ctx_fused), M, K, heads, 0.125, epi, _lib.ptr(stats_in), _lib.ptr(s_fold), 1e-12, 0, st)

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rounds = {"two": [], "fused": []}
    for fn in (two, fused):
        for _ in range(a.iters):  # (a whole untimed round: the clock settles)
            fn()
    torch.cuda.synchronize()
    diff = float((ctx_two - ctx_fused).abs().max())
    for _ in range(a.reps):
        for key, fn in (("two", two), ("fused", fused)):
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            rounds[key].append(round(e0.elapsed_time(e1) * 1000.0 / a.iters, 2))
    med = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
    line = json.dumps({"shape": "qkv_attn", "M": M, "K": K, "heads": heads, "epi": epi, "two_us": rounds["two"],
                       "fused_us": rounds["fused"], "two_med": med["two"], "fused_med": med["fused"],
                       "two_minus_fused_us": round(med["two"] - med["fused"], 2),
                       "max_abs_diff_ctx": diff})
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attn", action="store_true",
                    help="the QKV launch with the attention epilogue vs QKV + attention launches (see attn()); "
                         "with --ln-fold: the folded kinds")
    ap.add_argument("--ln-fold", action="store_true",
                    help="plain vs LayerNorm-fold epilogue per shape (see ln_fold()); with --ab: the pairs on the "
                         "LayerNorm-fold epilogues")
    ap.add_argument("--ab", default="", help="OLD:NEW tile code pairs to time alternating (see ab())")
    ap.add_argument("--out", default="", help="--ab / --attn: also append the JSON lines to this file")
    ap.add_argument("--check", action="store_true", help="--ab: bias epilogue, report max |err| vs float64")
    ap.add_argument("--epi", type=int, default=-1, choices=[-1, 0, 1, 2],
                    help="--ab: the kind of the non-residual shapes (default: the shape's own)")
    ap.add_argument("--split-bias", action="store_true",
                    help="--ab: the library was built with -DMQ_X6P_SPLIT_BIAS=1, so 20 / 21 differ on the bias "
                         "kinds too")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--f32-tiles", default="0,1,5,6,7")
    ap.add_argument("--x6p-tiles", default="-1,0,1,2,3")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    global REPS
    REPS = a.reps
    dev = torch.device("cuda", 0)
    st = _lib.stream_handle()
    if a.attn:
        attn(a, dev, st)
        return
    if a.ab:
        ab(a, dev, st)
        return
    if a.ln_fold:
        ln_fold(a, dev, st)
        return
    for name in a.shapes.split(","):
        M, N, K, epi = SHAPES[name]
        g = torch.Generator(device=dev).manual_seed(1)
        A = torch.randn(M, K, device=dev, generator=g)
        W = torch.randn(N, K, device=dev, generator=g) * 0.05
        b = torch.randn(N, device=dev, generator=g)
        R = torch.randn(M, N, device=dev, generator=g)
        out = torch.empty(M, N, device=dev)
        w3 = torch.empty(_lib.lib().mq_debug_w3_bytes(N, K), dtype=torch.uint8, device=dev)
        _lib.call("mq_debug_split_w3", _lib.ptr(W), N, K, _lib.ptr(w3), st)
        flop = 2.0 * M * N * K
        ref = None
        for t in [int(x) for x in a.f32_tiles.split(",") if x]:
            us = timed(lambda: _lib.call("mq_debug_gemm_f32", _lib.ptr(A), _lib.ptr(W), _lib.ptr(b), _lib.ptr(R),
                                         _lib.ptr(out), M, N, K, epi, t, st), a.iters)
            if t == 5:
                ref = out.clone()
            print(json.dumps({"shape": name, "kernel": "f32_tile%d" % t, "us": round(us, 2),
                              "tflops": round(flop / us / 1e6, 2)}), flush=True)
        for t in [int(x) for x in a.x6p_tiles.split(",") if x]:
            us = timed(lambda: _lib.call("mq_debug_gemm_x6p", _lib.ptr(A), _lib.ptr(w3), _lib.ptr(b), _lib.ptr(R),
                                         _lib.ptr(out), M, N, K, epi, t, st), a.iters)
            same = None if ref is None else bool(torch.equal(out, ref))
            print(json.dumps({"shape": name, "kernel": "x6p_tile%d" % t, "us": round(us, 2),
                              "tflops": round(flop / us / 1e6, 2), "frac_417": round(flop / us / 1e6 / 416.7, 3),
                              "bit_identical_to_x6": same}), flush=True)


if __name__ == "__main__":
    main()
