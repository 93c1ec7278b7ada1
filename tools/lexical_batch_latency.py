"""Batched against looped BM25 at the VectorStore surface: the store of tools/lexical_latency.py
(N rows of the synthetic documents, one token id per character) and batches of 1 / 2 / 4 / 16 / 64 /
256 query texts of 12 and of 30 characters.  In one process, alternating repetition by repetition:

  looped    one `_TokenMirror.plan` / `topk` per query: a df pass per query with uncached terms, one
            mq_lex_topk launch and one device-to-host copy per query (what the batch methods did
            before the batch path, and what one query alone still does);
  batched   one `plan_batch` (one mq_lex_df_batch) and one `topk_batch` (one mq_lex_topk_batch: a scan
            per group of up to 16 queries, one copy of the [nq, k] result);

each with the df cache emptied before every repetition ("cold") and kept ("warm"), then
`lexical_search_batch` and `hybrid_search_batch` end to end on either path (the looped one by
raising `vectorstore.LEX_BATCH_MIN`) beside `similarity_search_batch`.  Every figure is the p50 and
the [min, max] range of --reps repetitions in ms; a comparison counts only where the two ranges do
not overlap ("separated").  The number of groups is the ABI's grouping rule restated (at most 16
queries, 512 distinct keys and 1024 term slots a group, cut in order), and the token GB/s is the
mirror's bytes times the groups over the batched score call.  Both paths must return identical
ids and scores, or the tool fails.

  timeout -k 10 900 python tools/lexical_batch_latency.py [--rows 1000000] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mediquery-rag_amd"), ROOT, os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mediquery_hip import _lib, synth, vectorstore  # noqa: E402
from mediquery_hip.embeddings import HipBertEmbeddings  # noqa: E402
from mediquery_hip.vectorstore import HipChroma  # noqa: E402
from where_document_latency import synthetic_texts  # noqa: E402

TERM_SLOTS = 1024  # term slots of a group (csrc/lexical.hip, kBTerms)


def note(msg):
    print("[lexical_batch_latency] " + msg, file=sys.stderr, flush=True)


def groups_of(plans):
    """The number of scans mq_lex_topk_batch runs for these plans: the batch cut in order into
    groups of at most MQ_LEX_BATCH_GROUP queries, MQ_LEX_BATCH_UNION distinct keys and TERM_SLOTS
    terms."""
    count, union, n_q, terms = 0, set(), 0, 0
    for keys, _, _, _ in plans:
        ks = set(int(x) for x in keys)
        if count == 0 or n_q == _lib.MQ_LEX_BATCH_GROUP or terms + len(ks) > TERM_SLOTS \
                or len(union | ks) > _lib.MQ_LEX_BATCH_UNION:
            count, union, n_q, terms = count + 1, set(), 0, 0
        union |= ks
        n_q += 1
        terms += len(ks)
    return count


def stats(ms):
    return {"p50": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def separated(a, b):
    """a's range lies wholly below b's."""
    return a["max"] < b["min"]


def alternate(fns, reps, warm=1):
    """Run the functions in turn, `reps` times each after `warm` unrecorded rounds -> ms lists."""
    out = [[] for _ in fns]
    for it in range(reps + warm):
        for j, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= warm:
                out[j].append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 4, 16, 64, 256],
                    help="batch sizes (2 and 4 locate the crossover behind vectorstore.LEX_BATCH_MIN)")
    ap.add_argument("--out", default=None, help="append the JSON line to this file too")
    args = ap.parse_args()
    n = args.rows
    dev = torch.device("cuda", 0)
    texts = synthetic_texts(n)
    emb_fn = HipBertEmbeddings(synthetic=True)
    rows = torch.nn.functional.normalize(synth.corpus_device(n, 768, dev), dim=1).cpu().numpy()
    store = HipChroma(embedding_function=emb_fn, dim=768, auto_persist=False)
    store.add_embeddings(rows, texts, [{} for _ in range(n)], ["id%d" % i for i in range(n)])
    del rows
    mir = store._lex()
    torch.cuda.synchronize()
    token_bytes = 2 * mir.n_tokens
    out = {"rows": n, "lib": os.path.basename(_lib.LIB_PATH), "tokens": mir.n_tokens, "reps": args.reps, "k": 5, "fetch_k": 20,
           "lex_batch_min": vectorstore.LEX_BATCH_MIN, "cases": {}}
    note("store and mirror of %d rows, %d tokens built" % (n, mir.n_tokens))
    k1, b = store._bm25
    batch_min = vectorstore.LEX_BATCH_MIN

    for chars in (12, 30):
        pool = [t[3:3 + chars] for t in texts[1000:200000] if len(t) >= chars + 3]
        for nq in args.batches:
            qs = pool[:nq]
            case = {"query_chars": chars, "queries": nq}

            def looped(cold):
                if cold:
                    mir.df = {}
                res = []
                for q in qs:
                    plan = mir.plan(q, k1, b)
                    res.append(mir.topk(plan, 5, None) if plan is not None else None)
                return res

            def batched(cold):
                if cold:
                    mir.df = {}
                plans = mir.plan_batch(qs, k1, b)
                live = [p for p in plans if p is not None]
                s, i = mir.topk_batch(live, 5, None)
                it = iter(zip(s, i))
                return [next(it) if p is not None else None for p in plans]

            # parity first: identical ids and scores, bit for bit
            for x, y in zip(looped(True), batched(True)):
                assert (x is None) == (y is None)
                if x is not None:
                    assert np.array_equal(x[1], y[1]) and x[0].tobytes() == y[0].tobytes(), (chars, nq)
            plans = [p for p in mir.plan_batch(qs, k1, b) if p is not None]
            case["groups"] = groups_of(plans)
            case["terms_mean"] = round(float(np.mean([len(p[0]) for p in plans])), 1)
            for name, cold in (("cold", True), ("warm", False)):
                lo, ba = alternate([lambda: looped(cold), lambda: batched(cold)], args.reps)
                case["lexical_%s_looped_ms" % name], case["lexical_%s_batched_ms" % name] = stats(lo), stats(ba)
                case["lexical_%s_separated" % name] = separated(stats(ba), stats(lo)) or separated(stats(lo), stats(ba))
            # the score call alone (plans made, df cached): per-group scan rate
            sc, = alternate([lambda: mir.topk_batch(plans, 5, None)], args.reps)
            case["topk_batch_ms"] = stats(sc)
            case["group_scan_token_GBps"] = round(token_bytes * case["groups"] / statistics.median(sc) / 1e6, 1)

            # end to end on either path
            def with_min(value, fn):
                def run():
                    vectorstore.LEX_BATCH_MIN = value
                    try:
                        return fn()
                    finally:
                        vectorstore.LEX_BATCH_MIN = batch_min
                return run

            lex = lambda: store.lexical_search_batch(qs, k=5)  # noqa: E731
            hyb = lambda: store.hybrid_search_batch(qs, k=5, fetch_k=20)  # noqa: E731
            a, c = with_min(1 << 30, lex)(), with_min(2, lex)()
            assert [[d.id for d in h] for h in a] == [[d.id for d in h] for h in c], (chars, nq)
            a, c = with_min(1 << 30, hyb)(), with_min(2, hyb)()
            assert [[d.id for d in h] for h in a] == [[d.id for d in h] for h in c], (chars, nq)
            t = alternate([with_min(1 << 30, lex), with_min(2, lex), with_min(1 << 30, hyb), with_min(2, hyb),
                           lambda: store.similarity_search_batch(qs, k=5)], args.reps)
            for key, ms in zip(("lexical_search_batch_looped_ms", "lexical_search_batch_batched_ms",
                                "hybrid_search_batch_looped_ms", "hybrid_search_batch_batched_ms",
                                "similarity_search_batch_ms"), t):
                case[key] = stats(ms)
            case["hybrid_separated_batched_lower"] = separated(case["hybrid_search_batch_batched_ms"],
                                                               case["hybrid_search_batch_looped_ms"])
            case["lexical_separated_batched_lower"] = separated(case["lexical_search_batch_batched_ms"],
                                                                case["lexical_search_batch_looped_ms"])
            out["cases"]["chars%d_q%d" % (chars, nq)] = case
            note("%d chars x %d queries: %d groups, hybrid looped %.2f ms, batched %.2f ms (dense %.2f ms)"
                 % (chars, nq, case["groups"], case["hybrid_search_batch_looped_ms"]["p50"],
                    case["hybrid_search_batch_batched_ms"]["p50"], case["similarity_search_batch_ms"]["p50"]))
    line = json.dumps(out, ensure_ascii=False)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
