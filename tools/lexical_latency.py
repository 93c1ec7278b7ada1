"""BM25 lexical and hybrid retrieval cost at the VectorStore surface: `HipChroma` over N rows of
the synthetic documents of tools/where_document_latency.py (the golden corpus's characters at
its length distribution, three marker strings planted in ~1/1000, ~1/16 and ~1/2 of the rows),
tokenised one id per character.  Reports: the token mirror's build time (tokenisation + upload)
and HBM bytes; the df pass (mq_lex_df) and the score pass (mq_lex_topk) for queries of 4 / 16 /
64 terms, "frequent" (characters of the alphabet: each in roughly a tenth of the rows) and "rare"
(the markers' characters, then characters no row holds), with the token GB/s each implies;
single-query `lexical_search` (df cache cold and warm) and `hybrid_search` end to end beside
`similarity_search` from the same run; and the same queries through a float64 numpy BM25 over the
host tokens, the CPU baseline, whose top-k the device's must equal.

  python tools/lexical_latency.py [--rows 1000000] [--iters 30] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mediquery-rag_amd"), ROOT, os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mediquery_hip import _lib, synth  # noqa: E402
from mediquery_hip.embeddings import HipBertEmbeddings  # noqa: E402
from mediquery_hip.native import lex_df, lex_topk  # noqa: E402
from mediquery_hip.vectorstore import HipChroma, bm25_plan, body_tokens  # noqa: E402
from where_document_latency import MARKERS, p50, synthetic_texts  # noqa: E402


def host_bm25(flat, offs, keys, w, c0, c1, k):
    """Float64 numpy BM25 (ngram 1) over the host tokens -> the top-k row ids."""
    n = len(offs) - 1
    slot = np.searchsorted(keys, flat)
    slot[slot == len(keys)] = 0
    hit = np.flatnonzero(keys[slot] == flat)
    rows = np.searchsorted(offs, hit, side="right") - 1
    tf = np.zeros((n, len(keys)), np.float64)
    np.add.at(tf, (rows, slot[hit]), 1.0)
    norm = float(c0) + float(c1) * np.diff(offs).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        score = np.where(tf > 0, w.astype(np.float64)[None, :] * tf / (tf + norm[:, None]), 0.0).sum(axis=1)
    cand = np.flatnonzero(tf.sum(axis=1) > 0)
    return cand[np.lexsort((cand, -score[cand]))[:k]]


def note(msg):
    print("[lexical_latency] " + msg, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=30)
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
    out = {"rows": n}
    note("store of %d rows built" % n)

    # the mirror: tokenisation (chunked) + upload of every document, at the first lexical use
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mir = store._lex()
    torch.cuda.synchronize()
    out["mirror_build_s"] = round(time.perf_counter() - t0, 3)
    out["tokens"] = mir.n_tokens
    out["avgdl"] = round(mir.sum_dl / mir.n, 2)
    out["mirror_hbm_bytes"] = 2 * mir.n_tokens + 8 * (mir.n + 1)
    out["mirror_allocated_bytes"] = mir.nbytes()
    tokens, offs = mir._views()
    tok = store._lex_tok()
    note("mirror of %d tokens built in %.1f s" % (mir.n_tokens, out["mirror_build_s"]))
    token_bytes = 2 * mir.n_tokens

    # queries: characters as the tokenizer numbers them
    alphabet = sorted(set("".join(texts[:2000])) - set("".join(m for _, m, _ in MARKERS)))
    rare_chars = list(dict.fromkeys("".join(m for _, m, _ in MARKERS)))
    rare_chars += [chr(c) for c in range(0x3400, 0x3400 + 64)]  # CJK extension A: in no row
    rng = np.random.default_rng(0)

    def ids_of(chars):
        return np.unique(body_tokens(tok, ["".join(chars)])[0]).astype(np.uint32)

    passes = {}
    for kind, pool in (("frequent", list(rng.permutation(alphabet))), ("rare", rare_chars)):
        for n_terms in (4, 16, 64):
            keys = ids_of(pool[:n_terms + 8])[:n_terms]
            df = lex_df(tokens, offs, 1, keys, scratch=mir.scratch)
            k_, w, c0, c1 = bm25_plan(keys, np.ones(len(keys)), df, mir.n, mir.sum_dl / mir.n, 1.2, 0.75)

            def df_pass(_):
                lex_df(tokens, offs, 1, keys, scratch=mir.scratch)  # synchronous

            def score_pass(_):
                lex_topk(tokens, offs, 1, k_, w, c0, c1, 5, scratch=mir.scratch)
                torch.cuda.synchronize()
            d_ms, s_ms = p50(df_pass, args.iters), p50(score_pass, args.iters)
            passes["%s_%d" % (kind, n_terms)] = {
                "terms": int(len(keys)), "df_min": int(df.min()), "df_max": int(df.max()),
                "df_pass_ms": d_ms, "df_pass_token_GBps": round(token_bytes / d_ms / 1e6, 1),
                "score_pass_ms": s_ms, "score_pass_token_GBps": round(token_bytes / s_ms / 1e6, 1)}
            note("%s %d terms: df pass %.3f ms, score pass %.3f ms" % (kind, n_terms, d_ms, s_ms))
    out["passes"] = passes

    # end to end, one query text at a time (a fresh text every call; k = 5)
    qtexts = [t[3:3 + 12] for t in texts[1000:1064]]
    qtexts[::4] = [t[:6] + MARKERS[0][1] for t in qtexts[::4]]

    def cold(i):
        mir.df = {}
        store.lexical_search(qtexts[i % 64], k=5)
    out["lexical_search_df_cold_ms"] = p50(cold, args.iters)
    for q in qtexts:
        store.lexical_search(q, k=5)
    out["lexical_search_df_warm_ms"] = p50(lambda i: store.lexical_search(qtexts[i % 64], k=5), args.iters)
    out["similarity_search_ms"] = p50(lambda i: store.similarity_search(qtexts[i % 64], k=5), args.iters)
    out["hybrid_search_ms"] = p50(lambda i: store.hybrid_search(qtexts[i % 64], k=5, fetch_k=20), args.iters)

    note("end-to-end timings done")
    # the CPU baseline: float64 numpy over the host tokens (tokenised again, chunk by chunk)
    t0 = time.perf_counter()
    parts = [body_tokens(tok, texts[at:at + 4096]) for at in range(0, n, 4096)]
    out["host_tokenise_s"] = round(time.perf_counter() - t0, 3)
    flat = np.concatenate([p[0] for p in parts]).astype(np.uint32)
    hoffs = np.zeros(n + 1, np.int64)
    np.cumsum(np.concatenate([p[1] for p in parts]), out=hoffs[1:])
    del parts
    host = {}
    for name, q in (("query_12_chars", qtexts[1]), ("query_with_marker", qtexts[0])):
        plan = mir.plan(q, 1.2, 0.75)
        t0 = time.perf_counter()
        want = host_bm25(flat, hoffs, *plan, 5)
        ms = (time.perf_counter() - t0) * 1e3
        _, got = mir.topk(plan, 5, None)
        host[name] = {"terms": int(len(plan[0])), "host_numpy_ms": round(ms, 1),
                      "device_top5_equal": bool(np.array_equal(got[got >= 0], want))}
    out["host_baseline"] = host
    line = json.dumps(out, ensure_ascii=False)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
