"""`where_document` ($contains) cost at the VectorStore surface: `HipChroma` over N rows of
synthetic text drawn from the golden corpus's characters at the golden corpus's length
distribution, with three marker strings planted in ~1/1000, ~1/16 and ~1/2 of the rows.
Reports: the device text mirror's build time and size; the mask build (mq_mask_contains) per
condition with the text GB/s it implies; single-query p50 with a fresh clause every call, a
repeated clause (served from the store's one-entry mask cache) and no clause; the 256-query
batch with and without a clause; and, in the same run, the host way the kernel replaces: Python
`in` over the documents, numpy packbits, upload.

  python tools/where_document_latency.py [--rows 1000000] [--iters 50] [--out FILE]
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
from mediquery_hip import _lib, synth  # noqa: E402
from mediquery_hip.vectorstore import HipChroma  # noqa: E402

MARKERS = (("1000th", "二甲双胍缓释片", 1000), ("16th", "糖化血红蛋白", 16), ("half", "血压", 2))


def synthetic_texts(n, seed=0):
    with open(os.path.join(ROOT, "tests", "golden", "corpus_docs.json"), encoding="utf-8") as f:
        docs = [d["page_content"] for d in json.load(f)["docs"]]
    # the markers' characters stay out of the alphabet, so only planted markers match
    chars = sorted(set("".join(docs)) - set("".join(m for _, m, _ in MARKERS)))
    codes = np.array([ord(c) for c in chars], dtype=np.uint32)
    rng = np.random.default_rng(seed)
    lens = np.array([len(d) for d in docs])[rng.integers(0, len(docs), n)]
    ends = np.cumsum(lens)
    big = codes[rng.integers(0, len(codes), int(ends[-1]))].astype("<u4").tobytes().decode("utf-32-le")
    plant = [rng.random(n) < 1.0 / every for _, _, every in MARKERS]
    where = rng.random(n)
    texts, start = [], 0
    for r in range(n):
        t = big[start:int(ends[r])]
        start = int(ends[r])
        planted = "".join(marker for j, (_, marker, _) in enumerate(MARKERS) if plant[j][r])
        if planted:  # side by side at one random position: no marker cuts another
            cut = int(where[r] * len(t))
            t = t[:cut] + planted + t[cut:]
        texts.append(t)
    return texts


def p50(fn, iters, warm=3):
    lat = []
    for it in range(iters + warm):
        a = time.perf_counter()
        fn(it)
        if it >= warm:
            lat.append((time.perf_counter() - a) * 1e3)
    return round(statistics.median(lat), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="append the JSON line to this file too")
    args = ap.parse_args()
    n = args.rows
    dev = torch.device("cuda", 0)
    texts = synthetic_texts(n)
    emb = torch.nn.functional.normalize(synth.corpus_device(n, 768, dev), dim=1).cpu().numpy()
    store = HipChroma(dim=768, auto_persist=False)
    store.add_embeddings(emb, texts, [{} for _ in range(n)], ["id%d" % i for i in range(n)])
    rng = np.random.default_rng(0)
    qs = emb[rng.integers(0, n, 64)] + 0.01 * rng.standard_normal((64, 768)).astype(np.float32)
    qb = emb[rng.integers(0, n, 256)] + 0.01 * rng.standard_normal((256, 768)).astype(np.float32)
    del emb
    out = {"rows": n}

    # the mirror: encode + upload of every document, at the first where_document use
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    store._doc_bits({"$contains": MARKERS[0][1]})
    torch.cuda.synchronize()
    out["mirror_build_s"] = round(time.perf_counter() - t0, 3)
    mir = store._doc_mirror
    out["text_bytes"] = mir.nbytes
    out["mirror_hbm_bytes"] = mir.nbytes + 8 * (mir.n + 1)

    # one condition -> one row mask on the device (memset + scan + finish), device-synchronised
    bits = torch.empty((n + 31) // 32, dtype=torch.int32, device=dev)
    for name, marker, _ in MARKERS + (("chance", "头痛", 0), ("1byte", "a", 0)):
        pat = marker.encode("utf-8")

        def build(_):
            mir.contains(pat, bits, _lib.MQ_MASK_SET, False)
            torch.cuda.synchronize()
        ms = p50(build, args.iters)
        hits = int(store._mask_rows(bits).sum())
        out["mask_%s" % name] = {"pattern_bytes": len(pat), "rows_hit": hits, "ms": ms,
                                 "text_GBps": round(mir.nbytes / ms / 1e6, 1)}

    # the host way: Python `in` over the documents, packbits, upload
    for name, marker, _ in MARKERS:
        t0 = time.perf_counter()
        m = np.fromiter((marker in t for t in store._texts), bool, n)
        words = np.packbits(m, bitorder="little")
        words = np.concatenate([words, np.zeros(-len(words) % 4, np.uint8)]).view(np.int32)
        hb = torch.from_numpy(words).to(dev)
        torch.cuda.synchronize()
        out["host_mask_%s_ms" % name] = round((time.perf_counter() - t0) * 1e3, 1)
        assert torch.equal(hb, store._doc_bits({"$contains": marker})[:hb.numel()]), name

    # single query: no clause, a repeated clause (cached mask), a fresh clause every call
    out["single_no_clause_ms"] = p50(lambda i: store.similarity_search_by_vector(qs[i % 64], k=5), args.iters)
    for name, marker, _ in MARKERS:
        wd = {"$contains": marker}
        out["single_repeated_%s_ms" % name] = p50(
            lambda i: store.similarity_search_by_vector(qs[i % 64], k=5, where_document=wd), args.iters)
        # alternating $contains / the same rows as $and of itself: a new cache key every call
        out["single_fresh_%s_ms" % name] = p50(
            lambda i: store.similarity_search_by_vector(
                qs[i % 64], k=5, where_document=wd if i % 2 else {"$and": [wd]}), args.iters)
    out["masked_gathers"] = store._index.masked_gathers

    # 256 query vectors in one call
    ix = store._index
    out["batch256_no_clause_ms"] = p50(lambda i: ix.search(qb, 5), 10)
    for name, marker, _ in MARKERS:
        wd = {"$contains": marker}
        out["batch256_repeated_%s_ms" % name] = p50(
            lambda i: ix.search_masked(qb, 5, store._admit(5, None, wd)[1]), 10)
        out["batch256_fresh_%s_ms" % name] = p50(
            lambda i: ix.search_masked(qb, 5, store._admit(5, None, wd if i % 2 else {"$and": [wd]})[1]), 10)
    line = json.dumps(out, ensure_ascii=False)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
