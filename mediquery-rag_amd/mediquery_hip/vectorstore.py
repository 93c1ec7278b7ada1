"""`HipChroma` - drop-in for `langchain_chroma.Chroma` on MI355X.

Reference call sites (unchanged by the swap):
  * `Chroma(persist_directory=DB_PATH, embedding_function=embeddings)`
    src/medical_engine.py:52
  * `Chroma.from_documents(documents=docs, embedding=embeddings,
    persist_directory=DB_PATH)`  src/ingest_medical.py:106-110
  * `vectorstore.similarity_search(search_query, k=5)`  src/agents/nodes.py:93
    (and k=3 in the dead helper src/medical_engine.py:70)

The rows live in an HBM-resident flat index (libmqhip.so); documents and metadata stay
on the host, keyed by row id = insertion order.  Semantics follow Chroma's default
"l2" space: `similarity_search_with_score` returns squared L2 distance, which for the
unit-norm embeddings is 2 - 2*cos; `similarity_search` returns documents by ascending
distance, ties broken by insertion order.  k > N returns N documents; an empty store
returns [].  The device top-k holds at most MQ_MAX_K (64) results: a search whose result
count min(k, candidates) exceeds it raises instead of truncating.  Errors raise (the
reference's retrieve_node does not catch either).  Chroma's two query filters both run as
device row masks: `filter` / `where` over metadata code columns (`_MetaColumns`), and
`where_document` ($contains / $not_contains / $and / $or on the text) over a device mirror of
the documents (`_TextMirror`, built at its first use; `_match_document` is the definition).

Lexical and hybrid retrieval (LangChain's `BM25Retriever` and `EnsembleRetriever([bm25, dense])`):
`lexical_search*` ranks the rows by BM25 over a device mirror of their token ids (`_TokenMirror`,
mq_lex_df / mq_lex_topk; the definition is in include/mq.h), `hybrid_search*` fuses the dense
and the lexical top fetch_k by weighted reciprocal rank (`rrf_fuse`, on the host), and
`as_retriever(search_type="lexical" | "hybrid")` wraps them.  Both take `filter` and
`where_document`.  Nothing of it is persisted: the mirror is derived from the documents.  The
`*_batch` forms of two or more queries tokenise the batch once, fetch the document frequencies
the cache lacks with one mq_lex_df_batch and rank all queries with one mq_lex_topk_batch (one
scan of the mirror per group of up to 16 queries, one copy of the [nq, k] result); every row
is bit for bit the single query's, which one query alone still takes.

Grouped retrieval (LangChain's `ParentDocumentRetriever` / `MultiVectorRetriever`: small child
chunks that name their parent in metadata): `similarity_search_grouped*` returns the best child
of each of the top-k distinct values of a metadata key, over the whole store.  A query is
answered from the ordinary top-64 when that list certifies the answer (`collapse_candidates`)
and by the device group scan otherwise (mq_index_search_grouped, the definition: include/mq.h
"Grouped search"); `as_retriever(search_type="grouped")` wraps it, and
`parent_retriever.HipParentDocumentRetriever` maps the children back to their parents.

Range retrieval (LangChain's "similarity_score_threshold" retriever, candidate lists for a
reranker, counting): `similarity_search_range*` returns every row whose cosine to the query is at
least `min_cosine`, nearest first, up to `limit` <= MQ_RANGE_MAX_HITS (4096) of them, as a
`RangeResult` whose `total` is the exact number of such rows; `count_similar` returns that number
alone.  One device call (mq_index_search_range, the definition: include/mq.h "Range search"),
always in exact fp32.  `similarity_search_with_relevance_scores(score_threshold=...)` filters the
ordinary top-k the way LangChain's base class does, and `as_retriever` takes
`search_type="similarity_score_threshold"` and `"range"`.

Near-duplicate detection (LangChain's `EmbeddingsRedundantFilter`, at the scale of the store):
`duplicate_scan` asks the index about itself - for every row, or the rows of `ids`, how many other
rows have a cosine to it of at least `min_cosine`, which is the smallest and which the nearest - in
one device self-join (mq_index_self_join, the definition: include/mq.h "Self-join"; a bf16 MFMA
screen with a proven bound, its survivors verified in the range search's exact fp32 arithmetic, or
the exact walk alone: `mode`).  `deduplicate` deletes the rows the sequential greedy rule drops (a
row is kept iff no kept earlier row is its partner; `greedy_dedup_rounds`), `find_duplicates`
lists them with the kept row that makes each redundant.  All take `filter` and `where_document`.

Clustering (LangChain's `EmbeddingsClusteringFilter`, at the scale of the store): `cluster` runs
k-means over the rows - all of them, those the filters admit, or those of `ids`, such as a range
search's hits - as Lloyd iterations on the device in the range search's exact fp32 arithmetic, with
a deterministic sum (mq_index_kmeans, the definition: include/mq.h "K-means"), seeded by
k-means++ (`kmeanspp_rows`), random rows or given centres, and returns a `ClusterResult`;
`cluster_representatives` returns the documents nearest each centre by LangChain's rule
(`pick_representatives`), ranked by one range search with the centres as queries.

Persistence: `mq_<collection>.json` (ids, documents, metadatas, and the name of the slab
file) is the base commit point; a full write (the first write, `delete`, an upsert that
replaces rows, an explicit `persist()`) puts the rows in a fresh `mq_<collection>.<gen>.flat`
and then atomically replaces the JSON, so a crash leaves either the old or the new store,
never a slab/sidecar mismatch.  A plain append (`add_texts` of new ids) is append-only: the
new rows go to a segment `mq_<collection>@<gen>.seg.flat` (+ `.seg.json`, their ids,
documents and metadatas), committed by atomically replacing the small manifest
`mq_<collection>@tail.json` (the base slab it extends + the segment list), so one added
document costs a few KB of writes instead of the whole slab and sidecar ('@' cannot occur
in a collection name: no sibling collection's file can match).  Loading applies the
manifest's segments when it names the loaded base; a full write supersedes them, and after
MAX_SEGMENTS appends the next one compacts.  A directory that holds a stock Chroma database
(`chroma.sqlite3`, written by the reference's ingest) but no sidecar is refused: it must be
re-ingested with this store (`python src/ingest_medical.py` after the import swap).
"""
import json
import math
import os
import re
import uuid

import numpy as np

from . import _lib
from .compat import Document, VectorStoreBase
from .native import (FlatIndex, group_scratch_bytes, join_scratch_bytes, kmeans_scratch_bytes,
                     lex_batch_scratch_bytes, lex_df, lex_df_batch,
                     lex_scratch_bytes, lex_topk, lex_topk_batch, mask_combine, mask_contains, mask_eval,
                     mask_eval_bits, range_scratch_bytes)

# `*_batch` lexical / hybrid calls of at least this many queries take the batched scan
# (mq_lex_topk_batch); fewer take the single-query path.  Measured at 1M rows (DESIGN.md, K15,
# "Crossover"): two queries are never slower batched than looped, four or more always faster.
LEX_BATCH_MIN = 2
DEFAULT_K = 4  # LangChain VectorStore.similarity_search default; the reference passes k=5

# search arithmetic (`HipChroma(search_precision=...)`): "screen" (default) = exact fp32
# top-k through the certified screens (int8 / bf16 shadow scans for candidates, fp32
# re-rank, a proven bound per query, uncertified queries re-run exactly); "f32" = the
# direct exact fp32 scan; "f32x6" = the direct scan on the split-f32 MFMA (fp32-class);
# "bf16" = BASELINE config 5's bf16 coarse scan + fp32 re-rank (approximate: recall is
# measured, not guaranteed)
SEARCH_PRECISIONS = {"screen": _lib.MQ_DTYPE_F32_SCREEN, "f32": _lib.MQ_DTYPE_F32,
                     "f32x6": _lib.MQ_DTYPE_F32X6, "bf16": _lib.MQ_DTYPE_BF16}


def _match(meta, where):
    """Chroma-style metadata filter: {"k": v}, {"k": {"$op": v}}, {"$and"/"$or": [...]}."""
    for key, cond in where.items():
        if key == "$and":
            if not all(_match(meta, c) for c in cond):
                return False
        elif key == "$or":
            if not any(_match(meta, c) for c in cond):
                return False
        else:
            v = meta.get(key)
            if isinstance(cond, dict):
                for op, x in cond.items():
                    ok = {"$eq": lambda: v == x, "$ne": lambda: v != x,
                          "$gt": lambda: v is not None and v > x,
                          "$gte": lambda: v is not None and v >= x,
                          "$lt": lambda: v is not None and v < x,
                          "$lte": lambda: v is not None and v <= x,
                          "$in": lambda: v in x, "$nin": lambda: v not in x}.get(op)
                    if ok is None:
                        raise ValueError("unsupported filter operator %r" % op)
                    try:
                        hit = ok()
                    except TypeError:  # incomparable types: no match (see _pred)
                        hit = False
                    if not hit:
                        return False
            elif v != cond:
                return False
    return True


_DOC_LEAVES = ("$contains", "$not_contains")


def _check_where_document(clause, path="where_document"):
    """Validate a Chroma `where_document` clause: a dict with exactly one key, {"$contains": s}
    / {"$not_contains": s} (s a non-empty str of at most MQ_CONTAINS_MAX_BYTES UTF-8 bytes) or
    {"$and" / "$or": [clause, ...]} (a non-empty list, nesting allowed).  Anything else -
    Chroma's $regex / $not_regex included - raises ValueError naming the offending part.  The
    one validation of the host (`_match_document`) and device (`HipChroma._doc_bits`) paths."""
    if not isinstance(clause, dict) or len(clause) != 1:
        raise ValueError("%s must be a dict with exactly one key, got %r" % (path, clause))
    op, x = next(iter(clause.items()))
    if op in _DOC_LEAVES:
        if not isinstance(x, str) or not x:
            raise ValueError("%s: the operand of %s must be a non-empty str, got %r" % (path, op, x))
        nb = len(x.encode("utf-8"))
        if nb > _lib.MQ_CONTAINS_MAX_BYTES:
            raise ValueError("%s: the operand of %s is %d UTF-8 bytes, the limit is MQ_CONTAINS_MAX_BYTES=%d"
                             % (path, op, nb, _lib.MQ_CONTAINS_MAX_BYTES))
    elif op in ("$and", "$or"):
        if not isinstance(x, (list, tuple)) or not x:
            raise ValueError("%s: %s takes a non-empty list of clauses, got %r" % (path, op, x))
        for j, c in enumerate(x):
            _check_where_document(c, "%s[%r][%d]" % (path, op, j))
    else:
        raise ValueError("%s: unsupported where_document operator %r (supported: $contains, "
                         "$not_contains, $and, $or)" % (path, op))
    return clause


def _eval_where_document(text, clause):
    op, x = next(iter(clause.items()))
    if op == "$contains":
        return x in text
    if op == "$not_contains":
        return x not in text
    if op == "$and":
        return all(_eval_where_document(text, c) for c in x)
    return any(_eval_where_document(text, c) for c in x)


def _match_document(text, where_document):
    """Chroma-style document filter on one row's page_content, row by row in plain Python (as
    `_match` is for metadata): case-sensitive substring match, no normalisation, no
    tokenisation.  The device path (mq_mask_contains) matches the UTF-8 bytes instead; UTF-8
    is self-synchronising, so the two agree for every pair of str."""
    return _eval_where_document(text, _check_where_document(where_document))


_MISSING = object()


def _pred(op, v, x):
    """One Chroma where-operator on one metadata value (v None = key absent), as _match."""
    if op == "$eq":
        return v == x
    if op == "$ne":
        return v != x
    if op in ("$gt", "$gte", "$lt", "$lte"):
        if v is None:
            return False
        try:
            return {"$gt": lambda: v > x, "$gte": lambda: v >= x, "$lt": lambda: v < x,
                    "$lte": lambda: v <= x}[op]()
        except TypeError:  # incomparable types (a str value vs a number): no match, as in
            return False   # Chroma, whose typed SQL comparison never matches across types
    if op == "$in":
        return v in x
    if op == "$nin":
        return v not in x
    raise ValueError("unsupported filter operator %r" % op)


class _MetaColumns:
    """Metadata held column-wise for vectorised Chroma `where` filters: per key, int32
    codes [n] (-1 = key absent in that row) into the key's distinct values.  A condition
    is evaluated once per DISTINCT value (Python) into a truth table; the rows are mapped
    through it on the device (`dmask`: mq_mask_eval over a device mirror of the codes,
    a row bitmask the masked search reads) or by numpy (`mask`, for get()); results equal
    `_match` row by row."""

    def __init__(self):
        self.n = 0
        self.cols = {}  # key -> [codes np.int32 (capacity >= n), values list, {hash key: code}]
        self.ver = 0    # bumped by append / compact (device mirrors are per version)
        self.dev = {}   # key -> (ver, device int32 codes [n])
        self._num_cache = {}  # id(values list) -> (len, float64 array or None: not all numeric)

    @staticmethod
    def _hkey(v):
        try:
            return (type(v).__name__, v, hash(v))
        except TypeError:  # unhashable (list) values: keyed by their repr
            return (type(v).__name__, repr(v), None)

    def append(self, metas):
        m = len(metas)
        need = self.n + m
        for col in self.cols.values():
            if col[0].shape[0] < need:
                grown = np.full(max(need, 2 * col[0].shape[0]), -1, np.int32)
                grown[:self.n] = col[0][:self.n]
                col[0] = grown
            col[0][self.n:need] = -1
        for r, meta in enumerate(metas):
            for key, v in meta.items():
                col = self.cols.get(key)
                if col is None:
                    col = self.cols[key] = [np.full(max(need, 1024), -1, np.int32), [], {}]
                hk = self._hkey(v)
                code = col[2].get(hk)
                if code is None:
                    code = col[2][hk] = len(col[1])
                    col[1].append(v)
                col[0][self.n + r] = code
        self.n = need
        self.ver += 1

    def compact(self, keep):
        """Keep rows `keep` (sorted int64 row ids), in order."""
        for col in self.cols.values():
            col[0] = np.ascontiguousarray(col[0][:self.n][keep])
        self.n = len(keep)
        self.ver += 1

    _NUM_OPS = {"$eq": np.equal, "$ne": np.not_equal, "$gt": np.greater, "$gte": np.greater_equal,
                "$lt": np.less, "$lte": np.less_equal}

    @staticmethod
    def _is_num(v):  # a number float64 holds exactly (ints past 2^53 take the exact path)
        return (isinstance(v, float) or (isinstance(v, int) and abs(v) < 2 ** 53)) and not isinstance(v, bool)

    def _lut(self, values, op, x):
        """Truth table of one condition over a column's distinct values (+ absent, last).
        A comparison of a number against an all-numeric column is one numpy op (the
        per-value Python predicate cost ~0.4 us a value); anything else goes value by value
        through _pred (Chroma's typed comparison: mixed types never match)."""
        lut = np.zeros(len(values) + 1, np.uint8)
        lut[-1] = _pred(op, None, x)
        if op in self._NUM_OPS and self._is_num(x) and len(values) > 8:
            nums = self._num_cache.get(id(values))
            if nums is None or nums[0] != len(values):
                ok = all(self._is_num(v) for v in values)
                nums = (len(values), np.array(values, dtype=np.float64) if ok else None)
                self._num_cache[id(values)] = nums
            if nums[1] is not None:
                lut[:-1] = self._NUM_OPS[op](nums[1], float(x))
                return lut
        for cv, v in enumerate(values):
            lut[cv] = _pred(op, v, x)
        return lut

    def dev_codes(self, key, dev):
        got = self.dev.get(key)
        if got is None or got[0] != self.ver:
            import torch
            got = self.dev[key] = (self.ver, torch.from_numpy(self.cols[key][0][:self.n]).to(dev))
        return got[1]

    def dmask(self, where, device):
        """Row bitmask of `where` on the device (int32 words, bit r % 32 of word r / 32),
        built on `device` with that device's current stream whatever torch's current
        device is."""
        import torch
        dev = torch.device("cuda", device)
        with _lib.device_scope(device):
            bits = torch.empty(max(1, (self.n + 31) // 32), dtype=torch.int32, device=dev)
            mask_combine(bits, None, _lib.MQ_MASK_SET)  # all rows
            self._dapply(where, bits, dev)
        return bits

    def _dapply(self, where, bits, dev):
        """bits &= where (the conditions of one dict are ANDed)."""
        import torch
        for key, cond in where.items():
            if key == "$and":
                for c in cond:
                    self._dapply(c, bits, dev)
            elif key == "$or":
                acc, tmp = torch.empty_like(bits), torch.empty_like(bits)
                mask_combine(acc, None, _lib.MQ_MASK_CLEAR)
                for c in cond:
                    mask_combine(tmp, None, _lib.MQ_MASK_SET)
                    self._dapply(c, tmp, dev)
                    mask_combine(acc, tmp, _lib.MQ_MASK_OR)
                mask_combine(bits, acc, _lib.MQ_MASK_AND)
            else:
                col = self.cols.get(key)
                ops = cond.items() if isinstance(cond, dict) else (("$eq", cond),)
                for op, x in ops:
                    if col is None:  # no row has the key
                        if not _pred(op, None, x):
                            mask_combine(bits, None, _lib.MQ_MASK_CLEAR)
                        continue
                    lut = self._lut(col[1], op, x)
                    if len(lut) <= 256:  # by value: no host-to-device copy
                        mask_eval_bits(self.dev_codes(key, dev), lut, bits, _lib.MQ_MASK_AND)
                    else:
                        mask_eval(self.dev_codes(key, dev), torch.from_numpy(lut).to(dev), bits, _lib.MQ_MASK_AND)

    def mask(self, where):
        out = np.ones(self.n, bool)
        for key, cond in where.items():
            if key == "$and":
                for c in cond:
                    out &= self.mask(c)
            elif key == "$or":
                any_ = np.zeros(self.n, bool)
                for c in cond:
                    any_ |= self.mask(c)
                out &= any_
            else:
                col = self.cols.get(key)
                codes = col[0][:self.n] if col is not None else np.full(self.n, -1, np.int32)
                values = col[1] if col is not None else []
                ops = cond.items() if isinstance(cond, dict) else (("$eq", cond),)
                for op, x in ops:
                    # admitted codes -> one table lookup per row; code -1 (key absent)
                    # indexes the table's last entry
                    out &= self._lut(values, op, x).astype(bool)[codes]
        return out


class _TextMirror:
    """Device mirror of the documents for `where_document`: the rows' UTF-8 bytes concatenated
    (`blob`, uint8) and their int64 offsets [n + 1], both with capacity doubling, plus the
    scratch hit mask mq_mask_contains wants.  Built at the first `where_document` use; a plain
    append uploads only the new bytes and offsets; `epoch` (the store bumps its own on every
    delete, so also on a replacing upsert) tells when the rows were renumbered and the mirror
    must be rebuilt.  Costs the corpus's UTF-8 bytes + 8 bytes a row of HBM."""

    def __init__(self, device, epoch):
        import torch
        self.dev = torch.device("cuda", device)
        self.epoch = epoch
        self.version = -1  # the store's _version the mirror is in step with
        self.n = 0
        self.nbytes = 0
        self.blob = torch.empty(0, dtype=torch.uint8, device=self.dev)
        self.offs = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.scratch = torch.empty(1, dtype=torch.int32, device=self.dev)

    @staticmethod
    def _grown(buf, used, need):
        import torch
        if buf.numel() >= need:
            return buf
        out = torch.empty(max(need, 2 * buf.numel()), dtype=buf.dtype, device=buf.device)
        out[:used] = buf[:used]
        return out

    def extend(self, texts):
        """Append rows `texts` (the store's rows n .. n + len(texts))."""
        import torch
        if not texts:
            return
        enc = [t.encode("utf-8") for t in texts]
        ends = self.nbytes + np.cumsum(np.fromiter(map(len, enc), np.int64, len(enc)))
        new = b"".join(enc)
        self.blob = self._grown(self.blob, self.nbytes, self.nbytes + len(new))
        self.offs = self._grown(self.offs, self.n + 1, self.n + 1 + len(enc))
        if new:
            self.blob[self.nbytes:self.nbytes + len(new)] = torch.frombuffer(bytearray(new), dtype=torch.uint8).to(self.dev)
        self.offs[self.n + 1:self.n + 1 + len(enc)] = torch.from_numpy(ends).to(self.dev)
        self.n += len(enc)
        self.nbytes += len(new)
        self.scratch = self._grown(self.scratch, 0, (self.n + 31) // 32)

    def contains(self, pattern, bits, mode, negate):
        """bits (mode)= (row contains pattern) ^ negate over the mirror's rows."""
        mask_contains(self.blob[:self.nbytes], self.offs[:self.n + 1], pattern, bits, mode, negate,
                      scratch=self.scratch)


def body_tokens(tokenizer, texts):
    """-> (flat uint16 token ids, int64 lengths [len(texts)]): each text's body tokens, what
    `tokenizer(texts)` returns without [CLS] / [SEP] (so truncated as the tokenizer truncates),
    concatenated.  An id past 65535 raises ValueError (the mirror stores uint16)."""
    texts = list(texts)
    if not texts:
        return np.zeros(0, np.uint16), np.zeros(0, np.int64)
    ids, mask = tokenizer(texts)
    ids, mask = np.asarray(ids), np.asarray(mask)
    lens = np.maximum(mask.sum(axis=1).astype(np.int64) - 2, 0)
    cols = np.arange(ids.shape[1], dtype=np.int64)[None, :]
    flat = ids[(cols >= 1) & (cols <= lens[:, None])]
    if flat.size and (int(flat.max()) > 0xFFFF or int(flat.min()) < 0):
        raise ValueError("lexical search stores token ids as uint16: the tokenizer's vocabulary must not "
                         "exceed 65536 ids (got id %d)" % int(flat.max()))
    return flat.astype(np.uint16), lens


def term_keys(tokens, ngram):
    """The uint32 term keys of one row's body tokens: the ids (ngram 1) or (id[i] << 16) | id[i + 1]
    of adjacent tokens (ngram 2: max(L - 1, 0) terms)."""
    t = np.asarray(tokens).astype(np.uint32)
    if ngram == 1:
        return t
    return (t[:-1] << np.uint32(16)) | t[1:] if t.size > 1 else np.zeros(0, np.uint32)


def bm25_plan(keys, qf, df, n_rows, avgdl, k1, b, max_terms=_lib.MQ_LEX_MAX_TERMS):
    """The device call's arguments for one query (the definition: include/mq.h): the query's
    distinct term keys with counts qf and document frequencies df over n_rows rows ->
    (keys uint32, w float32, c0 float32, c1 float32), everything computed in float64 and rounded
    once.  More than max_terms terms: the max_terms with the largest idf stay (ties to the
    smaller key).  Slots are in ascending key order."""
    keys = np.asarray(keys, dtype=np.uint32)
    qf = np.asarray(qf, dtype=np.float64)
    df = np.asarray(df, dtype=np.float64)
    idf = np.log(1.0 + (float(n_rows) - df + 0.5) / (df + 0.5))
    if keys.size > max_terms:
        keep = np.sort(np.lexsort((keys, -idf))[:max_terms])  # by (-idf, key); back to key order
        keys, qf, idf = keys[keep], qf[keep], idf[keep]
    order = np.argsort(keys, kind="stable")
    keys, qf, idf = keys[order], qf[order], idf[order]
    w = (qf * (float(k1) + 1.0) * idf).astype(np.float32)
    return keys, w, np.float32(float(k1) * (1.0 - float(b))), np.float32(float(k1) * float(b) / float(avgdl))


def _check_rrf(weights, c):
    try:
        ws = [float(x) for x in weights]
    except (TypeError, ValueError):
        raise ValueError("weights must be two non-negative finite numbers, got %r" % (weights,))
    if len(ws) != 2 or not all(math.isfinite(x) and x >= 0.0 for x in ws) or ws[0] + ws[1] <= 0.0:
        raise ValueError("weights must be two non-negative finite numbers, not both zero, got %r" % (weights,))
    if isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) or c < 0:
        raise ValueError("c must be a non-negative finite number, got %r" % (c,))
    return ws, float(c)


def rrf_fuse(dense_rows, lexical_rows, weights=(0.5, 0.5), c=60, k=None):
    """LangChain's EnsembleRetriever.weighted_reciprocal_rank over two ranked lists of row ids:
    rrf[row] = sum over the lists holding it of weight / (rank + c), rank from 1, in float64;
    rows sorted by rrf descending with a stable sort over the order "dense list, then the
    lexical rows not yet seen".  -> [(row, rrf)], the first k."""
    ws, c = _check_rrf(weights, c)
    rrf, order = {}, []
    for rows, wt in ((dense_rows, ws[0]), (lexical_rows, ws[1])):
        for rank, r in enumerate(rows, start=1):
            r = int(r)
            if r not in rrf:
                rrf[r] = 0.0
                order.append(r)
            rrf[r] += wt / (rank + c)
    order.sort(key=lambda r: rrf[r], reverse=True)  # stable; reverse keeps equal rows in order
    out = [(r, rrf[r]) for r in order]
    return out if k is None else out[:max(0, int(k))]


class _TokenMirror:
    """Device mirror of the documents for lexical search, the twin of `_TextMirror`: the rows'
    body token ids concatenated (`blob`, uint16) and their int64 offsets [n + 1] in tokens, both
    with capacity doubling, plus the scratch mq_lex_df / mq_lex_topk want.  Built at the first
    lexical use, tokenising CHUNK texts at a time (the [n, L] id arrays of a whole corpus never
    exist on the host); a plain append tokenises and uploads only the new rows; `epoch` tells
    when the rows were renumbered and the mirror must be rebuilt.  `df` caches term key -> document
    frequency for one store version.  Costs 2 bytes a token + 8 bytes a row of HBM."""
    CHUNK = 4096

    def __init__(self, device, epoch, tokenizer, ngram):
        import torch
        self.dev = torch.device("cuda", device)
        self.epoch = epoch
        self.version = -1
        self.tokenizer = tokenizer
        self.ngram = ngram
        self.n = 0
        self.n_tokens = 0
        self.sum_dl = 0  # terms over all rows (avgdl = sum_dl / n)
        self.df = {}
        # int16 storage (every torch copy supports it), handed to the kernels as uint16 views
        self.blob = torch.empty(0, dtype=torch.int16, device=self.dev)
        self.offs = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.scratch = torch.empty(lex_scratch_bytes(1 << 40, _lib.MQ_MAX_K), dtype=torch.uint8, device=self.dev)
        self.batch_scratch = None  # mq_lex_df_batch / mq_lex_topk_batch: allocated at the first batch

    def nbytes(self):
        """HBM the mirror holds (allocated capacity, scratch included)."""
        return (self.blob.numel() * 2 + self.offs.numel() * 8 + self.scratch.numel()
                + (0 if self.batch_scratch is None else self.batch_scratch.numel()))

    def extend(self, texts):
        """Append rows `texts` (the store's rows n .. n + len(texts)); drops the df cache."""
        import torch
        self.df = {}
        for at in range(0, len(texts), self.CHUNK):
            flat, lens = body_tokens(self.tokenizer, texts[at:at + self.CHUNK])
            ends = self.n_tokens + np.cumsum(lens)
            self.blob = _TextMirror._grown(self.blob, self.n_tokens, self.n_tokens + flat.size)
            self.offs = _TextMirror._grown(self.offs, self.n + 1, self.n + 1 + lens.size)
            if flat.size:
                self.blob[self.n_tokens:self.n_tokens + flat.size] = torch.from_numpy(flat.view(np.int16)).to(self.dev)
            self.offs[self.n + 1:self.n + 1 + lens.size] = torch.from_numpy(ends).to(self.dev)
            self.n += int(lens.size)
            self.n_tokens += int(flat.size)
            self.sum_dl += int(lens.sum()) if self.ngram == 1 else int(np.maximum(lens - 1, 0).sum())

    def _views(self):
        import torch
        return self.blob[:self.n_tokens].view(torch.uint16), self.offs[:self.n + 1]

    def frequencies(self, keys):
        """df of the uint32 term keys (distinct), int64: cached ones cost nothing, the rest one
        df pass per MQ_LEX_MAX_TERMS."""
        miss = [int(x) for x in keys if int(x) not in self.df]
        tokens, offs = self._views()
        for at in range(0, len(miss), _lib.MQ_LEX_MAX_TERMS):
            part = miss[at:at + _lib.MQ_LEX_MAX_TERMS]
            got = lex_df(tokens, offs, self.ngram, np.array(part, np.uint32), scratch=self.scratch)
            self.df.update(zip(part, got.tolist()))
        return np.array([self.df[int(x)] for x in keys], dtype=np.int64)

    def plan(self, query, k1, b):
        """-> (keys, w, c0, c1) of mq_lex_topk for one query text, or None: no term, or no row
        has any (avgdl = 0)."""
        flat, _ = body_tokens(self.tokenizer, [query])
        terms = term_keys(flat, self.ngram)
        if not terms.size or self.sum_dl == 0:
            return None
        keys, qf = np.unique(terms, return_counts=True)
        return bm25_plan(keys, qf, self.frequencies(keys), self.n, self.sum_dl / self.n, k1, b)

    def topk(self, plan, k, bits):
        """-> (scores f32 [k], rows int64 [k]) on the host."""
        tokens, offs = self._views()
        keys, w, c0, c1 = plan
        s, i = lex_topk(tokens, offs, self.ngram, keys, w, c0, c1, k, bits=bits, scratch=self.scratch)
        return s.cpu().numpy(), i.cpu().numpy()

    def plan_batch(self, queries, k1, b):
        """`plan` for a batch -> one (keys, w, c0, c1) or None per query, each exactly what
        `plan` returns for it: one tokenizer call, and one mq_lex_df_batch for the batch's
        distinct keys the df cache lacks."""
        queries = list(queries)
        flat, lens = body_tokens(self.tokenizer, queries)
        if self.sum_dl == 0:
            return [None] * len(queries)
        ends = np.cumsum(lens)
        split = [np.unique(term_keys(flat[e - ln:e], self.ngram), return_counts=True) for e, ln in zip(ends, lens)]
        seen = np.unique(np.concatenate([keys for keys, _ in split])) if split else np.zeros(0, np.uint32)
        miss = [int(x) for x in seen if int(x) not in self.df]
        if miss:
            tokens, offs = self._views()
            self._batch_room(0, len(miss), 1)
            got = lex_df_batch(tokens, offs, self.ngram, np.array(miss, np.uint32), scratch=self.batch_scratch)
            self.df.update(zip(miss, got.tolist()))
        avgdl = self.sum_dl / self.n
        return [bm25_plan(keys, qf, np.array([self.df[int(x)] for x in keys], dtype=np.int64), self.n, avgdl, k1, b)
                if keys.size else None for keys, qf in split]

    def topk_batch(self, plans, k, bits):
        """-> (scores f32 [nq, k], rows int64 [nq, k]) on the host for plans (none None, of one
        `plan_batch`, so c0 and c1 are shared): one mq_lex_topk_batch, the result copied once."""
        tokens, offs = self._views()
        c0, c1 = plans[0][2], plans[0][3]
        assert all(p[2] == c0 and p[3] == c1 for p in plans)
        self._batch_room(len(plans), sum(len(p[0]) for p in plans), k)
        s, i = lex_topk_batch(tokens, offs, self.ngram, [(p[0], p[1]) for p in plans], c0, c1, k, bits=bits,
                              scratch=self.batch_scratch)
        return s.cpu().numpy(), i.cpu().numpy()

    def _batch_room(self, nq, total_terms, k):
        """The batch calls' scratch: grows on demand (to the size for any row count) and is kept."""
        import torch
        need = lex_batch_scratch_bytes(1 << 40, nq, total_terms, k)
        if self.batch_scratch is None or self.batch_scratch.numel() < need:
            self.batch_scratch = None  # release before growing
            self.batch_scratch = torch.empty(need, dtype=torch.uint8, device=self.dev)


def collapse_candidates(ids, scores, codes, k):
    """One query's top list of ROWS (ids / scores as the search returns them: best first by
    (score desc, row asc), padded with -1) collapsed to its distinct groups, LangChain's way:
    the first row of each new code, in list order; rows whose code is absent (< 0) are skipped.
    codes: the host group code of every row.  -> (rows, scores, certified): at most k
    representative rows with their scores, and whether they are THE top-k groups of the whole
    candidate set.  They are when the list holds at least k distinct groups - a group absent
    from a full list has best score <= the list's last score <= every present group's best, and
    in the (score desc, row asc) order every absent row comes after every listed one - or when
    the list is shorter than MQ_MAX_K valid entries, because then it holds every candidate."""
    rows, out, seen, valid = [], [], set(), 0
    for r, s in zip(ids, scores):
        r = int(r)
        if r < 0:
            continue
        valid += 1
        c = int(codes[r])
        if c < 0 or c in seen:
            continue
        seen.add(c)
        if len(rows) < k:
            rows.append(r)
            out.append(float(s))
    return rows, out, len(seen) >= k or valid < _lib.MQ_MAX_K


class RangeResult(list):
    """What the range searches return: a list (nearest first, at most `limit` entries) with one
    attribute, `total`: the number of rows at or above the threshold, >= len."""

    def __init__(self, items=(), total=None):
        super().__init__(items)
        self.total = len(self) if total is None else int(total)
        if self.total < len(self):
            raise ValueError("total %d is below the %d entries of the list" % (self.total, len(self)))


def _check_limit(limit, n_candidates):
    """Length of a range search's list over n_candidates rows; raises past the device limit."""
    kk = min(int(limit), int(n_candidates))
    if kk > _lib.MQ_RANGE_MAX_HITS:
        raise ValueError("a range search returning up to %d results (limit=%d over %d rows) exceeds the device "
                         "list limit MQ_RANGE_MAX_HITS=%d" % (kk, limit, n_candidates, _lib.MQ_RANGE_MAX_HITS))
    return kk


def _check_min_cosine(min_cosine):
    """None (no threshold) -> -inf; a finite number -> float; anything else raises."""
    if min_cosine is None:
        return -math.inf
    if isinstance(min_cosine, bool) or not isinstance(min_cosine, (int, float, np.integer, np.floating)) \
            or not math.isfinite(min_cosine):
        raise ValueError("min_cosine must be None or a finite number, got %r" % (min_cosine,))
    return float(min_cosine)


def _check_dup_cosine(min_cosine):
    """The threshold of the duplicate scans: a finite number (None is refused: every row would
    be every row's partner)."""
    if min_cosine is None:
        raise ValueError("min_cosine must be a finite number, got None")
    return _check_min_cosine(min_cosine)


JOIN_MODES = {"auto": _lib.MQ_JOIN_AUTO, "exact": _lib.MQ_JOIN_EXACT, "screen": _lib.MQ_JOIN_SCREEN}


class DuplicateScan:
    """What `HipChroma.duplicate_scan` returns, host arrays of one entry per left row: `rows`
    (the left rows, ascending), `counts` (partners: other admitted rows at or above the
    threshold), `first` (the smallest partner row, -1: none), `nearest` / `nearest_cosine` (the
    partner of the highest cosine, ties to the lowest row; -1 / -inf: none), and `info`
    (mq_index_self_join's out_info)."""

    def __init__(self, rows, counts, first, nearest, nearest_cosine, info):
        self.rows, self.counts, self.first = rows, counts, first
        self.nearest, self.nearest_cosine, self.info = nearest, nearest_cosine, info

    def __len__(self):
        return len(self.rows)


class DedupResult(list):
    """What `deduplicate` (deleted ids) and `find_duplicates` (triples) return: a list with
    `undecided`, the ids still undecided after max_rounds (they are kept), and `rounds`, the
    scans that ran."""

    def __init__(self, items=(), undecided=(), rounds=0):
        super().__init__(items)
        self.undecided, self.rounds = list(undecided), int(rounds)


def greedy_dedup_rounds(n, left, admitted, scan_first, max_rounds=32):
    """The sequential greedy rule - a left row is kept iff no KEPT earlier row is its partner -
    computed in rounds of whole scans.  left: the rows that may be dropped (ascending, distinct);
    admitted: bool [n], the rows that take part (a left row outside it is kept untouched); every
    admitted row outside `left` is kept.  scan_first(rows, mask) -> for each of `rows` its
    smallest partner among the rows of the bool mask [n], or -1.
    Each round scans the undecided rows under the mask of the kept and undecided rows and walks
    them in ascending order: no earlier partner (first < 0 or first > row) -> kept; `first` is a
    kept row -> dropped, with `first` as its keeper; otherwise (first is undecided, or was
    dropped in this round, so another earlier partner may remain) the row waits for the next
    round, whose mask leaves the dropped rows out.  The smallest undecided row is always decided
    (every earlier row of the mask is kept), so the rounds end.
    -> (dropped rows ascending, their keepers, undecided rows after max_rounds, rounds run)."""
    KEPT, UNDECIDED, DROPPED = 0, 1, 2
    admitted = np.asarray(admitted, bool)
    state = np.full(n, KEPT, np.int8)
    left = np.asarray(left, np.int64)
    left = left[admitted[left]] if len(left) else left
    state[left] = UNDECIDED
    keeper = {}
    undecided, rounds = left, 0
    while len(undecided) and rounds < max_rounds:
        rounds += 1
        first = scan_first(undecided, admitted & (state != DROPPED))
        for r, f in zip(undecided.tolist(), np.asarray(first).tolist()):
            if f < 0 or f > r:
                state[r] = KEPT
            elif state[f] == KEPT:
                state[r] = DROPPED
                keeper[r] = f
        undecided = undecided[state[undecided] == UNDECIDED]
    dropped = np.array(sorted(keeper), np.int64)
    return dropped, np.array([keeper[r] for r in dropped.tolist()], np.int64), undecided, rounds


class ClusterResult:
    """What `HipChroma.cluster` returns: `ids` (the admitted documents, in row order) and `labels`
    (int32, each one's cluster), `centroids` (float32 [n_clusters, dim]), `counts` (int64, the
    cluster sizes; 0: an empty cluster, whose centroid is its initial one), `iterations` (updates
    applied before the labels stopped changing), `converged` (they did stop within max_iter) and
    `inertia` (float64: the sum over the admitted rows of 1 - 2 dot + |c|^2, their squared
    distance to their centre, rows taken as unit)."""

    def __init__(self, ids, labels, centroids, counts, iterations, converged, inertia):
        self.ids, self.labels, self.centroids, self.counts = ids, labels, centroids, counts
        self.iterations, self.converged, self.inertia = int(iterations), bool(converged), float(inertia)

    def __len__(self):
        return len(self.ids)


def kmeanspp_rows(n_admitted_rows, n_clusters, rng, dots_of_row):
    """k-means++ seeding (D^2 sampling) over n_admitted_rows unit rows -> n_clusters distinct
    positions (int64, in the order drawn).  dots_of_row(p) -> the dots of row p with every row
    [n_admitted_rows]; the squared distance to p is 2 - 2 dot, clipped at 0.  The first seed is
    rng.integers(n); each further one is rng.choice(n, p = m / sum(m)), m the running minimum of
    the squared distances to the seeds so far (0 at the seeds themselves: no repeats); when every
    remaining row coincides with a seed (sum(m) = 0) it is rng.choice of the rows not yet drawn."""
    n, k = int(n_admitted_rows), int(n_clusters)
    if not 1 <= k <= n:
        raise ValueError("n_clusters %d needs at least as many rows (got %d)" % (k, n))
    first = int(rng.integers(n))
    picked = [first]
    m = np.clip(2.0 - 2.0 * np.asarray(dots_of_row(first), np.float64), 0.0, None)
    m[first] = 0.0
    while len(picked) < k:
        total = m.sum()
        if total > 0.0:
            nxt = int(rng.choice(n, p=m / total))
        else:
            free = np.ones(n, bool)
            free[picked] = False
            nxt = int(rng.choice(np.flatnonzero(free)))
        picked.append(nxt)
        m = np.minimum(m, np.clip(2.0 - 2.0 * np.asarray(dots_of_row(nxt), np.float64), 0.0, None))
        m[picked] = 0.0
    return np.array(picked, np.int64)


def pick_representatives(ranked_lists, num_closest, remove_duplicates=False, sorted=False):
    """LangChain's `EmbeddingsClusteringFilter` selection.  ranked_lists[j]: the rows ranked by
    nearness to centre j, nearest first (at least the first n_clusters x num_closest of them, or
    all).  Walk the clusters in order.  With remove_duplicates: take the first num_closest of
    the ranking and drop those already taken.  Without it: take the first num_closest of the
    ranking that are not already taken.  -> the rows in pick order, or ascending when `sorted`."""
    taken, seen = [], set()
    for ranking in ranked_lists:
        ranking = [int(r) for r in ranking]
        if remove_duplicates:
            new = [r for r in ranking[:num_closest] if r not in seen]
        else:
            new = [r for r in ranking if r not in seen][:num_closest]
        taken.extend(new)
        seen.update(new)
    if sorted:
        taken.sort()
    return taken


CLUSTER_INITS = ("k-means++", "random")


def _check_cluster_args(n_clusters, max_iter, init, seed, dim):
    """-> (n_clusters, max_iter, init): init a name of CLUSTER_INITS or a float32 [n_clusters, dim]."""
    for name, v, lo, hi in (("n_clusters", n_clusters, 1, _lib.MQ_KMEANS_MAX_CLUSTERS), ("max_iter", max_iter, 0, 1024)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError("%s must be an integer in [%d, %d], got %r" % (name, lo, hi, v))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0:
        raise ValueError("seed must be a non-negative integer, got %r" % (seed,))
    if isinstance(init, str):
        if init not in CLUSTER_INITS:
            raise ValueError("init must be one of %s or an [n_clusters, dim] array, got %r" % (CLUSTER_INITS, init))
    else:
        init = np.array(init, dtype=np.float32, order="C")
        if init.ndim != 2 or init.shape[0] != n_clusters or (dim and init.shape[1] != dim):
            raise ValueError("an init array must be [n_clusters = %d, dim = %d], got shape %r"
                             % (n_clusters, dim or 0, init.shape))
        if not np.isfinite(init).all():
            raise ValueError("an init array must be finite")
    return int(n_clusters), int(max_iter), init


def _check_score_threshold(score_threshold):
    if isinstance(score_threshold, bool) or not isinstance(score_threshold, (int, float, np.integer, np.floating)) \
            or math.isnan(score_threshold):
        raise ValueError("score_threshold must be a number, got %r" % (score_threshold,))
    return float(score_threshold)


class _LexicalRetriever:
    """What `HipChroma.as_retriever(search_type="lexical" | "hybrid" | "grouped" | "range")` returns:
    `invoke` / `get_relevant_documents` call the store's method with the retriever's
    search_kwargs."""

    def __init__(self, store, search_type, search_kwargs):
        self.vectorstore = store
        self.search_type = search_type
        self.search_kwargs = dict(search_kwargs or {})

    def invoke(self, query, config=None, **kwargs):
        fn = {"lexical": self.vectorstore.lexical_search, "hybrid": self.vectorstore.hybrid_search,
              "grouped": self.vectorstore.similarity_search_grouped,
              "range": self.vectorstore.similarity_search_range}[self.search_type]
        return fn(query, **self.search_kwargs)

    get_relevant_documents = invoke


class _IdRows:
    """id -> current row in O(1), kept across deletes without rebuilding a dict of every id:
    each id gets a stable slot when it is added (`slot`, a dict), and two int64 arrays map
    slot -> current row (-1 = deleted) and row -> slot.  A delete drops its ids' dict
    entries and renumbers the surviving rows with one numpy gather / scatter (a dict
    rebuild of a 1M-row store cost ~0.4 s per delete).  Dead slots are reclaimed by a
    rebuild once they outnumber the live rows."""

    def __init__(self, ids=()):
        self.slot = {}
        self._slot_row = np.zeros(1024, np.int64)
        self._row_slot = np.zeros(1024, np.int64)
        self.n_slots = 0
        self.n = 0
        self.extend(list(ids))

    def __contains__(self, i):
        return i in self.slot

    def __len__(self):
        return self.n

    def row(self, i):
        return int(self._slot_row[self.slot[i]])

    @staticmethod
    def _grow(a, need):
        if a.shape[0] >= need:
            return a
        b = np.zeros(max(need, 2 * a.shape[0]), np.int64)
        b[:a.shape[0]] = a
        return b

    def extend(self, ids):
        """ids (new, distinct) appended as rows n .. n + len(ids)."""
        m = len(ids)
        if not m:
            return
        s0, r0 = self.n_slots, self.n
        self._slot_row = self._grow(self._slot_row, s0 + m)
        self._row_slot = self._grow(self._row_slot, r0 + m)
        self._slot_row[s0:s0 + m] = np.arange(r0, r0 + m)
        self._row_slot[r0:r0 + m] = np.arange(s0, s0 + m)
        self.slot.update(zip(ids, range(s0, s0 + m)))
        self.n_slots += m
        self.n += m

    def compact(self, keep, dropped_ids):
        """Rows `keep` (sorted int64) survive, renumbered 0..len(keep); dropped_ids leave."""
        for i in dropped_ids:
            del self.slot[i]
        rs = self._row_slot[:self.n]
        keepm = np.zeros(self.n, bool)
        keepm[keep] = True
        self._slot_row[rs[~keepm]] = -1
        kept = rs[keepm]
        self._row_slot[:kept.shape[0]] = kept
        self._slot_row[kept] = np.arange(kept.shape[0])
        self.n = int(kept.shape[0])
        if self.n_slots > 2 * self.n + 1024:  # reclaim the dead slots
            order = sorted(self.slot, key=self.slot.__getitem__)
            rows = self._slot_row[[self.slot[i] for i in order]] if order else np.zeros(0, np.int64)
            ids_by_row = [None] * self.n
            for i, r in zip(order, rows.tolist()):
                ids_by_row[r] = i
            self.__init__(ids_by_row)


def _drop_sorted(lst, drop):
    """lst without the positions `drop` (sorted, distinct): list slices, no per-item Python."""
    out, prev = [], 0
    for d in drop:
        out += lst[prev:d]
        prev = d + 1
    out += lst[prev:]
    return out


def _check_k(k, n_candidates):
    """Result count of a top-k over n_candidates rows; raises past the device limit."""
    kk = min(int(k), int(n_candidates))
    if kk > _lib.MQ_MAX_K:
        raise ValueError("a search returning %d results (k=%d over %d rows) exceeds the device "
                         "top-k limit MQ_MAX_K=%d" % (kk, k, n_candidates, _lib.MQ_MAX_K))
    return kk


class HipChroma(VectorStoreBase):
    _FILES = ("mq_%s.flat", "mq_%s.json", "mq_%s@tail.json")
    FOREIGN_DB = "chroma.sqlite3"  # what langchain_chroma / chromadb persist
    _GEN = re.compile(r"[0-9a-f]{12}\.flat")  # slab generation suffix (persist() writes it)
    STALE_SLAB_S = 3600  # an uncommitted slab this old is a crashed writer's leftover
    _SEG = re.compile(r"[0-9a-f]{12}\.seg\.(flat|json)")  # segment files (after 'mq_<name>@')
    MAX_SEGMENTS = 256  # appends between compactions

    def __init__(self, collection_name="langchain", embedding_function=None,
                 persist_directory=None, client_settings=None, collection_metadata=None,
                 client=None, relevance_score_fn=None, *, device=0, dim=None,
                 auto_persist=True, search_precision="screen", lexical_tokenizer=None, lexical_ngram=1,
                 bm25_k1=1.2, bm25_b=0.75, _ingest=False, **kwargs):
        """auto_persist=False: writes stay in memory until `persist()` (bulk ingest);
        search_precision: SEARCH_PRECISIONS (default "screen": exact fp32 top-k);
        lexical_tokenizer: the tokenizer of `lexical_search` / `hybrid_search` (default: the
        embedding function's `tokenizer`), lexical_ngram 1 or 2, bm25_k1 / bm25_b the BM25
        parameters (include/mq.h)."""
        if lexical_ngram not in (1, 2):
            raise ValueError("lexical_ngram must be 1 or 2, got %r" % (lexical_ngram,))
        if not (math.isfinite(bm25_k1) and bm25_k1 >= 0 and math.isfinite(bm25_b) and 0 <= bm25_b <= 1):
            raise ValueError("bm25_k1 must be finite and >= 0 and bm25_b in [0, 1], got %r, %r" % (bm25_k1, bm25_b))
        self._lex_tokenizer = lexical_tokenizer
        self._lex_ngram = int(lexical_ngram)
        self._bm25 = (float(bm25_k1), float(bm25_b))
        self._lex_mirror = None        # _TokenMirror, built at the first lexical use
        self.group_scans = 0           # grouped queries the top-64 did not certify (sent to the scan)
        self._group_scratch = None     # the group scan's device scratch, grown on demand
        self._group_absent = None      # ((key, codes version), some row lacks the key)
        self._range_scratch = None     # the range search's device scratch, grown on demand
        self._join_scratch = None      # the self-join's device scratch, grown on demand
        self._kmeans_scratch = None    # the k-means scratch, grown on demand
        if search_precision not in SEARCH_PRECISIONS:
            raise ValueError("search_precision must be one of %s, got %r"
                             % (sorted(SEARCH_PRECISIONS), search_precision))
        self._search_precision = search_precision
        self._collection_name = collection_name
        self._embedding_function = embedding_function
        self._persist_directory = persist_directory
        self._collection_metadata = dict(collection_metadata or {})
        self.override_relevance_score_fn = relevance_score_fn
        self._device = device
        self._auto_persist = bool(auto_persist)
        self._ids, self._texts, self._metas = [], [], []
        self._id_row = _IdRows()       # id -> row (upsert / delete / get by id in O(1))
        self._cols = _MetaColumns()    # metadata column-wise, for vectorised filters
        self._version = 0              # bumped by every write
        self._text_epoch = 0           # bumped when rows are renumbered (delete, replacing upsert)
        self._doc_mirror = None        # _TextMirror, built at the first where_document use
        self._doc_cache = None         # ((clause JSON, _version), device mask) of the last clause
        self._index = None
        self._dim = dim
        self._slab_name = None
        self._segments = []    # committed segments after the base: {"slab", "delta", "n_rows"}
        self._written = set()  # slabs this instance wrote that no commit of its own names now
        if persist_directory and os.path.exists(self._path(1)):
            self._load()
        elif (persist_directory and not _ingest
              and os.path.exists(os.path.join(persist_directory, self.FOREIGN_DB))):
            raise RuntimeError(
                "%r holds a ChromaDB database (%s) but no %s sidecar: the MI355X store cannot "
                "read Chroma's files. Re-run the ingest (src/ingest_medical.py) with the "
                "mediquery_hip import swap to build it." % (persist_directory, self.FOREIGN_DB,
                                                            self._FILES[1] % collection_name))

    # ---- helpers ---------------------------------------------------------------------
    @property
    def embeddings(self):
        return self._embedding_function

    def _path(self, i):
        return os.path.join(self._persist_directory, self._FILES[i] % self._collection_name)

    def _ensure_index(self, dim):
        if self._index is None:
            self._dim = dim
            self._index = FlatIndex(dim=dim, device=self._device)
            self._index.set_precision(SEARCH_PRECISIONS[self._search_precision])
        elif dim != self._dim:
            raise ValueError("embedding dim %d != collection dim %d" % (dim, self._dim))

    def _persist(self):
        if self._auto_persist:
            self.persist()

    @staticmethod
    def _write_json(path, obj):
        """Write + fsync `path` + ".tmp", then atomically rename it to `path`."""
        tmp = path + ".tmp"
        with open(tmp, "w", encoding="utf-8") as f:
            json.dump(obj, f, ensure_ascii=False)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)

    def persist(self):
        """Write the whole store under persist_directory (crash-safe, see the module doc);
        supersedes (and deletes) the append segments."""
        if not self._persist_directory or self._index is None:
            return
        d = self._persist_directory
        os.makedirs(d, exist_ok=True)
        slab = "mq_%s.%s.flat" % (self._collection_name, uuid.uuid4().hex[:12])
        self._index.save(os.path.join(d, slab))
        self._write_json(self._path(1), {  # the commit point
            "dim": self._dim, "slab": slab, "n_rows": len(self._ids), "ids": self._ids,
            "documents": self._texts, "metadatas": self._metas,
            "collection_metadata": self._collection_metadata})
        replaced, self._slab_name = self._slab_name, slab
        if replaced:
            self._written.add(replaced)
        for seg in self._segments:  # superseded: the manifest names the old base
            self._written.update((seg["slab"], seg["delta"]))
        self._segments = []
        try:
            os.remove(self._path(2))
        except OSError:
            pass
        self._remove_orphan_slabs()

    def _persist_append(self, row0, m):
        """Commit rows [row0, row0 + m), just appended, as one segment (module doc)."""
        if not (self._auto_persist and self._persist_directory and self._index is not None):
            return
        if self._slab_name is None or len(self._segments) >= self.MAX_SEGMENTS:
            return self.persist()
        d = self._persist_directory
        stem = "mq_%s@%s.seg" % (self._collection_name, uuid.uuid4().hex[:12])
        seg = {"slab": stem + ".flat", "delta": stem + ".json", "n_rows": m}
        self._index.save_rows(os.path.join(d, seg["slab"]), row0, m)
        self._write_json(os.path.join(d, seg["delta"]), {
            "ids": self._ids[row0:], "documents": self._texts[row0:], "metadatas": self._metas[row0:]})
        self._write_json(self._path(2), {"base_slab": self._slab_name,  # the commit point
                                         "segments": self._segments + [seg]})
        self._segments.append(seg)

    def _own_slab(self, f):
        """Is file name `f` a slab or segment file of THIS collection (not of 'name.x', whose
        slabs also start with 'mq_name.')?  Its generated names and the legacy single-slab name."""
        prefix, sprefix = "mq_%s." % self._collection_name, "mq_%s@" % self._collection_name
        return f == self._FILES[0] % self._collection_name or (
            f.startswith(prefix) and self._GEN.fullmatch(f[len(prefix):]) is not None) or (
            f.startswith(sprefix) and self._SEG.fullmatch(f[len(sprefix):]) is not None)

    def _remove_orphan_slabs(self):
        """After a commit: delete the slabs this instance replaced (the one it loaded or
        wrote before), and this collection's slabs older than the sidecar by more than
        STALE_SLAB_S (a crashed writer's leftovers).  A younger uncommitted slab may be
        another process's write in flight (ingest and app share the directory), so it is
        left alone; nothing is deleted on load."""
        d = self._persist_directory
        try:
            side_mtime = os.path.getmtime(self._path(1))
        except OSError:
            return
        live = {self._slab_name}
        for seg in self._segments:
            live.update((seg["slab"], seg["delta"]))
        for f in os.listdir(d):
            if f in live or not self._own_slab(f):
                continue
            p = os.path.join(d, f)
            try:
                if f in self._written or os.path.getmtime(p) < side_mtime - self.STALE_SLAB_S:
                    os.remove(p)
            except OSError:
                pass
        self._written.clear()

    def _reindex_host(self):
        self._id_row = _IdRows(self._ids)
        self._cols = _MetaColumns()
        self._cols.append(self._metas)
        self._version += 1

    def _load(self):
        with open(self._path(1), "r", encoding="utf-8") as f:
            side = json.load(f)
        self._ensure_index(side["dim"])
        self._slab_name = side.get("slab", self._FILES[0] % self._collection_name)
        self._written.add(self._slab_name)  # replaced (so deleted) by this instance's first commit
        self._index.load(os.path.join(self._persist_directory, self._slab_name))
        self._ids, self._texts, self._metas = side["ids"], side["documents"], side["metadatas"]
        self._collection_metadata = side.get("collection_metadata", {})
        if len(self._index) != len(self._ids):
            raise RuntimeError("persisted index (%d rows) and sidecar (%d ids) disagree"
                               % (len(self._index), len(self._ids)))
        tail = None
        if os.path.exists(self._path(2)):
            with open(self._path(2), "r", encoding="utf-8") as f:
                tail = json.load(f)
        if tail and tail.get("base_slab") == self._slab_name:  # else superseded by a full write
            d = self._persist_directory
            for seg in tail["segments"]:
                self._index.load_append(os.path.join(d, seg["slab"]))
                with open(os.path.join(d, seg["delta"]), "r", encoding="utf-8") as f:
                    delta = json.load(f)
                self._ids += delta["ids"]
                self._texts += delta["documents"]
                self._metas += delta["metadatas"]
                if len(self._index) != len(self._ids):
                    raise RuntimeError("segment %s (%d rows) and its delta disagree"
                                       % (seg["slab"], seg["n_rows"]))
                self._segments.append(seg)
                self._written.update((seg["slab"], seg["delta"]))  # superseded by the next full write
        self._reindex_host()

    def _embed_query(self, query):
        if self._embedding_function is None:
            raise ValueError("HipChroma needs an embedding_function to search by text")
        return np.asarray(self._embedding_function.embed_query(query), dtype=np.float32)

    def _doc(self, row):
        return Document(page_content=self._texts[row], metadata=dict(self._metas[row]),
                        id=self._ids[row])

    # ---- writes -------------------------------------------------------------------------
    def add_texts(self, texts, metadatas=None, ids=None, **kwargs):
        texts = list(texts)
        if not texts:
            return []
        if ids is None:
            ids = [str(uuid.uuid4()) for _ in texts]
        ids = [str(i) for i in ids]
        metadatas = [dict(m or {}) for m in (metadatas or [{}] * len(texts))]
        if len(metadatas) != len(texts) or len(ids) != len(texts):
            raise ValueError("texts, metadatas and ids must have the same length")
        if self._embedding_function is None:
            raise ValueError("HipChroma needs an embedding_function to add texts")
        if hasattr(self._embedding_function, "embed_array"):
            emb = self._embedding_function.embed_array(texts)
        else:
            emb = np.asarray(self._embedding_function.embed_documents(texts), dtype=np.float32)
        self.add_embeddings(emb, texts, metadatas, ids)
        return ids

    def add_embeddings(self, embeddings, texts, metadatas, ids):
        """Upsert semantics as in Chroma: an existing id is replaced (row rebuilt)."""
        emb = np.ascontiguousarray(embeddings, dtype=np.float32)
        self._ensure_index(emb.shape[1])
        if len(set(ids)) != len(ids):  # last write of a repeated id wins, as in an upsert
            last = {i: j for j, i in enumerate(ids)}
            pick = sorted(last.values())
            emb, texts = emb[pick], [texts[j] for j in pick]
            metadatas, ids = [metadatas[j] for j in pick], [ids[j] for j in pick]
        existing = [i for i in ids if i in self._id_row]
        if existing:
            self.delete(existing, _persist=False)
        self._index.add(emb)
        base = len(self._ids)
        self._ids += ids
        self._texts += texts
        self._metas += metadatas
        self._id_row.extend(ids)
        self._cols.append(metadatas)
        self._version += 1
        if existing:  # rows were replaced: a full write (compaction)
            self._persist()
        else:
            self._persist_append(base, len(ids))

    def delete(self, ids=None, _persist=True, **kwargs):
        if not ids or self._index is None:
            return None
        gone = [i for i in set(ids) if i in self._id_row]
        if not gone:
            return True
        drop = sorted(self._id_row.row(i) for i in gone)
        keepm = np.ones(len(self._ids), bool)
        keepm[drop] = False
        keep = np.flatnonzero(keepm)
        self._index.select(keep, out=self._index)  # device compaction, rows bit-identical
        for name in ("_ids", "_texts", "_metas"):
            setattr(self, name, _drop_sorted(getattr(self, name), drop))
        self._cols.compact(keep)
        self._id_row.compact(keep, gone)
        self._version += 1
        self._text_epoch += 1
        if _persist:
            self._persist()
        return True

    def get(self, ids=None, where=None, limit=None, offset=None, include=None, where_document=None, **kwargs):
        if where_document is not None:
            _check_where_document(where_document)
        rows = np.arange(len(self._ids))
        if ids is not None:
            want = [ids] if isinstance(ids, str) else ids
            rows = np.array(sorted({self._id_row.row(i) for i in want if i in self._id_row}), np.int64)
        if where:
            rows = rows[self._cols.mask(where)[rows]]
        if where_document is not None and len(rows):
            rows = rows[self._mask_rows(self._doc_bits(where_document))[rows]]
        rows = rows.tolist()[offset or 0:]
        if limit is not None:
            rows = rows[:limit]
        return {"ids": [self._ids[r] for r in rows], "documents": [self._texts[r] for r in rows],
                "metadatas": [self._metas[r] for r in rows]}

    # ---- search -------------------------------------------------------------------------
    def _doc_apply(self, clause, bits, mode):
        """bits (mode)= clause on the device: a leaf is one mq_mask_contains ($not_contains:
        negate); $and / $or chain ANDs / ORs, through a scratch mask when `mode` is not theirs."""
        import torch
        op, x = next(iter(clause.items()))
        if op in _DOC_LEAVES:
            self._doc_mirror.contains(x.encode("utf-8"), bits, mode, op == "$not_contains")
            return
        own = _lib.MQ_MASK_AND if op == "$and" else _lib.MQ_MASK_OR
        if mode == own:
            for c in x:
                self._doc_apply(c, bits, own)
            return
        tmp = torch.empty_like(bits)
        self._doc_apply(x[0], tmp, _lib.MQ_MASK_SET)
        for c in x[1:]:
            self._doc_apply(c, tmp, own)
        mask_combine(bits, tmp, mode)

    def _doc_bits(self, where_document):
        """Device row mask of a (validated) where_document clause over the current rows.  The
        mask of the last clause is kept, keyed by the clause's canonical JSON and _version: a
        retriever with fixed search_kwargs scans the text once, not once per query, and any
        write misses.  The text mirror is built here on first use, extended after plain appends
        and rebuilt after a delete.  The returned tensor is shared: callers only read it."""
        import torch
        key = (json.dumps(where_document, sort_keys=True, ensure_ascii=False), self._version)
        if self._doc_cache is not None and self._doc_cache[0] == key:
            return self._doc_cache[1]
        self._doc_cache = None
        mir = self._doc_mirror
        if mir is None or mir.epoch != self._text_epoch:
            self._doc_mirror = None  # release the old mirror before building the new one
            mir = self._doc_mirror = _TextMirror(self._device, self._text_epoch)
        if mir.version != self._version:
            mir.extend(self._texts[mir.n:])
            mir.version = self._version
        with _lib.device_scope(self._device):
            bits = torch.empty(max(1, (mir.n + 31) // 32), dtype=torch.int32, device=mir.dev)
            self._doc_apply(where_document, bits, _lib.MQ_MASK_SET)
        self._doc_cache = (key, bits)
        return bits

    def _mask_rows(self, bits):
        """A device row mask read back as bool [n rows]."""
        n = len(self._ids)
        return np.unpackbits(bits.cpu().numpy().view(np.uint8), bitorder="little")[:n].astype(bool)

    def _admit(self, k, filter, where_document):
        """-> (k, bits): the device row mask of `filter` and `where_document` together (a row is
        admitted when both admit it; at least one is given) and k clipped for it as the filtered
        search clips it: past MQ_MAX_K the admitted-row count decides between raising and
        returning them all (k = 0: no row is admitted, bits None)."""
        if where_document is None:
            if k > _lib.MQ_MAX_K:
                k = _check_k(k, int(self._cols.mask(filter).sum()))
                if k == 0:
                    return 0, None
            return k, self._cols.dmask(filter, self._device)
        bits = self._doc_bits(where_document)
        if filter:
            both = self._cols.dmask(filter, self._device)
            mask_combine(both, bits, _lib.MQ_MASK_AND)
            bits = both
        if k > _lib.MQ_MAX_K:  # the count comes from the combined mask
            k = _check_k(k, int(self._mask_rows(bits).sum()))
            if k == 0:
                return 0, None
        return k, bits

    def _search_rows(self, vec, k, filter=None, where_document=None):
        """-> list of (row, cosine) for one query vector, best first."""
        if where_document is not None:
            _check_where_document(where_document)
        n = 0 if self._index is None else len(self._index)
        if n == 0 or k <= 0:
            return []
        q = np.ascontiguousarray(vec, dtype=np.float32).reshape(1, -1)
        if not filter and where_document is None:
            kk = _check_k(k, n)
            s, i = self._index.search(q, kk)
            return [(int(r), float(c)) for r, c in zip(i[0], s[0]) if r >= 0]
        # exact filtered search on the device: the where-mask built from the device codes
        # (mq_mask_eval), then the masked search (int8 certified screen with the mask, or
        # the allowed rows gathered on the device); nothing row-sized crosses PCIe
        # (a where_document clause: mq_mask_contains over the device text mirror, ANDed in)
        k, bits = self._admit(k, filter, where_document)  # the result count decides between
        if k == 0:                                        # raising and returning all
            return []
        s, i = self._index.search_masked(q, int(k), bits)
        return [(int(r), float(c)) for r, c in zip(i[0], s[0]) if r >= 0]

    def similarity_search_by_vector_with_score(self, embedding, k=DEFAULT_K, filter=None, where_document=None,
                                               **kwargs):
        return [(self._doc(r), max(0.0, 2.0 - 2.0 * c))
                for r, c in self._search_rows(embedding, k, filter, where_document)]

    def similarity_search_by_vector(self, embedding, k=DEFAULT_K, filter=None, where_document=None, **kwargs):
        return [d for d, _ in self.similarity_search_by_vector_with_score(embedding, k, filter, where_document)]

    def similarity_search_with_score(self, query, k=DEFAULT_K, filter=None, where_document=None, **kwargs):
        if where_document is not None:
            _check_where_document(where_document)
        return self.similarity_search_by_vector_with_score(self._embed_query(query), k, filter, where_document)

    def similarity_search(self, query, k=DEFAULT_K, filter=None, where_document=None, **kwargs):
        return [d for d, _ in self.similarity_search_with_score(query, k, filter, where_document)]

    def similarity_search_with_cosine(self, query, k=DEFAULT_K, filter=None, where_document=None):
        """(Document, cosine similarity) pairs - the index's native score."""
        if where_document is not None:
            _check_where_document(where_document)
        return [(self._doc(r), c)
                for r, c in self._search_rows(self._embed_query(query), k, filter, where_document)]

    def similarity_search_batch(self, queries, k=DEFAULT_K, filter=None, where_document=None):
        """Many queries in one encoder batch + one device search (the throughput path).
        With `filter`, the where-mask is built once on the device and ONE masked search
        call serves the whole batch (mq_index_search_masked_batch); `where_document` is ANDed
        into that mask."""
        if where_document is not None:
            _check_where_document(where_document)
        n = 0 if self._index is None else len(self._index)
        if n == 0 or not queries or k <= 0:
            return [[] for _ in queries]
        if hasattr(self._embedding_function, "embed_array"):
            q = self._embedding_function.embed_array(list(queries))
        else:
            q = np.asarray(self._embedding_function.embed_documents(list(queries)), np.float32)
        if filter or where_document is not None:
            kk, bits = self._admit(k, filter, where_document)
            if kk == 0:
                return [[] for _ in queries]
            _, rows = self._index.search_masked(q, int(kk), bits)
            return [[self._doc(int(r)) for r in row if r >= 0] for row in rows]
        kk = _check_k(k, n)
        _, ids = self._index.search(q, kk)
        return [[self._doc(int(r)) for r in row if r >= 0] for row in ids]

    # ---- maximal marginal relevance --------------------------------------------------------
    def _mmr_rows(self, q, k, fetch_k, lambda_mult, filter=None, where_document=None):
        """-> per query the rows LangChain's maximal_marginal_relevance picks from the top
        fetch_k, in selection order: one search + one selection launch on the device
        (mq_index_search_mmr).  fetch_k is clipped to the candidate rows (the store's, or the
        filter's and where_document's) and must then fit the device top-k; k > fetch_k returns
        fetch_k rows."""
        if where_document is not None:
            _check_where_document(where_document)
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, self._dim or 1)
        n = 0 if self._index is None else len(self._index)
        if n == 0 or k <= 0 or fetch_k <= 0 or not len(q):
            return [[] for _ in range(len(q))]
        bits = None
        if filter or where_document is not None:
            # the admitted-row count decides between raising and clipping, as in _search_rows
            fetch_k, bits = self._admit(fetch_k, filter, where_document)
            if fetch_k == 0:
                return [[] for _ in range(len(q))]
            fetch_k = min(int(fetch_k), n)
        else:
            fetch_k = _check_k(fetch_k, n)
        _, ids = self._index.search_mmr(q, min(int(k), fetch_k), fetch_k, float(lambda_mult), bits)
        return [[int(r) for r in row if r >= 0] for row in ids]

    def max_marginal_relevance_search_by_vector(self, embedding, k=DEFAULT_K, fetch_k=20, lambda_mult=0.5,
                                                filter=None, where_document=None, **kwargs):
        """LangChain's MMR search: the k of the fetch_k most similar rows that trade similarity
        to the query (weight lambda_mult) against similarity to the rows already picked
        (weight 1 - lambda_mult), as Documents in selection order."""
        return [self._doc(r) for r in self._mmr_rows(embedding, k, fetch_k, lambda_mult, filter, where_document)[0]]

    def max_marginal_relevance_search(self, query, k=DEFAULT_K, fetch_k=20, lambda_mult=0.5, filter=None,
                                      where_document=None, **kwargs):
        if where_document is not None:
            _check_where_document(where_document)
        if (self._index is None or len(self._index) == 0) or k <= 0:
            return []
        return self.max_marginal_relevance_search_by_vector(self._embed_query(query), k, fetch_k, lambda_mult,
                                                            filter, where_document)

    def max_marginal_relevance_search_batch(self, queries, k=DEFAULT_K, fetch_k=20, lambda_mult=0.5, filter=None,
                                            where_document=None):
        """Many queries: one encoder batch, one device search and one selection launch."""
        if where_document is not None:
            _check_where_document(where_document)
        n = 0 if self._index is None else len(self._index)
        if n == 0 or not queries or k <= 0:
            return [[] for _ in queries]
        if hasattr(self._embedding_function, "embed_array"):
            q = self._embedding_function.embed_array(list(queries))
        else:
            q = np.asarray(self._embedding_function.embed_documents(list(queries)), np.float32)
        return [[self._doc(r) for r in rows]
                for rows in self._mmr_rows(q, k, fetch_k, lambda_mult, filter, where_document)]

    # ---- grouped search: the top-k distinct values of a metadata key -------------------------
    def _group_room(self, n_groups, nq, k):
        """The group scan's scratch: grows on demand and is kept."""
        import torch
        need = group_scratch_bytes(n_groups, nq, k)
        if self._group_scratch is None or self._group_scratch.numel() < need:
            self._group_scratch = None  # release before growing
            with _lib.device_scope(self._device):
                self._group_scratch = torch.empty(need, dtype=torch.uint8, device=torch.device("cuda", self._device))
        return self._group_scratch

    def _grouped_rows(self, q, k, group_by, filter=None, where_document=None, force_scan=False):
        """-> per query [(row, cosine)]: the representative child row of each of the top-k
        groups of metadata key `group_by`, best first (include/mq.h, "Grouped search").
        Stage 1, the certificate: the ordinary top min(64, rows) (the masked search when a
        filter, a where_document clause or rows without the key are in play, its mask ANDed
        with "has the key") collapsed on the host; `collapse_candidates` says when that is the
        answer.  Stage 2: the uncertified queries of the batch go to ONE mq_index_search_grouped
        call (counted in `group_scans`).  search_precision "bf16" is approximate, so its list
        certifies nothing: it always scans, as `force_scan` does."""
        if where_document is not None:
            _check_where_document(where_document)
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, self._dim or 1)
        nothing = [[] for _ in range(len(q))]
        n = 0 if self._index is None else len(self._index)
        col = self._cols.cols.get(group_by)
        if n == 0 or k <= 0 or not len(q) or col is None or not col[1]:
            return nothing
        if self._dim % 64 or self._dim > 1024:
            raise ValueError("grouped search serves stores of dim %% 64 == 0, dim <= 1024 (this store's dim is %d)"
                             % self._dim)
        n_groups = len(col[1])
        if k > _lib.MQ_MAX_K and n_groups > _lib.MQ_MAX_K:
            raise ValueError("a grouped search returning %d groups (k=%d over %d groups) exceeds the device "
                             "top-k limit MQ_MAX_K=%d" % (min(k, n_groups), k, n_groups, _lib.MQ_MAX_K))
        k = min(int(k), n_groups)
        codes = col[0][:n]
        import torch
        dev = torch.device("cuda", self._device)
        dcodes = self._cols.dev_codes(group_by, dev)
        bits = None
        if filter or where_document is not None:
            _, bits = self._admit(1, filter, where_document)
        out = [None] * len(q)
        todo = list(range(len(q)))
        if not force_scan and self._search_precision != "bf16":
            key = (group_by, self._cols.ver)
            if self._group_absent is None or self._group_absent[0] != key:
                self._group_absent = (key, bool((codes < 0).any()))
            mask1 = bits
            if self._group_absent[1]:  # rows without the key would crowd the list: mask them out
                with _lib.device_scope(self._device):
                    if bits is None:
                        mask1 = torch.empty(max(1, (n + 31) // 32), dtype=torch.int32, device=dev)
                        mask_combine(mask1, None, _lib.MQ_MASK_SET)
                    else:
                        mask1 = bits.clone()
                    lut = np.ones(n_groups + 1, np.uint8)
                    lut[-1] = 0  # the absent entry
                    if len(lut) <= 256:
                        mask_eval_bits(dcodes, lut, mask1, _lib.MQ_MASK_AND)
                    else:
                        mask_eval(dcodes, torch.from_numpy(lut).to(dev), mask1, _lib.MQ_MASK_AND)
            kk = min(_lib.MQ_MAX_K, n)
            s, i = self._index.search(q, kk) if mask1 is None else self._index.search_masked(q, kk, mask1)
            todo = []
            for j in range(len(q)):
                rows, sc, certified = collapse_candidates(i[j], s[j], codes, k)
                if certified:
                    out[j] = list(zip(rows, sc))
                else:
                    todo.append(j)
        if todo:
            self.group_scans += len(todo)
            s, i = self._index.search_grouped(q[todo], k, dcodes, n_groups, bits,
                                              self._group_room(n_groups, len(todo), k))
            for j, sj, ij in zip(todo, s, i):
                out[j] = [(int(r), float(c)) for r, c in zip(ij, sj) if r >= 0]
        return out

    def similarity_search_grouped_by_vector_with_score(self, embedding, k=DEFAULT_K, group_by="doc_id", filter=None,
                                                       where_document=None, _force_scan=False, **kwargs):
        """(Document, squared L2 distance) of the best child of each of the top-k distinct
        `group_by` values, best first: k counts groups, not rows.  Rows without the key are
        skipped (as LangChain's MultiVectorRetriever skips them); a key no row has returns []."""
        return [(self._doc(r), max(0.0, 2.0 - 2.0 * c))
                for r, c in self._grouped_rows(embedding, k, group_by, filter, where_document, _force_scan)[0]]

    def similarity_search_grouped_with_score(self, query, k=DEFAULT_K, group_by="doc_id", filter=None,
                                             where_document=None, _force_scan=False, **kwargs):
        if where_document is not None:
            _check_where_document(where_document)
        if self._index is None or len(self._index) == 0 or k <= 0:
            return []
        return self.similarity_search_grouped_by_vector_with_score(self._embed_query(query), k, group_by, filter,
                                                                   where_document, _force_scan)

    def similarity_search_grouped(self, query, k=DEFAULT_K, group_by="doc_id", filter=None, where_document=None,
                                  _force_scan=False, **kwargs):
        return [d for d, _ in self.similarity_search_grouped_with_score(query, k, group_by, filter, where_document,
                                                                        _force_scan)]

    def similarity_search_grouped_batch(self, queries, k=DEFAULT_K, group_by="doc_id", filter=None,
                                        where_document=None, _force_scan=False):
        """Many queries: one encoder batch, one device search for the certificates, and one
        group scan call for the queries it leaves uncertified."""
        if where_document is not None:
            _check_where_document(where_document)
        queries = list(queries)
        n = 0 if self._index is None else len(self._index)
        if n == 0 or not queries or k <= 0:
            return [[] for _ in queries]
        if hasattr(self._embedding_function, "embed_array"):
            q = self._embedding_function.embed_array(queries)
        else:
            q = np.asarray(self._embedding_function.embed_documents(queries), np.float32)
        return [[self._doc(r) for r, _ in rows]
                for rows in self._grouped_rows(q, k, group_by, filter, where_document, _force_scan)]

    # ---- range search: every row at or above a cosine threshold ----------------------------
    def _range_room(self, n, nq, limit):
        """The range search's scratch: grows on demand and is kept."""
        import torch
        need = range_scratch_bytes(n, nq, limit)
        if self._range_scratch is None or self._range_scratch.numel() < need:
            self._range_scratch = None  # release before growing
            with _lib.device_scope(self._device):
                self._range_scratch = torch.empty(need, dtype=torch.uint8, device=torch.device("cuda", self._device))
        return self._range_scratch

    def _range_rows(self, q, min_cosine=None, limit=None, filter=None, where_document=None):
        """-> per query ([(row, cosine)], total): the rows whose cosine to the query is >=
        min_cosine (None: every row; rounded to fp32, the arithmetic of the comparison), among
        those `filter` / `where_document` admit, best first, at most `limit` of them (None:
        MQ_RANGE_MAX_HITS), and their exact number (include/mq.h, "Range search").  `limit` is
        clipped to the candidate rows and must then fit MQ_RANGE_MAX_HITS.  One
        mq_index_search_range call for the batch, in exact fp32 whatever search_precision is."""
        if where_document is not None:
            _check_where_document(where_document)
        min_score = _check_min_cosine(min_cosine)
        limit = _lib.MQ_RANGE_MAX_HITS if limit is None else int(limit)
        q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, self._dim or 1)
        n = 0 if self._index is None else len(self._index)
        if n == 0 or not len(q):
            return [([], 0) for _ in range(len(q))]
        if self._dim % 64 or self._dim > 1024:
            raise ValueError("range search serves stores of dim %% 64 == 0, dim <= 1024 (this store's dim is %d)"
                             % self._dim)
        bits = None
        if filter or where_document is not None:
            _, bits = self._admit(1, filter, where_document)
        if limit > _lib.MQ_RANGE_MAX_HITS:  # the candidate count decides between raising and clipping
            limit = _check_limit(limit, n if bits is None else int(self._mask_rows(bits).sum()))
        hits = max(1, min(limit, n))        # limit <= 0: the count alone
        counts, s, i = self._index.search_range(q, hits, min_score, bits, self._range_room(n, len(q), hits))
        keep = max(0, min(limit, hits))
        return [([(int(r), float(c)) for r, c in zip(ij[:keep], sj[:keep]) if r >= 0], int(cj))
                for cj, sj, ij in zip(counts, s, i)]

    def similarity_search_range_by_vector_with_score(self, embedding, min_cosine=None, limit=None, filter=None,
                                                     where_document=None, **kwargs):
        """(Document, squared L2 distance) of every row whose cosine to `embedding` is >=
        min_cosine, nearest first (ties: insertion order): a `RangeResult` of at most `limit`
        (None: MQ_RANGE_MAX_HITS) entries whose `total` counts them all."""
        rows, total = self._range_rows(embedding, min_cosine, limit, filter, where_document)[0]
        return RangeResult([(self._doc(r), max(0.0, 2.0 - 2.0 * c)) for r, c in rows], total)

    def similarity_search_range_with_score(self, query, min_cosine=None, limit=None, filter=None,
                                           where_document=None, **kwargs):
        if where_document is not None:
            _check_where_document(where_document)
        _check_min_cosine(min_cosine)
        if self._index is None or len(self._index) == 0:
            return RangeResult()
        return self.similarity_search_range_by_vector_with_score(self._embed_query(query), min_cosine, limit, filter,
                                                                 where_document)

    def similarity_search_range(self, query, min_cosine=None, limit=None, filter=None, where_document=None,
                                **kwargs):
        hits = self.similarity_search_range_with_score(query, min_cosine, limit, filter, where_document)
        return RangeResult([d for d, _ in hits], hits.total)

    def similarity_search_range_batch(self, queries, min_cosine=None, limit=None, filter=None,
                                      where_document=None):
        """Many queries: one encoder batch and one device call -> a `RangeResult` of Documents
        per query."""
        if where_document is not None:
            _check_where_document(where_document)
        _check_min_cosine(min_cosine)
        queries = list(queries)
        n = 0 if self._index is None else len(self._index)
        if n == 0 or not queries:
            return [RangeResult() for _ in queries]
        if hasattr(self._embedding_function, "embed_array"):
            q = self._embedding_function.embed_array(queries)
        else:
            q = np.asarray(self._embedding_function.embed_documents(queries), np.float32)
        return [RangeResult([self._doc(r) for r, _ in rows], total)
                for rows, total in self._range_rows(q, min_cosine, limit, filter, where_document)]

    def count_similar_by_vector(self, embedding, min_cosine, filter=None, where_document=None):
        """The number of rows whose cosine to `embedding` is >= min_cosine, among those `filter`
        / `where_document` admit: the count of the range search, no list."""
        return self._range_rows(embedding, min_cosine, 1, filter, where_document)[0][1]

    def count_similar(self, query, min_cosine, filter=None, where_document=None):
        if where_document is not None:
            _check_where_document(where_document)
        _check_min_cosine(min_cosine)
        if self._index is None or len(self._index) == 0:
            return 0
        return self.count_similar_by_vector(self._embed_query(query), min_cosine, filter, where_document)

    # ---- near-duplicate detection: the self-join of the store ------------------------------
    def _join_room(self, n, n_left):
        """The self-join's scratch: grows on demand and is kept."""
        import torch
        need = join_scratch_bytes(n, n_left)
        if self._join_scratch is None or self._join_scratch.numel() < need:
            self._join_scratch = None  # release before growing
            with _lib.device_scope(self._device):
                self._join_scratch = torch.empty(need, dtype=torch.uint8, device=torch.device("cuda", self._device))
        return self._join_scratch

    def _host_bits(self, mask):
        """bool [n] -> a device row mask in the masked search's layout."""
        import torch
        padded = np.zeros((len(mask) + 31) // 32 * 32 or 32, np.uint8)
        padded[:len(mask)] = mask
        words = np.packbits(padded, bitorder="little").view(np.int32)
        return torch.from_numpy(words).to(torch.device("cuda", self._device))

    def _dup_setup(self, min_cosine, ids, filter, where_document, mode):
        """The checks the duplicate calls share -> (min_score, mode, left rows ascending or None
        for every row, device mask or None)."""
        if where_document is not None:
            _check_where_document(where_document)
        min_score = _check_dup_cosine(min_cosine)
        if mode not in JOIN_MODES:
            raise ValueError("mode must be one of %s, got %r" % (sorted(JOIN_MODES), mode))
        n = 0 if self._index is None else len(self._index)
        if n and (self._dim % 64 or self._dim > 1024):
            raise ValueError("the duplicate scan serves stores of dim %% 64 == 0, dim <= 1024 (this store's dim is %d)"
                             % self._dim)
        if mode == "screen" and n and self._dim not in (256, 512, 768):
            raise ValueError("mode='screen' serves stores of dim 256, 512 or 768 (this store's dim is %d)" % self._dim)
        left = None
        if ids is not None:
            want = [ids] if isinstance(ids, str) else ids
            left = np.array(sorted({self._id_row.row(str(i)) for i in want if str(i) in self._id_row}), np.int64)
        bits = None
        if n and (filter or where_document is not None):
            _, bits = self._admit(1, filter, where_document)
        return min_score, JOIN_MODES[mode], left, bits

    def duplicate_scan(self, min_cosine=0.95, ids=None, filter=None, where_document=None, mode="auto"):
        """Which rows are near-copies of other rows: for every left row (`ids`: those documents,
        for example the ids `add_texts` just returned; None: every row) the number of its
        partners - the other rows `filter` / `where_document` admit whose cosine to it is >=
        min_cosine (in fp32, the range search's arithmetic) - the smallest partner row and the
        nearest partner, as a `DuplicateScan` of host arrays.  A left row the filters do not admit
        has no partner.  One mq_index_self_join call (include/mq.h, "Self-join"); mode "auto",
        "exact" or "screen" picks its path, never its answer."""
        min_score, jmode, left, bits = self._dup_setup(min_cosine, ids, filter, where_document, mode)
        n = 0 if self._index is None else len(self._index)
        rows = np.arange(n, dtype=np.int64) if left is None else left
        if n == 0 or not len(rows):
            e = np.empty(0, np.int64)
            return DuplicateScan(e, e.copy(), e.copy(), e.copy(), np.empty(0, np.float32), np.zeros(4, np.int64))
        c, f, nn, s, info = self._index.self_join(min_score, bits, left, jmode, self._join_room(n, len(rows)))
        return DuplicateScan(rows, c, f, nn, s, info)

    def _dedup_plan(self, min_cosine, ids, filter, where_document, mode, max_rounds):
        """-> (dropped rows, their keepers, undecided rows, rounds) of `greedy_dedup_rounds` over
        the store, each round one mq_index_self_join of the undecided rows."""
        if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or max_rounds < 1:
            raise ValueError("max_rounds must be a positive integer, got %r" % (max_rounds,))
        min_score, jmode, left, bits = self._dup_setup(min_cosine, ids, filter, where_document, mode)
        n = 0 if self._index is None else len(self._index)
        e = np.empty(0, np.int64)
        if n == 0 or (left is not None and not len(left)):
            return e, e, e, 0
        admitted = np.ones(n, bool) if bits is None else self._mask_rows(bits)
        whole = [bits is None]  # the first round of an unfiltered store needs no mask at all

        def scan_first(rows, mask):
            dbits = None if whole[0] and mask.all() else self._host_bits(mask)
            whole[0] = False
            return self._index.self_join(min_score, dbits, rows, jmode, self._join_room(n, len(rows)))[1]

        return greedy_dedup_rounds(n, np.arange(n, dtype=np.int64) if left is None else left, admitted, scan_first,
                                   int(max_rounds))

    def find_duplicates(self, min_cosine=0.95, ids=None, filter=None, where_document=None, mode="auto",
                        max_rounds=32):
        """[(Document, kept Document, cosine)] for every row `deduplicate` would drop with the
        same arguments: the document, the earlier kept document that makes it redundant (the
        smallest such row) and their cosine.  Deletes nothing."""
        dropped, keepers, undecided, rounds = self._dedup_plan(min_cosine, ids, filter, where_document, mode,
                                                               max_rounds)
        out = DedupResult((), [self._ids[r] for r in undecided.tolist()], rounds)
        if len(dropped):
            pairs = self._index.select(np.concatenate([dropped, keepers])).get().astype(np.float64)
            cos = (pairs[:len(dropped)] * pairs[len(dropped):]).sum(1)
            out.extend((self._doc(r), self._doc(k), float(c))
                       for r, k, c in zip(dropped.tolist(), keepers.tolist(), cos.tolist()))
        return out

    def deduplicate(self, min_cosine=0.95, ids=None, filter=None, where_document=None, mode="auto", max_rounds=32):
        """Delete the near-copies and return their ids (a `DedupResult`).  A row is kept iff no
        KEPT earlier row is its partner (cosine >= min_cosine, both admitted by the filters): the
        sequential greedy rule in insertion order, well defined although "near" is not
        transitive.  `ids` limits the rows that may be dropped (for example to the ids
        `add_texts` just returned; every other row is kept and still makes later copies of it
        redundant).  Computed in rounds of whole device scans (`greedy_dedup_rounds`); rows still
        undecided after max_rounds are kept and listed in the result's `undecided`."""
        dropped, _, undecided, rounds = self._dedup_plan(min_cosine, ids, filter, where_document, mode, max_rounds)
        gone = [self._ids[r] for r in dropped.tolist()]
        out = DedupResult(gone, [self._ids[r] for r in undecided.tolist()], rounds)
        if gone:
            self.delete(gone)
        return out

    # ---- clustering: k-means over the store's rows ------------------------------------------
    def _kmeans_room(self, n, n_clusters):
        """The k-means scratch: grows on demand and is kept."""
        import torch
        need = kmeans_scratch_bytes(n, n_clusters)
        if self._kmeans_scratch is None or self._kmeans_scratch.numel() < need:
            self._kmeans_scratch = None  # release before growing
            with _lib.device_scope(self._device):
                self._kmeans_scratch = torch.empty(need, dtype=torch.uint8, device=torch.device("cuda", self._device))
        return self._kmeans_scratch

    def _cluster_run(self, n_clusters, max_iter, init, seed, ids, filter, where_document):
        """-> (ClusterResult, device mask or None, admitted rows ascending): the checks, the mask
        (`ids` ANDed with the filters), the seeding and one mq_index_kmeans call."""
        if where_document is not None:
            _check_where_document(where_document)
        n_clusters, max_iter, init = _check_cluster_args(n_clusters, max_iter, init, seed, self._dim)
        n = 0 if self._index is None else len(self._index)
        if n and (self._dim % 64 or self._dim > 1024):
            raise ValueError("clustering serves stores of dim %% 64 == 0, dim <= 1024 (this store's dim is %d)"
                             % self._dim)
        bits, admitted = None, np.ones(n, bool)
        if n and (filter or where_document is not None):
            _, bits = self._admit(1, filter, where_document)
            admitted = np.asarray(self._mask_rows(bits), bool)
        if ids is not None:
            want = [ids] if isinstance(ids, str) else ids
            named = np.zeros(n, bool)
            named[[self._id_row.row(str(i)) for i in want if str(i) in self._id_row]] = True
            admitted = admitted & named
            bits = self._host_bits(admitted) if n else None
        adm = np.flatnonzero(admitted)
        if len(adm) < n_clusters:
            raise ValueError("n_clusters=%d exceeds the %d rows the filters admit" % (n_clusters, len(adm)))
        room = self._kmeans_room(n, n_clusters)
        if isinstance(init, str):
            rng = np.random.default_rng(seed)
            if init == "random":
                seeds = rng.choice(adm, n_clusters, replace=False)
            else:
                def dots_of_row(p):
                    return self._index.kmeans(self._index.get(int(adm[p]), 1), 0, bits, room)[2][adm]
                seeds = adm[kmeanspp_rows(len(adm), n_clusters, rng, dots_of_row)]
            init = self._index.select(np.asarray(seeds, np.int64)).get()
        cent, assign, dots, counts, info = self._index.kmeans(init, max_iter, bits, room)
        labels = assign[adm]
        c2 = (cent.astype(np.float64) ** 2).sum(1)
        inertia = float((1.0 - 2.0 * dots[adm].astype(np.float64) + c2[labels]).sum())
        res = ClusterResult([self._ids[r] for r in adm.tolist()], labels, cent, counts, info[0], info[1] == 0, inertia)
        return res, bits, adm

    def cluster(self, n_clusters=5, max_iter=25, init="k-means++", seed=0, ids=None, filter=None,
                where_document=None):
        """K-means over the store's rows (LangChain's `EmbeddingsClusteringFilter`, at the scale of
        the store): Lloyd iterations on the device in exact fp32 (mq_index_kmeans, the definition:
        include/mq.h "K-means") -> a `ClusterResult`.  The rows are those `filter` /
        `where_document` admit and, with `ids`, those documents only (for example a range search's
        hits).  init: an [n_clusters, dim] array of centres, "random" (default_rng(seed).choice of
        the admitted rows, without replacement) or "k-means++" (`kmeanspp_rows`; every draw costs
        one pass over the rows).  max_iter = 0 with an array init only labels the rows against the
        given centres.  Fewer admitted rows than n_clusters raise ValueError.  Deterministic: the
        same store, arguments and seed give the same bits."""
        return self._cluster_run(n_clusters, max_iter, init, seed, ids, filter, where_document)[0]

    def cluster_representatives(self, n_clusters=5, num_closest=1, sorted=False, remove_duplicates=False,
                                **cluster_kwargs):
        """The documents nearest each cluster centre: LangChain's `EmbeddingsClusteringFilter
        .transform_documents` over the store.  After `cluster(n_clusters, **cluster_kwargs)` the
        clusters are walked in order, each with the admitted rows ranked by nearness to its centre
        (cosine descending, ties in insertion order - for unit rows the Euclidean order LangChain
        sorts by).  With remove_duplicates: the first num_closest of the ranking, minus those
        already taken.  Without it: the first num_closest of the ranking not already taken.  The
        documents come in pick order, or in insertion order when `sorted` (`pick_representatives`).
        The rankings are one range search with the centres as queries under the same mask, of
        min(n_clusters x num_closest, admitted rows) entries each - enough, since at most
        (n_clusters - 1) x num_closest rows are taken earlier; past MQ_RANGE_MAX_HITS it raises."""
        if isinstance(num_closest, bool) or not isinstance(num_closest, (int, np.integer)) or num_closest < 1:
            raise ValueError("num_closest must be a positive integer, got %r" % (num_closest,))
        res, bits, adm = self._cluster_run(n_clusters, cluster_kwargs.pop("max_iter", 25),
                                           cluster_kwargs.pop("init", "k-means++"), cluster_kwargs.pop("seed", 0),
                                           cluster_kwargs.pop("ids", None), cluster_kwargs.pop("filter", None),
                                           cluster_kwargs.pop("where_document", None))
        if cluster_kwargs:
            raise TypeError("unexpected arguments %s" % list(cluster_kwargs))
        hits = _check_limit(int(n_clusters) * int(num_closest), len(adm))
        n = len(self._index)
        _, _, rows = self._index.search_range(res.centroids, hits, -math.inf, bits,
                                              self._range_room(n, len(res.centroids), hits))
        picks = pick_representatives([r[r >= 0] for r in rows], int(num_closest), bool(remove_duplicates), bool(sorted))
        return [self._doc(r) for r in picks]

    # ---- lexical (BM25) and hybrid (reciprocal rank fusion) retrieval ----------------------
    def _lex_tok(self):
        tok = self._lex_tokenizer
        if tok is None:
            tok = getattr(self._embedding_function, "tokenizer", None)
        if tok is None:
            raise ValueError("lexical search needs a tokenizer: pass HipChroma(lexical_tokenizer=) or an "
                             "embedding_function with a `tokenizer`")
        vocab = getattr(tok, "vocab_size", None)
        if isinstance(vocab, int) and vocab > 65536:
            raise ValueError("lexical search stores token ids as uint16: the tokenizer's vocabulary must not "
                             "exceed 65536 ids (got %d)" % vocab)
        return tok

    def _lex(self):
        """The token mirror in step with the store: built at the first use, extended after plain
        appends (df cache dropped), rebuilt when a delete renumbered the rows."""
        tok = self._lex_tok()
        mir = self._lex_mirror
        if mir is None or mir.epoch != self._text_epoch or mir.tokenizer is not tok:
            self._lex_mirror = None  # release the old mirror before building the new one
            mir = self._lex_mirror = _TokenMirror(self._device, self._text_epoch, tok, self._lex_ngram)
        if mir.version != self._version:
            mir.extend(self._texts[mir.n:])
            mir.version = self._version
        return mir

    def _candidates(self, k, filter, where_document):
        """-> (k, bits) for a top-k over the store's rows or the rows `filter` / `where_document`
        admit (bits None: all rows), k clipped as every search here clips it; k = 0: nothing."""
        n = 0 if self._index is None else len(self._index)
        if n == 0 or k <= 0:
            return 0, None
        if filter or where_document is not None:
            k, bits = self._admit(k, filter, where_document)
            return min(int(k), n), bits
        return _check_k(k, n), None

    def _lex_rows(self, mir, query, k, bits):
        """-> [(row, bm25 score)] of one query, best first (k already clipped)."""
        plan = mir.plan(query, *self._bm25) if k > 0 else None
        if plan is None:
            return []
        s, i = mir.topk(plan, int(k), bits)
        return [(int(r), float(x)) for r, x in zip(i, s) if r >= 0]

    def _lex_rows_batch(self, mir, queries, k, bits):
        """`_lex_rows` of every query.  Two or more queries take the batch path: one plan_batch
        (one tokenizer call, one df call) and one topk_batch (one scan per group of queries, one
        copy of the result); a query without terms gets [].  One query keeps the single path."""
        if len(queries) < LEX_BATCH_MIN or k <= 0:
            return [self._lex_rows(mir, q, k, bits) for q in queries]
        plans = mir.plan_batch(queries, *self._bm25)
        live = [j for j, p in enumerate(plans) if p is not None]
        out = [[] for _ in queries]
        if live:
            s, i = mir.topk_batch([plans[j] for j in live], int(k), bits)
            for j, sj, ij in zip(live, s, i):
                out[j] = [(int(r), float(x)) for r, x in zip(ij, sj) if r >= 0]
        return out

    def lexical_search_with_score(self, query, k=DEFAULT_K, filter=None, where_document=None, **kwargs):
        """(Document, BM25 score) pairs, best first: the rows holding at least one of the query's
        terms, ranked on the device over the token mirror (include/mq.h, "Lexical retrieval")."""
        return self.lexical_search_batch_with_score([query], k, filter, where_document)[0]

    def lexical_search(self, query, k=DEFAULT_K, filter=None, where_document=None, **kwargs):
        return [d for d, _ in self.lexical_search_with_score(query, k, filter, where_document)]

    def lexical_search_batch_with_score(self, queries, k=DEFAULT_K, filter=None, where_document=None):
        if where_document is not None:
            _check_where_document(where_document)
        self._lex_tok()
        queries = list(queries)
        k, bits = self._candidates(k, filter, where_document)
        if k == 0 or not queries:
            return [[] for _ in queries]
        mir = self._lex()
        return [[(self._doc(r), x) for r, x in rows] for rows in self._lex_rows_batch(mir, queries, k, bits)]

    def lexical_search_batch(self, queries, k=DEFAULT_K, filter=None, where_document=None):
        """Many queries: the mask is built once and two or more queries are ranked by the batch
        path (mq_lex_df_batch / mq_lex_topk_batch: one scan of the token mirror per group of up
        to 16 queries instead of one per query); each result is the single query's exactly."""
        return [[d for d, _ in hits]
                for hits in self.lexical_search_batch_with_score(queries, k, filter, where_document)]

    def _hybrid(self, queries, k, fetch_k, weights, c, filter, where_document):
        if where_document is not None:
            _check_where_document(where_document)
        _check_rrf(weights, c)
        self._lex_tok()
        queries = list(queries)
        if self._embedding_function is None:
            raise ValueError("HipChroma needs an embedding_function to search by text")
        # fetch_k is clipped to MQ_MAX_K and to the candidate rows (fetch_k <= 0: nothing, as MMR's);
        # k follows the rule of every search here: past MQ_MAX_K it raises unless no more than
        # MQ_MAX_K rows are candidates
        fk, bits = self._candidates(min(int(fetch_k), _lib.MQ_MAX_K), filter, where_document)
        if fk == 0 or k <= 0 or not queries:
            return [[] for _ in queries]
        if k > _lib.MQ_MAX_K:
            k, _ = self._candidates(k, filter, where_document)
        if len(queries) == 1:
            q = self._embed_query(queries[0]).reshape(1, -1)
        elif hasattr(self._embedding_function, "embed_array"):
            q = self._embedding_function.embed_array(queries)
        else:
            q = np.asarray(self._embedding_function.embed_documents(queries), np.float32)
        q = np.ascontiguousarray(q, dtype=np.float32)
        _, dense = self._index.search(q, fk) if bits is None else self._index.search_masked(q, fk, bits)
        mir = self._lex()
        out = []
        for lrow, drow in zip(self._lex_rows_batch(mir, queries, fk, bits), dense):
            lex = [r for r, _ in lrow]
            fused = rrf_fuse([int(r) for r in drow if r >= 0], lex, weights, c, k)
            out.append([(self._doc(r), x) for r, x in fused])
        return out

    def hybrid_search_with_score(self, query, k=DEFAULT_K, fetch_k=20, weights=(0.5, 0.5), c=60, filter=None,
                                 where_document=None, **kwargs):
        """(Document, rrf) pairs: the dense top fetch_k (the store's own search) and the lexical
        top fetch_k fused by weighted reciprocal rank (`rrf_fuse`: LangChain's EnsembleRetriever
        over [dense, BM25]), the first k.  fetch_k is clipped to the candidate rows and to
        MQ_MAX_K."""
        return self._hybrid([query], k, fetch_k, weights, c, filter, where_document)[0]

    def hybrid_search(self, query, k=DEFAULT_K, fetch_k=20, weights=(0.5, 0.5), c=60, filter=None,
                      where_document=None, **kwargs):
        return [d for d, _ in self.hybrid_search_with_score(query, k, fetch_k, weights, c, filter, where_document)]

    def hybrid_search_batch(self, queries, k=DEFAULT_K, fetch_k=20, weights=(0.5, 0.5), c=60, filter=None,
                            where_document=None):
        """Many queries: one encoder batch, one dense search, one batched lexical call (as
        `lexical_search_batch`); the fusion stays on the host."""
        return [[d for d, _ in hits]
                for hits in self._hybrid(queries, k, fetch_k, weights, c, filter, where_document)]

    def as_retriever(self, **kwargs):
        """search_type "lexical" / "hybrid" / "grouped" / "range": a retriever over
        `lexical_search` / `hybrid_search` / `similarity_search_grouped` /
        `similarity_search_range` with search_kwargs passed on (range: min_cosine, limit, filter,
        where_document); every other type is the base class's, "similarity_score_threshold"
        (score_threshold, k, filter, where_document -> `similarity_search_with_relevance_scores`)
        among them."""
        if kwargs.get("search_type") in ("lexical", "hybrid", "grouped", "range"):
            return _LexicalRetriever(self, kwargs["search_type"], kwargs.get("search_kwargs"))
        return super().as_retriever(**kwargs)

    def _select_relevance_score_fn(self):
        if self.override_relevance_score_fn:
            return self.override_relevance_score_fn
        return lambda d: 1.0 - d / math.sqrt(2)  # LangChain's euclidean relevance

    def similarity_search_with_relevance_scores(self, query, k=DEFAULT_K, score_threshold=None, **kwargs):
        """(Document, relevance) of the top k; with `score_threshold`, the pairs of them whose
        relevance is >= it (the filter of LangChain's base class, whatever relevance_score_fn is)."""
        if score_threshold is not None:
            score_threshold = _check_score_threshold(score_threshold)
        fn = self._select_relevance_score_fn()
        pairs = [(d, fn(s)) for d, s in self.similarity_search_with_score(query, k, **kwargs)]
        if score_threshold is not None:
            pairs = [(d, r) for d, r in pairs if r >= score_threshold]
        return pairs

    # ---- constructors ------------------------------------------------------------------
    @classmethod
    def from_texts(cls, texts, embedding=None, metadatas=None, ids=None,
                   collection_name="langchain", persist_directory=None, **kwargs):
        store = cls(collection_name=collection_name, embedding_function=embedding,
                    persist_directory=persist_directory, _ingest=True, **kwargs)
        store.add_texts(texts, metadatas=metadatas, ids=ids)
        return store

    @classmethod
    def from_documents(cls, documents, embedding=None, ids=None, collection_name="langchain",
                       persist_directory=None, **kwargs):
        documents = list(documents)
        return cls.from_texts([d.page_content for d in documents], embedding,
                              metadatas=[d.metadata for d in documents], ids=ids,
                              collection_name=collection_name,
                              persist_directory=persist_directory, **kwargs)

    def __len__(self):
        return len(self._ids)
