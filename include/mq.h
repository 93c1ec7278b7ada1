/*
 * mq.h - C ABI of the MI355X dense-retrieval backend (libmqhip.so).
 *
 * Drop-in boundary for MediQuery-RAG's retrieval pair:
 *   - the encoder replaces OllamaEmbeddings("shaw/dmeta-embedding-zh")
 *       reference src/medical_engine.py:43, src/ingest_medical.py:104
 *       (LangChain Embeddings.embed_query / embed_documents)
 *   - the index replaces the Chroma collection's k-NN
 *       reference src/medical_engine.py:52, src/ingest_medical.py:106-110,
 *       called as vectorstore.similarity_search(query, k=5) at src/agents/nodes.py:93
 * The reference is pure Python; its "FFI" for this path is the LangChain interface.
 * The Python classes in mediquery-rag_amd/mediquery_hip/ bind these entry points with
 * ctypes.
 *
 * Conventions
 *   - Every entry point returns MQ_OK (0) or a negative MQ_E* status; the message of
 *     the last failure on the calling thread is in mq_last_error().
 *   - Pointers flagged "device" are HIP device pointers (e.g. torch data_ptr()); host
 *     pointers are plain malloc/numpy memory.  `stream` is a hipStream_t (NULL = the
 *     default stream).  Host-pointer calls synchronise before returning; device-pointer
 *     calls are asynchronous on `stream`.
 *   - Handles own their device memory; the caller owns every buffer it passes in.
 *   - One handle is used by one thread at a time (each handle has an internal mutex).
 *   - Row identity = insertion order (0..N-1).  Scores are cosine similarities of the
 *     query with the L2-normalised stored row; results are ordered by score desc, then
 *     row id asc.  k > N returns N results and pads the rest with (-inf, -1); an empty
 *     index returns only padding.
 */
#ifndef MQ_H
#define MQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MQ_OK 0
#define MQ_EINVAL -1   /* bad argument                       */
#define MQ_ENOMEM -2   /* device or host allocation failed   */
#define MQ_EHIP -3     /* HIP runtime error                  */
#define MQ_EIO -4      /* file I/O error (save/load)         */
#define MQ_ESTATE -5   /* handle in the wrong state          */

#define MQ_DTYPE_F32 0    /* exact fp32 MFMA (v_mfma_f32_32x32x2_f32)                     */
#define MQ_DTYPE_BF16 1   /* bf16 storage (coarse paths)                                    */
#define MQ_DTYPE_F32X6 2  /* fp32 operands split exactly into 3 bf16 pieces, 6 bf16 MFMAs per
                           * product, fp32 accumulate: fp32-class error, 2.67x the MFMA rate;
                           * encoder GEMMs too small to fill the chip (few-row / long single
                           * queries) run exact fp32, which is faster there */
#define MQ_DTYPE_F32_SCREEN 3 /* search only: exact fp32 top-k through certified screens -
                               * bf16 shadow scan for k + 8..16 candidates, fp32 re-rank,
                               * proven error bound; uncertified queries re-run on the
                               * split-f32 screen, then the direct exact scan */

#define MQ_GELU_ERF 0  /* exact erf GELU (HF BERT "gelu")            */
#define MQ_GELU_TANH 1 /* tanh approximation (ggml / llama.cpp gelu)  */
#define MQ_POOL_CLS 0
#define MQ_POOL_MEAN 1

#define MQ_MAX_K 64    /* largest k one search call returns          */
#define MQ_RANGE_MAX_HITS 4096 /* longest list of mq_index_search_range */

typedef struct mq_index mq_index;
typedef struct mq_encoder mq_encoder;

/* Thread-local message of the most recent failure ("" if none). */
const char* mq_last_error(void);
/* Library build string (arch, version). */
const char* mq_version(void);
/* Build provenance: the first 16 hex digits of the SHA-256 of the csrc/ sources, the
 * Makefile and this header the library was built from (csrc/Makefile STAMPED). */
const char* mq_build_source_hash(void);
/* Number of visible HIP devices (0 without a GPU); never fails. */
int mq_device_count(void);

/* ---------------------------------------------------------------- index ---- */
/* Flat, HBM-resident index of `dim`-wide rows (dim % 32 == 0).  `capacity` rows are
 * reserved up front (it grows on demand by re-allocation).  dtype MQ_DTYPE_F32 is the
 * exact path; MQ_DTYPE_BF16 stores rows in bf16 (coarse path). */
int mq_index_create(int device, int dim, int64_t capacity, int dtype, mq_index** out);
int mq_index_destroy(mq_index* ix);
int mq_index_size(const mq_index* ix, int64_t* n_rows);
int mq_index_dim(const mq_index* ix, int* dim);
/* Append n rows (K8): each row is L2-normalised on the device and stored at the next
 * row ids.  `rows` is [n, dim] f32, host or device. */
int mq_index_add(mq_index* ix, const float* rows, int64_t n, int rows_on_device, void* stream);
/* Drop every row (capacity kept). */
int mq_index_reset(mq_index* ix);
/* Exact top-k (K9 fused score + per-block top-k, K10 merge).
 * queries [nq, dim] f32; out_scores [nq, k] f32; out_ids [nq, k] int64.
 * All three host (io_on_device = 0) or all device (io_on_device = 1). 1 <= k <= MQ_MAX_K.
 * Device calls are asynchronous on `stream` for k <= 16; for k > 16 the call reads a
 * 4-byte overflow flag back (the scan keeps 16 candidates per list and re-scans with
 * 64 when a list may have dropped a top-k member), so it returns after the search. */
int mq_index_search(mq_index* ix, const float* queries, int64_t nq, int k,
                    float* out_scores, int64_t* out_ids, int io_on_device, void* stream);
/* Replace dst's rows with src's rows[0..n) (host int64 row ids in [0, size(src)), any
 * order, repeats allowed), gathered on the device - no host copy of the slab.  dst may be
 * src (in-place compaction after a delete).  Used for Chroma-style `filter` searches
 * and `delete` (reference VectorStore surface).  Synchronous. */
int mq_index_select(mq_index* src, const int64_t* rows, int64_t n, mq_index* dst);
/* Copy stored (normalised) rows [row0, row0 + n) into out [n, dim] f32 (host or device). */
int mq_index_get(mq_index* ix, int64_t row0, int64_t n, float* out, int out_on_device, void* stream);
/* Arithmetic of the fused scan: MQ_DTYPE_F32 (default, exact), MQ_DTYPE_F32X6 (split
 * fp32, large batches; small batches stay on the exact kernel, HBM-bound there), or
 * MQ_DTYPE_BF16: bf16 shadow slab scanned on bf16 MFMA for the top max(k, 50) (capped
 * at MQ_MAX_K) candidates, then an exact fp32 re-rank to the top-k (BASELINE config 5;
 * approximate: recall vs exact is measured, not guaranteed).  dim % 64 == 0.
 * MQ_DTYPE_F32_SCREEN: exact fp32 results via certified screens (above): single queries
 * stream the bf16 shadow (half the HBM bytes), batches scan it on bf16 MFMA; scores are
 * the fp32 re-rank's dot products.  Batches are asynchronous on `stream` (uncertified
 * queries are re-run exactly on the device, mq_index_set_async_screen); single queries
 * and the synchronous batch path read the certificate count back. */
int mq_index_set_precision(mq_index* ix, int dtype);
/* Batches of at most `max_queries` queries (default 4, 0..16; dim % 64 == 0, dim <= 1024)
 * use the streaming fp32 kernel instead of the MFMA tiles, whatever the precision. */
int mq_index_set_stream_threshold(mq_index* ix, int max_queries);
/* Batched bf16 candidate scans (MQ_DTYPE_F32_SCREEN batches, MQ_DTYPE_BF16) of more than
 * 64 queries over >= 65536 rows with dim 256/512/768: 1 (default) = the threshold scan
 * (sample pass -> per-query threshold -> one streaming pass keeping the rows that clear
 * it -> top-kc of the survivors), 0 = the tiled scan with per-lane lists + merge.
 * Same candidates either way up to bf16-score ties at the kc-th place. */
int mq_index_set_threshold_scan(mq_index* ix, int enabled);
/* Single-query MQ_DTYPE_F32_SCREEN searches over >= 65536 rows of dim 256/512/768/1024:
 * 1 (default) = screen on an int8 shadow first (one byte per element + a per-row scale,
 * threshold scan for 64 candidates, fp32 re-rank, certificate with the int8 shadow's
 * measured error bound); uncertified queries re-run on the bf16 stream tier, and after a
 * run of failures (a corpus whose top scores crowd within the int8 bound) the int8 tier
 * sits out the next 256 searches.  0 = start at the bf16 stream tier.  Same results. */
int mq_index_set_int8_screen(mq_index* ix, int enabled);
/* Batched MQ_DTYPE_F32_SCREEN searches: 1 (default) = asynchronous - the certificate
 * failures are never read back; kernels enqueued after the certificate gather the
 * uncertified queries and re-run ALL of them in one exact-f32 MFMA pass over the slab
 * (the direct scan's tile, shape picked on the device from the failure count), merge
 * and write their results in place, returning at once when nothing failed; once a
 * failure has been seen (polled without waiting) the next 16 batches take the
 * synchronous path, and a failure share above 0.2 there sends the next 64 batches
 * straight to the split-f32 screen.
 * The bf16 tier serves k <= 16 only (its 64 candidates leave no margin past that): larger
 * k runs the split-f32 screen (batches > 64) or the direct exact scan.
 * 0 = synchronous: read the failure count, re-run the failures one tier down (split-f32
 * screen, then the direct exact scan).  Same results up to fp32 ties. */
int mq_index_set_async_screen(mq_index* ix, int enabled);
/* Counters of the k > 16 overflow checks so far (either pointer may be NULL): searches
 * re-scanned with 64-entry scan lists, and merges re-run with 64-entry thread lists. */
int mq_index_rescans(const mq_index* ix, int64_t* rescans, int64_t* remerges);
/* Screen counters (MQ_DTYPE_F32_SCREEN; either pointer may be NULL): queries whose
 * certificates failed and that were re-run on the direct exact scan (or on the device
 * by the asynchronous batch path: counting those waits for the last asynchronous
 * search's count copy on its stream), and queries passed down to the next screen
 * (bf16 batch -> split-f32, int8 single -> bf16 stream). */
int mq_index_screen_fallbacks(const mq_index* ix, int64_t* to_direct, int64_t* to_split);
/* Screened searches that bypassed a tier after a run of failed certificates (either
 * pointer may be NULL): batches that skipped the bf16 tier (failure share above 0.2: it
 * sits out 64 searches, then is tried again), and single queries that skipped the int8
 * tier (share above 0.3: it sits out 256). */
int mq_index_screen_skips(const mq_index* ix, int64_t* bf16_skips, int64_t* int8_skips);
/* Device pointer of the row slab ([capacity, dim] of the index dtype). */
int mq_index_data(mq_index* ix, void** device_rows);
/* Device-time accounting with HIP events on the launch stream (off by default).
 * read_timing returns the ms accumulated since the last read: [0] K9 score + top-k,
 * [1] K10 merge; it synchronises on the recorded events and resets the counters. */
int mq_index_set_timing(mq_index* ix, int enabled);
int mq_index_read_timing(mq_index* ix, float* ms, int n);
/* Filtered search (Chroma's `similarity_search(filter=...)`, src/medical_engine.py:52,
 * the LangChain VectorStore surface): a row mask on the device, bit r % 32 of word r / 32
 * set = row r allowed, built from the store's metadata columns by mq_mask_eval /
 * mq_mask_combine (device pointers, async on stream), then one exact search over the
 * allowed rows.  mq_mask_eval: bits (mode)= lut[codes[r]] for rows [0, n), codes[r] = -1
 * (key absent) or >= n_lut - 1 read lut[n_lut - 1]; mq_mask_combine: dst (mode)= src,
 * src NULL = all ones, MQ_MASK_CLEAR zeroes dst. */
#define MQ_MASK_SET 0
#define MQ_MASK_AND 1
#define MQ_MASK_OR 2
#define MQ_MASK_CLEAR 3
int mq_mask_eval(const int32_t* codes, int64_t n, const uint8_t* lut, int n_lut, uint32_t* bits, int mode,
                 void* stream);
/* mq_mask_eval with the table passed by value: lut_words a HOST array of ceil(n_lut / 64)
 * words, bit i % 64 of word i / 64 = lut[i], n_lut <= 256 (a key with few distinct values:
 * no host-to-device copy per condition). */
int mq_mask_eval_bits(const int32_t* codes, int64_t n, const uint64_t* lut_words, int n_lut, uint32_t* bits,
                      int mode, void* stream);
int mq_mask_combine(uint32_t* dst, const uint32_t* src, int64_t n_words, int mode, void* stream);
/* Exact top-k of one query over the allowed rows (same ranking and padding as
 * mq_index_search; bits: a device mask of >= ceil(n / 32) words on the index's GPU).  The
 * int8 certified screen runs with the mask; an uncertified query is answered by the
 * streaming exact scan with the mask (counted by mq_index_masked_gathers).  Synchronous.
 * The mq_mask_* calls launch on the GPU their buffers live on (`stream` must belong to it).
 * Replaces Chroma's `similarity_search(filter=)` / `query(where=)` (src/medical_engine.py:52). */
int mq_index_search_masked(mq_index* ix, const float* query, int k, const uint32_t* bits, float* out_scores,
                           int64_t* out_ids, int io_on_device, void* stream);
/* The same for nq queries at once (queries [nq, dim], outputs [nq, k]; one mask for all) -
 * Chroma's batched `query(query_embeddings=[...], where=)`.  Batches of > 64 queries with
 * k <= 16 run the bf16 threshold scan (K9t) with the mask + fp32 re-rank + certificate;
 * uncertified queries and other batches run the masked streaming exact scan. */
int mq_index_search_masked_batch(mq_index* ix, const float* queries, int64_t nq, int k, const uint32_t* bits,
                                 float* out_scores, int64_t* out_ids, int io_on_device, void* stream);
int mq_index_masked_gathers(const mq_index* ix, int64_t* count);
/* Document-text conditions (Chroma's `where_document={"$contains": s}` / `$not_contains` on
 * `similarity_search*`, `max_marginal_relevance_search*` and `get` of the LangChain Chroma
 * surface, which the store replaces: src/medical_engine.py:52) as a row mask for the masked
 * searches above: bits (mode)= contains(r) ^ negate for rows [0, n), where contains(r) = the
 * pattern's bytes occur in row r's bytes (a byte-substring match: on UTF-8 text it equals the
 * substring match of the decoded strings; a match never spans two rows).  mode MQ_MASK_SET /
 * AND / OR as mq_mask_eval; the bits past n in the last word come out 0 under SET and AND
 * (also with negate) and unchanged under OR; n == 0 is a no-op.
 *   text     device, the rows' UTF-8 bytes concatenated, 16-byte aligned (any hipMalloc'ed or
 *            torch buffer's start); only [0, text_bytes) is read, no padding behind it is
 *            needed.  May be NULL when text_bytes == 0.
 *   offsets  device int64 [n + 1], non-decreasing, offsets[0] == 0, offsets[n] == text_bytes;
 *            row r is text[offsets[r], offsets[r + 1]) (zero-length rows allowed).  The kernel
 *            trusts them, but writes no bit outside rows [0, n) whatever they hold.
 *   pattern  HOST pointer, pattern_len in [1, MQ_CONTAINS_MAX_BYTES] bytes, passed to the
 *            kernel by value (no host-to-device copy per condition, as mq_mask_eval_bits).
 *   negate   0 or 1.
 *   scratch  device, ceil(n / 32) words the call overwrites (the hit mask the scan ORs into
 *            before negate and mode are applied; the caller provides it so that the call
 *            allocates and frees no device memory); not bits.
 * The scan (contains_scan_kernel, K12) gives each workgroup one span of
 * MQ_CONTAINS_SPAN_BYTES text bytes (+ a halo of pattern_len - 1), 64-bit byte addressing
 * throughout.  Asynchronous on `stream`; launches on the GPU the buffers live on.  The argument
 * checks (sizes, pattern_len, mode, negate, NULL pointers with n > 0, alignment) come before
 * any HIP call. */
#define MQ_CONTAINS_MAX_BYTES 256
#define MQ_CONTAINS_SPAN_BYTES 16384
int mq_mask_contains(const uint8_t* text, int64_t text_bytes, const int64_t* offsets, int64_t n,
                     const uint8_t* pattern, int pattern_len, int negate, uint32_t* bits, int mode,
                     uint32_t* scratch, void* stream);

/* Lexical retrieval: Okapi BM25 over a device mirror of the documents' token ids, brute force
 * (no inverted index), as the flat index and mq_mask_contains are; it replaces LangChain's
 * BM25Retriever next to the dense search (EnsembleRetriever, fused by reciprocal rank on the
 * host: vectorstore.py).  The definition:
 *   terms    a row's terms are its body token ids (the tokenizer's ids without [CLS] / [SEP]),
 *            stored as uint16.  ngram = 1: a term key is the id; ngram = 2: a term key is
 *            (id[i] << 16) | id[i + 1] for adjacent tokens of one row (never across a row
 *            start), so a row of L tokens has max(L - 1, 0) terms.
 *   stats    over ALL n rows (masked-out and zero-length rows count): N = n, dl_r = the number
 *            of terms of row r, avgdl = sum dl_r / N, df_t = the rows holding term t.
 *   score    Lucene's non-negative idf with the classic numerator; for the query's distinct
 *            terms t with query counts qf_t:
 *              idf_t   = ln(1 + (N - df_t + 0.5) / (df_t + 0.5))
 *              w_t     = qf_t (k1 + 1) idf_t                    host, float64, rounded to fp32
 *              c0, c1  = k1 (1 - b),  k1 b / avgdl              host, float64, rounded to fp32
 *              score_r = sum_t w_t tf_rt / (tf_rt + c0 + c1 dl_r)      device, fp32
 *            tf_rt is an exact integer count.  The device sums the terms with tf_rt > 0 in slot
 *            order (the order of `keys`), every operation rounded to nearest and never
 *            contracted, written once below as MQ_LEX_NORM / MQ_LEX_TERM over the caller's
 *            rounding primitives: two rows with equal counts and equal dl score bitwise equal.
 *   result   only rows with at least one query term (sum tf > 0) that the mask admits are
 *            candidates; ordered by (score desc, row id asc), padded with (-inf, -1).
 * A caller with more than MQ_LEX_MAX_TERMS distinct query terms computes df for all of them in
 * chunks and keeps the MQ_LEX_MAX_TERMS with the largest idf (ties to the smaller key).
 *   tokens   device uint16 [n_tokens], the rows' token ids concatenated, 16-byte aligned; only
 *            [0, n_tokens) is read.  May be NULL when n_tokens == 0.
 *   offsets  device int64 [n + 1] counted in tokens, non-decreasing, offsets[0] == 0,
 *            offsets[n] == n_tokens (zero-length rows allowed).  The kernel trusts them but
 *            reads no token outside [0, n_tokens) and counts into its own rows only.
 *   keys, w  HOST arrays of n_terms distinct keys / their weights, passed to the kernel by
 *            value (1 <= n_terms <= MQ_LEX_MAX_TERMS).
 *   bits     device row mask (bit r % 32 of word r / 32, >= ceil(n / 32) words) or NULL = all.
 *   scratch  device, mq_lex_scratch_bytes(n, k) bytes (k = MQ_MAX_K serves every k; mq_lex_df
 *            needs mq_lex_scratch_bytes(n, 1)), 16-byte aligned; neither call allocates or
 *            frees device memory; not one of the outputs.
 * lex_scan_kernel (K14): a workgroup owns blocks of 64 consecutive rows, whose tokens are one
 * contiguous stretch of the blob; it streams the stretch position-parallel (16-byte loads, 8
 * tokens a lane), probes an open-addressed hash of the query's keys in LDS per position, and on
 * a hit adds 1 to an integer LDS counter tf[row][slot].  mq_lex_df counts per block and slot
 * the rows with tf > 0 and adds them with one integer global atomic each; it is synchronous
 * (df is a host array of n_terms counts).  mq_lex_topk scores the block's rows, one lane a
 * row, keeps a sorted running top-k per workgroup over a persistent grid and merges the
 * workgroups' lists with mq_topk_merge_device; out_scores [k] / out_ids [k] are both device
 * (io_on_device = 1, asynchronous on `stream`) or both host (synchronous).  n == 0 gives
 * padding only.  Launches run on the GPU the buffers live on.  The argument checks (sizes,
 * ngram, n_terms, distinct keys, k, NULL pointers with n > 0, alignment, scratch not an
 * output) come before any HIP call. */
#define MQ_LEX_MAX_TERMS 128
#define MQ_LEX_NORM(fmul, fadd, c0, c1, dl) fadd((c0), fmul((c1), (dl)))
#define MQ_LEX_TERM(fmul, fadd, fdiv, w, tf, norm) fdiv(fmul((w), (tf)), fadd((tf), (norm)))
int64_t mq_lex_scratch_bytes(int64_t n, int k);
int mq_lex_df(const uint16_t* tokens, int64_t n_tokens, const int64_t* offsets, int64_t n, int ngram,
              const uint32_t* keys, int n_terms, int64_t* df, void* scratch, void* stream);
int mq_lex_topk(const uint16_t* tokens, int64_t n_tokens, const int64_t* offsets, int64_t n, int ngram,
                const uint32_t* keys, const float* w, int n_terms, float c0, float c1,
                const uint32_t* bits, int k, float* out_scores, int64_t* out_ids, int io_on_device,
                void* scratch, void* stream);
/* The same for a batch: one walk of the token blob serves a group of queries, so nq queries
 * cost about nq / MQ_LEX_BATCH_GROUP scans instead of nq.  Nothing about the definition
 * changes: row j of mq_lex_topk_batch equals, bit for bit in scores and ids, what mq_lex_topk
 * returns for query j's arguments, whatever else the batch holds and wherever query j stands
 * in it, and mq_lex_df_batch's df[i] equals mq_lex_df's for keys[i].
 *   mq_lex_df_batch    keys: HOST, n_keys >= 1 distinct keys (any number: the call runs as many
 *                      passes as it needs and synchronises once at the end); df: HOST [n_keys].
 *                      n == 0: every df is 0.
 *   mq_lex_topk_batch  term_start: HOST int64 [nq + 1], non-decreasing from 0; query j's terms
 *                      are keys / w [term_start[j], term_start[j + 1]) (HOST arrays of
 *                      term_start[nq] entries), 0 .. MQ_LEX_MAX_TERMS of them, distinct within
 *                      the query (different queries may share keys); a query of 0 terms returns
 *                      padding only.  c0, c1, bits and k are shared by the batch.  The score of
 *                      a row is the MQ_LEX_NORM / MQ_LEX_TERM sequence over the query's terms
 *                      with tf > 0 in the query's own slot order.  out_scores / out_ids [nq, k],
 *                      both device (io_on_device = 1, asynchronous on `stream` once the packed
 *                      tables are copied) or both host (synchronous).  nq == 0 is a no-op,
 *                      n == 0 gives padding only.
 *   scratch            device, mq_lex_batch_scratch_bytes(n, nq, total_terms, k) bytes
 *                      (total_terms = term_start[nq], or n_keys with nq = 0 and k = 1 for the df
 *                      call), 16-byte aligned, not an output.  The size is non-decreasing in
 *                      every argument and bounded in nq and total_terms (the per-workgroup
 *                      lists are reused from group to group in stream order), so a buffer sized
 *                      for larger arguments serves smaller ones.  Neither call allocates or
 *                      frees device memory: the merged key tables, per-query slot lists and
 *                      weights are packed on the host and copied into scratch by the call.
 * lex_batch_kernel (K15): the host cuts the batch, in order, into groups of at most
 * MQ_LEX_BATCH_GROUP queries whose keys' union has at most MQ_LEX_BATCH_UNION entries; per group
 * one scan walks the blob as K14 does, counts into tf[row][union slot] (u32, LDS) through a hash
 * of the union that is at most half full, and wave w of a workgroup scores queries w, w + 4, ...
 * of the group from those counts, one register-resident sorted list a query; the workgroups'
 * lists [lists, group, k] go through mq_topk_merge_device into the group's output rows.  The df
 * pass is the same walk over MQ_LEX_BATCH_UNION keys a pass.  Every argument check (sizes, ngram,
 * n_keys, term_start, the per-query term count, distinct keys, k, NULL pointers, alignment,
 * scratch not an output) comes before any HIP call and names the offending value. */
#define MQ_LEX_BATCH_GROUP 16
#define MQ_LEX_BATCH_UNION 512
int64_t mq_lex_batch_scratch_bytes(int64_t n, int64_t nq, int64_t total_terms, int k);
int mq_lex_df_batch(const uint16_t* tokens, int64_t n_tokens, const int64_t* offsets, int64_t n, int ngram,
                    const uint32_t* keys, int64_t n_keys, int64_t* df, void* scratch, void* stream);
int mq_lex_topk_batch(const uint16_t* tokens, int64_t n_tokens, const int64_t* offsets, int64_t n, int ngram,
                      int64_t nq, const int64_t* term_start, const uint32_t* keys, const float* w, float c0,
                      float c1, const uint32_t* bits, int k, float* out_scores, int64_t* out_ids,
                      int io_on_device, void* scratch, void* stream);

/* Maximal marginal relevance (LangChain's maximal_marginal_relevance, the selection behind
 * VectorStore.max_marginal_relevance_search): from each query's candidate list pick k rows
 * greedily, trading similarity to the query against similarity to the rows already picked.
 * Candidates c_0 .. c_{m-1} in list order, s_i = cand_scores[i] (taken as given: the search's
 * exact fp32 dot, never recomputed), G[i][j] = the fp32 dot of stored rows cand_ids[i] and
 * cand_ids[j] (unit-norm already, not renormalised):
 *   pick 0    = argmax_i s_i
 *   pick t    = argmax over the unpicked i of MQ_MMR_SCORE(lambda, s_i, red_i),
 *               red_i = max over the picked p of G[i][p]
 * Ties go to the lowest list position i (LangChain compares with a strict >).  The score is
 * fixed fp32 arithmetic, each operation rounded to nearest, never contracted into an FMA:
 *   score = fsub(fmul(lambda, s), fmul(fsub(1.0f, lambda), red))
 * written once below as MQ_MMR_SCORE over the caller's rounding primitives (the kernel
 * passes __fmul_rn / __fsub_rn; a host restatement passes non-contracting float ops).
 * (mmr_select_kernel, K11: one workgroup per query; the fetch_k x fetch_k Gram matrix on
 * the exact-f32 MFMA from K-slices of the candidate rows staged through LDS, bitwise
 * symmetric; then one wave runs the greedy loop with lane i owning candidate i.)
 * cand_scores [nq, fetch_k] f32 and cand_ids [nq, fetch_k] int64 need not be sorted; an id
 * outside [0, size) is padding: its row is never read and it is never picked.
 * out_ids [nq, k] = the picked row ids in selection order, out_scores [nq, k] = their s_i;
 * with fewer than k valid candidates the rest is (-inf, -1).  All four buffers host
 * (io_on_device = 0, synchronous) or all device (asynchronous on `stream`).
 * 1 <= k <= fetch_k <= MQ_MAX_K, lambda finite in [0, 1], nq >= 0.  A query's result does
 * not depend on the rest of the batch. */
#define MQ_MMR_SCORE(fmul, fsub, lambda, s, red) \
  fsub(fmul((lambda), (s)), fmul(fsub(1.0f, (lambda)), (red)))
int mq_index_mmr_select(mq_index* ix, const float* cand_scores, const int64_t* cand_ids, int64_t nq,
                        int fetch_k, int k, float lambda, float* out_scores, int64_t* out_ids,
                        int io_on_device, void* stream);
/* Search, then select: the top min(fetch_k, size) of each query at the index's current
 * precision (bits == NULL: mq_index_search; a device mask: the masked search, as
 * mq_index_search_masked_batch) go into a workspace kept for the index's handle (grown on
 * demand, never allocated per call; kept under the handle's address for the life of the
 * process, so mq_index_destroy does not free it and a later handle at that address reuses
 * it), and mmr_select_kernel runs on them on the same stream: no host round trip beyond the
 * search's own.  queries [nq, dim], outputs [nq, k] as mq_index_mmr_select; an empty index
 * returns only padding.
 * Both MMR calls hold a mutex of the handle's workspace from start to end, so they serialise
 * with each other on one handle as the other mq_index_* calls do on the index's own mutex.
 * That mutex is not the index's: the selection reads the row slab (pointer and row count)
 * as it stood when the call began, so an mq_index_add / _select / _reset / _load on the same
 * handle must not run concurrently with an MMR call (an add that regrows the slab frees
 * the rows the kernel reads). */
int mq_index_search_mmr(mq_index* ix, const float* queries, int64_t nq, int k, int fetch_k,
                        float lambda, const uint32_t* bits, float* out_scores, int64_t* out_ids,
                        int io_on_device, void* stream);

/* Grouped search (K16; LangChain's ParentDocumentRetriever / MultiVectorRetriever: embed
 * small child chunks, return the distinct parents): the top-k GROUPS of a row-to-group map,
 * each by its best row, over the whole index - not the distinct groups among a top-k of rows.
 * Inputs: the index rows; a device int32 codes[n], the group code of each row; n_groups; an
 * optional device row mask `bits` in the layout of the masked search (NULL: every row); nq
 * queries; k.
 * Candidates: row r is a candidate of a query when the mask admits it and
 * 0 <= codes[r] < n_groups.  Code -1 means the metadata key is absent, and any other code out
 * of range is treated the same way: such rows are ignored, never read as a group and never
 * written anywhere (MultiVectorRetriever skips children without its id_key).
 * Scores: score(q, r) = the exact fp32 dot of the query with the stored, already normalised
 * row; the query is taken as given, as on mq_index_search's exact path.  A group's score is
 * the maximum over its candidate rows and its representative the row reaching it, equal
 * scores going to the lowest row id.  Groups rank by (score desc, representative row id asc).
 * Output: out_scores / out_ids [nq, k] = (score, representative row id) of the top-k groups,
 * padded with (-inf, -1) when fewer than k groups have a candidate; an empty index,
 * n_groups == 0 or an all-zero mask return padding only.  1 <= k <= MQ_MAX_K.
 * Equivalently: the distinct codes of the full ranking of the candidate rows, in order of
 * first appearance, with the row that introduced each - what LangChain's collapse of a
 * top-k yields when that k covers every row.
 *
 * group_scan_kernel walks the rows as the streaming exact scan does (16 lanes per row, at most
 * 16 queries per pass, mq_group_scan_blocks(n, CUs) workgroups of 16 lane groups, two rows in
 * flight per lane group) and raises best[query][code], a uint64 [<= 16][n_groups] table in the
 * scratch that the call zeroes on the stream first, by an atomic maximum of the key
 * (orderable score bits << 32) | (0xFFFFFFFF - row); group_select_kernel takes each query's
 * top-k keys in up to 64 workgroup lists that mq_topk_merge_device merges.  More than 16
 * queries run as successive passes that reuse the table in stream order.  The maximum does
 * not depend on the order the rows arrive in: repeated calls return the same bits.
 *
 * queries [nq, dim] and the outputs are all host (io_on_device = 0: staged through the scratch,
 * the call synchronises) or all device (asynchronous on `stream`); codes, bits and scratch are
 * device memory of the index's GPU.  Checked before any HIP call, each with a message naming
 * the offending value: k, nq, n_groups >= 0, dim % 64 == 0 and dim <= 1024, n < 2^31 (the
 * slab is fp32: no other index dtype exists), non-NULL buffers, scratch 16-byte aligned, at
 * least mq_group_scratch_bytes(n_groups, nq, k) bytes and overlapping neither output.  The
 * call allocates and frees no device memory, and always runs the full scan: it is the
 * definition (the store answers most queries from a certified top-64 first).
 * It reads the slab as it stood when the call began: an mq_index_add / _select / _reset /
 * _load on the same handle must not run concurrently with it.
 * mq_group_scratch_bytes is non-decreasing in every argument and bounded in nq (a multiple
 * of 256; arguments out of range are clamped).  mq_debug_group_check runs the HIP-free checks
 * alone on a stated index shape (dim, n_rows), for hosts without a GPU to make an index on. */
int64_t mq_group_scratch_bytes(int64_t n_groups, int64_t nq, int k);
int mq_group_scan_blocks(int64_t n_rows, int compute_units);
int mq_index_search_grouped(mq_index* ix, const float* queries, int64_t nq, int k, const int32_t* codes,
                            int32_t n_groups, const uint32_t* bits, float* out_scores, int64_t* out_ids,
                            int io_on_device, void* scratch, int64_t scratch_bytes, void* stream);
int mq_debug_group_check(int dim, int64_t n_rows, const float* queries, int64_t nq, int k, const int32_t* codes,
                         int32_t n_groups, const float* out_scores, const int64_t* out_ids, const void* scratch,
                         int64_t scratch_bytes);

/* Range search (K17; LangChain's "similarity_score_threshold" retriever, candidate lists
 * longer than MQ_MAX_K for a reranker, and "how many rows are this similar"): every row at or
 * above a score threshold, counted exactly, and the best max_hits of them.
 * Inputs: the index rows; an optional device row mask `bits` in the layout of the masked
 * search (NULL: every row); nq queries; min_score, a float (-inf: no threshold; NaN is
 * refused); max_hits in [1, MQ_RANGE_MAX_HITS].
 * Candidates: row r is a candidate of a query when the mask admits it.
 * Scores: score(q, r) = the exact fp32 dot of the query, taken as given, with the stored row,
 * as in the grouped search, + 0.0f (a -0.0 sum ranks as +0.0).  A hit is a candidate with
 * score >= min_score, compared in fp32.  Hits rank by (score desc, row asc).
 * Output: out_counts [nq] (int64) = the number of hits, exact, which may exceed max_hits;
 * out_scores / out_ids [nq, max_hits] = the first min(count, max_hits) hits of the ranking,
 * padded with (-inf, -1).  An empty index or an all-zero mask gives count 0 and padding only.
 * Repeated calls return the same bits.
 *
 * range_score_kernel walks the rows as group_scan_kernel does (16 lanes per row, at most 16
 * queries per pass, mq_range_scan_blocks(n, CUs) workgroups of 16 lane groups, two rows in
 * flight per lane group) and writes keys[query][row], a uint32 [<= 16][n] array in the
 * scratch: the score as an order-preserving unsigned for a hit (never 0 for a finite score),
 * 0 for any other row; every cell of a pass is written exactly once.  The selection works on
 * the unique 64-bit keys K = (keys[q][row] << 32) | (0xFFFFFFFF - row): a radix select over six
 * digits of at most 11 bits from the top (range_hist_kernel: per-workgroup LDS histograms
 * added into hist[query][bins]; range_pick_kernel: one workgroup per query fixes the digit in
 * which the key of rank max_hits falls; the first histogram's total is the count) finds the
 * cut K*, range_collect_kernel gathers the cells with K >= K* (one returning atomic add per
 * wave) and range_sort_kernel sorts them in LDS and writes the list.  A query is settled, and
 * its later histogram and pick launches return at once, when count <= max_hits or when the
 * bin chosen at some digit is wanted whole.  The histogram and collect kernels run
 * mq_range_select_blocks(n, CUs) workgroups per query, each over cells b * 256 + t,
 * + 256 * blocks, ...  The launches are enqueued unconditionally: the call runs a fixed number
 * of passes, reads nothing back in between, and has no overflow case to retry.  More than 16
 * queries run as successive passes that reuse the scratch in stream order.
 *
 * queries [nq, dim] and the three outputs are all host (io_on_device = 0: staged through the
 * scratch, the call synchronises) or all device (asynchronous on `stream`); bits and scratch
 * are device memory of the index's GPU.  Checked before any HIP call, each with a message
 * naming the offending value: max_hits, a NaN min_score, nq (these three before the handle is
 * looked at), dim % 64 == 0 and dim <= 1024, n < 2^31, non-NULL buffers, scratch 16-byte
 * aligned, at least mq_range_scratch_bytes(n, nq, max_hits) bytes and overlapping none of the
 * outputs.  The call allocates and frees no device memory.  It reads the slab as it stood when
 * the call began: an mq_index_add / _select / _reset / _load on the same handle must not run
 * concurrently with it.
 * mq_range_scratch_bytes is non-decreasing in every argument and bounded in nq (a multiple of
 * 256; arguments out of range are clamped): 4 bytes x min(nq, 16) x n for the keys, plus, per
 * query of a pass, an 8 KB histogram, 12 bytes per list entry (the candidates, which also
 * stage a host call's ids, and its staged scores) and 4 KB of query staging - under 1 MB in
 * all, about 65 MB at a million rows.  mq_debug_range_check runs the HIP-free checks alone on
 * a stated index shape (dim, n_rows), for hosts without a GPU to make an index on. */
int64_t mq_range_scratch_bytes(int64_t n_rows, int64_t nq, int max_hits);
int mq_range_scan_blocks(int64_t n_rows, int compute_units);
int mq_range_select_blocks(int64_t n_rows, int compute_units);
int mq_index_search_range(mq_index* ix, const float* queries, int64_t nq, int max_hits, float min_score,
                          const uint32_t* bits, int64_t* out_counts, float* out_scores, int64_t* out_ids,
                          int io_on_device, void* scratch, int64_t scratch_bytes, void* stream);
int mq_debug_range_check(int dim, int64_t n_rows, const float* queries, int64_t nq, int max_hits, float min_score,
                         const int64_t* out_counts, const float* out_scores, const int64_t* out_ids,
                         const void* scratch, int64_t scratch_bytes);

/* Self-join (K18; near-duplicate detection, LangChain's EmbeddingsRedundantFilter at index
 * scale): which stored rows are near-copies of other stored rows.
 * Inputs: the index rows; an optional device row mask `bits` in the layout of the masked search
 * (NULL: every row); an optional list of left rows, left_rows int64 [n_left], distinct and each
 * in [0, n) (NULL: rows 0 .. n - 1, and n_left must be n); min_score, a float (-inf is allowed;
 * NaN is refused).
 * Score: score(i, j) is exactly what mq_index_search_range returns for row j when the query is
 * stored row i: range_score_kernel's fp32 FMA chain and 16-lane butterfly, + 0.0f.  The chain's
 * order depends on the coordinate index alone, so score(i, j) and score(j, i) have the same bits.
 * Partner: j is a partner of left row i when the mask admits both i and j, j != i and
 * score(i, j) >= min_score in fp32.
 * Outputs, all [n_left]: out_counts (int64) the number of partners; out_first the smallest
 * partner row, or -1; out_nearest the partner that ranks first by (score desc, row asc), or -1;
 * out_nearest_scores that partner's score, or -inf.  A left row outside the mask gets
 * (0, -1, -1, -inf).  out_info is int64 [4]: [0] the sum of the counts, [1] left rows answered by
 * the screen, [2] screen candidates that were verified, [3] left rows answered by the exact
 * walk.  Repeated calls return the same bits.  An empty index or n_left = 0 succeeds and writes
 * nothing but out_info.
 *
 * mode: MQ_JOIN_EXACT walks the fp32 slab once per 16 left rows (join_exact_kernel: the range
 * search's row walk with the left rows staged in LDS by index; the lane that owns (row, left)
 * keeps a running count, first and best key, each workgroup stores one partial per left row and
 * join_finish_kernel folds them in a fixed order - no atomics).  MQ_JOIN_SCREEN (dim 256, 512 or
 * 768; refused otherwise) takes the left rows in panels of 256: join_tau_kernel gathers the
 * panel's rows from the bf16 shadow and sets tau = min_score - E, E a proven bound on
 * |score - bf16 score| from the shadow's rounding maxima (csrc/join.hip); the bf16 threshold
 * scan's appending pass lists every pair whose bf16 MFMA score clears tau; join_verify_kernel
 * recomputes the listed pairs with the exact chain.  A left row with more than 4096 listed
 * pairs goes to a redo list that the exact walk serves after the last panel, so the modes
 * return identical outputs (out_info aside).  MQ_JOIN_AUTO screens where the dim allows it and
 * the index holds at least 1024 rows, and walks otherwise.
 *
 * left_rows, the four outputs and out_info are all host (io_on_device = 0: staged through the
 * scratch) or all device; bits and scratch are device memory of the index's GPU.  Unlike the
 * range search the call always synchronises `stream` before it returns: the redo count is read
 * back.  Checked before any HIP call, each with a message naming the offending value: a NaN
 * min_score, mode, n_left (these before the handle is looked at), dim % 64 == 0 and dim <= 1024,
 * MQ_JOIN_SCREEN's dims, n < 2^31, n_left == n under a NULL left_rows, non-NULL buffers, scratch
 * 16-byte aligned, at least mq_join_scratch_bytes(n, n_left) bytes and overlapping none of the
 * other buffers.  Host left rows outside [0, n) are refused; a device left row outside [0, n)
 * is treated as a row outside the mask.  The call allocates no device memory of its own (the
 * screen brings the index's bf16 shadow up to date, as a bf16 search does) and reads the slab as
 * it stood when the call began.
 * mq_join_scratch_bytes is non-decreasing in both arguments (a multiple of 256; arguments out of
 * range are clamped): about 9 MB for a panel's survivor lists, plus 40 bytes per left row.
 * mq_debug_join_check runs the HIP-free checks alone on a stated index shape (dim, n_rows). */
#define MQ_JOIN_AUTO 0
#define MQ_JOIN_EXACT 1
#define MQ_JOIN_SCREEN 2
int64_t mq_join_scratch_bytes(int64_t n_rows, int64_t n_left);
int mq_index_self_join(mq_index* ix, float min_score, const uint32_t* bits, const int64_t* left_rows, int64_t n_left,
                       int mode, int64_t* out_counts, int64_t* out_first, int64_t* out_nearest,
                       float* out_nearest_scores, int64_t* out_info, int io_on_device, void* scratch,
                       int64_t scratch_bytes, void* stream);
int mq_debug_join_check(int dim, int64_t n_rows, float min_score, int mode, const int64_t* left_rows, int64_t n_left,
                        const int64_t* out_counts, const int64_t* out_first, const int64_t* out_nearest,
                        const float* out_nearest_scores, const int64_t* out_info, const void* scratch,
                        int64_t scratch_bytes);

/* K-means (K19; LangChain's EmbeddingsClusteringFilter at index scale: the themes of a corpus
 * and a representative of each): Lloyd iterations over the stored rows, on the device.
 * Inputs: the index rows; an optional device row mask `bits` in the layout of the masked search
 * (NULL: every row) - a row is admitted when the mask admits it; n_clusters in
 * [1, MQ_KMEANS_MAX_CLUSTERS] centroids, centroids float [n_clusters, dim], read and
 * overwritten; n_iter in [0, 1024].
 * Score: score(c, r) is the chain of csrc/score_chain.hpp exactly - chain_step over the 16-byte
 * pieces `it` ascending, then chain_reduce16 - with centroid c as the vector in LDS and stored
 * row r from the slab: the arithmetic of the range search and the self-join.  (The chain starts
 * from +0, so a score is never -0.0.)  half_j = 0.5f * score(c_j, c_j), computed by the same
 * chain once per set of centroids and kept in memory.  d_j(r) = (score(c_j, r) - half_j) + 0.0f,
 * a plain fp32 subtraction of two stored values.  For unit rows |r - c_j|^2 = |r|^2 - 2 d_j(r),
 * so the largest d is the Euclidean nearest centre: what sklearn's KMeans assigns to.
 * assign(C): an admitted row gets a[r] = argmax_j d_j(r), equal d to the lowest j - the order of
 * the keys chain_key(chain_score_word(d), j) - and out_dots[r] = score(c_a[r], r); any other row
 * gets a[r] = -1 and out_dots[r] = -inf.
 * update(a, C): counts[j] = #{r : a[r] = j}; a cluster with counts[j] > 0 gets, per coordinate,
 * c_j = S_j / (float)counts[j], S_j the fp32 sum of its members' coordinate and the division one
 * IEEE fp32 division (__fdiv_rn); an empty cluster keeps its centroid bit for bit.  The order of
 * the sum is fixed by (n, n_clusters, the labels): the rows are cut into chunks (at least 256
 * rows each, at most min(1024, 8192 / n_clusters) of them), a chunk's members of a cluster are
 * added in ascending row order and the chunks' sums in ascending chunk order.  No floating-point
 * atomics; repeated calls return the same bits.
 * The call: a_0 = assign(C_0); for t = 0 .. n_iter - 1: C_{t+1} = update(a_t, C_t), a_{t+1} =
 * assign(C_{t+1}).  It writes C_{n_iter} back into `centroids` and a_{n_iter}, its dots and its
 * counts to out_assign int32 [n], out_dots float [n], out_counts int64 [n_clusters]: labels,
 * counts and centroids are always consistent with each other, and n_iter = 0 is a pure predict.
 * Convergence: with changed_t = #{r : a_t[r] != a_{t-1}[r]} (a_{-1} = -1 everywhere), once some
 * changed_t = 0 every later step would reproduce the same bits, and the later launches return at
 * once on a device flag.  They are still enqueued: nothing is read back during the call and the
 * number of launches is a function of (n_clusters, n_iter) alone.
 * out_info int64 [4]: [0] updates applied before convergence, [1] `changed` at the last assign
 * that ran (0: converged), [2] admitted rows, [3] empty clusters at the end.
 * An empty index or an all-zero mask: every label -1, every count 0, the centroids untouched.
 * n_clusters may exceed the admitted rows; the surplus clusters stay empty.
 *
 * kmeans_half_kernel computes the halves, one 16-lane group per centroid.  kmeans_assign_kernel
 * is range_score_kernel's row walk (16 lanes per row, non-temporal 16-byte loads, two rows in
 * flight, mq_range_scan_blocks(n, CUs) workgroups) over the centroids in passes of 16; the lane
 * that owns (row, j) forms the key, a row's running best key lives in a uint64 [n] array of the
 * scratch between passes and the winner's score in out_dots, each written by the row's one lane
 * group; the last pass writes the label and counts `changed`, one integer atomic per wave.
 * kmeans_partial_kernel (grid: chunk x cluster) compacts a chunk's members in row order and adds
 * their rows, each thread owning four coordinates; kmeans_finish_kernel folds the chunks, divides
 * and writes the centroid.  Every hand-off is a kernel boundary on one stream.
 *
 * centroids and the four outputs are all host (io_on_device = 0: staged through the scratch, the
 * call synchronises) or all device (asynchronous on `stream`); bits and scratch are device
 * memory of the index's GPU.  Checked before any HIP call, each with a message naming the
 * offending value: n_clusters and n_iter (both before the handle is looked at), dim % 64 == 0 and
 * dim <= 1024, n < 2^31, non-NULL buffers, scratch 16-byte aligned, at least
 * mq_kmeans_scratch_bytes(n, n_clusters) bytes and overlapping no other buffer, host centroids
 * all finite.  Device centroids that are not finite give unspecified labels in [0, n_clusters)
 * and write nothing out of bounds.  The call allocates no device memory and reads the slab as it
 * stood when the call began.
 * mq_kmeans_scratch_bytes is non-decreasing in both arguments (a multiple of 256; arguments out
 * of range are clamped): 16 bytes per row (the best keys and a host call's staged labels and
 * dots), the update's partial sums (4 KB for each of at most min(n_clusters x min(1024,
 * ceil(n / 256)), 8192) cluster chunks: 32 MB at most) and 4 KB of staging per centroid.
 * mq_debug_kmeans_check runs the HIP-free checks alone on a stated index shape (dim, n_rows). */
#define MQ_KMEANS_MAX_CLUSTERS 256
int64_t mq_kmeans_scratch_bytes(int64_t n_rows, int n_clusters);
int mq_index_kmeans(mq_index* ix, const uint32_t* bits, int n_clusters, int n_iter, float* centroids,
                    int32_t* out_assign, float* out_dots, int64_t* out_counts, int64_t* out_info, int io_on_device,
                    void* scratch, int64_t scratch_bytes, void* stream);
int mq_debug_kmeans_check(int dim, int64_t n_rows, int n_clusters, int n_iter, const float* centroids,
                          const int32_t* out_assign, const float* out_dots, const int64_t* out_counts,
                          const int64_t* out_info, int io_on_device, const void* scratch, int64_t scratch_bytes);

/* Persistence: a flat binary slab (header + rows); written files are
 * fsync'ed before the call returns. */
int mq_index_save(mq_index* ix, const char* path);
int mq_index_load(mq_index* ix, const char* path);
/* Append-only persistence (the store's segments): save_rows writes rows
 * [row0, row0 + n) as a slab file of n rows; load_append appends a slab file's rows after
 * the index's own, bit-identical (no re-normalisation).  Replace the whole-slab rewrite
 * of Chroma's persist on every add (src/ingest_medical.py:106-110 and
 * src/medical_engine.py:52 share the persist directory). */
int mq_index_save_rows(mq_index* ix, const char* path, int64_t row0, int64_t n);
int mq_index_load_append(mq_index* ix, const char* path);

/* Host-side k-way merge of per-shard candidate lists (the step after the RCCL
 * all-gather).  scores/ids are [n_lists, nq, k_in] (list-major, as an
 * all-gather stacks them); output [nq, k_out] by (score desc, id asc); ids < 0 are
 * padding.  Pure CPU, no device needed.
 * Preconditions of both merges (the callers' to keep, not checked): the valid ids of a
 * query are distinct across its lists (the device merge places an entry by counting the
 * entries better than it); no score is NaN.  -0.0 ranks as +0.0: the two tie and the
 * lower id (compared as unsigned) goes first; -inf with a valid id ranks above padding. */
int mq_topk_merge_host(const float* scores, const int64_t* ids, int n_lists, int64_t nq,
                       int k_in, int k_out, float* out_scores, int64_t* out_ids);
/* Same merge on the device (inputs/outputs device pointers, async on stream).  Each
 * input list must be sorted (score desc, id asc, padding last), as mq_index_search
 * returns it: the kernel stops reading a list at its first non-qualifying entry. */
int mq_topk_merge_device(const float* scores, const int64_t* ids, int n_lists, int64_t nq,
                         int k_in, int k_out, float* out_scores, int64_t* out_ids, void* stream);

/* -------------------------------------------------------------- encoder ---- */
typedef struct mq_bert_config {
  int vocab_size;     /* 21128 */
  int hidden;         /* 768   */
  int layers;         /* 12    */
  int heads;          /* 12    */
  int ffn;            /* 3072  */
  int max_positions;  /* 1024  */
  int type_vocab;     /* 2     */
  float ln_eps;       /* 1e-12 */
  int gelu;           /* MQ_GELU_* */
  int pooling;        /* MQ_POOL_* */
} mq_bert_config;

int mq_encoder_create(int device, const mq_bert_config* cfg, mq_encoder** out);
int mq_encoder_destroy(mq_encoder* enc);
/* Number of f32 values the weight blob must hold (layout: DESIGN.md / weights.py). */
int64_t mq_encoder_weight_count(const mq_bert_config* cfg);
/* Upload the fp32 weight blob (host pointer, n_floats values). */
int mq_encoder_load_weights(mq_encoder* enc, const float* blob, int64_t n_floats);
/* Arithmetic of the GEMMs: MQ_DTYPE_F32 (exact fp32 MFMA, default) or MQ_DTYPE_F32X6. */
int mq_encoder_set_precision(mq_encoder* enc, int dtype);
/* Device-time accounting per kernel class (HIP events on the launch stream, off by
 * default).  read_timing returns ms since the last read for the stages
 * [0] embed+LN, [1] QKV GEMM, [2] attention, [3] out-proj GEMM, [4] LayerNorm,
 * [5] FFN-up GEMM, [6] FFN-down GEMM, [7] pool+normalise, and resets them. */
#define MQ_ENC_STAGES 8
/* Replay each forward shape as a captured hipGraph (default off; never while timing is
 * on).  Results are bit-identical either way.  On MI355X the host enqueues the ~110
 * launches of a forward faster than the device runs them, so eager launches measured
 * faster for one query (0.628 vs 0.645 ms: the graph path stages ids / mask / out through
 * its own captured buffers); graphs help a host-bound caller. */
int mq_encoder_set_graphs(mq_encoder* enc, int enabled);
/* Tuning options of the forward (explicit, per handle; results stay within the parity
 * tolerances whatever they are set to - each non-default value has a GPU test):
 *   MQ_ENC_OPT_ROWS_MAX          token rows (B x L) up to which the few-row forward runs
 *                                (0..256, default 64; 0 = always the tiled path)
 *   MQ_ENC_OPT_ROWS_SPLITS       few-row FFN-down K splits (0 = automatic, else 1..4 when
 *                                it divides ffn / 256 into an instantiated depth)
 *   MQ_ENC_OPT_SPLITK_MAX        deepest split-K of the tiled path's few-row GEMMs (2..64,
 *                                default 16)
 *   MQ_ENC_OPT_FUSE_ATTN_OPROJ   few-row forward: attention + output projection in one
 *                                launch (1, default) or two (0)
 *   MQ_ENC_OPT_SPLITK_TILES      tiled path, M <= 256 rows: a GEMM is split over K only when
 *                                its direct grid has at most this many 32 x 128 tiles
 *                                (0..4096, default 0 = one tile per CU)
 *   MQ_ENC_OPT_RESIDENT_LAYERS   few-row forward: layers [0, value) load their weights with
 *                                the default cache policy, later layers non-temporally, so
 *                                back-to-back single queries keep the first layers' weights
 *                                in MALL (0..1024, default 8: BERT-base single query
 *                                0.446 -> 0.427 ms encoder p50; 0 = all non-temporal is the
 *                                slowest, 0.463)
 *   MQ_ENC_OPT_X6_PRESPLIT       split-f32 precision, batched GEMMs: 1 (default) = K2p on the
 *                                weights' W3 plane images (split once, at weight load or
 *                                set_precision), 0 = the split-f32 tiles that split both
 *                                operands while staging them.  Bit-identical results.
 *   MQ_ENC_OPT_ROWS_PLANES       few-row forward: 0 (default) = FFN-down's two K splits and the
 *                                fused attention's two head groups add into ONE output plane
 *                                (two addends per element: bitwise the sum the consumer took), so
 *                                the next QKV / FFN-up reads one plane of rows; 1 = two planes.
 *   MQ_ENC_OPT_LN_FOLD           split-f32 precision, batched forward, hidden 768, every full-M
 *                                GEMM on the split-f32 tiles (ceil(M / 128) * (hidden / 192) >=
 *                                CUs): 1 = the LayerNorms folded into the GEMMs - out-proj /
 *                                FFN-down write the raw sums and per-row partials, FFN-up / the
 *                                next QKV multiply them by gamma-scaled weights and apply mean /
 *                                rstd in their epilogue (no LayerNorm launch on the full-M
 *                                layers); 0 = a LayerNorm launch each.  Shapes outside the gate
 *                                run as with 0, bit for bit.
 *   MQ_ENC_OPT_CLS_KFREE         CLS pooling, batched forward, L > 1, hidden <= 768: 1 (default) =
 *                                the last layer projects neither K nor V - the CLS query is
 *                                carried to the layer's input side (u = Wk_h^T q), one pass over
 *                                the input rows gives the softmax-weighted row sums z, and ctx =
 *                                Wv_h z + bv - and its closing LayerNorm, pooling and L2
 *                                normalisation run in the FFN-down reduction; 0 = the K / V
 *                                projection of every token and the attention kernel.  The same
 *                                sums re-associated: results agree to fp32 rounding.  Mean pooling
 *                                and L = 1 run as with 0, bit for bit.
 *   MQ_ENC_OPT_QKV_ATTN          split-f32 precision, x6_presplit 1, batched forward, L == 32, hidden
 *                                == 64 * heads and a multiple of 192, the QKV GEMM one that fills
 *                                the chip on the 128 x 192 split-f32 tile: 1 (default) = the QKV
 *                                launch of every full-M layer but a CLS-only last one ends in the
 *                                attention itself - one head per tile, Q | K | V kept in the
 *                                accumulators, ctx written straight from them; no qkv buffer
 *                                traffic and no attention launch on those layers; 0 = the QKV
 *                                launch and the attention launch.  Q, K, V are the same bits; the
 *                                softmax sums are associated differently: results agree to fp32
 *                                rounding.  With x6_presplit 0 the same attention follows the QKV
 *                                launch as a launch of its own: the same bits as x6_presplit 1.
 *                                Every other shape runs as with 0, bit for bit.
 *   MQ_ENC_OPT_EPI_SPLIT         split-f32 precision, x6_presplit 1, the GELU GEMMs (FFN-up, folded
 *                                or not) on the 128 x 192 / 256 x 96 loader-wave tiles: 1 (default)
 *                                = at each tile end a compute wave hands two of its four 16-row
 *                                blocks to the loader wave of its SIMD through the ring slot
 *                                that is free there, and both finish their rows at the same time;
 *                                0 = the compute wave finishes the whole wave tile.  The same
 *                                function on the same values: the same bits either way.
 * Setting an option drops the handle's captured graphs.
 * (Ids 3, 5 and 7: retired, never reuse.) */
#define MQ_ENC_OPT_ROWS_MAX 0
#define MQ_ENC_OPT_ROWS_SPLITS 1
#define MQ_ENC_OPT_SPLITK_MAX 2
#define MQ_ENC_OPT_FUSE_ATTN_OPROJ 4
#define MQ_ENC_OPT_SPLITK_TILES 6
#define MQ_ENC_OPT_RESIDENT_LAYERS 8
#define MQ_ENC_OPT_X6_PRESPLIT 9
#define MQ_ENC_OPT_ROWS_PLANES 10
#define MQ_ENC_OPT_LN_FOLD 11
#define MQ_ENC_OPT_CLS_KFREE 12
#define MQ_ENC_OPT_QKV_ATTN 13
#define MQ_ENC_OPT_EPI_SPLIT 14
int mq_encoder_set_option(mq_encoder* enc, int option, int value);
int mq_encoder_get_option(const mq_encoder* enc, int option, int* value);
int mq_encoder_set_timing(mq_encoder* enc, int enabled);
int mq_encoder_read_timing(mq_encoder* enc, float* ms, int n);
/* Forward: ids/mask [B, L] int32 -> out [B, hidden] f32, unit-norm (K1..K7).
 * All host (io_on_device = 0) or all device (io_on_device = 1).  L <= max_positions. */
int mq_encoder_embed(mq_encoder* enc, const int32_t* ids, const int32_t* mask, int B, int L,
                     float* out, int io_on_device, void* stream);

/* Cross-encoder scoring (reranking): a BERT cross-encoder is this encoder run on
 * [CLS] query [SEP] document [SEP] with segment ids, followed by BertPooler and a classifier
 * (transformers' BertForSequenceClassification; LangChain's CrossEncoderReranker re-orders the
 * documents of similarity_search(q, k), reference src/agents/nodes.py:93, whose first two the
 * Grade step reads, src/core/utils.py:64):
 *   pooled = tanh(Wp h_cls + bp),  logits = Wc pooled + bc
 * with h_cls the CLS row of the last LayerNorm, NOT L2-normalised.
 * mq_encoder_load_head uploads the head (host fp32: pooler_w [H][H], pooler_b [H], cls_w
 * [n_labels][H], cls_b [n_labels]; 1 <= n_labels <= MQ_HEAD_MAX_LABELS, checked before any HIP
 * call).  It is a separate upload: the blob of mq_encoder_load_weights and
 * mq_encoder_weight_count do not include it.  Loading again replaces the head; MQ_ESTATE
 * before mq_encoder_load_weights. */
#define MQ_HEAD_MAX_LABELS 8
int mq_encoder_load_head(mq_encoder* enc, const float* pooler_w, const float* pooler_b, const float* cls_w,
                         const float* cls_b, int n_labels);
/* ids / types / mask [B, L] int32 -> logits [B, n_labels] f32.  The forward is
 * mq_encoder_embed's (every path, precision and option of it) with two differences: the
 * embedding sum takes token-type row types[t], clamped to [0, type_vocab) on the device as the
 * ids are clamped to the vocabulary, and the tail leaves the CLS rows un-normalised in a
 * [B, hidden] buffer of the handle; then one launch of cls_head_kernel (K13: fp32 MFMA, fixed
 * summation order - repeated calls are bit-identical).  All buffers host (io_on_device = 0, the
 * call synchronises) or all device (asynchronous on `stream`, no allocation once the handle's
 * buffers have grown to the shape, no host synchronisation).  MQ_ESTATE without a head or when
 * pooling != MQ_POOL_CLS; B == 0 is a no-op; L <= max_positions.
 * Scoring always launches eagerly: captured graphs (mq_encoder_set_graphs) stay a feature of
 * mq_encoder_embed, and no embed graph is ever replayed for a score call. */
int mq_encoder_score(mq_encoder* enc, const int32_t* ids, const int32_t* types, const int32_t* mask, int B,
                     int L, float* logits, int io_on_device, void* stream);

/* ------------------------------------------------------------ tokenizer ---- */
/* Host-side BERT tokenisation (the step Ollama runs before the forward, reference
 * src/medical_engine.py:43).  WordPiece over a local vocab.txt, or the deterministic
 * char tokenizer (id = 106 + crc32(char) % (vocab - 106)).  Sequences are
 * [CLS] body [SEP], truncated to max_length, right-padded with 0. */
typedef struct mq_tokenizer mq_tokenizer;
int mq_tokenizer_create_wordpiece(const char* vocab_path, int lower_case, int max_length,
                                  mq_tokenizer** out);
/* The same WordPiece tokenizer over an in-memory vocabulary: tokens[i] is the NUL-terminated
 * UTF-8 token of id i (e.g. the vocab a GGUF model file embeds). */
int mq_tokenizer_create_wordpiece_tokens(const char* const* tokens, int n_tokens, int lower_case,
                                         int max_length, mq_tokenizer** out);
int mq_tokenizer_create_char(int vocab_size, int max_length, mq_tokenizer** out);
int mq_tokenizer_destroy(mq_tokenizer* tok);
/* Encode n NUL-terminated UTF-8 texts.  ids / mask must hold n * max(max_length, pad_to)
 * int32; they are written as [n, L] row-major with L = max(longest sequence, pad_to),
 * returned in *out_len. */
int mq_tokenizer_encode_batch(mq_tokenizer* tok, const char* const* texts, int n, int pad_to,
                              int32_t* ids, int32_t* mask, int* out_len);

/* Encode n (first, second) text pairs for a cross-encoder: [CLS] A [SEP] B [SEP], types 0
 * through the first [SEP] and 1 for B and its [SEP]; padding is id 0, type 0, mask 0.  Both the
 * WordPiece and the char tokenizer.  ids / types / mask hold n * max(max_length, pad_to) int32
 * and are written [n, L] row-major, L as mq_tokenizer_encode_batch.  Needs max_length >= 5.
 * A pair longer than max_length is truncated as HF's truncation=True (longest first) truncates
 * it: with T = max_length - 3, a = |A|, b = |B| - nothing when a + b <= T; else s = the shorter
 * (the first text when equal): 2 s <= T keeps it whole and cuts the longer to T - s, else the
 * shorter keeps T / 2 tokens and the longer T - T / 2.  An empty second text is an empty body
 * that still carries its type-1 [SEP]. */
int mq_tokenizer_encode_pairs(mq_tokenizer* tok, const char* const* first, const char* const* second, int n,
                              int pad_to, int32_t* ids, int32_t* types, int32_t* mask, int* out_len);

/* ------------------------------------------------------- testing hooks ---- */
/* One encoder GEMM on device buffers: out[M,N] = epi(A[M,K] W[N,K]^T + bias (+ resid)),
 * epi 0 bias, 1 bias+GELU(erf), 2 bias+GELU(tanh), 3 bias+residual; tile 0 = 128x128,
 * 1 = 128x96, 2 = 128x64, 3 = 32x128 (exact f32), 4 = split-K (32x128 tiles + ordered
 * slab reduction; synchronous, N % 4 == 0), 5-7 = split-f32 (x6) 128x128 / 128x96 /
 * 128x64, 8 / 9 = exact / split-f32 128x192 on 8-wave workgroups.  K % 32 == 0.  For
 * kernel unit tests. */
int mq_debug_gemm_f32(const float* A, const float* W, const float* bias, const float* resid,
                      float* out, int M, int N, int K, int epi, int tile, void* stream);
/* The W3 plane image of a weight W [N][K] (K % 16 == 0): three bf16 planes of
 * the exact split in 1 KB MFMA fragments.  mq_debug_w3_bytes gives its size (-1 for a bad
 * shape), mq_debug_split_w3 writes it (device buffers, asynchronous on `stream`). */
int64_t mq_debug_w3_bytes(int N, int K);
int mq_debug_split_w3(const float* W, int N, int K, void* w3, void* stream);
/* The encoder GEMM on the pre-split split-f32 kernel (K2p) with W given as its W3 image:
 * tile 0 = 128x192, 1 = 256x96 (4 compute + 4 loader waves), 2 = 128x192, 3 = 256x192
 * (8 compute waves), 7 = 64x192, -1 = the default pick; 4-6 = measurement variants
 * (gemm_x6p.hip);
 * codes >= 100: tile code % 100 with the tile walk cut into one region per XCD,
 * code / 100 - 1 column blocks (0 = the plain round-robin walk; below 100: the pick).
 * Bit-identical to the split-f32 tiles 5-7 / 9 of mq_debug_gemm_f32 (both on the 16x16x32
 * bf16 MFMA).  16 / 17 = tiles 0 / 7 on the former 32x32x16 k-step, kept for measurement:
 * the same products with 16 k summed per MFMA, fp32-class but not bit-identical.
 * 20 / 21 = tiles 0 / 1 with the former epilogue, kept for measurement: epi 1 / 2 (GELU) finish
 * the whole wave tile on its compute wave instead of sharing it with the loader wave
 * (MQ_ENC_OPT_EPI_SPLIT); bit-identical.  epi 0 / 3 have one form and run as tiles 0 / 1.
 * Asynchronous on `stream`.  K % 32 == 0. */
int mq_debug_gemm_x6p(const float* A, const void* W3, const float* bias, const float* resid,
                      float* out, int M, int N, int K, int epi, int tile, void* stream);
/* One K2p launch with a LayerNorm-fold epilogue (tile 0, 1 or -1 = the pick; 20 / 21 = tiles
 * 0 / 1 with the former epilogues - the producer's own residual loads on every tile, no
 * loader-wave hand-off; the GELU consumers' whole wave tile on its compute wave, no split
 * (MQ_ENC_OPT_EPI_SPLIT); epi 6 has one form - bit-identical, kept for measurement; no
 * fill-the-chip gate).
 * epi 5 = the producer: out = acc + bias + LN(resid) with the residual normalised from
 * stats_in [M][8] (mean, M2) pairs and g / b [N] (stats_in NULL: the residual as it is), and
 * the partials of out written to stats_out [M][8]; N = 768.  epi 6 / 7 / 8 = the consumers
 * (bias / GELU erf / GELU tanh): out = epi(rho_r (acc - mu_r s_fold[n]) + bias[n]), (mu, rho)
 * from stats_in and eps (the encoder's run at K = 768).  mq_debug_ln_fold_weight builds Wg = g W (whose W3 image the
 * consumer multiplies), s and c (the consumer's bias) from W [N][K], bias, g, b. */
int mq_debug_gemm_x6p_ln(const float* A, const void* W3, const float* bias, const float* resid,
                         float* out, int M, int N, int K, int epi, int tile, const float* stats_in,
                         float* stats_out, const float* g, const float* b, const float* s_fold,
                         float eps, void* stream);
int mq_debug_ln_fold_weight(const float* W, const float* bias, const float* g, const float* b, int N,
                            int K, float* Wg, float* s_out, float* c_out, void* stream);
/* One K2p QKV launch whose epilogue is the L = 32 attention (MQ_ENC_OPT_QKV_ATTN; the 128 x 192
 * tile): ctx [M][64 heads] = attention of qkv = A W^T + bias (epi 9) or rho_r (A W^T - mu_r
 * s_fold[n]) + bias[n] (epi 10, (mu, rho) from stats_in [M][8] and eps) over sequences of 32
 * rows, W3 the image of W [3 * 64 heads][K], mask [M] int32, Q scaled by `scale`.  No qkv is
 * written.  M % 32 == 0, K % 32 == 0.  max_workgroups 0 = one workgroup per CU, else a multiple
 * of 8: at most that many, each walking more tiles.  Asynchronous on `stream`. */
int mq_debug_gemm_x6p_attn(const float* A, const void* W3, const float* bias, const int* mask,
                           float* ctx, int M, int K, int heads, float scale, int epi,
                           const float* stats_in, const float* s_fold, float eps, int max_workgroups,
                           void* stream);
/* One attention launch (K3) on device buffers: ctx [B*L][H] = softmax(scale Q K^T over the
 * keys with mask != 0) V per (sequence, head); a query whose keys are all masked gives 0.
 * qkv is [B*L][3H] row-major, Q | K | V columns, head h at column h * 64 of each third
 * (H == heads * 64); mask is [B*L] int32.  variant -1 = the forward's own pick; 1 / 2 / 4 / 8 =
 * attention_kernel with that many key-split waves; 12 = one workgroup of 12 head waves
 * (heads == 12, L <= 32); 16 = attention_rows_kernel (L <= 64).  The product's kernels,
 * unchanged.  Asynchronous on `stream`. */
int mq_debug_attention(const float* qkv, const int* mask, int B, int L, int H, int heads, float scale,
                       int variant, float* ctx, void* stream);
/* The CLS query's attention without K and V (MQ_ENC_OPT_CLS_KFREE), steps u = Wk_h^T q, the pass
 * over the input rows and ctx = Wv_h z + bv, on device buffers: ctx [B][H] = row 0 of
 * softmax(scale q K^T over the keys with mask != 0) V per (sequence, head) with K = X Wk^T + bk
 * (bk shifts a head's scores alike and drops out), V = X Wv^T + bv; a sequence whose keys are all
 * masked gives 0.  q is [B][H] (the CLS rows' queries, bias included); x is [B*L][H]: the input
 * rows X themselves (stats NULL), or raw rows y with stats [B*L][8] (mean, M2) partials per 96
 * columns and X = LayerNorm(y; ln_g, ln_b, eps) (H = 768).  Wk, Wv are [H][H] row-major, bv [H],
 * mask [B*L] int32; H == heads * 64, H <= 768.  Allocates its scratch (Wk^T, u, z): synchronous. */
int mq_debug_cls_attention(const float* q, const float* x, const float* stats, const float* ln_g,
                           const float* ln_b, float eps, const int* mask, int B, int L, int H, int heads,
                           float scale, const float* Wk, const float* Wv, const float* bv, float* ctx,
                           void* stream);
/* The few-row forward's fused attention + output projection (K3o) on device buffers, launched
 * as forward_rows launches it: out = attention(qkv, mask) Wo^T + bo + resid, as heads / hg
 * planes [heads/hg][rows][H] (plane g holds head group g's share, plane 0 also bias +
 * residual); acc != 0: the two planes added into ONE plane, zeroed here first (heads / hg
 * == 2).  qkv [B*L][3H], Wo [H][H] and resid [B*L][H] are row-major; the hook builds Wo's
 * frag16 image and, for qf != 0, the frag16 image of qkv with V^T blocks (L % 16 == 0).
 * cls_only != 0: query 0 of each sequence only, rows = B compact output rows (else rows =
 * B * L).  hg 4 or 6, dividing heads; L <= 64.  Allocates its operand images: synchronous. */
int mq_debug_attn_oproj(const float* qkv, const int* mask, int B, int L, int H, int heads, float scale,
                        const float* Wo, const float* bo, const float* resid, int cls_only, int hg, int qf,
                        int acc, float* out, void* stream);
/* One few-row GEMM launch (K2r, rows_gemm_kernel: the product's kernel and launchers, unchanged)
 * on device buffers, with the arguments forward_rows passes for the launch `kind` names:
 *   MQ_ROWS_QKV    out = LN(a) W^T + bias.  a [M][K] = the sum of s_in (1..4) row-major planes
 *                  of A, a_plane floats apart, or (s_in 0) the embedding sum A[ids[r]] +
 *                  pos[r % L] + typ[types[r]] with A the word table [vocab][K], ids / types
 *                  clamped into range (types NULL: row 0).  variant 0: out [M][N] row-major;
 *                  variant 1: out in frag16 with the last third of the columns (V) as V^T blocks
 *                  (N % 48 == 0).  ln_out (may be NULL) [M][K] gets LN(a).
 *   MQ_ROWS_UP     out = GELU(LN(a) W^T + bias) in frag16; variant 0 erf, 1 tanh; s_in 1..4.
 *   MQ_ROWS_OPROJ  out [M][N] = A W^T + bias + resid, A row-major with row stride lda, resid with
 *                  row stride ldr (forward_rows passes L * H for both on the CLS-only layer).
 *   MQ_ROWS_DOWN   A [M][K] given in frag16 (K columns); variant 0: `splits` (1..4) planes
 *                  [M][N], o_plane floats apart, plane z = A[:, Kz] W[:, Kz]^T (+ bias + resid
 *                  for z = 0); variant 1: the two planes added into ONE plane, zeroed here first
 *                  (splits == 2).
 * frag16 of a [R][C] matrix: 16 x 16 blocks, column block fastest, 256 floats each; element (r, c)
 * of a block at float ((r + 16 (c >> 2)) * 4 + (c & 3)); a V^T block holds its transpose.  A
 * frag16 buffer spans whole 16-row blocks; rows >= M of the last block are neither read into
 * rows < M nor written.  W is [N][K] row-major: the hook builds its frag16 image.  The LN kinds
 * need K = hidden in 256 / 512 / 768 / 1024 and splits 1; every kind K % (256 splits) == 0 with a
 * per-split depth K / splits / 256 in {1, 2, 3, 4, 6, 8, 12, 16}; 1 <= M <= 256, N % 16 == 0.
 * nt_w 0 / 1: weights loaded with the default / the non-temporal policy.  zbuf (may be NULL):
 * zn floats (zn % 4 == 0) the launch zeroes beside its own work.  Arguments a kind does not
 * read are ignored.  Allocates W's image: synchronous. */
enum { MQ_ROWS_QKV = 0, MQ_ROWS_UP = 1, MQ_ROWS_OPROJ = 2, MQ_ROWS_DOWN = 3 };
int mq_debug_rows_gemm(int kind, int variant, const float* A, int lda, int64_t a_plane, int s_in, const float* W,
                       const float* bias, const float* resid, int ldr, float* out, int64_t o_plane, int M, int N,
                       int K, int splits, const float* ln_g, const float* ln_b, float eps, float* ln_out,
                       const int* ids, const int* types, int L, int vocab, const float* pos, const float* typ,
                       int type_vocab, int nt_w, float* zbuf, int64_t zn, void* stream);
/* One launch of the few-row forward's tail (ln_pool_kernel, unchanged): out [B][H] = the pooled,
 * L2-normalised (raw != 0: not normalised) rows of LN(sum of `planes` (1..4) planes of hs,
 * `plane` floats apart; ln_g, ln_b, eps).  hs holds `rows` rows per sequence: L ([B*L][H]), or 1
 * with CLS pooling (the compact [B][H] CLS rows of a CLS-only last layer).  MQ_POOL_CLS takes
 * row 0 of each sequence; MQ_POOL_MEAN the mean over the rows with mask [B*L] != 0 (none: 0).
 * H 256 / 512 / 768 / 1024.  Asynchronous on `stream`. */
int mq_debug_ln_pool(const float* hs, int planes, int64_t plane, const int* mask, int B, int L, int rows, int pooling,
                     const float* ln_g, const float* ln_b, float eps, int H, float* out, int raw, void* stream);

/* One launch of the cross-encoder head (K13, cls_head_kernel: the product's kernel, unchanged)
 * on device buffers: logits [B][n_labels] = cls_w tanh(pooler_w cls_b + pooler_b) + cls_b for
 * cls [B][H], H 256 / 512 / 768 / 1024, 1 <= n_labels <= MQ_HEAD_MAX_LABELS.  Asynchronous on
 * `stream`. */
int mq_debug_cls_head(const float* cls, int B, int H, const float* pooler_w, const float* pooler_b,
                      const float* cls_w, const float* cls_b, int n_labels, float* logits, void* stream);

/* The int8 screen (K9q) alone for one host query: its kc candidates (screen scores
 * desc, ids; slots past the survivors hold (tau, -1)) and the int8 shadow's statistics
 * stats[0] = max ||c - scale r8||, stats[1] = max ||scale r8||.  For kernel unit tests. */
int mq_debug_int8_screen(mq_index* ix, const float* query, int kc, float* out_scores, int64_t* out_ids,
                         float* stats);

/* The device merge (K10) with every choice the library makes for it in the caller's hands,
 * on device buffers, asynchronous on `stream`; it launches the product's kernels unchanged.
 * scores / ids are [n_lists, nq, k_in] as for mq_topk_merge_device, ids int32 (id_bits 32,
 * what the index's own scans hand over) or int64 (id_bits 64); out_scores / out_ids
 * [nq, k_out].  list_kc: 0 = no truncated-list check, else 1 <= list_kc <= k_in, the
 * entries a scan kept per list (overflow bit 0 is tested at position list_kc - 1).  kc: 0 =
 * the library's thread-list length for k_out, else 8, 16 or 64 (kc < k_out is exact only
 * where bit 1 stays clear).  form: 0 = the library's pick (thread lists iff k_out <= 16
 * and nq > 32), 1 = the thread-list kernel, 2 = the threshold kernel (which falls back to
 * thread lists past 4096 lists or 2048 survivors).  flag: NULL = no overflow checks, else
 * one int the call zeroes on the stream first; bit 0 = a truncated list may hide a member
 * of the top k_out, bit 1 = a thread list may have dropped one.  For kernel unit tests. */
int mq_debug_topk_merge(const float* scores, const void* ids, int id_bits, int n_lists, int64_t nq,
                        int k_in, int k_out, int list_kc, int kc, int form,
                        float* out_scores, int64_t* out_ids, int* flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MQ_H */
