// lexical.hip - BM25 lexical retrieval over the store's device token mirror (include/mq.h,
// "Lexical retrieval"): mq_lex_df counts the rows that hold each query term, mq_lex_topk scores
// every row and returns the top-k.  Both are one brute-force pass of lex_scan_kernel (K14) over
// the token blob; there is no inverted index and no state to maintain through deletes.
//
// A workgroup owns blocks of kRows = 64 consecutive rows (a persistent grid: block b, b + grid,
// ...).  The rows' tokens are one contiguous stretch of the blob, so no row is shared between
// workgroups and only df needs a cross-workgroup reduction.  The workgroup walks the stretch
// position-parallel: each lane loads 8 tokens (16 bytes; the chunks that would cross n_tokens
// token by token, nothing behind the blob is read), forms the term key of each position (a
// bigram pairs the token with the one before it, fetched from the blob at a lane's first
// position, and counts only if both tokens lie in one row) and probes an open-addressed hash
// of the query's keys in LDS, built on the host and passed by value: one 8-byte LDS read
// answers a miss.  On a hit the lane finds the row by a binary search of the block's row
// starts staged in LDS (kept from one hit to the lane's next) and adds 1 to the integer LDS
// counter tf[row][slot].  The stretch may be any length: the walk loops over it.
//   df pass     per block, thread t counts the rows with tf[.][t] > 0 and adds them to df[t] in
//               scratch with one integer global atomic (order-independent).
//   score pass  lane i of wave 0 computes row i's score from the integer counts by one fixed
//               fp32 instruction sequence (MQ_LEX_NORM / MQ_LEX_TERM, slot order), applies the
//               mask and the sum tf > 0 rule; the wave keeps a sorted running top-k in its
//               registers (lane j = entry j) and, when a row of the block beats its tail, ranks
//               the block's rows by counting and merges the two sorted lists by counting too.
//               The per-workgroup lists go through mq_topk_merge_device.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.hpp"

namespace {

using namespace mq;

constexpr int kRows = 64;                      // rows of a block: one lane of the scoring wave each
constexpr int kThreads = 256;
constexpr int kStep = kThreads * 8;            // tokens the workgroup covers per step of the walk
constexpr int kHash = 2 * MQ_LEX_MAX_TERMS;    // hash cells: at most half full, a probe always ends
constexpr int kFewTerms = 16;                  // queries of at most this many terms: the small-LDS build
constexpr int kMaxLists = 2048;                // workgroups of the score pass: 8 per CU (few terms), else 4
constexpr int kMaxDfGrid = 2048;
constexpr unsigned kEmpty = 0xffu;
static_assert(kHash == 256, "lex_hash returns 8 bits");
static_assert(kRows == kWave, "one lane of the scoring wave per row");

// the query by value: keys and weights in slot order, and the host-built hash (cell -> slot)
struct LexQuery {
  uint32_t key[MQ_LEX_MAX_TERMS];
  float w[MQ_LEX_MAX_TERMS];
  uint8_t cell[kHash];
};

__host__ __device__ __forceinline__ unsigned lex_hash(uint32_t key) { return (key * 0x9E3779B1u) >> 24; }

// 8 tokens at token offset p (a multiple of 8; tokens is 16-byte aligned); tokens at or past
// n_tokens read as 0 and are never loaded
__device__ __forceinline__ uint4 load8(const uint16_t* __restrict__ tokens, int64_t p, int64_t n_tokens) {
  if (p + 8 <= n_tokens) return *reinterpret_cast<const uint4*>(tokens + p);
  unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    unsigned v = 0;
    if (p + j < n_tokens) v = tokens[p + j];
    w[j >> 1] |= v << (16 * (j & 1));
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ float lane_f(float v, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}
__device__ __forceinline__ int64_t lane_i64(int64_t v, int j) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffll), j);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), j);
  return (int64_t)(((unsigned long long)hi << 32) | lo);
}

constexpr int kModeDf = 0, kModeScore = 1;

// TMAX: the most terms the build takes (n_terms <= TMAX).  tf is 64 x (TMAX + 1) words of LDS: 33 KB
// at 128 terms allow 4 workgroups a CU, 4 KB at 16 terms allow 8 (the walk waits on HBM
// latency once per block, so the workgroups in flight set its rate)
template <int MODE, int TMAX>
__global__ __launch_bounds__(kThreads) void lex_scan_kernel(const uint16_t* __restrict__ tokens, int64_t n_tokens,
                                                            const int64_t* __restrict__ offsets, int64_t n,
                                                            int ngram, LexQuery q, int n_terms, float c0, float c1,
                                                            const uint32_t* __restrict__ bits, int k,
                                                            unsigned long long* __restrict__ df,
                                                            float* __restrict__ list_s,
                                                            int64_t* __restrict__ list_id) {
  __shared__ uint2 s_hash[kHash];        // (key, slot); slot kEmpty = free cell
  __shared__ int64_t s_off[kRows + 1];   // the block's row starts (and its last row's end)
  __shared__ unsigned s_tf[kRows * (TMAX + 1)];
  __shared__ float s_w[TMAX];
  __shared__ float s_xs[kRows];          // the merge's scatter target
  __shared__ int64_t s_xi[kRows];

  const int tid = threadIdx.x;
  const int ts = n_terms | 1;  // odd row stride of tf: the scoring lanes (one row each) hit distinct banks
  {
    const unsigned sl = q.cell[tid];  // kHash == kThreads
    s_hash[tid] = sl == kEmpty ? make_uint2(0u, kEmpty) : make_uint2(q.key[sl], sl);
    if (tid < TMAX) s_w[tid] = tid < n_terms ? q.w[tid] : 0.f;
  }
  float top_s = -INFINITY;  // wave 0: lane j holds entry j of the running top-k (j >= k: padding)
  int64_t top_i = -1;

  const int64_t n_blocks = (n + kRows - 1) / kRows;
  // row start tid of a block (rows past n: the blob's end), loaded one block ahead of its use
  auto row_start = [&](int64_t blk) -> int64_t {
    const int64_t r = blk * kRows + tid;
    if (tid > kRows || blk >= n_blocks || r > n) return n_tokens;
    const int64_t o = offsets[r];
    return o < 0 ? 0 : o > n_tokens ? n_tokens : o;
  };
  int64_t ahead = row_start(blockIdx.x);
  for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const int64_t r0 = blk * kRows;
    const int nr = n - r0 < kRows ? (int)(n - r0) : kRows;
    __syncthreads();  // the previous block's readers of s_off / s_tf are done (and s_hash is written)
    if (tid <= nr) s_off[tid] = ahead;
    ahead = row_start(blk + gridDim.x);  // in flight during this block's walk
    for (int i = tid; i < nr * ts; i += kThreads) s_tf[i] = 0u;
    __syncthreads();

    const int64_t p0 = s_off[0], p1 = s_off[nr];
    int row = -1;
    for (int64_t base = p0 & ~(int64_t)7; base < p1; base += kStep) {
      const int64_t pos = base + (int64_t)tid * 8;
      if (pos >= p1) continue;
      const uint4 v = load8(tokens, pos, n_tokens);
      unsigned prev = 0;
      if (ngram == 2 && pos > 0) prev = tokens[pos - 1];  // pos - 1 < p1 <= n_tokens
      const unsigned wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned tok = (wv[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        const unsigned key = ngram == 2 ? (prev << 16) | tok : tok;
        prev = tok;
        const int64_t i = pos + j;
        if (i < p0 || i >= p1) continue;
        unsigned h = lex_hash(key);
        uint2 e = s_hash[h];
        while (e.y != kEmpty && e.x != key) {
          h = (h + 1) & (kHash - 1);
          e = s_hash[h];
        }
        if (e.y == kEmpty) continue;
        // the row of position i: the first r with s_off[r + 1] > i (zero-length rows are
        // skipped); positions grow within a lane, so the search starts at the last hit's row
        if (row < 0 || s_off[row + 1] <= i) {
          int lo = row < 0 ? 0 : row, hi = nr - 1;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid + 1] > i) hi = mid;
            else lo = mid + 1;
          }
          row = lo;
        }
        if (ngram == 2 && i <= s_off[row]) continue;  // the pair's first token is the row before's
        atomicAdd(&s_tf[row * ts + (int)e.y], 1u);
      }
    }
    __syncthreads();

    if (MODE == kModeDf) {
      if (tid < n_terms) {
        unsigned c = 0;
        for (int r = 0; r < nr; ++r) c += s_tf[r * ts + tid] != 0u ? 1u : 0u;
        if (c) atomicAdd(&df[tid], (unsigned long long)c);
      }
      continue;
    }
    if (tid >= kWave) continue;  // wave 0 scores and selects; the others go on to the next block's barrier

    const int lane = tid;
    float sc = -INFINITY;
    int64_t id = -1;
    if (lane < nr) {
      int64_t dl = s_off[lane + 1] - s_off[lane];
      if (ngram == 2) dl = dl > 0 ? dl - 1 : 0;
      const float norm = MQ_LEX_NORM(__fmul_rn, __fadd_rn, c0, c1, (float)dl);
      float s = 0.f;
      unsigned any = 0u;
      for (int t = 0; t < n_terms; ++t) {
        const unsigned tf = s_tf[lane * ts + t];
        if (tf) {
          any = 1u;
          s = __fadd_rn(s, MQ_LEX_TERM(__fmul_rn, __fadd_rn, __fdiv_rn, s_w[t], (float)tf, norm));
        }
      }
      const int64_t r = r0 + lane;
      if (any && (bits == nullptr || ((bits[r >> 5] >> (r & 31)) & 1u))) {
        sc = s;
        id = r;
      }
    }
    const float tail_s = lane_f(top_s, k - 1);
    const int64_t tail_i = lane_i64(top_i, k - 1);
    if (__ballot(id >= 0 && better(sc, id, tail_s, tail_i)) == 0ull) continue;  // wave-uniform
    // rank the block's rows (rows grow with the lane: a tie goes to the lower lane) and merge
    // them with the running list: an entry's place is its place in its own list plus the
    // entries of the other list that beat it.  (score, id) is a total order over distinct
    // rows, so the places are distinct; padding never beats anything and is not placed.
    int place_new = 0, place_old = lane;
    for (int j = 0; j < kWave; ++j) {
      const float sj = lane_f(sc, j), tj = lane_f(top_s, j);
      const int64_t ij = lane_i64(id, j), uj = lane_i64(top_i, j);
      if (ij >= 0) {
        place_new += better(sj, ij, sc, id) ? 1 : 0;
        place_old += better(sj, ij, top_s, top_i) ? 1 : 0;
      }
      if (uj >= 0) place_new += better(tj, uj, sc, id) ? 1 : 0;
    }
    s_xs[lane] = -INFINITY;
    s_xi[lane] = -1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (id >= 0 && place_new < k) {
      s_xs[place_new] = sc;
      s_xi[place_new] = id;
    }
    if (top_i >= 0 && place_old < k) {
      s_xs[place_old] = top_s;
      s_xi[place_old] = top_i;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    top_s = s_xs[lane];
    top_i = s_xi[lane];
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (MODE == kModeScore && tid < k) {
    list_s[(int64_t)blockIdx.x * k + tid] = top_s;
    list_id[(int64_t)blockIdx.x * k + tid] = top_i;
  }
}

__global__ void lex_pad_kernel(float* __restrict__ out_s, int64_t* __restrict__ out_i, int k) {
  const int t = threadIdx.x;
  if (t < k) {
    out_s[t] = -INFINITY;
    out_i[t] = -1;
  }
}

int pointer_device(const void* p) {
  hipPointerAttribute_t a;
  if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  return a.type == hipMemoryTypeDevice ? a.device : -1;
}

int64_t round16(int64_t x) { return (x + 15) & ~(int64_t)15; }

int score_lists(int64_t n) {
  const int64_t blocks = (n + kRows - 1) / kRows;
  return blocks < 1 ? 1 : blocks > kMaxLists ? kMaxLists : (int)blocks;
}

// scratch layout: df counters | the workgroups' score lists | their id lists | a k-entry result
// staging for host outputs (scores, then ids)
constexpr int64_t kDfBytes = MQ_LEX_MAX_TERMS * 8;
struct Scratch {
  unsigned long long* df;
  float* list_s;
  int64_t* list_id;
  float* out_s;
  int64_t* out_i;
  int64_t bytes;
};
Scratch carve(void* scratch, int64_t n, int k) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(scratch);  // NULL: only the size is wanted
  const int64_t lists = score_lists(n);
  Scratch s;
  int64_t at = 0;
  s.df = reinterpret_cast<unsigned long long*>(p + at);
  at += kDfBytes;
  s.list_s = reinterpret_cast<float*>(p + at);
  at += round16(lists * k * 4);
  s.list_id = reinterpret_cast<int64_t*>(p + at);
  at += round16(lists * k * 8);
  s.out_s = reinterpret_cast<float*>(p + at);
  at += round16((int64_t)k * 4);
  s.out_i = reinterpret_cast<int64_t*>(p + at);
  at += round16((int64_t)k * 8);
  s.bytes = at;
  return s;
}

// the shared argument checks; fills the by-value query (keys, weights, hash) on success
int check_and_pack(const uint16_t* tokens, int64_t n_tokens, const int64_t* offsets, int64_t n, int ngram,
                   const uint32_t* keys, const float* w, int n_terms, LexQuery* q) {
  MQ_CHECK_ARG(n >= 0 && n_tokens >= 0, "negative size (n %lld, n_tokens %lld)", (long long)n, (long long)n_tokens);
  MQ_CHECK_ARG(ngram == 1 || ngram == 2, "ngram must be 1 or 2 (got %d)", ngram);
  MQ_CHECK_ARG(n_terms >= 1 && n_terms <= MQ_LEX_MAX_TERMS, "n_terms must be in [1, %d] (got %d)",
               MQ_LEX_MAX_TERMS, n_terms);
  MQ_CHECK_ARG(keys, "NULL keys");
  memset(q->cell, (int)kEmpty, sizeof(q->cell));
  memset(q->key, 0, sizeof(q->key));
  memset(q->w, 0, sizeof(q->w));
  for (int t = 0; t < n_terms; ++t) {
    unsigned h = lex_hash(keys[t]);
    while (q->cell[h] != kEmpty) {
      MQ_CHECK_ARG(q->key[q->cell[h]] != keys[t], "keys must be distinct (key %u is repeated)", keys[t]);
      h = (h + 1) & (kHash - 1);
    }
    q->cell[h] = (uint8_t)t;
    q->key[t] = keys[t];
    if (w) q->w[t] = w[t];
  }
  if (n > 0) {
    MQ_CHECK_ARG(offsets && (tokens || n_tokens == 0), "NULL buffer");
    MQ_CHECK_ARG((reinterpret_cast<uintptr_t>(tokens) & 15) == 0, "tokens must be 16-byte aligned");
  }
  return MQ_OK;
}

}  // namespace

extern "C" int64_t mq_lex_scratch_bytes(int64_t n, int k) {
  if (n < 0) n = 0;
  if (k < 1) k = 1;
  if (k > MQ_MAX_K) k = MQ_MAX_K;
  return carve(nullptr, n, k).bytes;
}

extern "C" int mq_lex_df(const uint16_t* tokens, int64_t n_tokens, const int64_t* offsets, int64_t n, int ngram,
                         const uint32_t* keys, int n_terms, int64_t* df, void* scratch, void* stream) {
  clear_error();
  LexQuery q;
  const int rc = check_and_pack(tokens, n_tokens, offsets, n, ngram, keys, nullptr, n_terms, &q);
  if (rc != MQ_OK) return rc;
  MQ_CHECK_ARG(df, "NULL df");
  if (n == 0) {
    for (int t = 0; t < n_terms; ++t) df[t] = 0;
    return MQ_OK;
  }
  MQ_CHECK_ARG(scratch, "NULL buffer");
  MQ_CHECK_ARG((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "scratch must be 16-byte aligned");
  const int dev = pointer_device(scratch);
  MQ_CHECK_ARG(dev >= 0 && pointer_device(offsets) == dev && (n_tokens == 0 || pointer_device(tokens) == dev),
               "tokens, offsets and scratch must be device memory of one GPU");
  DeviceGuard dg(dev);
  hipStream_t s = (hipStream_t)stream;
  const Scratch sc = carve(scratch, n, 1);
  MQ_HIP(hipMemsetAsync(sc.df, 0, (size_t)n_terms * 8, s));
  const int64_t blocks = (n + kRows - 1) / kRows;
  const unsigned grid = (unsigned)(blocks > kMaxDfGrid ? kMaxDfGrid : blocks);
  if (n_terms <= kFewTerms)
    hipLaunchKernelGGL((lex_scan_kernel<kModeDf, kFewTerms>), dim3(grid), dim3(kThreads), 0, s, tokens, n_tokens,
                       offsets, n, ngram, q, n_terms, 0.f, 0.f, (const uint32_t*)nullptr, 1, sc.df, (float*)nullptr,
                       (int64_t*)nullptr);
  else
    hipLaunchKernelGGL((lex_scan_kernel<kModeDf, MQ_LEX_MAX_TERMS>), dim3(grid), dim3(kThreads), 0, s, tokens,
                       n_tokens, offsets, n, ngram, q, n_terms, 0.f, 0.f, (const uint32_t*)nullptr, 1, sc.df,
                       (float*)nullptr, (int64_t*)nullptr);
  MQ_HIP(hipGetLastError());
  MQ_HIP(hipMemcpyAsync(df, sc.df, (size_t)n_terms * 8, hipMemcpyDeviceToHost, s));
  MQ_HIP(hipStreamSynchronize(s));
  return MQ_OK;
}

extern "C" int mq_lex_topk(const uint16_t* tokens, int64_t n_tokens, const int64_t* offsets, int64_t n, int ngram,
                           const uint32_t* keys, const float* w, int n_terms, float c0, float c1,
                           const uint32_t* bits, int k, float* out_scores, int64_t* out_ids, int io_on_device,
                           void* scratch, void* stream) {
  clear_error();
  LexQuery q;
  const int rc = check_and_pack(tokens, n_tokens, offsets, n, ngram, keys, w, n_terms, &q);
  if (rc != MQ_OK) return rc;
  MQ_CHECK_ARG(w, "NULL w");
  MQ_CHECK_ARG(k >= 1 && k <= MQ_MAX_K, "k must be in [1, %d] (got %d)", MQ_MAX_K, k);
  MQ_CHECK_ARG(out_scores && out_ids, "NULL output");
  MQ_CHECK_ARG(io_on_device == 0 || io_on_device == 1, "io_on_device must be 0 or 1 (got %d)", io_on_device);
  MQ_CHECK_ARG(scratch == nullptr || (scratch != (void*)out_scores && scratch != (void*)out_ids),
               "scratch must not be an output");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    if (!io_on_device) {
      for (int j = 0; j < k; ++j) {
        out_scores[j] = -INFINITY;
        out_ids[j] = -1;
      }
      return MQ_OK;
    }
    const int dev = pointer_device(out_scores);
    MQ_CHECK_ARG(dev >= 0 && pointer_device(out_ids) == dev, "the outputs must be device memory of one GPU");
    DeviceGuard dg(dev);
    hipLaunchKernelGGL(lex_pad_kernel, dim3(1), dim3(kWave), 0, s, out_scores, out_ids, k);
    MQ_HIP(hipGetLastError());
    return MQ_OK;
  }
  MQ_CHECK_ARG(scratch, "NULL buffer");
  MQ_CHECK_ARG((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "scratch must be 16-byte aligned");
  const int dev = pointer_device(scratch);
  MQ_CHECK_ARG(dev >= 0 && pointer_device(offsets) == dev && (n_tokens == 0 || pointer_device(tokens) == dev) &&
                   (bits == nullptr || pointer_device(bits) == dev) &&
                   (!io_on_device || (pointer_device(out_scores) == dev && pointer_device(out_ids) == dev)),
               "tokens, offsets, bits, scratch and device outputs must be device memory of one GPU");
  DeviceGuard dg(dev);
  const Scratch sc = carve(scratch, n, k);
  int lists = score_lists(n);
  if (n_terms <= kFewTerms) {
    hipLaunchKernelGGL((lex_scan_kernel<kModeScore, kFewTerms>), dim3((unsigned)lists), dim3(kThreads), 0, s, tokens,
                       n_tokens, offsets, n, ngram, q, n_terms, c0, c1, bits, k, (unsigned long long*)nullptr,
                       sc.list_s, sc.list_id);
  } else {
    lists = lists > kMaxLists / 2 ? kMaxLists / 2 : lists;
    hipLaunchKernelGGL((lex_scan_kernel<kModeScore, MQ_LEX_MAX_TERMS>), dim3((unsigned)lists), dim3(kThreads), 0, s,
                       tokens, n_tokens, offsets, n, ngram, q, n_terms, c0, c1, bits, k, (unsigned long long*)nullptr,
                       sc.list_s, sc.list_id);
  }
  MQ_HIP(hipGetLastError());
  float* os = io_on_device ? out_scores : sc.out_s;
  int64_t* oi = io_on_device ? out_ids : sc.out_i;
  const int mrc = mq_topk_merge_device(sc.list_s, sc.list_id, lists, 1, k, k, os, oi, stream);
  if (mrc != MQ_OK) return mrc;
  if (!io_on_device) {
    MQ_HIP(hipMemcpyAsync(out_scores, os, (size_t)k * 4, hipMemcpyDeviceToHost, s));
    MQ_HIP(hipMemcpyAsync(out_ids, oi, (size_t)k * 8, hipMemcpyDeviceToHost, s));
    MQ_HIP(hipStreamSynchronize(s));
  }
  return MQ_OK;
}

// ------------------------------------------------------------------ batched scan (K15) ----
// mq_lex_topk_batch / mq_lex_df_batch: one walk of the token blob serves a GROUP of queries.
// The host cuts the batch, in order, into groups of at most kBG queries whose union of keys
// has at most kBU entries (and whose term counts sum to at most kBTerms) and packs one
// LexGroup record per group: the union's open-addressed hash (2 * kBU cells of (key, union
// slot), at most half full by construction, so a probe always ends), and per query its slot
// list (the union slot of each of its terms, in the query's own slot order) and weights.  The
// records are copied into scratch, kBSlots at a time, and lex_batch_kernel is launched once a
// group.  It walks exactly as K14 does (load8, the bigram rule, the row search) and counts
// into tf[row][union slot]; then wave w scores queries w, w + 4, ... of the group from those
// counts, 64 / ROWS queries at a time (lane = (query, row)), each by K14's fp32 sequence over
// the query's own terms in its own order, and keeps one register-resident sorted list per
// query (lane j = entry j) with K14's tail reject and counting merge.  ROWS is picked by the
// union's size so that tf stays 33 KB: 64 rows up to 128 keys, 32 up to 256, 16 up to 512.
// The per-workgroup lists [lists, n_q, k] are reused from group to group in stream order and
// merged by mq_topk_merge_device into the group's output rows.  The df pass is the same walk
// over up to kBU keys with no query structure.
namespace {

constexpr int kBG = MQ_LEX_BATCH_GROUP;   // queries of a group: 4 per wave
constexpr int kBU = MQ_LEX_BATCH_UNION;   // keys of a group's union
constexpr int kBHash = 2 * kBU;   // hash cells
constexpr int kBTerms = 1024;     // term slots of a group (sum of its queries' term counts)
constexpr int kBTfWords = 8192;   // tf holds ROWS x (kBTfWords / ROWS + 1) words
constexpr int kBLists = 768;      // workgroups of a scan: 3 per CU
constexpr int kBSlots = 64;       // group records held in scratch at a time
constexpr int kBQueriesPerWave = kBG / (kThreads / kWave);
constexpr unsigned kBEmpty = 0xffffffffu;
static_assert(kBHash == 1024, "lex_batch_hash returns 10 bits");
static_assert(kBQueriesPerWave * (kThreads / kWave) == kBG, "every wave owns the same number of queries");
static_assert(kBG * MQ_LEX_MAX_TERMS >= kBTerms && kBTerms >= MQ_LEX_MAX_TERMS && kBU >= MQ_LEX_MAX_TERMS,
              "one query always fits an empty group");

__host__ __device__ __forceinline__ unsigned lex_batch_hash(uint32_t key) { return (key * 0x9E3779B1u) >> 22; }

// one group as the kernel reads it (host-built, copied into scratch)
struct LexGroup {
  int n_q;                  // queries (0: a df pass)
  int n_union;              // distinct keys
  int qstart[kBG + 1];      // query g's terms are [qstart[g], qstart[g + 1]) of qslot / qw
  int pad[32 - 2 - (kBG + 1)];
  uint2 hash[kBHash];       // (key, union slot); slot kBEmpty = free cell
  float qw[kBTerms];
  uint16_t qslot[kBTerms];
};
static_assert(sizeof(LexGroup) % 16 == 0, "records stay 16-byte aligned in scratch");

__device__ __forceinline__ float shfl_f(float v, int src) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(v)));
}
__device__ __forceinline__ int64_t shfl_i64(int64_t v, int src) {
  const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute(src << 2, (int)(unsigned)(v & 0xffffffffll));
  const unsigned hi = (unsigned)__builtin_amdgcn_ds_bpermute(src << 2, (int)(unsigned)((unsigned long long)v >> 32));
  return (int64_t)(((unsigned long long)hi << 32) | lo);
}

// ROWS: rows of a block (64, 32 or 16); the union has at most kBTfWords / ROWS keys
template <int MODE, int ROWS>
__global__ __launch_bounds__(kThreads) void lex_batch_kernel(const uint16_t* __restrict__ tokens, int64_t n_tokens,
                                                             const int64_t* __restrict__ offsets, int64_t n,
                                                             int ngram, const LexGroup* __restrict__ grp, float c0,
                                                             float c1, const uint32_t* __restrict__ bits, int k,
                                                             unsigned long long* __restrict__ df,
                                                             float* __restrict__ list_s,
                                                             int64_t* __restrict__ list_id) {
  constexpr int UMAX = kBTfWords / ROWS;
  constexpr int SUBS = kWave / ROWS;  // queries a wave scores at once
  static_assert(UMAX <= kBU && kWave % ROWS == 0 && kBQueriesPerWave % SUBS == 0, "bad block shape");
  __shared__ uint2 s_hash[kBHash];
  __shared__ int64_t s_off[ROWS + 1];
  __shared__ unsigned s_tf[ROWS * (UMAX + 1)];
  __shared__ float s_qw[kBTerms];
  __shared__ uint16_t s_qslot[kBTerms];
  __shared__ int s_qstart[kBG + 1];
  __shared__ float s_xs[kThreads / kWave][kWave];  // each wave's merge scatter target
  __shared__ int64_t s_xi[kThreads / kWave][kWave];

  const int tid = threadIdx.x;
  int n_q = grp->n_q, n_union = grp->n_union;
  n_q = n_q < 0 ? 0 : n_q > kBG ? kBG : n_q;
  n_union = n_union < 0 ? 0 : n_union > UMAX ? UMAX : n_union;
  const int ts = n_union | 1;  // odd row stride of tf
  for (int i = tid; i < kBHash; i += kThreads) s_hash[i] = grp->hash[i];
  if (MODE == kModeScore) {
    int total = grp->qstart[n_q];
    total = total < 0 ? 0 : total > kBTerms ? kBTerms : total;
    for (int i = tid; i < total; i += kThreads) {
      s_qw[i] = grp->qw[i];
      const unsigned sl = grp->qslot[i];
      s_qslot[i] = (uint16_t)(sl < (unsigned)n_union ? sl : 0u);
    }
    if (tid <= kBG) {
      const int v = grp->qstart[tid <= n_q ? tid : n_q];
      s_qstart[tid] = v < 0 ? 0 : v > total ? total : v;
    }
  }
  // wave w: entry j of the running top-k of its m-th query (w + 4 m) in lane j
  float top_s[kBQueriesPerWave];
  int64_t top_i[kBQueriesPerWave];
#pragma unroll
  for (int m = 0; m < kBQueriesPerWave; ++m) {
    top_s[m] = -INFINITY;
    top_i[m] = -1;
  }

  const int64_t n_blocks = (n + ROWS - 1) / ROWS;
  auto row_start = [&](int64_t blk) -> int64_t {
    const int64_t r = blk * ROWS + tid;
    if (tid > ROWS || blk >= n_blocks || r > n) return n_tokens;
    const int64_t o = offsets[r];
    return o < 0 ? 0 : o > n_tokens ? n_tokens : o;
  };
  int64_t ahead = row_start(blockIdx.x);
  for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const int64_t r0 = blk * ROWS;
    const int nr = n - r0 < ROWS ? (int)(n - r0) : ROWS;
    __syncthreads();  // the previous block's readers of s_off / s_tf are done (and the tables are written)
    if (tid <= nr) s_off[tid] = ahead;
    ahead = row_start(blk + gridDim.x);
    for (int i = tid; i < nr * ts; i += kThreads) s_tf[i] = 0u;
    __syncthreads();

    const int64_t p0 = s_off[0], p1 = s_off[nr];
    int row = -1;
    for (int64_t base = p0 & ~(int64_t)7; base < p1; base += kStep) {
      const int64_t pos = base + (int64_t)tid * 8;
      if (pos >= p1) continue;
      const uint4 v = load8(tokens, pos, n_tokens);
      unsigned prev = 0;
      if (ngram == 2 && pos > 0) prev = tokens[pos - 1];  // pos - 1 < p1 <= n_tokens
      const unsigned wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned tok = (wv[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        const unsigned key = ngram == 2 ? (prev << 16) | tok : tok;
        prev = tok;
        const int64_t i = pos + j;
        if (i < p0 || i >= p1) continue;
        unsigned h = lex_batch_hash(key);
        uint2 e = s_hash[h];
        // ends: the host fills at most kBU of the kBHash cells, so a free cell is always met
        while (e.y != kBEmpty && e.x != key) {
          h = (h + 1) & (kBHash - 1);
          e = s_hash[h];
        }
        if (e.y >= (unsigned)n_union) continue;  // a free cell (or a slot the record may not hold)
        if (row < 0 || s_off[row + 1] <= i) {
          int lo = row < 0 ? 0 : row, hi = nr - 1;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid + 1] > i) hi = mid;
            else lo = mid + 1;
          }
          row = lo;
        }
        if (ngram == 2 && i <= s_off[row]) continue;  // the pair's first token is the row before's
        atomicAdd(&s_tf[row * ts + (int)e.y], 1u);
      }
    }
    __syncthreads();

    if (MODE == kModeDf) {
      for (int t = tid; t < n_union; t += kThreads) {
        unsigned c = 0;
        for (int r = 0; r < nr; ++r) c += s_tf[r * ts + t] != 0u ? 1u : 0u;
        if (c) atomicAdd(&df[t], (unsigned long long)c);
      }
      continue;
    }

    const int wave = tid >> 6, lane = tid & (kWave - 1);
    const int sub = lane / ROWS, rw = lane % ROWS;
#pragma unroll
    for (int p = 0; p < kBQueriesPerWave / SUBS; ++p) {
      if (wave + 4 * (p * SUBS) >= n_q) break;  // wave-uniform: no query of this pass exists
      // lane (sub, rw) scores row rw for the wave's query number p * SUBS + sub
      const int g = wave + 4 * (p * SUBS + sub);
      float sc = -INFINITY;
      int64_t id = -1;
      if (g < n_q && rw < nr) {
        int64_t dl = s_off[rw + 1] - s_off[rw];
        if (ngram == 2) dl = dl > 0 ? dl - 1 : 0;
        const float norm = MQ_LEX_NORM(__fmul_rn, __fadd_rn, c0, c1, (float)dl);
        float s = 0.f;
        unsigned any = 0u;
        const int t1 = s_qstart[g + 1];
        // the query's own slot order, four terms' LDS reads in flight at a time (slot -> count is
        // a dependent pair); a term with tf = 0 is computed and dropped, never added
        for (int t = s_qstart[g]; t < t1; t += 4) {
          unsigned tf[4];
          float wt[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int tu = t + u < t1 ? t + u : t1 - 1;
            const unsigned c = s_tf[rw * ts + (int)s_qslot[tu]];
            tf[u] = t + u < t1 ? c : 0u;
            wt[u] = s_qw[tu];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float term = MQ_LEX_TERM(__fmul_rn, __fadd_rn, __fdiv_rn, wt[u], (float)tf[u], norm);
            const float sum = __fadd_rn(s, term);
            s = tf[u] ? sum : s;
            any |= tf[u];
          }
        }
        const int64_t r = r0 + rw;
        if (any && (bits == nullptr || ((bits[r >> 5] >> (r & 31)) & 1u))) {
          sc = s;
          id = r;
        }
      }
#pragma unroll
      for (int u = 0; u < SUBS; ++u) {
        const int m = p * SUBS + u;
        if (wave + 4 * m >= n_q) break;  // wave-uniform
        const float tail_s = lane_f(top_s[m], k - 1);
        const int64_t tail_i = lane_i64(top_i[m], k - 1);
        if (__ballot(sub == u && id >= 0 && better(sc, id, tail_s, tail_i)) == 0ull) continue;  // wave-uniform
        // this query's candidates into lanes 0 .. ROWS - 1 (the rest: padding), then K14's
        // counting merge of the two sorted-by-construction rankings
        float cs = sc;
        int64_t ci = id;
        if (SUBS > 1) {
          const float xs = shfl_f(sc, u * ROWS + rw);
          const int64_t xi = shfl_i64(id, u * ROWS + rw);
          cs = lane < ROWS ? xs : -INFINITY;
          ci = lane < ROWS ? xi : -1;
        }
        const float os = top_s[m];
        const int64_t oi = top_i[m];
        int place_new = 0, place_old = lane;
        for (int j = 0; j < ROWS; ++j) {
          const float sj = lane_f(cs, j);
          const int64_t ij = lane_i64(ci, j);
          if (ij >= 0) {
            place_new += better(sj, ij, cs, ci) ? 1 : 0;
            place_old += better(sj, ij, os, oi) ? 1 : 0;
          }
        }
        for (int j = 0; j < k; ++j) {
          const float tj = lane_f(os, j);
          const int64_t uj = lane_i64(oi, j);
          if (uj < 0) break;  // the list is sorted, padding last
          place_new += better(tj, uj, cs, ci) ? 1 : 0;
        }
        s_xs[wave][lane] = -INFINITY;
        s_xi[wave][lane] = -1;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (ci >= 0 && place_new < k) {
          s_xs[wave][place_new] = cs;
          s_xi[wave][place_new] = ci;
        }
        if (oi >= 0 && place_old < k) {
          s_xs[wave][place_old] = os;
          s_xi[wave][place_old] = oi;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        top_s[m] = s_xs[wave][lane];
        top_i[m] = s_xi[wave][lane];
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the next merge of this wave clears the target
      }
    }
  }
  if (MODE == kModeScore) {
    const int wave = tid >> 6, lane = tid & (kWave - 1);
#pragma unroll
    for (int m = 0; m < kBQueriesPerWave; ++m) {
      const int g = wave + 4 * m;
      if (g < n_q && lane < k) {
        list_s[((int64_t)blockIdx.x * n_q + g) * k + lane] = top_s[m];
        list_id[((int64_t)blockIdx.x * n_q + g) * k + lane] = top_i[m];
      }
    }
  }
}

__global__ void lex_pad_rows_kernel(float* __restrict__ out_s, int64_t* __restrict__ out_i, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) {
    out_s[i] = -INFINITY;
    out_i[i] = -1;
  }
}

// rows per block of a group's scan: the most that keep tf within kBTfWords for its union.
// MQ_LEX_BATCH_MAX_ROWS (a build-time knob of the A/B in DESIGN.md, K15) caps it.
#ifndef MQ_LEX_BATCH_MAX_ROWS
#define MQ_LEX_BATCH_MAX_ROWS 64
#endif
int batch_rows(int n_union) {
  const int rows = n_union <= kBTfWords / 64 ? 64 : n_union <= kBTfWords / 32 ? 32 : 16;
  return rows < MQ_LEX_BATCH_MAX_ROWS ? rows : MQ_LEX_BATCH_MAX_ROWS;
}

int batch_lists(int64_t n, int rows) {
  const int64_t blocks = (n + rows - 1) / rows;
  return blocks < 1 ? 1 : blocks > kBLists ? kBLists : (int)blocks;
}

// scratch layout: group records | df counters, kBU a record | the workgroups' score lists |
// their id lists | result staging for host outputs (scores, then ids), one chunk of groups
struct BatchScratch {
  LexGroup* groups;
  unsigned long long* df;
  float* list_s;
  int64_t* list_id;
  float* out_s;
  int64_t* out_i;
  int slots;
  int64_t bytes;
};
BatchScratch carve_batch(void* scratch, int64_t n, int64_t nq, int64_t total_terms, int k) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(scratch);  // NULL: only the size is wanted
  if (nq < 0) nq = 0;
  if (total_terms < 0) total_terms = 0;
  int64_t slots = (total_terms + kBU - 1) / kBU;
  slots = slots < nq ? nq : slots;
  slots = slots < 1 ? 1 : slots > kBSlots ? kBSlots : slots;
  const int64_t lists = batch_lists(n, 16);  // the 16-row build has the most blocks
  const int64_t stage = nq < slots * kBG ? nq : slots * kBG;
  BatchScratch s;
  int64_t at = 0;
  s.slots = (int)slots;
  s.groups = reinterpret_cast<LexGroup*>(p + at);
  at += slots * (int64_t)sizeof(LexGroup);
  s.df = reinterpret_cast<unsigned long long*>(p + at);
  at += slots * kBU * 8;
  s.list_s = reinterpret_cast<float*>(p + at);
  at += round16(lists * kBG * k * 4);
  s.list_id = reinterpret_cast<int64_t*>(p + at);
  at += round16(lists * kBG * k * 8);
  s.out_s = reinterpret_cast<float*>(p + at);
  at += round16(stage * k * 4);
  s.out_i = reinterpret_cast<int64_t*>(p + at);
  at += round16(stage * k * 8);
  s.bytes = at;
  return s;
}

void group_clear(LexGroup* g) {
  memset(g, 0, sizeof(*g));
  for (int i = 0; i < kBHash; ++i) g->hash[i] = make_uint2(0u, kBEmpty);
}

// the union slot of key in g's hash, or -1
int group_find(const LexGroup* g, uint32_t key) {
  unsigned h = lex_batch_hash(key);
  while (g->hash[h].y != kBEmpty) {
    if (g->hash[h].x == key) return (int)g->hash[h].y;
    h = (h + 1) & (kBHash - 1);
  }
  return -1;
}

// adds key (not yet in the hash; n_union < kBU keeps it at most half full) -> its slot
int group_insert(LexGroup* g, uint32_t key) {
  unsigned h = lex_batch_hash(key);
  while (g->hash[h].y != kBEmpty) h = (h + 1) & (kBHash - 1);
  g->hash[h] = make_uint2(key, (unsigned)g->n_union);
  return g->n_union++;
}

template <int MODE>
void launch_batch(int rows, unsigned grid, hipStream_t s, const uint16_t* tokens, int64_t n_tokens,
                  const int64_t* offsets, int64_t n, int ngram, const LexGroup* grp, float c0, float c1,
                  const uint32_t* bits, int k, unsigned long long* df, float* list_s, int64_t* list_id) {
  if (rows == 64)
    hipLaunchKernelGGL((lex_batch_kernel<MODE, 64>), dim3(grid), dim3(kThreads), 0, s, tokens, n_tokens, offsets, n,
                       ngram, grp, c0, c1, bits, k, df, list_s, list_id);
  else if (rows == 32)
    hipLaunchKernelGGL((lex_batch_kernel<MODE, 32>), dim3(grid), dim3(kThreads), 0, s, tokens, n_tokens, offsets, n,
                       ngram, grp, c0, c1, bits, k, df, list_s, list_id);
  else
    hipLaunchKernelGGL((lex_batch_kernel<MODE, 16>), dim3(grid), dim3(kThreads), 0, s, tokens, n_tokens, offsets, n,
                       ngram, grp, c0, c1, bits, k, df, list_s, list_id);
}

int check_batch_common(const uint16_t* tokens, int64_t n_tokens, const int64_t* offsets, int64_t n, int ngram) {
  MQ_CHECK_ARG(n >= 0 && n_tokens >= 0, "negative size (n %lld, n_tokens %lld)", (long long)n, (long long)n_tokens);
  MQ_CHECK_ARG(ngram == 1 || ngram == 2, "ngram must be 1 or 2 (got %d)", ngram);
  if (n > 0) {
    MQ_CHECK_ARG(offsets && (tokens || n_tokens == 0), "NULL buffer");
    MQ_CHECK_ARG((reinterpret_cast<uintptr_t>(tokens) & 15) == 0, "tokens must be 16-byte aligned");
  }
  return MQ_OK;
}

}  // namespace

extern "C" int64_t mq_lex_batch_scratch_bytes(int64_t n, int64_t nq, int64_t total_terms, int k) {
  if (n < 0) n = 0;
  if (k < 1) k = 1;
  if (k > MQ_MAX_K) k = MQ_MAX_K;
  return carve_batch(nullptr, n, nq, total_terms, k).bytes;
}

extern "C" int mq_lex_df_batch(const uint16_t* tokens, int64_t n_tokens, const int64_t* offsets, int64_t n,
                               int ngram, const uint32_t* keys, int64_t n_keys, int64_t* df, void* scratch,
                               void* stream) {
  clear_error();
  const int rc = check_batch_common(tokens, n_tokens, offsets, n, ngram);
  if (rc != MQ_OK) return rc;
  MQ_CHECK_ARG(n_keys >= 1, "n_keys must be at least 1 (got %lld)", (long long)n_keys);
  MQ_CHECK_ARG(keys, "NULL keys");
  MQ_CHECK_ARG(df, "NULL df");
  {
    std::vector<uint32_t> sorted(keys, keys + n_keys);
    std::sort(sorted.begin(), sorted.end());
    const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
    MQ_CHECK_ARG(dup == sorted.end(), "keys must be distinct (key %u is repeated)", dup == sorted.end() ? 0u : *dup);
  }
  if (n == 0) {
    for (int64_t t = 0; t < n_keys; ++t) df[t] = 0;
    return MQ_OK;
  }
  MQ_CHECK_ARG(scratch, "NULL buffer");
  MQ_CHECK_ARG((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "scratch must be 16-byte aligned");
  // pack every pass before the first HIP call: kBU keys a record
  const int64_t passes = (n_keys + kBU - 1) / kBU;
  std::vector<LexGroup> host((size_t)passes);
  for (int64_t p = 0; p < passes; ++p) {
    LexGroup* g = &host[(size_t)p];
    group_clear(g);
    const int64_t t1 = (p + 1) * kBU < n_keys ? (p + 1) * kBU : n_keys;
    for (int64_t t = p * kBU; t < t1; ++t) group_insert(g, keys[t]);
    MQ_CHECK_ARG(g->n_union >= 1 && g->n_union <= kBHash / 2, "internal: a df pass of %d keys", g->n_union);
  }
  const int dev = pointer_device(scratch);
  MQ_CHECK_ARG(dev >= 0 && pointer_device(offsets) == dev && (n_tokens == 0 || pointer_device(tokens) == dev),
               "tokens, offsets and scratch must be device memory of one GPU");
  DeviceGuard dg(dev);
  hipStream_t s = (hipStream_t)stream;
  const BatchScratch sc = carve_batch(scratch, n, 0, n_keys, 1);
  // a chunk of sc.slots passes at a time; the records and counters of a chunk are reused by
  // the next in stream order, and `host` lives until the one synchronise at the end
  for (int64_t p0 = 0; p0 < passes; p0 += sc.slots) {
    const int64_t p1 = p0 + sc.slots < passes ? p0 + sc.slots : passes;
    const int64_t k0 = p0 * kBU, k1 = p1 * kBU < n_keys ? p1 * kBU : n_keys;
    MQ_HIP(hipMemsetAsync(sc.df, 0, (size_t)(k1 - k0) * 8, s));
    MQ_HIP(hipMemcpyAsync(sc.groups, &host[(size_t)p0], (size_t)(p1 - p0) * sizeof(LexGroup), hipMemcpyHostToDevice, s));
    for (int64_t p = p0; p < p1; ++p) {
      const int rows = batch_rows(host[(size_t)p].n_union);
      launch_batch<kModeDf>(rows, (unsigned)batch_lists(n, rows), s, tokens, n_tokens, offsets, n, ngram,
                            sc.groups + (p - p0), 0.f, 0.f, nullptr, 1, sc.df + (p - p0) * kBU, nullptr, nullptr);
      MQ_HIP(hipGetLastError());
    }
    MQ_HIP(hipMemcpyAsync(df + k0, sc.df, (size_t)(k1 - k0) * 8, hipMemcpyDeviceToHost, s));
  }
  MQ_HIP(hipStreamSynchronize(s));
  return MQ_OK;
}

extern "C" int mq_lex_topk_batch(const uint16_t* tokens, int64_t n_tokens, const int64_t* offsets, int64_t n,
                                 int ngram, int64_t nq, const int64_t* term_start, const uint32_t* keys,
                                 const float* w, float c0, float c1, const uint32_t* bits, int k, float* out_scores,
                                 int64_t* out_ids, int io_on_device, void* scratch, void* stream) {
  clear_error();
  const int rc = check_batch_common(tokens, n_tokens, offsets, n, ngram);
  if (rc != MQ_OK) return rc;
  MQ_CHECK_ARG(nq >= 0, "nq must not be negative (got %lld)", (long long)nq);
  MQ_CHECK_ARG(k >= 1 && k <= MQ_MAX_K, "k must be in [1, %d] (got %d)", MQ_MAX_K, k);
  MQ_CHECK_ARG(io_on_device == 0 || io_on_device == 1, "io_on_device must be 0 or 1 (got %d)", io_on_device);
  if (nq == 0) return MQ_OK;
  MQ_CHECK_ARG(term_start, "NULL term_start");
  MQ_CHECK_ARG(term_start[0] == 0, "term_start must start at 0 (got %lld)", (long long)term_start[0]);
  for (int64_t j = 0; j < nq; ++j) {
    const int64_t nt = term_start[j + 1] - term_start[j];
    MQ_CHECK_ARG(nt >= 0, "term_start must not decrease (term_start[%lld] = %lld after %lld)", (long long)(j + 1),
                 (long long)term_start[j + 1], (long long)term_start[j]);
    MQ_CHECK_ARG(nt <= MQ_LEX_MAX_TERMS, "a query takes at most %d terms (query %lld has %lld)", MQ_LEX_MAX_TERMS,
                 (long long)j, (long long)nt);
  }
  const int64_t total_terms = term_start[nq];
  MQ_CHECK_ARG(total_terms == 0 || keys, "NULL keys");
  MQ_CHECK_ARG(total_terms == 0 || w, "NULL w");
  MQ_CHECK_ARG(out_scores && out_ids, "NULL output");
  MQ_CHECK_ARG(scratch == nullptr || (scratch != (void*)out_scores && scratch != (void*)out_ids),
               "scratch must not be an output");
  // cut the batch into groups and pack their records (host only); a query's keys are checked
  // for repeats on the way: the group's hash finds a repeat as a key whose slot the query
  // has already used
  std::vector<LexGroup> host;
  std::vector<int64_t> first;  // first query of each group
  {
    bool used[kBU];
    for (int64_t j = 0; j < nq; ++j) {
      const int64_t t0 = term_start[j], nt = term_start[j + 1] - t0;
      LexGroup* g = host.empty() ? nullptr : &host.back();
      bool fits = g != nullptr && g->n_q < kBG && g->qstart[g->n_q] + nt <= kBTerms;
      if (fits) {
        int fresh = 0;
        for (int64_t t = 0; t < nt; ++t) fresh += group_find(g, keys[t0 + t]) < 0 ? 1 : 0;
        fits = g->n_union + fresh <= kBU;  // `fresh` over-counts a repeated key: caught below
      }
      if (!fits) {
        host.emplace_back();
        first.push_back(j);
        g = &host.back();
        group_clear(g);
      }
      memset(used, 0, sizeof(used));
      int at = g->qstart[g->n_q];
      for (int64_t t = 0; t < nt; ++t) {
        int slot = group_find(g, keys[t0 + t]);
        if (slot < 0) {
          MQ_CHECK_ARG(g->n_union < kBU, "keys must be distinct within a query (query %lld)", (long long)j);
          slot = group_insert(g, keys[t0 + t]);
        }
        MQ_CHECK_ARG(!used[slot], "keys must be distinct within a query (key %u is repeated in query %lld)",
                     keys[t0 + t], (long long)j);
        used[slot] = true;
        g->qslot[at] = (uint16_t)slot;
        g->qw[at] = w[t0 + t];
        ++at;
      }
      g->qstart[++g->n_q] = at;
    }
    for (const LexGroup& g : host)  // what makes the kernel's probe loop end
      MQ_CHECK_ARG(g.n_union <= kBHash / 2 && g.n_q >= 1 && g.n_q <= kBG && g.qstart[g.n_q] <= kBTerms,
                   "internal: a group of %d queries, %d keys", g.n_q, g.n_union);
  }
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    if (!io_on_device) {
      for (int64_t j = 0; j < nq * k; ++j) {
        out_scores[j] = -INFINITY;
        out_ids[j] = -1;
      }
      return MQ_OK;
    }
    const int dev = pointer_device(out_scores);
    MQ_CHECK_ARG(dev >= 0 && pointer_device(out_ids) == dev, "the outputs must be device memory of one GPU");
    DeviceGuard dg(dev);
    hipLaunchKernelGGL(lex_pad_rows_kernel, dim3((unsigned)((nq * k + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                       out_scores, out_ids, nq * k);
    MQ_HIP(hipGetLastError());
    return MQ_OK;
  }
  MQ_CHECK_ARG(scratch, "NULL buffer");
  MQ_CHECK_ARG((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "scratch must be 16-byte aligned");
  const int dev = pointer_device(scratch);
  MQ_CHECK_ARG(dev >= 0 && pointer_device(offsets) == dev && (n_tokens == 0 || pointer_device(tokens) == dev) &&
                   (bits == nullptr || pointer_device(bits) == dev) &&
                   (!io_on_device || (pointer_device(out_scores) == dev && pointer_device(out_ids) == dev)),
               "tokens, offsets, bits, scratch and device outputs must be device memory of one GPU");
  DeviceGuard dg(dev);
  const BatchScratch sc = carve_batch(scratch, n, nq, total_terms, k);
  const int64_t n_groups = (int64_t)host.size();
  first.push_back(nq);
  // sc.slots groups at a time: their records go up with one copy that has finished before the
  // call goes on (`host` need not outlive the call), in stream order behind the chunk before
  for (int64_t g0 = 0; g0 < n_groups; g0 += sc.slots) {
    const int64_t g1 = g0 + sc.slots < n_groups ? g0 + sc.slots : n_groups;
    MQ_HIP(hipMemcpyAsync(sc.groups, &host[(size_t)g0], (size_t)(g1 - g0) * sizeof(LexGroup), hipMemcpyHostToDevice, s));
    MQ_HIP(hipStreamSynchronize(s));
    const int64_t q0 = first[(size_t)g0], q1 = first[(size_t)g1];
    float* os = io_on_device ? out_scores + q0 * k : sc.out_s;
    int64_t* oi = io_on_device ? out_ids + q0 * k : sc.out_i;
    for (int64_t g = g0; g < g1; ++g) {
      const LexGroup& hg = host[(size_t)g];
      const int64_t row = (first[(size_t)g] - q0) * k;
      if (hg.n_union == 0) {  // queries without terms only: padding
        const int64_t count = (int64_t)hg.n_q * k;
        hipLaunchKernelGGL(lex_pad_rows_kernel, dim3((unsigned)((count + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                           s, os + row, oi + row, count);
        MQ_HIP(hipGetLastError());
        continue;
      }
      const int rows = batch_rows(hg.n_union);
      const int lists = batch_lists(n, rows);
      launch_batch<kModeScore>(rows, (unsigned)lists, s, tokens, n_tokens, offsets, n, ngram, sc.groups + (g - g0), c0,
                               c1, bits, k, nullptr, sc.list_s, sc.list_id);
      MQ_HIP(hipGetLastError());
      const int mrc = mq_topk_merge_device(sc.list_s, sc.list_id, lists, hg.n_q, k, k, os + row, oi + row, stream);
      if (mrc != MQ_OK) return mrc;
    }
    if (!io_on_device) {
      MQ_HIP(hipMemcpyAsync(out_scores + q0 * k, os, (size_t)(q1 - q0) * k * 4, hipMemcpyDeviceToHost, s));
      MQ_HIP(hipMemcpyAsync(out_ids + q0 * k, oi, (size_t)(q1 - q0) * k * 8, hipMemcpyDeviceToHost, s));
    }
  }
  if (!io_on_device) MQ_HIP(hipStreamSynchronize(s));
  return MQ_OK;
}
