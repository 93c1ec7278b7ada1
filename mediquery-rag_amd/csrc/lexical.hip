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
#include <cstring>

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
