// range.hip - K17: range search, every row at or above a score threshold, counted exactly,
// and the best max_hits (<= MQ_RANGE_MAX_HITS) of them (include/mq.h "Range search",
// mq_index_search_range / mq_range_scratch_bytes).
//
// range_score_kernel is the row walk of grouped.hip's group_scan_kernel (16 lanes per row,
// 16-byte non-temporal loads, queries in LDS, two rows in flight per lane group, the same
// fp32 FMA chain and 16-lane butterfly); where that kernel raises a table cell, the lane that
// owns (row, query j) writes keys[j][row]: the score as an order-preserving unsigned when the
// row is a hit, 0 when it is not.  The selection then works on the unique 64-bit keys
// K = (keys[j][row] << 32) | (0xFFFFFFFF - row), whose descending order is the ranking
// (score desc, row asc): a radix select from the top digit down (range_hist_kernel /
// range_pick_kernel, six digits of 11, 11, 10, 11, 11, 10 bits) finds the key K* of rank
// max_hits, range_collect_kernel gathers the cells with K >= K* in any order, and
// range_sort_kernel sorts them in LDS and writes the list.  Every hand-off is a kernel
// boundary on one stream; the launches are enqueued unconditionally and nothing is read back
// in between.
//
// This file talks to the index through its public ABI only (mq_index_data, _size, _dim) and
// allocates no device memory: keys, histograms, state, candidates and the host calls' staging
// live in the caller's scratch.
#include <algorithm>
#include <atomic>
#include <cmath>

#include "common.hpp"

namespace mq {

constexpr int kRangePassQ = 16;      // queries per pass: one per lane of a row's lane group
constexpr int kRangeMaxNV = 16;      // 16-B loads per lane per row: dim <= 1024
constexpr int kRangeMaxDim = 64 * kRangeMaxNV;
constexpr int kRangeBins = 2048;     // bins of one histogram: the widest digit has 11 bits
constexpr int kRangeDigits = 6;
constexpr int kRangeSelSpan = 4096;  // cells per select workgroup before another one is added
constexpr int kRangeSortThreads = 1024;

// Digit d of the 64-bit key is its bits [shift, shift + bits): three digits of the score
// word from the top, then three of the row word.
__host__ __device__ constexpr int range_digit_shift(int d) {
  return d == 0 ? 53 : d == 1 ? 42 : d == 2 ? 32 : d == 3 ? 21 : d == 4 ? 10 : 0;
}
__host__ __device__ constexpr int range_digit_bits(int d) { return (d == 2 || d == 5) ? 10 : 11; }

// The selection's state of one query of a pass (zeroed on the stream before the scan).
struct RangeState {
  unsigned long long prefix;  // the digits fixed so far, the others 0
  unsigned long long cut;     // K*: collect takes the keys >= cut (valid once settled)
  unsigned rank;              // the wanted key's rank among the keys that share the prefix, from 1
  unsigned settled;           // the cut is final: later histogram and pick launches return at once
};

// The score as an order-preserving unsigned (the high word of grouped.hip's group_key: sign
// bit flipped for non-negative scores, every bit inverted for negative ones); never 0 for a
// finite score, so 0 can say "no hit".
__device__ __forceinline__ unsigned range_score_word(float score) {
  const unsigned b = __float_as_uint(score);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float range_word_score(unsigned hi) {
  return __uint_as_float((hi & 0x80000000u) ? (hi ^ 0x80000000u) : ~hi);
}
__device__ __forceinline__ unsigned long long range_key(unsigned word, int64_t row) {
  return ((unsigned long long)word << 32) | (0xFFFFFFFFu - (unsigned)row);
}

// Grid: blocks of 16 lane groups; lane group g walks rows g, g + G, g + 2G, ... (G = 16 x
// blocks), two per iteration.  keys: [nq][n_rows] words; cell (j, r) is written exactly once,
// by lane j of the lane group that walks row r, so the call never clears them.
template <int NQ, int NV>
__global__ __launch_bounds__(256) void range_score_kernel(const float* __restrict__ Q, int nq,
                                                          const float* __restrict__ C, int64_t n_rows, int dim,
                                                          const unsigned* __restrict__ mask, float min_score,
                                                          unsigned* __restrict__ keys) {
  extern __shared__ __attribute__((aligned(16))) float qs[];  // [NQ][dim], zero padded
  const int tid = threadIdx.x, gl = tid & 15;
  for (int i = tid; i < NQ * dim; i += 256) {
    const int j = i / dim;
    qs[i] = j < nq ? Q[(int64_t)j * dim + (i - j * dim)] : 0.f;
  }
  __syncthreads();
  const int nv = NV == kRangeMaxNV ? dim / 64 : NV;  // NV < max: compiled for dim = 64 NV
  const int64_t group = (int64_t)blockIdx.x * 16 + (tid >> 4);
  const int64_t n_lane_groups = (int64_t)gridDim.x * 16;
  const bool owner = gl < nq && gl < NQ;  // lane gl writes query gl's cells
  const float* qbase = qs + gl * 4;
  unsigned* mine_row = keys + (size_t)gl * (size_t)n_rows;

  for (int64_t r0 = group; r0 < n_rows; r0 += 2 * n_lane_groups) {
    const int nr = r0 + n_lane_groups < n_rows ? 2 : 1;
    floatx4 v[2][NV];
    unsigned mw[2] = {~0u, ~0u};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t r = u < nr ? r0 + u * n_lane_groups : r0;
      const floatx4* rp = reinterpret_cast<const floatx4*>(C + r * dim) + gl;
#pragma unroll
      for (int it = 0; it < NV; ++it)
        if (it < nv) v[u][it] = __builtin_nontemporal_load(rp + it * 16);
      if (mask) mw[u] = mask[r >> 5];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float mine = 0.f;
      constexpr int kUnrollQ = NQ <= 2 ? NQ : 1;
#pragma unroll kUnrollQ
      for (int j = 0; j < NQ; ++j) {
        const float* qj = qbase + j * dim;
        if constexpr (NQ > 2) asm volatile("" : "+v"(qj));
        float acc = 0.f;
#pragma unroll
        for (int it = 0; it < NV; ++it) {
          if (it < nv) {
            const floatx4 qv = *reinterpret_cast<const floatx4*>(qj + it * 64);
            acc = fmaf(v[u][it].x, qv.x, fmaf(v[u][it].y, qv.y, fmaf(v[u][it].z, qv.z, fmaf(v[u][it].w, qv.w, acc))));
          }
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 16);
        mine = gl == j ? acc : mine;
      }
      const int64_t r = r0 + u * n_lane_groups;
      if (u < nr && owner) {
        // + 0.0f: a -0.0 sum would key below +0.0, which the ranking holds equal to it
        const float s = mine + 0.0f;
        const bool here = (mw[u] >> (r & 31)) & 1u;
        mine_row[r] = (here && s >= min_score) ? range_score_word(s) : 0u;
      }
    }
  }
}

// Grid (blocks, queries of the pass).  Workgroup (b, j) counts digit D of query j's keys that
// share the prefix fixed so far, over cells b * 256 + tid, + 256 * blocks, ..., in an LDS
// histogram, and adds its non-empty bins to hist[j][bins] (zero when the launch begins).
template <int D>
__global__ __launch_bounds__(256) void range_hist_kernel(const unsigned* __restrict__ keys, int64_t n_rows,
                                                         const RangeState* __restrict__ state,
                                                         unsigned* __restrict__ hist) {
  constexpr int kShift = range_digit_shift(D), kBits = range_digit_bits(D);
  __shared__ unsigned bins[kRangeBins];
  const int j = blockIdx.y, tid = threadIdx.x;
  if (state[j].settled) return;
  const unsigned long long prefix = state[j].prefix;
  for (int i = tid; i < (1 << kBits); i += 256) bins[i] = 0;
  __syncthreads();
  const unsigned* kj = keys + (size_t)j * (size_t)n_rows;
  for (int64_t r = (int64_t)blockIdx.x * 256 + tid; r < n_rows; r += (int64_t)gridDim.x * 256) {
    const unsigned w = kj[r];
    if (w == 0) continue;
    const unsigned long long key = range_key(w, r);
    if constexpr (D > 0) {
      if ((key ^ prefix) >> (kShift + kBits)) continue;  // outside the prefix chosen so far
    }
    atomicAdd(&bins[(unsigned)(key >> kShift) & ((1u << kBits) - 1)], 1u);
  }
  __syncthreads();
  for (int i = tid; i < (1 << kBits); i += 256)
    if (bins[i]) atomicAdd(&hist[(size_t)j * kRangeBins + i], bins[i]);
}

// One workgroup per query.  Reads digit D's histogram, from the top bin down, fixes the bin in
// which the key of the wanted rank falls, and clears the histogram for the next digit.  D == 0:
// the histogram's total is the hit count.  The query is settled when every hit is wanted
// (count <= max_hits: cut 1, below every key) or when the chosen bin is wanted whole (cut =
// the prefix: the ranking splits at a digit boundary); the last digit's bins hold one key
// each, so it always settles.
template <int D>
__global__ __launch_bounds__(256) void range_pick_kernel(unsigned* __restrict__ hist, RangeState* __restrict__ state,
                                                         int max_hits, int64_t* __restrict__ out_counts) {
  constexpr int kShift = range_digit_shift(D), kBits = range_digit_bits(D);
  constexpr int kPer = kRangeBins / 256;  // bins per thread, thread 0 holding the top ones
  __shared__ unsigned sums[256];
  const int j = blockIdx.x, tid = threadIdx.x;
  if (state[j].settled) return;
  // read before the first barrier: one thread rewrites them at the end
  const unsigned long long prefix0 = state[j].prefix;
  unsigned rank = D == 0 ? (unsigned)max_hits : state[j].rank;
  unsigned* h = hist + (size_t)j * kRangeBins;
  unsigned c[kPer];
  unsigned mine = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int bin = kRangeBins - 1 - (tid * kPer + e);
    c[e] = bin < (1 << kBits) ? h[bin] : 0u;
    h[bin] = 0;
    mine += c[e];
  }
  sums[tid] = mine;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {  // inclusive scan, top bins first
    const unsigned add = tid >= off ? sums[tid - off] : 0u;
    __syncthreads();
    sums[tid] += add;
    __syncthreads();
  }
  const unsigned total = sums[255];
  if (D == 0) {
    if (tid == 0) out_counts[j] = (int64_t)total;
    if (total <= (unsigned)max_hits) {
      if (tid == 0) {
        state[j].cut = 1ull;
        state[j].settled = 1u;
      }
      return;
    }
  }
  // total >= rank: exactly one thread's bins straddle the rank
  unsigned before = sums[tid] - mine;
  if (before < rank && rank <= before + mine) {
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      if (before < rank && rank <= before + c[e]) {
        const int bin = kRangeBins - 1 - (tid * kPer + e);
        const unsigned long long prefix = prefix0 | ((unsigned long long)bin << kShift);
        state[j].prefix = prefix;
        state[j].rank = rank - before;
        if (rank - before == c[e] || D == kRangeDigits - 1) {
          state[j].cut = prefix;
          state[j].settled = 1u;
        }
        rank = 0;  // taken: no later bin of this thread matches
      }
      before += c[e];
    }
  }
}

// Grid (blocks, queries of the pass).  The cells with K >= cut go to cand[j][slot], the slot
// from one returning atomicAdd per wave (ballot and popcount).  Keys are unique, so exactly
// min(count, max_hits) arrive; the bound on the slot only keeps a wrong cut inside the array.
__global__ __launch_bounds__(256) void range_collect_kernel(const unsigned* __restrict__ keys, int64_t n_rows,
                                                            const RangeState* __restrict__ state, int max_hits,
                                                            unsigned* __restrict__ cand_count,
                                                            unsigned long long* __restrict__ cand) {
  const int j = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const unsigned long long cut = state[j].cut;
  const unsigned* kj = keys + (size_t)j * (size_t)n_rows;
  unsigned long long* cj = cand + (size_t)j * max_hits;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n_rows; base += stride) {  // uniform per workgroup
    const int64_t r = base + tid;
    const unsigned w = r < n_rows ? kj[r] : 0u;
    const unsigned long long key = range_key(w, r);
    const bool take = w != 0 && key >= cut;
    const unsigned long long votes = __ballot(take);
    if (votes == 0) continue;
    unsigned slot0 = 0;
    if (lane == 0) slot0 = atomicAdd(&cand_count[j], (unsigned)__popcll(votes));
    slot0 = __shfl(slot0, 0);
    if (take) {
      const unsigned slot = slot0 + (unsigned)__popcll(votes & ((1ull << lane) - 1));
      if (slot < (unsigned)max_hits) cj[slot] = key;
    }
  }
}

// One workgroup per query: the candidates into LDS (padded with 0 to a power of two), a
// bitonic sort descending, then (score, row) of each key and (-inf, -1) after them.  Sorting
// unique keys makes the list independent of the order they arrived in.  out_ids may be the
// candidate array itself (the host calls' staging): workgroup j reads cand[j] whole before it
// writes out_ids[j], and touches no other query's.
__global__ __launch_bounds__(kRangeSortThreads) void range_sort_kernel(const unsigned long long* cand,
                                                                       const unsigned* __restrict__ cand_count,
                                                                       int max_hits, float* __restrict__ out_scores,
                                                                       int64_t* out_ids) {
  __shared__ unsigned long long ks[MQ_RANGE_MAX_HITS];
  const int j = blockIdx.x, tid = threadIdx.x;
  const int cnt = (int)min(cand_count[j], (unsigned)max_hits);
  int p2 = 1;
  while (p2 < cnt) p2 <<= 1;
  const unsigned long long* cj = cand + (size_t)j * max_hits;
  for (int i = tid; i < p2; i += kRangeSortThreads) ks[i] = i < cnt ? cj[i] : 0ull;
  __syncthreads();
  for (int k = 2; k <= p2; k <<= 1) {
    for (int s = k >> 1; s > 0; s >>= 1) {
      for (int i = tid; i < p2; i += kRangeSortThreads) {
        const int l = i ^ s;
        if (l > i) {
          const unsigned long long a = ks[i], b = ks[l];
          const bool desc = (i & k) == 0;
          if (desc ? a < b : a > b) {
            ks[i] = b;
            ks[l] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < max_hits; i += kRangeSortThreads) {
    const unsigned long long key = i < cnt ? ks[i] : 0ull;
    out_scores[(size_t)j * max_hits + i] = i < cnt ? range_word_score((unsigned)(key >> 32)) : -INFINITY;
    out_ids[(size_t)j * max_hits + i] = i < cnt ? (int64_t)(0xFFFFFFFFu - (unsigned)key) : -1;
  }
}

// (0 hits, (-inf, -1) everywhere): what an empty index returns.
__global__ __launch_bounds__(256) void range_pad_kernel(int64_t* __restrict__ out_counts, int64_t nq,
                                                        float* __restrict__ out_scores, int64_t* __restrict__ out_ids,
                                                        int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nq) out_counts[i] = 0;
  if (i < count) {
    out_scores[i] = -INFINITY;
    out_ids[i] = -1;
  }
}

}  // namespace mq

using namespace mq;

namespace {

int64_t up256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// Sections of the scratch, each a multiple of 256 bytes: the keys, then what the call zeroes
// at the start of every pass (histograms, state, candidate counters, the staged counts), the
// candidates, and the staging of one pass of a host-pointer call.  A host call's ids are
// staged in the candidate array itself (range_sort_kernel).
struct RangeLayout {
  int64_t keys, hist, state, cand_count, stage_c, zero_end, cand, stage_q, stage_s, total;
};

RangeLayout range_layout(int64_t n, int64_t nq, int max_hits) {
  n = std::min<int64_t>(std::max<int64_t>(n, 0), (1ll << 31) - 1);
  const int64_t tq = std::min<int64_t>(std::max<int64_t>(nq, 0), kRangePassQ);  // queries per pass
  max_hits = std::min(std::max(max_hits, 1), MQ_RANGE_MAX_HITS);
  RangeLayout l;
  l.keys = 0;
  l.hist = l.keys + up256(tq * n * 4);
  l.state = l.hist + up256(tq * kRangeBins * 4);
  l.cand_count = l.state + up256(tq * (int64_t)sizeof(RangeState));
  l.stage_c = l.cand_count + up256(tq * 4);
  l.zero_end = l.stage_c + up256(tq * 8);
  l.cand = l.zero_end;
  l.stage_q = l.cand + up256(tq * max_hits * 8);
  l.stage_s = l.stage_q + up256(tq * kRangeMaxDim * 4);
  l.total = l.stage_s + up256(tq * max_hits * 4);
  return l;
}

bool overlaps(const void* a, int64_t ab, const void* b, int64_t bb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bb && b0 < a0 + (uintptr_t)ab;
}

// The checks of the scalars, which need neither a handle nor a shape.
int check_range_scalars(int64_t nq, int max_hits, float min_score) {
  MQ_CHECK_ARG(max_hits >= 1 && max_hits <= MQ_RANGE_MAX_HITS, "max_hits must be in [1, %d] (got %d)",
               MQ_RANGE_MAX_HITS, max_hits);
  MQ_CHECK_ARG(!std::isnan(min_score), "min_score must not be NaN (-inf means no threshold)");
  MQ_CHECK_ARG(nq >= 0 && nq <= (1ll << 24), "query count %lld out of range", (long long)nq);
  return MQ_OK;
}

// Every check of mq_index_search_range that needs no HIP call, on the index's shape (dim, n
// rows): nothing here touches the runtime, so a bad call fails the same way on a machine
// without a GPU.
int check_range_args(int dim, int64_t n, const float* queries, int64_t nq, int max_hits, float min_score,
                     const int64_t* out_counts, const float* out_scores, const int64_t* out_ids, const void* scratch,
                     int64_t scratch_bytes) {
  if (int rc = check_range_scalars(nq, max_hits, min_score)) return rc;
  MQ_CHECK_ARG(dim > 0 && dim % 64 == 0 && dim <= kRangeMaxDim,
               "the range scan serves dim %% 64 == 0, dim <= %d (got %d)", kRangeMaxDim, dim);
  MQ_CHECK_ARG(n >= 0 && n < (1ll << 31), "the range scan serves fewer than 2^31 rows (got %lld)", (long long)n);
  if (nq == 0) return MQ_OK;
  MQ_CHECK_ARG(queries, "NULL queries");
  MQ_CHECK_ARG(out_counts && out_scores && out_ids, "NULL output buffer");
  if (n == 0) return MQ_OK;  // zero counts and padding only: the scratch is not read
  MQ_CHECK_ARG(scratch, "NULL scratch");
  MQ_CHECK_ARG((uintptr_t)scratch % 16 == 0, "scratch must be 16-byte aligned (got %p)", scratch);
  const int64_t need = range_layout(n, nq, max_hits).total;
  MQ_CHECK_ARG(scratch_bytes >= need,
               "scratch_bytes %lld is below the %lld bytes mq_range_scratch_bytes(%lld, %lld, %d) asks",
               (long long)scratch_bytes, (long long)need, (long long)n, (long long)nq, max_hits);
  MQ_CHECK_ARG(!overlaps(scratch, scratch_bytes, out_counts, nq * 8), "scratch overlaps out_counts (%p)",
               (const void*)out_counts);
  MQ_CHECK_ARG(!overlaps(scratch, scratch_bytes, out_scores, nq * max_hits * 4), "scratch overlaps out_scores (%p)",
               (const void*)out_scores);
  MQ_CHECK_ARG(!overlaps(scratch, scratch_bytes, out_ids, nq * max_hits * 8), "scratch overlaps out_ids (%p)",
               (const void*)out_ids);
  return MQ_OK;
}

// Device of a pointer (HIP device memory), or -1 (host / unknown).
int pointer_device(const void* p) {
  hipPointerAttribute_t a;
  if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  return a.type == hipMemoryTypeDevice ? a.device : -1;
}

constexpr int kMaxDevices = 64;
std::atomic<int> g_cus[kMaxDevices];  // compute units of each GPU, read once

int num_cus(int device) {
  const bool known = device >= 0 && device < kMaxDevices;
  int cus = known ? g_cus[device].load(std::memory_order_relaxed) : 0;
  if (cus > 0) return cus;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
  if (known) g_cus[device].store(cus, std::memory_order_relaxed);
  return cus;
}

template <int NQ>
void launch_score_nq(const float* q, int nq, const float* rows, int64_t n, int dim, const unsigned* bits,
                     float min_score, unsigned* keys, int blocks, hipStream_t s) {
  const size_t lds = (size_t)NQ * dim * sizeof(float);  // <= 64 KB: the default dynamic-LDS limit
  if (dim == 768)  // the BERT-base width, register arrays sized exactly
    hipLaunchKernelGGL((range_score_kernel<NQ, 12>), dim3(blocks), dim3(256), lds, s, q, nq, rows, n, dim, bits,
                       min_score, keys);
  else
    hipLaunchKernelGGL((range_score_kernel<NQ, kRangeMaxNV>), dim3(blocks), dim3(256), lds, s, q, nq, rows, n, dim,
                       bits, min_score, keys);
}

void launch_score(const float* q, int nq, const float* rows, int64_t n, int dim, const unsigned* bits,
                  float min_score, unsigned* keys, int blocks, hipStream_t s) {
  if (nq <= 1)
    launch_score_nq<1>(q, nq, rows, n, dim, bits, min_score, keys, blocks, s);
  else if (nq <= 2)
    launch_score_nq<2>(q, nq, rows, n, dim, bits, min_score, keys, blocks, s);
  else if (nq <= 4)
    launch_score_nq<4>(q, nq, rows, n, dim, bits, min_score, keys, blocks, s);
  else if (nq <= 8)
    launch_score_nq<8>(q, nq, rows, n, dim, bits, min_score, keys, blocks, s);
  else
    launch_score_nq<16>(q, nq, rows, n, dim, bits, min_score, keys, blocks, s);
}

template <int D>
void launch_digit(const unsigned* keys, int64_t n, RangeState* state, unsigned* hist, int pq, int max_hits,
                  int64_t* counts, int blocks, hipStream_t s) {
  hipLaunchKernelGGL(range_hist_kernel<D>, dim3(blocks, pq), dim3(256), 0, s, keys, n, state, hist);
  hipLaunchKernelGGL(range_pick_kernel<D>, dim3(pq), dim3(256), 0, s, hist, state, max_hits, counts);
}

}  // namespace

extern "C" {

int64_t mq_range_scratch_bytes(int64_t n_rows, int64_t nq, int max_hits) {
  return range_layout(n_rows, nq, max_hits).total;
}

int mq_range_scan_blocks(int64_t n_rows, int compute_units) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(2 * (int64_t)std::max(compute_units, 1), (n_rows + 127) / 128));
}

int mq_range_select_blocks(int64_t n_rows, int compute_units) {
  return (int)std::max<int64_t>(
      1, std::min<int64_t>((int64_t)std::max(compute_units, 1), (n_rows + kRangeSelSpan - 1) / kRangeSelSpan));
}

int mq_debug_range_check(int dim, int64_t n_rows, const float* queries, int64_t nq, int max_hits, float min_score,
                         const int64_t* out_counts, const float* out_scores, const int64_t* out_ids,
                         const void* scratch, int64_t scratch_bytes) {
  clear_error();
  return check_range_args(dim, n_rows, queries, nq, max_hits, min_score, out_counts, out_scores, out_ids, scratch,
                          scratch_bytes);
}

int mq_index_search_range(mq_index* ix, const float* queries, int64_t nq, int max_hits, float min_score,
                          const uint32_t* bits, int64_t* out_counts, float* out_scores, int64_t* out_ids,
                          int io_on_device, void* scratch, int64_t scratch_bytes, void* stream) {
  clear_error();
  // the scalars first: they need no handle
  if (int rc = check_range_scalars(nq, max_hits, min_score)) return rc;
  MQ_CHECK_ARG(ix, "NULL index");
  int64_t n = 0;
  int dim = 0;
  void* slab = nullptr;
  int rc = mq_index_size(ix, &n);
  if (!rc) rc = mq_index_dim(ix, &dim);
  if (!rc) rc = mq_index_data(ix, &slab);
  if (rc) return rc;
  rc = check_range_args(dim, n, queries, nq, max_hits, min_score, out_counts, out_scores, out_ids, scratch,
                        scratch_bytes);
  if (rc || nq == 0) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t cells = nq * max_hits;

  if (n == 0) {  // no hits: zero counts, padding only
    if (!io_on_device) {
      for (int64_t i = 0; i < nq; ++i) out_counts[i] = 0;
      for (int64_t i = 0; i < cells; ++i) {
        out_scores[i] = -INFINITY;
        out_ids[i] = -1;
      }
      return MQ_OK;
    }
    const int dev = pointer_device(out_scores);
    MQ_CHECK_ARG(dev >= 0 && pointer_device(out_ids) == dev && pointer_device(out_counts) == dev,
                 "the outputs must be device memory of one GPU");
    DeviceGuard dg(dev);
    hipLaunchKernelGGL(range_pad_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, out_counts, nq,
                       out_scores, out_ids, cells);
    MQ_HIP(hipGetLastError());
    return MQ_OK;
  }

  const int device = pointer_device(slab);
  if (device < 0) MQ_FAIL(MQ_ESTATE, "the index's row slab is not device memory");
  MQ_CHECK_ARG(!bits || pointer_device(bits) == device, "the mask must be device memory of the index's GPU %d", device);
  MQ_CHECK_ARG(pointer_device(scratch) == device, "scratch must be device memory of the index's GPU %d", device);
  if (io_on_device)
    MQ_CHECK_ARG(pointer_device(queries) == device && pointer_device(out_counts) == device &&
                     pointer_device(out_scores) == device && pointer_device(out_ids) == device,
                 "queries and outputs must be device memory of the index's GPU %d", device);
  DeviceGuard dg(device);

  const RangeLayout l = range_layout(n, nq, max_hits);
  char* base = static_cast<char*>(scratch);
  unsigned* keys = reinterpret_cast<unsigned*>(base + l.keys);
  unsigned* hist = reinterpret_cast<unsigned*>(base + l.hist);
  RangeState* state = reinterpret_cast<RangeState*>(base + l.state);
  unsigned* cand_count = reinterpret_cast<unsigned*>(base + l.cand_count);
  int64_t* stage_c = reinterpret_cast<int64_t*>(base + l.stage_c);
  unsigned long long* cand = reinterpret_cast<unsigned long long*>(base + l.cand);
  float* stage_q = reinterpret_cast<float*>(base + l.stage_q);
  float* stage_s = reinterpret_cast<float*>(base + l.stage_s);
  const float* rows = static_cast<const float*>(slab);
  const int cus = num_cus(device);
  const int scan_blocks = mq_range_scan_blocks(n, cus);
  const int sel_blocks = mq_range_select_blocks(n, cus);

  // successive passes of at most 16 queries reuse the whole scratch in stream order
  for (int64_t p0 = 0; p0 < nq; p0 += kRangePassQ) {
    const int pq = (int)std::min<int64_t>(kRangePassQ, nq - p0);
    const float* dq = queries + p0 * dim;
    int64_t* doc = out_counts + p0;
    float* dos = out_scores + p0 * max_hits;
    int64_t* doi = out_ids + p0 * max_hits;
    if (!io_on_device) {
      MQ_HIP(hipMemcpyAsync(stage_q, dq, (size_t)pq * dim * 4, hipMemcpyHostToDevice, s));
      dq = stage_q;
      doc = stage_c;
      dos = stage_s;
      doi = reinterpret_cast<int64_t*>(cand);
    }
    MQ_HIP(hipMemsetAsync(base + l.hist, 0, (size_t)(l.zero_end - l.hist), s));
    launch_score(dq, pq, rows, n, dim, bits, min_score, keys, scan_blocks, s);
    MQ_HIP(hipGetLastError());
    launch_digit<0>(keys, n, state, hist, pq, max_hits, doc, sel_blocks, s);
    launch_digit<1>(keys, n, state, hist, pq, max_hits, doc, sel_blocks, s);
    launch_digit<2>(keys, n, state, hist, pq, max_hits, doc, sel_blocks, s);
    launch_digit<3>(keys, n, state, hist, pq, max_hits, doc, sel_blocks, s);
    launch_digit<4>(keys, n, state, hist, pq, max_hits, doc, sel_blocks, s);
    launch_digit<5>(keys, n, state, hist, pq, max_hits, doc, sel_blocks, s);
    MQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(range_collect_kernel, dim3(sel_blocks, pq), dim3(256), 0, s, keys, n, state, max_hits,
                       cand_count, cand);
    hipLaunchKernelGGL(range_sort_kernel, dim3(pq), dim3(kRangeSortThreads), 0, s, cand, cand_count, max_hits, dos,
                       doi);
    MQ_HIP(hipGetLastError());
    if (!io_on_device) {
      MQ_HIP(hipMemcpyAsync(out_counts + p0, stage_c, (size_t)pq * 8, hipMemcpyDeviceToHost, s));
      MQ_HIP(hipMemcpyAsync(out_scores + p0 * max_hits, stage_s, (size_t)pq * max_hits * 4, hipMemcpyDeviceToHost, s));
      MQ_HIP(hipMemcpyAsync(out_ids + p0 * max_hits, cand, (size_t)pq * max_hits * 8, hipMemcpyDeviceToHost, s));
    }
  }
  if (!io_on_device) MQ_HIP(hipStreamSynchronize(s));
  return MQ_OK;
}

}  // extern "C"
