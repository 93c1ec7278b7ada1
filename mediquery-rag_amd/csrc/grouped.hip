// grouped.hip - K16: grouped search, the top-k distinct groups of a row-to-group map
// (include/mq.h "Grouped search", mq_index_search_grouped / mq_group_scratch_bytes).
//
// group_scan_kernel is the row walk of index.hip's stream_search_kernel (16 lanes per row,
// 16-byte non-temporal loads, queries in LDS, two rows in flight per lane group, fp32 FMA,
// a 16-lane butterfly per (row, query)) with a group maximum where that kernel inserts into
// a per-lane list: the lane that owns (row, query j) raises best[j][codes[row]], a table of
// 64-bit keys in the caller's scratch.  group_select_kernel then takes the top-k of each
// query's n_groups keys: grid-stride workgroups keep register lists (topk.hpp), emit them
// sorted, and mq_topk_merge_device merges the workgroups' lists.
//
// This file talks to the index through its public ABI only (mq_index_data, _size, _dim) and
// allocates no device memory: table, lists and the host calls' staging live in the scratch.
#include <algorithm>
#include <atomic>
#include <cmath>

#include "common.hpp"
#include "topk.hpp"

namespace mq {

constexpr int kGroupPassQ = 16;       // queries per pass: one per lane of a row's lane group
constexpr int kGroupMaxNV = 16;       // 16-B loads per lane per row: dim <= 1024
constexpr int kGroupMaxDim = 64 * kGroupMaxNV;
constexpr int kGroupSelBlocks = 64;   // most select workgroups (lists the merge reads) per query
constexpr int kGroupSelSpan = 2048;   // groups per select workgroup before another one is added

// (score, row) as one unsigned key: the high word is the score mapped to an order-preserving
// unsigned (sign bit flipped for non-negative scores, every bit inverted for negative ones),
// the low word 0xFFFFFFFF - row, so an unsigned maximum picks the highest score and then the
// lowest row.  0 is no key: rows stay below 2^31, so the low word is never 0.
__device__ __forceinline__ unsigned long long group_key(float score, int row) {
  const unsigned b = __float_as_uint(score);
  const unsigned hi = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((unsigned long long)hi << 32) | (0xFFFFFFFFu - (unsigned)row);
}
__device__ __forceinline__ float group_key_score(unsigned long long key) {
  const unsigned hi = (unsigned)(key >> 32);
  return __uint_as_float((hi & 0x80000000u) ? (hi ^ 0x80000000u) : ~hi);
}
__device__ __forceinline__ int group_key_row(unsigned long long key) {
  return (int)(0xFFFFFFFFu - (unsigned)key);
}

// Grid: blocks of 16 lane groups; lane group g walks rows g, g + G, g + 2G, ... (G = 16 x
// blocks), two per iteration.  best: [NQ rows used][n_groups] keys, zeroed by the caller on
// the stream.  Row r counts for query j when its mask bit is set (mask != NULL) and
// 0 <= codes[r] < n_groups; any other code is ignored: no cell is addressed from it.
template <int NQ, int NV>
__global__ __launch_bounds__(256) void group_scan_kernel(const float* __restrict__ Q, int nq,
                                                         const float* __restrict__ C, int64_t n_rows, int dim,
                                                         const int* __restrict__ codes, int n_groups,
                                                         const unsigned* __restrict__ mask,
                                                         unsigned long long* __restrict__ best) {
  extern __shared__ __attribute__((aligned(16))) float qs[];  // [NQ][dim], zero padded
  const int tid = threadIdx.x, gl = tid & 15;
  for (int i = tid; i < NQ * dim; i += 256) {
    const int j = i / dim;
    qs[i] = j < nq ? Q[(int64_t)j * dim + (i - j * dim)] : 0.f;
  }
  __syncthreads();
  const int nv = NV == kGroupMaxNV ? dim / 64 : NV;  // NV < max: compiled for dim = 64 NV
  const int64_t group = (int64_t)blockIdx.x * 16 + (tid >> 4);
  const int64_t n_lane_groups = (int64_t)gridDim.x * 16;
  const bool owner = gl < nq && gl < NQ;  // lane gl raises query gl's cells
  const float* qbase = qs + gl * 4;
  unsigned long long* mine_row = best + (size_t)gl * n_groups;

  for (int64_t r0 = group; r0 < n_rows; r0 += 2 * n_lane_groups) {
    const int nr = r0 + n_lane_groups < n_rows ? 2 : 1;
    floatx4 v[2][NV];
    unsigned mw[2] = {~0u, ~0u};
    int cd[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t r = u < nr ? r0 + u * n_lane_groups : r0;
      const floatx4* rp = reinterpret_cast<const floatx4*>(C + r * dim) + gl;
#pragma unroll
      for (int it = 0; it < NV; ++it)
        if (it < nv) v[u][it] = __builtin_nontemporal_load(rp + it * 16);
      if (mask) mw[u] = mask[r >> 5];
      cd[u] = codes[r];
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
      const bool here = (mw[u] >> (r & 31)) & 1u;
      if (u < nr && owner && here && (unsigned)cd[u] < (unsigned)n_groups) {
        // + 0.0f: a -0.0 sum would key below +0.0, which the ranking holds equal to it
        const unsigned long long key = group_key(mine + 0.0f, (int)r);
        unsigned long long* cell = mine_row + cd[u];
        // The pre-check is sound because a cell only grows within a call (it is zeroed on the
        // stream before the scan and raised by atomic maxima alone): a stale value read from
        // another XCD's L2 can only be too small, so it costs a redundant atomic and never
        // skips a needed one.  The maximum does not depend on the order of arrival, so the
        // table, and with it the result, is the same bits on every call.
        if (key > __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(cell, key);
      }
    }
  }
}

// Grid (blocks, queries of the pass).  Workgroup (b, j) walks groups b * 256 + tid,
// + 256 * blocks, ... of query j's keys, each thread keeping the best KC (>= k) in a sorted
// register list; k rounds of a block-wide arg-best then emit the workgroup's list sorted by
// (score desc, row asc), padded with (-inf, -1): lists [b][j][0..k) for the merge.
template <int KC>
__global__ __launch_bounds__(256) void group_select_kernel(const unsigned long long* __restrict__ best, int n_groups,
                                                           int nq, int k, float* __restrict__ cand_s,
                                                           int64_t* __restrict__ cand_i) {
  __shared__ float ws[4];
  __shared__ int wi[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = blockIdx.y;
  const unsigned long long* keys = best + (size_t)j * n_groups;
  TopList<KC> top;
  top.init();
  for (int64_t g = (int64_t)blockIdx.x * 256 + tid; g < n_groups; g += (int64_t)gridDim.x * 256) {
    const unsigned long long key = keys[g];
    if (key == 0) continue;  // no candidate row in this group
    const float s = group_key_score(key);
    const int row = group_key_row(key);
    if (top.beats_tail(s, row)) top.insert(s, row);
  }
  const int64_t base = ((int64_t)blockIdx.x * nq + j) * k;
  for (int r = 0; r < k; ++r) {
    float bs = top.s[0];
    int bi = top.id[0];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float os = __shfl_xor(bs, off);
      const int oi = __shfl_xor(bi, off);
      if (better(os, oi, bs, bi)) {
        bs = os;
        bi = oi;
      }
    }
    if (lane == 0) {
      ws[wave] = bs;
      wi[wave] = bi;
    }
    __syncthreads();
    bs = ws[0];
    bi = wi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (better(ws[w], wi[w], bs, bi)) {
        bs = ws[w];
        bi = wi[w];
      }
    if (tid == 0) {
      cand_s[base + r] = bi >= 0 ? bs : -INFINITY;
      cand_i[base + r] = bi;
    }
    // representative rows are distinct (a row has one group, a group one thread): the head
    // that equals the winner is the winner
    if (bi >= 0 && top.id[0] == bi) top.pop_front();
    __syncthreads();
  }
}

// (-inf, -1) into count result slots: what an empty index or n_groups == 0 returns.
__global__ __launch_bounds__(256) void group_pad_kernel(float* __restrict__ out_scores, int64_t* __restrict__ out_ids,
                                                        int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) {
    out_scores[i] = -INFINITY;
    out_ids[i] = -1;
  }
}

}  // namespace mq

using namespace mq;

namespace {

int64_t up256(int64_t b) { return (b + 255) & ~(int64_t)255; }

int select_blocks(int64_t n_groups) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(kGroupSelBlocks, (n_groups + kGroupSelSpan - 1) / kGroupSelSpan));
}

// Sections of the scratch, each a multiple of 256 bytes: the key table, the select
// workgroups' lists, and the staging of one pass of a host-pointer call.
struct GroupLayout {
  int64_t table, cand_i, cand_s, stage_q, stage_i, stage_s, total;
};

GroupLayout group_layout(int64_t n_groups, int64_t nq, int k) {
  n_groups = std::max<int64_t>(n_groups, 0);
  const int64_t tq = std::min<int64_t>(std::max<int64_t>(nq, 0), kGroupPassQ);  // queries per pass
  k = std::min(std::max(k, 1), MQ_MAX_K);
  const int64_t lists = (int64_t)select_blocks(n_groups) * tq * k;
  GroupLayout l;
  l.table = 0;
  l.cand_i = l.table + up256(tq * n_groups * 8);
  l.cand_s = l.cand_i + up256(lists * 8);
  l.stage_q = l.cand_s + up256(lists * 4);
  l.stage_i = l.stage_q + up256(tq * kGroupMaxDim * 4);
  l.stage_s = l.stage_i + up256(tq * k * 8);
  l.total = l.stage_s + up256(tq * k * 4);
  return l;
}

bool overlaps(const void* a, int64_t ab, const void* b, int64_t bb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bb && b0 < a0 + (uintptr_t)ab;
}

// Every check of mq_index_search_grouped that needs no HIP call, on the index's shape
// (dim, n rows): nothing here touches the runtime, so a bad call fails the same way on a
// machine without a GPU.  The slab is fp32 by construction: mq_index_create admits no other
// index dtype, and mq_index_data returns that slab.
int check_group_args(int dim, int64_t n, const float* queries, int64_t nq, int k, const int32_t* codes,
                     int32_t n_groups, const float* out_scores, const int64_t* out_ids, const void* scratch,
                     int64_t scratch_bytes) {
  MQ_CHECK_ARG(k >= 1 && k <= MQ_MAX_K, "k must be in [1, %d] (got %d)", MQ_MAX_K, k);
  MQ_CHECK_ARG(nq >= 0 && nq <= (1ll << 24), "query count %lld out of range", (long long)nq);
  MQ_CHECK_ARG(n_groups >= 0, "n_groups must be >= 0 (got %d)", (int)n_groups);
  MQ_CHECK_ARG(dim > 0 && dim % 64 == 0 && dim <= kGroupMaxDim,
               "the grouped scan serves dim %% 64 == 0, dim <= %d (got %d)", kGroupMaxDim, dim);
  MQ_CHECK_ARG(n >= 0 && n < (1ll << 31), "the grouped scan serves fewer than 2^31 rows (got %lld)", (long long)n);
  if (nq == 0) return MQ_OK;
  MQ_CHECK_ARG(queries, "NULL queries");
  MQ_CHECK_ARG(out_scores && out_ids, "NULL output buffer");
  if (n == 0 || n_groups == 0) return MQ_OK;  // padding only: neither codes nor scratch is read
  MQ_CHECK_ARG(codes, "NULL codes");
  MQ_CHECK_ARG(scratch, "NULL scratch");
  MQ_CHECK_ARG((uintptr_t)scratch % 16 == 0, "scratch must be 16-byte aligned (got %p)", scratch);
  const int64_t need = group_layout(n_groups, nq, k).total;
  MQ_CHECK_ARG(scratch_bytes >= need, "scratch_bytes %lld is below the %lld bytes mq_group_scratch_bytes(%d, %lld, %d) asks",
               (long long)scratch_bytes, (long long)need, (int)n_groups, (long long)nq, k);
  MQ_CHECK_ARG(!overlaps(scratch, scratch_bytes, out_scores, nq * k * 4), "scratch overlaps out_scores (%p)",
               (const void*)out_scores);
  MQ_CHECK_ARG(!overlaps(scratch, scratch_bytes, out_ids, nq * k * 8), "scratch overlaps out_ids (%p)",
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
void launch_scan_nq(const float* q, int nq, const float* rows, int64_t n, int dim, const int* codes, int n_groups,
                    const unsigned* bits, unsigned long long* best, int blocks, hipStream_t s) {
  const size_t lds = (size_t)NQ * dim * sizeof(float);  // <= 64 KB: the default dynamic-LDS limit
  if (dim == 768)  // the BERT-base width, register arrays sized exactly
    hipLaunchKernelGGL((group_scan_kernel<NQ, 12>), dim3(blocks), dim3(256), lds, s, q, nq, rows, n, dim, codes,
                       n_groups, bits, best);
  else
    hipLaunchKernelGGL((group_scan_kernel<NQ, kGroupMaxNV>), dim3(blocks), dim3(256), lds, s, q, nq, rows, n, dim,
                       codes, n_groups, bits, best);
}

void launch_scan(const float* q, int nq, const float* rows, int64_t n, int dim, const int* codes, int n_groups,
                 const unsigned* bits, unsigned long long* best, int blocks, hipStream_t s) {
  if (nq <= 1)
    launch_scan_nq<1>(q, nq, rows, n, dim, codes, n_groups, bits, best, blocks, s);
  else if (nq <= 2)
    launch_scan_nq<2>(q, nq, rows, n, dim, codes, n_groups, bits, best, blocks, s);
  else if (nq <= 4)
    launch_scan_nq<4>(q, nq, rows, n, dim, codes, n_groups, bits, best, blocks, s);
  else if (nq <= 8)
    launch_scan_nq<8>(q, nq, rows, n, dim, codes, n_groups, bits, best, blocks, s);
  else
    launch_scan_nq<16>(q, nq, rows, n, dim, codes, n_groups, bits, best, blocks, s);
}

void launch_select(const unsigned long long* best, int n_groups, int nq, int k, float* cs, int64_t* ci, int blocks,
                   hipStream_t s) {
  const dim3 grid(blocks, nq);
  if (k <= 8)
    hipLaunchKernelGGL(group_select_kernel<8>, grid, dim3(256), 0, s, best, n_groups, nq, k, cs, ci);
  else if (k <= 16)
    hipLaunchKernelGGL(group_select_kernel<16>, grid, dim3(256), 0, s, best, n_groups, nq, k, cs, ci);
  else
    hipLaunchKernelGGL(group_select_kernel<64>, grid, dim3(256), 0, s, best, n_groups, nq, k, cs, ci);
}

}  // namespace

extern "C" {

int64_t mq_group_scratch_bytes(int64_t n_groups, int64_t nq, int k) { return group_layout(n_groups, nq, k).total; }

int mq_group_scan_blocks(int64_t n_rows, int compute_units) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(2 * (int64_t)std::max(compute_units, 1), (n_rows + 127) / 128));
}

int mq_debug_group_check(int dim, int64_t n_rows, const float* queries, int64_t nq, int k, const int32_t* codes,
                         int32_t n_groups, const float* out_scores, const int64_t* out_ids, const void* scratch,
                         int64_t scratch_bytes) {
  clear_error();
  return check_group_args(dim, n_rows, queries, nq, k, codes, n_groups, out_scores, out_ids, scratch, scratch_bytes);
}

int mq_index_search_grouped(mq_index* ix, const float* queries, int64_t nq, int k, const int32_t* codes,
                            int32_t n_groups, const uint32_t* bits, float* out_scores, int64_t* out_ids,
                            int io_on_device, void* scratch, int64_t scratch_bytes, void* stream) {
  clear_error();
  // the scalars first: they need no handle
  MQ_CHECK_ARG(k >= 1 && k <= MQ_MAX_K, "k must be in [1, %d] (got %d)", MQ_MAX_K, k);
  MQ_CHECK_ARG(nq >= 0 && nq <= (1ll << 24), "query count %lld out of range", (long long)nq);
  MQ_CHECK_ARG(n_groups >= 0, "n_groups must be >= 0 (got %d)", (int)n_groups);
  MQ_CHECK_ARG(ix, "NULL index");
  int64_t n = 0;
  int dim = 0;
  void* slab = nullptr;
  int rc = mq_index_size(ix, &n);
  if (!rc) rc = mq_index_dim(ix, &dim);
  if (!rc) rc = mq_index_data(ix, &slab);
  if (rc) return rc;
  rc = check_group_args(dim, n, queries, nq, k, codes, n_groups, out_scores, out_ids, scratch, scratch_bytes);
  if (rc || nq == 0) return rc;
  hipStream_t s = (hipStream_t)stream;

  if (n == 0 || n_groups == 0) {  // padding only
    if (!io_on_device) {
      for (int64_t i = 0; i < nq * k; ++i) {
        out_scores[i] = -INFINITY;
        out_ids[i] = -1;
      }
      return MQ_OK;
    }
    const int dev = pointer_device(out_scores);
    MQ_CHECK_ARG(dev >= 0 && pointer_device(out_ids) == dev, "the outputs must be device memory of one GPU");
    DeviceGuard dg(dev);
    hipLaunchKernelGGL(group_pad_kernel, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, s, out_scores, out_ids,
                       nq * k);
    MQ_HIP(hipGetLastError());
    return MQ_OK;
  }

  const int device = pointer_device(slab);
  if (device < 0) MQ_FAIL(MQ_ESTATE, "the index's row slab is not device memory");
  MQ_CHECK_ARG(pointer_device(codes) == device, "codes must be device memory of the index's GPU %d", device);
  MQ_CHECK_ARG(!bits || pointer_device(bits) == device, "the mask must be device memory of the index's GPU %d", device);
  MQ_CHECK_ARG(pointer_device(scratch) == device, "scratch must be device memory of the index's GPU %d", device);
  if (io_on_device)
    MQ_CHECK_ARG(pointer_device(queries) == device && pointer_device(out_scores) == device &&
                     pointer_device(out_ids) == device,
                 "queries and outputs must be device memory of the index's GPU %d", device);
  DeviceGuard dg(device);

  const GroupLayout l = group_layout(n_groups, nq, k);
  char* base = static_cast<char*>(scratch);
  unsigned long long* best = reinterpret_cast<unsigned long long*>(base + l.table);
  int64_t* cand_i = reinterpret_cast<int64_t*>(base + l.cand_i);
  float* cand_s = reinterpret_cast<float*>(base + l.cand_s);
  float* stage_q = reinterpret_cast<float*>(base + l.stage_q);
  int64_t* stage_i = reinterpret_cast<int64_t*>(base + l.stage_i);
  float* stage_s = reinterpret_cast<float*>(base + l.stage_s);
  const float* rows = static_cast<const float*>(slab);
  const int scan_blocks = mq_group_scan_blocks(n, num_cus(device));
  const int sel_blocks = select_blocks(n_groups);

  // successive passes of at most 16 queries reuse the table and the lists in stream order
  for (int64_t p0 = 0; p0 < nq; p0 += kGroupPassQ) {
    const int pq = (int)std::min<int64_t>(kGroupPassQ, nq - p0);
    const float* dq = queries + p0 * dim;
    float* dos = out_scores + p0 * k;
    int64_t* doi = out_ids + p0 * k;
    if (!io_on_device) {
      MQ_HIP(hipMemcpyAsync(stage_q, dq, (size_t)pq * dim * 4, hipMemcpyHostToDevice, s));
      dq = stage_q;
      dos = stage_s;
      doi = stage_i;
    }
    MQ_HIP(hipMemsetAsync(best, 0, (size_t)pq * n_groups * 8, s));
    launch_scan(dq, pq, rows, n, dim, codes, n_groups, bits, best, scan_blocks, s);
    MQ_HIP(hipGetLastError());
    launch_select(best, n_groups, pq, k, cand_s, cand_i, sel_blocks, s);
    MQ_HIP(hipGetLastError());
    rc = mq_topk_merge_device(cand_s, cand_i, sel_blocks, pq, k, k, dos, doi, stream);
    if (rc) return rc;
    if (!io_on_device) {
      MQ_HIP(hipMemcpyAsync(out_scores + p0 * k, stage_s, (size_t)pq * k * 4, hipMemcpyDeviceToHost, s));
      MQ_HIP(hipMemcpyAsync(out_ids + p0 * k, stage_i, (size_t)pq * k * 8, hipMemcpyDeviceToHost, s));
    }
  }
  if (!io_on_device) MQ_HIP(hipStreamSynchronize(s));
  return MQ_OK;
}

}  // extern "C"
