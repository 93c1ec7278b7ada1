// kmeans.hip - K19: k-means clustering of the index, Lloyd iterations on the device
// (include/mq.h "K-means", mq_index_kmeans / mq_kmeans_scratch_bytes).
//
// An iteration is an update of the centroids from the labels and an assign of every admitted
// row to its nearest centroid:
//  half     kmeans_half_kernel: half_j = 0.5 score(c_j, c_j) with the chain of score_chain.hpp,
//           kept in memory for the assign.
//  assign   kmeans_assign_kernel is the row walk of range.hip's range_score_kernel with up to 16
//           centroids of a pass in LDS.  The lane that owns (row, j) forms the key
//           chain_key(chain_score_word((score - half_j) + 0.0f), j); the 16 keys of a row are
//           maximised over its lane group.  With more than 16 centroids the row's best key lives
//           in best[row] between the passes, and the winner's score in out_dots[row]; both are
//           written by the row's one lane group, so there are no atomics.  The last pass writes
//           the label and counts the rows whose label changed, one integer atomic per wave.
//  step     kmeans_step_kernel: changed == 0 sets the convergence flag, on which every later
//           launch of the call returns at once.
//  update   kmeans_partial_kernel, grid (row chunk b, cluster j): compacts the members of j in
//           the chunk in ascending row order (tiles of 1024 rows, a prefix sum over the
//           workgroup) and adds their rows in that order, every thread owning four coordinates;
//           kmeans_finish_kernel folds the chunks' partials in ascending b, divides and writes
//           the centroid.  The order of the sum is a function of (n, n_clusters, the labels):
//           no float atomics.
//  counts   kmeans_count_kernel / kmeans_info_kernel: the sizes of the final clusters (LDS
//           histograms, integer atomics) and out_info.
// Every hand-off is a kernel boundary on one stream; the launches are enqueued unconditionally
// and nothing is read back in between.
//
// This file talks to the index through its public ABI only (mq_index_data, _size, _dim) and
// allocates no device memory.
#include <algorithm>
#include <atomic>
#include <cmath>

#include "score_chain.hpp"

namespace mq {

constexpr int kKmPassQ = 16;       // centroids per pass: one per lane of a row's lane group
constexpr int kKmMaxNV = 16;       // 16-B loads per lane per row: dim <= 1024
constexpr int kKmMaxDim = 64 * kKmMaxNV;
constexpr int kKmMaxIter = 1024;
constexpr int kKmTile = 1024;      // rows one compaction of the partial kernel covers
constexpr int kKmMaxChunks = 1024; // row chunks per cluster at most (the finish kernel's LDS)
constexpr int kKmTargetBlocks = 8192;  // (cluster, chunk) workgroups of the partial kernel, about

// The device words of a call (zeroed on the stream when it begins).
struct KmState {
  unsigned changed;       // rows whose label changed in the assign that is running
  unsigned converged;     // some assign changed no label: later launches return at once
  unsigned updates;       // updates applied
  unsigned last_changed;  // `changed` of the last assign that ran
};

// One 16-lane group per centroid: half[j] = 0.5 score(c_j, c_j).
__global__ __launch_bounds__(256) void kmeans_half_kernel(const float* __restrict__ cent, int n_clusters, int dim,
                                                          const KmState* __restrict__ st,
                                                          float* __restrict__ half) {
  if (st->converged) return;
  const int gl = threadIdx.x & 15;
  const int nv = dim / 64;
  for (int j = threadIdx.x >> 4; j < n_clusters; j += 16) {
    const float* c = cent + (size_t)j * dim + gl * 4;
    float acc = 0.f;
    for (int it = 0; it < nv; ++it) {
      const floatx4 v = {c[it * 64], c[it * 64 + 1], c[it * 64 + 2], c[it * 64 + 3]};
      acc = chain_step(acc, v, v);
    }
    acc = chain_reduce16(acc);
    if (gl == 0) half[j] = 0.5f * acc;
  }
}

// Grid: blocks of 16 lane groups; lane group g walks rows g, g + G, g + 2G, ... (G = 16 x
// blocks), two per iteration, as range_score_kernel.  The pass serves centroids j0 .. j0 + nq - 1
// (nq <= NQ <= 16).  first: no earlier pass of this assign (best is not read); last: no later
// one (best is not written; labels, the masked rows' outputs and `changed` are).
template <int NQ, int NV>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const float* __restrict__ cent,
                                                            const float* __restrict__ half, int j0, int nq,
                                                            int first, int last, const float* __restrict__ C,
                                                            int64_t n_rows, int dim,
                                                            const unsigned* __restrict__ mask,
                                                            unsigned long long* __restrict__ best,
                                                            int32_t* __restrict__ assign, float* __restrict__ dots,
                                                            KmState* __restrict__ st) {
  extern __shared__ __attribute__((aligned(16))) float qs[];  // [NQ][dim], zero padded
  if (st->converged) return;
  const int tid = threadIdx.x, gl = tid & 15;
  const float* cj0 = cent + (size_t)j0 * dim;
  for (int i = tid; i < NQ * dim; i += 256) qs[i] = i < nq * dim ? cj0[i] : 0.f;
  const bool valid = gl < nq && gl < NQ;  // lane gl owns centroid j0 + gl
  const float hj = valid ? half[j0 + gl] : 0.f;
  __syncthreads();
  const int nv = NV == kKmMaxNV ? dim / 64 : NV;  // NV < max: compiled for dim = 64 NV
  const int64_t group = (int64_t)blockIdx.x * 16 + (tid >> 4);
  const int64_t n_lane_groups = (int64_t)gridDim.x * 16;
  const float* qbase = qs + gl * 4;
  unsigned chg = 0;

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
        for (int it = 0; it < NV; ++it)
          if (it < nv) acc = chain_step(acc, v[u][it], *reinterpret_cast<const floatx4*>(qj + it * 64));
        acc = chain_reduce16(acc);
        mine = gl == j ? acc : mine;
      }
      const int64_t r = r0 + u * n_lane_groups;
      const bool row = u < nr;  // uniform over the lane group, as `here` is
      const bool here = row && ((mw[u] >> (r & 31)) & 1u);
      // a valid lane's key is never 0 (its low word is 0xFFFFFFFF - j, j <= 255); the shuffles
      // run outside every branch
      const unsigned long long key = valid ? chain_key(chain_score_word((mine - hj) + 0.0f), j0 + gl) : 0ull;
      unsigned long long kmax = key;
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(kmax, off, 16);
        kmax = o > kmax ? o : kmax;
      }
      if (here) {
        const unsigned long long prev = first ? 0ull : best[r];
        if (valid && key == kmax && kmax > prev) {  // at most one lane: the keys of a row differ in j
          dots[r] = mine;
          if (!last) best[r] = kmax;
        }
        if (last && gl == 0) {
          const unsigned long long fin = kmax > prev ? kmax : prev;
          const int32_t label = (int32_t)(0xFFFFFFFFu - (unsigned)fin);
          chg += assign[r] != label;
          assign[r] = label;
        }
      } else if (row && last && gl == 0) {
        chg += assign[r] != -1;
        assign[r] = -1;
        dots[r] = -INFINITY;
      }
    }
  }
  if (last) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) chg += __shfl_xor(chg, off, 64);
    if ((tid & 63) == 0 && chg) atomicAdd(&st->changed, chg);
  }
}

// One thread, after the last pass of every assign.
__global__ void kmeans_step_kernel(KmState* __restrict__ st) {
  if (threadIdx.x != 0 || st->converged) return;
  const unsigned c = st->changed;
  st->last_changed = c;
  st->changed = 0;
  if (c == 0) st->converged = 1u;
}

// Grid (chunks, clusters).  Workgroup (b, j) owns rows [b x chunk, (b + 1) x chunk) and cluster
// j: per tile of 1024 rows, thread t reads the labels of rows 4t .. 4t + 3 of the tile, a prefix
// sum over the workgroup places the members of j in LDS in ascending row order, and thread t <
// dim / 4 adds coordinates 4t .. 4t + 3 of the members' rows in that order.  Writes
// pcount[j][b], and partial[j][b][dim] when the count is not 0.
__global__ __launch_bounds__(256) void kmeans_partial_kernel(const float* __restrict__ C, int64_t n_rows, int dim,
                                                             const int32_t* __restrict__ assign, int64_t chunk,
                                                             const KmState* __restrict__ st,
                                                             float* __restrict__ partial,
                                                             unsigned* __restrict__ pcount) {
  __shared__ int members[kKmTile];
  __shared__ int wsum[4];
  if (st->converged) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, j = blockIdx.y, n_chunks = gridDim.x;
  const int64_t lo = (int64_t)b * chunk, hi = lo + chunk < n_rows ? lo + chunk : n_rows;
  const bool owner = tid < dim / 4;
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  unsigned total = 0;
  for (int64_t t0 = lo; t0 < hi; t0 += kKmTile) {
    bool is[4];
    int mine = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t r = t0 + tid * 4 + k;
      is[k] = r < hi && assign[r] == j;
      mine += is[k];
    }
    int incl = mine;  // inclusive prefix over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = incl - mine, cnt = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      before += w < wave ? wsum[w] : 0;
      cnt += wsum[w];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (is[k]) members[before++] = (int)(t0 + tid * 4 + k);
    __syncthreads();
    if (owner) {
      int m = 0;
      for (; m + 4 <= cnt; m += 4) {
        floatx4 x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          x[k] = __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(C + (int64_t)members[m + k] * dim) + tid);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += x[k];
      }
      for (; m < cnt; ++m)
        acc += __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(C + (int64_t)members[m] * dim) + tid);
    }
    total += (unsigned)cnt;
    __syncthreads();  // the list and the wave sums are rewritten by the next tile
  }
  const size_t cell = (size_t)j * n_chunks + b;
  if (tid == 0) pcount[cell] = total;
  if (owner && total) reinterpret_cast<floatx4*>(partial + cell * dim)[tid] = acc;
}

// One workgroup per cluster: thread t < dim / 4 folds coordinates 4t .. 4t + 3 of the chunks'
// partials in ascending b (chunks without a member are skipped), divides by the count (one
// IEEE division) and writes the centroid; an empty cluster's centroid is not touched.
__global__ __launch_bounds__(256) void kmeans_finish_kernel(const float* __restrict__ partial,
                                                            const unsigned* __restrict__ pcount, int n_chunks,
                                                            int dim, KmState* __restrict__ st,
                                                            float* __restrict__ cent) {
  __shared__ unsigned pc[kKmMaxChunks];
  if (st->converged) return;
  const int tid = threadIdx.x, j = blockIdx.x;
  for (int i = tid; i < n_chunks; i += 256) pc[i] = pcount[(size_t)j * n_chunks + i];
  __syncthreads();
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  unsigned total = 0;
  const bool owner = tid < dim / 4;
  const floatx4* pj = reinterpret_cast<const floatx4*>(partial + (size_t)j * n_chunks * dim) + tid;
  for (int b = 0; b < n_chunks; ++b) {
    if (pc[b] == 0) continue;
    total += pc[b];
    if (owner) acc += pj[(size_t)b * (dim / 4)];
  }
  if (owner && total) {
    const float cnt = (float)total;
    float* c = cent + (size_t)j * dim + tid * 4;
    c[0] = __fdiv_rn(acc.x, cnt);
    c[1] = __fdiv_rn(acc.y, cnt);
    c[2] = __fdiv_rn(acc.z, cnt);
    c[3] = __fdiv_rn(acc.w, cnt);
  }
  if (j == 0 && tid == 0) st->updates += 1u;
}

// counts32[256] (zero when the call begins) += the labels' histogram.
__global__ __launch_bounds__(256) void kmeans_count_kernel(const int32_t* __restrict__ assign, int64_t n_rows,
                                                           unsigned* __restrict__ counts32) {
  static_assert(MQ_KMEANS_MAX_CLUSTERS == 256, "one bin per thread");
  __shared__ unsigned bins[MQ_KMEANS_MAX_CLUSTERS];
  const int tid = threadIdx.x;
  bins[tid] = 0;
  __syncthreads();
  for (int64_t r = (int64_t)blockIdx.x * 256 + tid; r < n_rows; r += (int64_t)gridDim.x * 256) {
    const int32_t a = assign[r];
    if (a >= 0 && a < MQ_KMEANS_MAX_CLUSTERS) atomicAdd(&bins[a], 1u);
  }
  __syncthreads();
  if (bins[tid]) atomicAdd(&counts32[tid], bins[tid]);
}

// One workgroup: out_counts and out_info.  counts32 / st NULL: an empty index.
__global__ __launch_bounds__(256) void kmeans_info_kernel(const unsigned* __restrict__ counts32,
                                                          const KmState* __restrict__ st, int n_clusters,
                                                          int64_t* __restrict__ out_counts,
                                                          int64_t* __restrict__ info) {
  __shared__ long long sums[256];
  __shared__ int empties[256];
  const int tid = threadIdx.x;
  const unsigned c = (counts32 && tid < n_clusters) ? counts32[tid] : 0u;
  if (tid < n_clusters) out_counts[tid] = (int64_t)c;
  sums[tid] = c;
  empties[tid] = tid < n_clusters && c == 0;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      sums[tid] += sums[tid + off];
      empties[tid] += empties[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    info[0] = st ? (int64_t)st->updates : 0;
    info[1] = st ? (int64_t)st->last_changed : 0;
    info[2] = sums[0];
    info[3] = empties[0];
  }
}

}  // namespace mq

using namespace mq;

namespace {

int64_t up256(int64_t b) { return (b + 255) & ~(int64_t)255; }

int64_t clamp_rows(int64_t n) { return std::min<int64_t>(std::max<int64_t>(n, 0), (1ll << 31) - 1); }
int clamp_clusters(int64_t c) { return (int)std::min<int64_t>(std::max<int64_t>(c, 1), MQ_KMEANS_MAX_CLUSTERS); }

// The update's geometry: rows per chunk (a multiple of 256) and chunks, a function of (n,
// n_clusters) alone.  About kKmTargetBlocks (cluster, chunk) workgroups, at most kKmMaxChunks
// chunks, at least 256 rows each.
void update_geometry(int64_t n, int n_clusters, int64_t* chunk, int* n_chunks) {
  const int64_t max_chunks = std::min<int64_t>(kKmMaxChunks, kKmTargetBlocks / n_clusters);
  int64_t rows = std::max<int64_t>(256, (n + max_chunks - 1) / max_chunks);
  rows = (rows + 255) & ~(int64_t)255;
  *chunk = rows;
  *n_chunks = (int)std::max<int64_t>(1, (n + rows - 1) / rows);
}

// Sections of the scratch, each a multiple of 256 bytes: the words the call zeroes when it
// begins (state, the final histogram), the halves, the rows' best keys, the update's partial
// sums and counts (sized for dim 1024 and an upper bound of clusters x chunks that is
// non-decreasing in both arguments), and the staging of a host-pointer call.
struct KmLayout {
  int64_t state, counts32, zero_end, half, best, pcount, partial, st_cent, st_assign, st_dots, st_counts, st_info,
      total;
};

KmLayout kmeans_layout(int64_t n, int64_t n_clusters) {
  n = clamp_rows(n);
  const int64_t c = clamp_clusters(n_clusters);
  // clusters x chunks <= this, whatever update_geometry picks
  const int64_t cells =
      std::max<int64_t>(1, std::min<int64_t>(c * std::min<int64_t>(kKmMaxChunks, (n + 255) / 256), kKmTargetBlocks));
  KmLayout l;
  l.state = 0;
  l.counts32 = l.state + 256;
  l.zero_end = l.counts32 + up256(MQ_KMEANS_MAX_CLUSTERS * 4);
  l.half = l.zero_end;
  l.best = l.half + up256(MQ_KMEANS_MAX_CLUSTERS * 4);
  l.pcount = l.best + up256(n * 8);
  l.partial = l.pcount + up256(cells * 4);
  l.st_cent = l.partial + up256(cells * kKmMaxDim * 4);
  l.st_assign = l.st_cent + up256(c * kKmMaxDim * 4);
  l.st_dots = l.st_assign + up256(n * 4);
  l.st_counts = l.st_dots + up256(n * 4);
  l.st_info = l.st_counts + up256(c * 8);
  l.total = l.st_info + 256;
  return l;
}

bool overlaps(const void* a, int64_t ab, const void* b, int64_t bb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bb && b0 < a0 + (uintptr_t)ab;
}

// The checks of the scalars, which need neither a handle nor a shape.
int check_kmeans_scalars(int n_clusters, int n_iter) {
  MQ_CHECK_ARG(n_clusters >= 1 && n_clusters <= MQ_KMEANS_MAX_CLUSTERS, "n_clusters must be in [1, %d] (got %d)",
               MQ_KMEANS_MAX_CLUSTERS, n_clusters);
  MQ_CHECK_ARG(n_iter >= 0 && n_iter <= kKmMaxIter, "n_iter must be in [0, %d] (got %d)", kKmMaxIter, n_iter);
  return MQ_OK;
}

// Every check of mq_index_kmeans that needs no HIP call, on the index's shape (dim, n rows).
int check_kmeans_args(int dim, int64_t n, int n_clusters, int n_iter, const float* centroids,
                      const int32_t* out_assign, const float* out_dots, const int64_t* out_counts,
                      const int64_t* out_info, int io_on_device, const void* scratch, int64_t scratch_bytes) {
  if (int rc = check_kmeans_scalars(n_clusters, n_iter)) return rc;
  MQ_CHECK_ARG(dim > 0 && dim % 64 == 0 && dim <= kKmMaxDim, "k-means serves dim %% 64 == 0, dim <= %d (got %d)",
               kKmMaxDim, dim);
  MQ_CHECK_ARG(n >= 0 && n < (1ll << 31), "k-means serves fewer than 2^31 rows (got %lld)", (long long)n);
  MQ_CHECK_ARG(centroids, "NULL centroids");
  MQ_CHECK_ARG(out_counts && out_info, "NULL output buffer");
  MQ_CHECK_ARG(n == 0 || (out_assign && out_dots), "NULL output buffer");
  if (n > 0) {  // an empty index: zero counts and out_info only, the scratch is not read
    MQ_CHECK_ARG(scratch, "NULL scratch");
    MQ_CHECK_ARG((uintptr_t)scratch % 16 == 0, "scratch must be 16-byte aligned (got %p)", scratch);
    const int64_t need = kmeans_layout(n, n_clusters).total;
    MQ_CHECK_ARG(scratch_bytes >= need, "scratch_bytes %lld is below the %lld bytes mq_kmeans_scratch_bytes(%lld, %d) asks",
                 (long long)scratch_bytes, (long long)need, (long long)n, n_clusters);
    MQ_CHECK_ARG(!overlaps(scratch, scratch_bytes, centroids, (int64_t)n_clusters * dim * 4),
                 "scratch overlaps centroids (%p)", (const void*)centroids);
    MQ_CHECK_ARG(!overlaps(scratch, scratch_bytes, out_assign, n * 4), "scratch overlaps out_assign (%p)",
                 (const void*)out_assign);
    MQ_CHECK_ARG(!overlaps(scratch, scratch_bytes, out_dots, n * 4), "scratch overlaps out_dots (%p)",
                 (const void*)out_dots);
    MQ_CHECK_ARG(!overlaps(scratch, scratch_bytes, out_counts, (int64_t)n_clusters * 8),
                 "scratch overlaps out_counts (%p)", (const void*)out_counts);
    MQ_CHECK_ARG(!overlaps(scratch, scratch_bytes, out_info, 4 * 8), "scratch overlaps out_info (%p)",
                 (const void*)out_info);
  }
  if (!io_on_device)
    for (int64_t i = 0; i < (int64_t)n_clusters * dim; ++i)
      MQ_CHECK_ARG(std::isfinite(centroids[i]), "centroids[%lld][%lld] = %g is not finite", (long long)(i / dim),
                   (long long)(i % dim), (double)centroids[i]);
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

struct AssignArgs {
  const float* cent;
  const float* half;
  int n_clusters;
  const float* rows;
  int64_t n;
  int dim;
  const unsigned* bits;
  unsigned long long* best;
  int32_t* assign;
  float* dots;
  KmState* st;
  int blocks;
};

template <int NQ>
void launch_pass_nq(const AssignArgs& a, int j0, int nq, int first, int last, hipStream_t s) {
  const size_t lds = (size_t)NQ * a.dim * sizeof(float);  // <= 64 KB: the default dynamic-LDS limit
  if (a.dim == 768)  // the BERT-base width, register arrays sized exactly
    hipLaunchKernelGGL((kmeans_assign_kernel<NQ, 12>), dim3(a.blocks), dim3(256), lds, s, a.cent, a.half, j0, nq,
                       first, last, a.rows, a.n, a.dim, a.bits, a.best, a.assign, a.dots, a.st);
  else
    hipLaunchKernelGGL((kmeans_assign_kernel<NQ, kKmMaxNV>), dim3(a.blocks), dim3(256), lds, s, a.cent, a.half, j0,
                       nq, first, last, a.rows, a.n, a.dim, a.bits, a.best, a.assign, a.dots, a.st);
}

// half, then ceil(n_clusters / 16) passes of the walk, then the step.
void launch_assign(const AssignArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(kmeans_half_kernel, dim3(1), dim3(256), 0, s, a.cent, a.n_clusters, a.dim, a.st,
                     const_cast<float*>(a.half));
  for (int j0 = 0; j0 < a.n_clusters; j0 += kKmPassQ) {
    const int nq = std::min(kKmPassQ, a.n_clusters - j0);
    const int first = j0 == 0, last = j0 + nq == a.n_clusters;
    if (nq <= 1)
      launch_pass_nq<1>(a, j0, nq, first, last, s);
    else if (nq <= 2)
      launch_pass_nq<2>(a, j0, nq, first, last, s);
    else if (nq <= 4)
      launch_pass_nq<4>(a, j0, nq, first, last, s);
    else if (nq <= 8)
      launch_pass_nq<8>(a, j0, nq, first, last, s);
    else
      launch_pass_nq<16>(a, j0, nq, first, last, s);
  }
  hipLaunchKernelGGL(kmeans_step_kernel, dim3(1), dim3(64), 0, s, a.st);
}

}  // namespace

extern "C" {

int64_t mq_kmeans_scratch_bytes(int64_t n_rows, int n_clusters) { return kmeans_layout(n_rows, n_clusters).total; }

int mq_debug_kmeans_check(int dim, int64_t n_rows, int n_clusters, int n_iter, const float* centroids,
                          const int32_t* out_assign, const float* out_dots, const int64_t* out_counts,
                          const int64_t* out_info, int io_on_device, const void* scratch, int64_t scratch_bytes) {
  clear_error();
  return check_kmeans_args(dim, n_rows, n_clusters, n_iter, centroids, out_assign, out_dots, out_counts, out_info,
                           io_on_device, scratch, scratch_bytes);
}

int mq_index_kmeans(mq_index* ix, const uint32_t* bits, int n_clusters, int n_iter, float* centroids,
                    int32_t* out_assign, float* out_dots, int64_t* out_counts, int64_t* out_info, int io_on_device,
                    void* scratch, int64_t scratch_bytes, void* stream) {
  clear_error();
  // the scalars first: they need no handle
  if (int rc = check_kmeans_scalars(n_clusters, n_iter)) return rc;
  MQ_CHECK_ARG(ix, "NULL index");
  int64_t n = 0;
  int dim = 0;
  void* slab = nullptr;
  int rc = mq_index_size(ix, &n);
  if (!rc) rc = mq_index_dim(ix, &dim);
  if (!rc) rc = mq_index_data(ix, &slab);
  if (rc) return rc;
  rc = check_kmeans_args(dim, n, n_clusters, n_iter, centroids, out_assign, out_dots, out_counts, out_info,
                         io_on_device, scratch, scratch_bytes);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;

  if (n == 0) {  // no row: zero counts, every cluster empty, the centroids untouched
    if (!io_on_device) {
      for (int j = 0; j < n_clusters; ++j) out_counts[j] = 0;
      out_info[0] = out_info[1] = out_info[2] = 0;
      out_info[3] = n_clusters;
      return MQ_OK;
    }
    const int dev = pointer_device(out_info);
    MQ_CHECK_ARG(dev >= 0 && pointer_device(out_counts) == dev, "the outputs must be device memory of one GPU");
    DeviceGuard dg(dev);
    hipLaunchKernelGGL(kmeans_info_kernel, dim3(1), dim3(256), 0, s, (const unsigned*)nullptr,
                       (const KmState*)nullptr, n_clusters, out_counts, out_info);
    MQ_HIP(hipGetLastError());
    return MQ_OK;
  }

  const int device = pointer_device(slab);
  if (device < 0) MQ_FAIL(MQ_ESTATE, "the index's row slab is not device memory");
  MQ_CHECK_ARG(!bits || pointer_device(bits) == device, "the mask must be device memory of the index's GPU %d", device);
  MQ_CHECK_ARG(pointer_device(scratch) == device, "scratch must be device memory of the index's GPU %d", device);
  if (io_on_device)
    MQ_CHECK_ARG(pointer_device(centroids) == device && pointer_device(out_assign) == device &&
                     pointer_device(out_dots) == device && pointer_device(out_counts) == device &&
                     pointer_device(out_info) == device,
                 "centroids and outputs must be device memory of the index's GPU %d", device);
  DeviceGuard dg(device);

  const KmLayout l = kmeans_layout(n, n_clusters);
  char* base = static_cast<char*>(scratch);
  KmState* st = reinterpret_cast<KmState*>(base + l.state);
  unsigned* counts32 = reinterpret_cast<unsigned*>(base + l.counts32);
  float* half = reinterpret_cast<float*>(base + l.half);
  unsigned long long* best = reinterpret_cast<unsigned long long*>(base + l.best);
  unsigned* pcount = reinterpret_cast<unsigned*>(base + l.pcount);
  float* partial = reinterpret_cast<float*>(base + l.partial);
  const float* rows = static_cast<const float*>(slab);

  float* cent = centroids;
  int32_t* oa = out_assign;
  float* od = out_dots;
  int64_t *oc = out_counts, *oi = out_info;
  if (!io_on_device) {
    cent = reinterpret_cast<float*>(base + l.st_cent);
    oa = reinterpret_cast<int32_t*>(base + l.st_assign);
    od = reinterpret_cast<float*>(base + l.st_dots);
    oc = reinterpret_cast<int64_t*>(base + l.st_counts);
    oi = reinterpret_cast<int64_t*>(base + l.st_info);
    MQ_HIP(hipMemcpyAsync(cent, centroids, (size_t)n_clusters * dim * 4, hipMemcpyHostToDevice, s));
  }
  MQ_HIP(hipMemsetAsync(base + l.state, 0, (size_t)(l.zero_end - l.state), s));
  MQ_HIP(hipMemsetAsync(oa, 0xFF, (size_t)n * 4, s));  // a_{-1} = -1

  const int cus = num_cus(device);
  int64_t chunk = 0;
  int n_chunks = 0;
  update_geometry(n, n_clusters, &chunk, &n_chunks);
  const AssignArgs aa{cent, half, n_clusters, rows, n, dim, bits, best, oa, od, st, mq_range_scan_blocks(n, cus)};

  launch_assign(aa, s);
  MQ_HIP(hipGetLastError());
  for (int t = 0; t < n_iter; ++t) {
    hipLaunchKernelGGL(kmeans_partial_kernel, dim3(n_chunks, n_clusters), dim3(256), 0, s, rows, n, dim, oa, chunk, st,
                       partial, pcount);
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3(n_clusters), dim3(256), 0, s, partial, pcount, n_chunks, dim, st,
                       cent);
    launch_assign(aa, s);
    MQ_HIP(hipGetLastError());
  }
  const int count_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(cus, (n + 4095) / 4096));
  hipLaunchKernelGGL(kmeans_count_kernel, dim3(count_blocks), dim3(256), 0, s, oa, n, counts32);
  hipLaunchKernelGGL(kmeans_info_kernel, dim3(1), dim3(256), 0, s, counts32, st, n_clusters, oc, oi);
  MQ_HIP(hipGetLastError());
  if (!io_on_device) {
    MQ_HIP(hipMemcpyAsync(centroids, cent, (size_t)n_clusters * dim * 4, hipMemcpyDeviceToHost, s));
    MQ_HIP(hipMemcpyAsync(out_assign, oa, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    MQ_HIP(hipMemcpyAsync(out_dots, od, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    MQ_HIP(hipMemcpyAsync(out_counts, oc, (size_t)n_clusters * 8, hipMemcpyDeviceToHost, s));
    MQ_HIP(hipMemcpyAsync(out_info, oi, 4 * 8, hipMemcpyDeviceToHost, s));
    MQ_HIP(hipStreamSynchronize(s));
  }
  return MQ_OK;
}

}  // extern "C"
