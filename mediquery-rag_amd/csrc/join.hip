// join.hip - K18: the self-join of the index, near-duplicate detection on the device
// (include/mq.h "Self-join", mq_index_self_join / mq_join_scratch_bytes).  For every left row i
// the partners are the admitted rows j != i with score(i, j) >= min_score, score being the exact
// fp32 score of the range search (score_chain.hpp); the call returns each left row's partner
// count, smallest partner and nearest partner.
//
// Two paths, the same answers:
//  exact   join_exact_kernel is the row walk of range.hip's range_score_kernel with up to 16
//          left rows staged in LDS from the slab by index.  Where that kernel writes a key, the
//          lane that owns (row, left j) keeps a running (count, first, best key) in registers;
//          each workgroup writes one partial per left row with plain stores and
//          join_finish_kernel folds the partials in a fixed order.  No atomics.
//  screen  (dim 256 / 512 / 768) panels of 256 left rows: join_tau_kernel gathers the panel's
//          bf16 rows from the index's bf16 shadow and sets tau = min_score - E, E the proven
//          bound on |score - bf16 MFMA score| below; K9t's appending scan (thresh.hip) lists
//          every (left, row) whose bf16 score clears tau - a superset of the partners;
//          join_verify_kernel recomputes the listed pairs with the exact chain.  A left row
//          with more than kTsCap survivors goes to a redo list, which the exact path serves
//          after the last panel: the one value the call reads back.
//
// This file reads the slab through the public ABI (mq_index_data, _size, _dim) and the shadow
// through index_shadow (common.hpp); it allocates no device memory.
#include <algorithm>
#include <atomic>
#include <cmath>

#include "score_chain.hpp"
#include "thresh.hpp"

namespace mq {

constexpr int kJoinPassQ = 16;      // left rows per pass of the exact walk
constexpr int kJoinPanel = 256;     // left rows per panel of the screen (K9t's query group)
constexpr int kJoinMaxNV = 16;      // 16-B loads per lane per row: dim <= 1024
constexpr int kJoinMaxDim = 64 * kJoinMaxNV;
constexpr int kJoinMaxBlocks = 1024;  // workgroups of the exact walk the partials are sized for
// MQ_JOIN_AUTO screens from this many rows on: the smallest index measured, where a
// panel of the screen already beats one pass of the exact walk (0.072 against 0.096 ms for 16 left
// rows at dim 256); no smaller index was timed, so below it AUTO keeps the walk
constexpr int64_t kJoinAutoMinRows = 1024;

// What one workgroup (exact walk) or one lane group (verify) knows about a left row.
struct JoinPartial {
  unsigned long long key;  // best chain_key of a partner, 0: none
  unsigned count;          // partners
  unsigned first;          // smallest partner row, 0xFFFFFFFF: none
};

__device__ __forceinline__ void join_fold(JoinPartial& a, const JoinPartial& b) {
  a.key = b.key > a.key ? b.key : a.key;
  a.count += b.count;
  a.first = b.first < a.first ? b.first : a.first;
}

__device__ __forceinline__ void join_write(const JoinPartial& p, int64_t pos, int64_t* __restrict__ out_counts,
                                           int64_t* __restrict__ out_first, int64_t* __restrict__ out_nearest,
                                           float* __restrict__ out_scores) {
  out_counts[pos] = (int64_t)p.count;
  out_first[pos] = p.count ? (int64_t)p.first : -1;
  out_nearest[pos] = p.count ? (int64_t)(0xFFFFFFFFu - (unsigned)p.key) : -1;
  out_scores[pos] = p.count ? chain_word_score((unsigned)(p.key >> 32)) : -INFINITY;
}

// Left row of position `pos` of the left list (NULL: the row `pos` itself), or -1 when it lies
// outside [0, n_rows) or the mask does not admit it: such a row is never read and has no partner.
__device__ __forceinline__ int64_t join_left_row(const int64_t* __restrict__ left_rows, int64_t pos, int64_t n_rows,
                                                 const unsigned* __restrict__ mask) {
  const int64_t r = left_rows ? left_rows[pos] : pos;
  if (r < 0 || r >= n_rows) return -1;
  if (mask && !((mask[r >> 5] >> (r & 31)) & 1u)) return -1;
  return r;
}

// Grid: blocks of 16 lane groups, lane group g walks rows g, g + G, ... two per iteration, as
// range_score_kernel.  Left j of the pass is position pos_list[p0 + j] of the left list
// (pos_list NULL: p0 + j).  part: [blocks][16]; workgroup b writes part[b][0 .. 15].
// Dynamic LDS: max(NQ x dim x 4, 4096) bytes - the staged left rows, then the workgroup's fold.
template <int NQ, int NV>
__global__ __launch_bounds__(256) void join_exact_kernel(const float* __restrict__ C, int64_t n_rows, int dim,
                                                         const unsigned* __restrict__ mask,
                                                         const int64_t* __restrict__ left_rows,
                                                         const int* __restrict__ pos_list, int64_t p0, int nq,
                                                         float min_score, JoinPartial* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float qs[];  // [NQ][dim], zeros for an absent left
  const int tid = threadIdx.x, gl = tid & 15;
  for (int j = 0; j < NQ; ++j) {
    int64_t lr = -1;
    if (j < nq) lr = join_left_row(left_rows, pos_list ? (int64_t)pos_list[p0 + j] : p0 + j, n_rows, mask);
    for (int i = tid; i < dim; i += 256) qs[j * dim + i] = lr >= 0 ? C[lr * dim + i] : 0.f;
  }
  // the left row this lane owns
  int64_t li = -1;
  if (gl < nq && gl < NQ) li = join_left_row(left_rows, pos_list ? (int64_t)pos_list[p0 + gl] : p0 + gl, n_rows, mask);
  __syncthreads();
  const int nv = NV == kJoinMaxNV ? dim / 64 : NV;  // NV < max: compiled for dim = 64 NV
  const int64_t group = (int64_t)blockIdx.x * 16 + (tid >> 4);
  const int64_t n_lane_groups = (int64_t)gridDim.x * 16;
  const float* qbase = qs + gl * 4;
  JoinPartial my{0ull, 0u, 0xFFFFFFFFu};

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
      if (u < nr && li >= 0) {
        const float s = mine + 0.0f;  // a -0.0 sum ranks as +0.0
        const bool here = (mw[u] >> (r & 31)) & 1u;
        if (here && r != li && s >= min_score) {
          const unsigned long long key = chain_key(chain_score_word(s), r);
          my.key = key > my.key ? key : my.key;
          my.count += 1u;
          my.first = (unsigned)r < my.first ? (unsigned)r : my.first;
        }
      }
    }
  }
  __syncthreads();  // every lane group is done with the staged rows
  JoinPartial* red = reinterpret_cast<JoinPartial*>(qs);  // [16 lane groups][16 lefts]
  red[tid] = my;
  __syncthreads();
  if (tid < 16) {
    JoinPartial p = red[tid];
    for (int g = 1; g < 16; ++g) join_fold(p, red[g * 16 + tid]);
    part[(size_t)blockIdx.x * 16 + tid] = p;
  }
}

// One workgroup: thread (g, j) folds the partials of workgroups g, g + 16, ... of left j, the 16
// of a left are folded in LDS, and thread j writes the four outputs of its position.
__global__ __launch_bounds__(256) void join_finish_kernel(const JoinPartial* __restrict__ part, int blocks,
                                                          const int* __restrict__ pos_list, int64_t p0, int nq,
                                                          int64_t* __restrict__ out_counts,
                                                          int64_t* __restrict__ out_first,
                                                          int64_t* __restrict__ out_nearest,
                                                          float* __restrict__ out_scores) {
  __shared__ JoinPartial red[256];
  const int tid = threadIdx.x, j = tid & 15;
  JoinPartial p{0ull, 0u, 0xFFFFFFFFu};
  for (int b = tid >> 4; b < blocks; b += 16) join_fold(p, part[(size_t)b * 16 + j]);
  red[tid] = p;
  __syncthreads();
  if (tid < nq) {
    JoinPartial t = red[tid];
    for (int g = 1; g < 16; ++g) join_fold(t, red[g * 16 + tid]);
    join_write(t, pos_list ? (int64_t)pos_list[p0 + tid] : p0 + tid, out_counts, out_first, out_nearest, out_scores);
  }
}

// The screen's threshold.  The screen score of (i, j) is K9t's: the bf16 rows bc_i, bc_j of the
// shadow multiplied on the MFMA with fp32 accumulation.  Against the exact score (the fp32 chain
// over the stored rows c_i, c_j):
//   c_i.c_j - bc_i.bc_j = (c_i - bc_i).c_j + bc_i.(c_j - bc_j), by Cauchy-Schwarz at most
//     ||c_i - bc_i|| ||c_j|| + ||bc_i|| ||c_j - bc_j|| <= d c + (c + d) d = 2 d c + d^2
//     with d = dmax >= ||c - bc|| and c = cmax >= ||c|| the shadow's measured maxima (stats16),
//     ||bc|| <= c + d;
//   the MFMA chain's fp32 accumulation over the rounded rows: <= g ||bc_i|| ||bc_j|| <= g (c + d)^2,
//     g = 2 dim 2^-24;
//   the exact chain's own accumulation: <= g ||c_i|| ||c_j|| <= g c^2.
// With d and c taken x 1.001 (slack for the fp32 evaluation of the norms and of this bound, as
// screen_bound in index.hip does):
//   E = (2 d c + d^2 + g (c + d)^2 + g c^2) * 1.001 + 1e-7,
// so score(i, j) >= min_score implies screen(i, j) >= min_score - E, and tau is that difference
// rounded down (one more ulp, whatever the subtraction's rounding).  A left row that is absent
// (outside the index or the mask) gets +inf: nothing survives.
// One wave per left row of the panel; the wave also copies the row's bf16 shadow into the
// panel's contiguous query block (the shadow's rows have the layout K9t reads its queries in).
__global__ __launch_bounds__(256) void join_tau_kernel(const unsigned char* __restrict__ rows16,
                                                       const unsigned* __restrict__ stats, int64_t n_rows, int dim,
                                                       const unsigned* __restrict__ mask,
                                                       const int64_t* __restrict__ left_rows, int64_t p0, int nq,
                                                       float min_score, uint2* __restrict__ q16,
                                                       float* __restrict__ tau) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  const int64_t lr = join_left_row(left_rows, p0 + q, n_rows, mask);
  const uint2* src = reinterpret_cast<const uint2*>(rows16 + (lr >= 0 ? lr : 0) * dim * 2);
  for (int i = lane; i < (dim >> 2); i += 64) q16[(size_t)q * (dim >> 2) + i] = src[i];
  if (lane == 0) {
    const float d = __uint_as_float(stats[0]) * 1.001f, c = __uint_as_float(stats[1]) * 1.001f;
    const float g = 2.f * (float)dim * 5.9604645e-8f;
    const float E = (2.f * d * c + d * d + g * (c + d) * (c + d) + g * c * c) * 1.001f + 1e-7f;
    float t = min_score - E;
    if (!isinf(t)) t -= fabsf(t) * 1.2e-7f + 1e-37f;
    tau[q] = lr >= 0 ? t : INFINITY;
  }
}

// One workgroup per left row of the panel.  More than kTsCap survivors: the list is incomplete,
// the position goes to the redo list and nothing is written.  Otherwise lane group g takes
// survivors g, g + 16, ...: row j from the slab against row i in LDS with the exact chain;
// j == i and pairs below min_score are dropped; the 16 lane groups' (count, first, best key)
// are folded in LDS and thread 0 writes the row's four outputs.
__global__ __launch_bounds__(256) void join_verify_kernel(const float* __restrict__ C, int64_t n_rows, int dim,
                                                          const unsigned* __restrict__ mask,
                                                          const int64_t* __restrict__ left_rows, int64_t p0,
                                                          float min_score, const int* __restrict__ count,
                                                          const int* __restrict__ ci, int* __restrict__ redo,
                                                          unsigned* __restrict__ redo_count,
                                                          unsigned long long* __restrict__ verified,
                                                          int64_t* __restrict__ out_counts,
                                                          int64_t* __restrict__ out_first,
                                                          int64_t* __restrict__ out_nearest,
                                                          float* __restrict__ out_scores) {
  extern __shared__ __attribute__((aligned(16))) float qi[];  // [dim]: row i
  __shared__ JoinPartial red[16];
  const int tid = threadIdx.x, gl = tid & 15, g = tid >> 4;
  const int q = blockIdx.x;
  const int64_t pos = p0 + q;
  const int cnt = count[q];
  if (cnt > kTsCap) {
    if (tid == 0) redo[atomicAdd(redo_count, 1u)] = (int)pos;
    return;
  }
  const int64_t li = join_left_row(left_rows, pos, n_rows, mask);
  JoinPartial my{0ull, 0u, 0xFFFFFFFFu};
  if (cnt <= 0 || li < 0) {  // (an absent left row has tau = +inf: no survivor)
    if (tid == 0) join_write(my, pos, out_counts, out_first, out_nearest, out_scores);
    return;
  }
  for (int i = tid; i < dim; i += 256) qi[i] = C[li * dim + i];
  __syncthreads();
  const int nv = dim / 64;
  const int* cq = ci + (size_t)q * kTsCap;
  for (int s = g; s < cnt; s += 16) {
    const int64_t j = cq[s];
    if (j < 0 || j >= n_rows) continue;  // (never: the scan lists stored rows only)
    const floatx4* rp = reinterpret_cast<const floatx4*>(C + j * dim) + gl;
    float acc = 0.f;
    for (int it = 0; it < nv; ++it)
      acc = chain_step(acc, rp[it * 16], *reinterpret_cast<const floatx4*>(qi + gl * 4 + it * 64));
    const float sc = chain_reduce16(acc) + 0.0f;
    if (j != li && sc >= min_score) {
      const unsigned long long key = chain_key(chain_score_word(sc), j);
      my.key = key > my.key ? key : my.key;
      my.count += 1u;
      my.first = (unsigned)j < my.first ? (unsigned)j : my.first;
    }
  }
  if (gl == 0) red[g] = my;
  __syncthreads();
  if (tid == 0) {
    JoinPartial p = red[0];
    for (int k = 1; k < 16; ++k) join_fold(p, red[k]);
    join_write(p, pos, out_counts, out_first, out_nearest, out_scores);
    atomicAdd(verified, (unsigned long long)cnt);
  }
}

// out_info: [0] the sum of the counts, [1] left rows the screen answered, [2] screen candidates
// verified, [3] left rows the exact walk answered.  One workgroup.
__global__ __launch_bounds__(256) void join_info_kernel(const int64_t* __restrict__ counts, int64_t n_left,
                                                        const unsigned long long* __restrict__ verified,
                                                        int64_t n_exact, int64_t* __restrict__ info) {
  __shared__ long long sums[256];
  const int tid = threadIdx.x;
  long long t = 0;
  for (int64_t i = tid; i < n_left; i += 256) t += counts[i];
  sums[tid] = t;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) sums[tid] += sums[tid + off];
    __syncthreads();
  }
  if (tid == 0) {
    info[0] = sums[0];
    info[1] = n_left - n_exact;
    info[2] = (int64_t)*verified;
    info[3] = n_exact;
  }
}

}  // namespace mq

using namespace mq;

namespace {

int64_t up256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// Sections of the scratch, each a multiple of 256 bytes: the screen's panel (bf16 left rows,
// tau, survivor counts and rows; K9t's survivor scores are written and not read), the counters
// the call zeroes once (redo count, verified candidates), the redo list, the exact walk's
// partials, and the staging of a host-pointer call (left rows in, the outputs and out_info back).
struct JoinLayout {
  int64_t q16, tau, count, cs, ci, ctr, redo, part, st_left, st_counts, st_first, st_nearest, st_scores, st_info,
      total;
};

JoinLayout join_layout(int64_t n, int64_t n_left) {
  n = std::min<int64_t>(std::max<int64_t>(n, 0), (1ll << 31) - 1);
  n_left = std::min<int64_t>(std::max<int64_t>(n_left, 0), (1ll << 31) - 1);
  const int64_t blocks = std::min<int64_t>(kJoinMaxBlocks, std::max<int64_t>(1, (n + 127) / 128));
  JoinLayout l;
  l.q16 = 0;
  l.tau = l.q16 + up256((int64_t)kJoinPanel * kJoinMaxDim * 2);
  l.count = l.tau + up256(kJoinPanel * 4);
  l.cs = l.count + up256(kJoinPanel * 4);
  l.ci = l.cs + up256((int64_t)kJoinPanel * kTsCap * 4);
  l.ctr = l.ci + up256((int64_t)kJoinPanel * kTsCap * 4);
  l.redo = l.ctr + 256;
  l.part = l.redo + up256(n_left * 4);
  l.st_left = l.part + up256(blocks * 16 * (int64_t)sizeof(JoinPartial));
  l.st_counts = l.st_left + up256(n_left * 8);
  l.st_first = l.st_counts + up256(n_left * 8);
  l.st_nearest = l.st_first + up256(n_left * 8);
  l.st_scores = l.st_nearest + up256(n_left * 8);
  l.st_info = l.st_scores + up256(n_left * 4);
  l.total = l.st_info + 256;
  return l;
}

bool overlaps(const void* a, int64_t ab, const void* b, int64_t bb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bb && b0 < a0 + (uintptr_t)ab;
}

bool screen_dim(int dim) { return dim == 256 || dim == 512 || dim == 768; }

// The checks of the scalars, which need neither a handle nor a shape.
int check_join_scalars(float min_score, int mode, int64_t n_left) {
  MQ_CHECK_ARG(!std::isnan(min_score), "min_score must not be NaN (-inf means no threshold)");
  MQ_CHECK_ARG(mode == MQ_JOIN_AUTO || mode == MQ_JOIN_EXACT || mode == MQ_JOIN_SCREEN,
               "mode must be MQ_JOIN_AUTO (%d), MQ_JOIN_EXACT (%d) or MQ_JOIN_SCREEN (%d) (got %d)", MQ_JOIN_AUTO,
               MQ_JOIN_EXACT, MQ_JOIN_SCREEN, mode);
  MQ_CHECK_ARG(n_left >= 0 && n_left < (1ll << 31), "left row count %lld out of range", (long long)n_left);
  return MQ_OK;
}

// Every check of mq_index_self_join that needs no HIP call, on the index's shape (dim, n rows).
int check_join_args(int dim, int64_t n, float min_score, int mode, const int64_t* left_rows, int64_t n_left,
                    const int64_t* out_counts, const int64_t* out_first, const int64_t* out_nearest,
                    const float* out_nearest_scores, const int64_t* out_info, const void* scratch,
                    int64_t scratch_bytes) {
  if (int rc = check_join_scalars(min_score, mode, n_left)) return rc;
  MQ_CHECK_ARG(dim > 0 && dim % 64 == 0 && dim <= kJoinMaxDim,
               "the self-join serves dim %% 64 == 0, dim <= %d (got %d)", kJoinMaxDim, dim);
  MQ_CHECK_ARG(mode != MQ_JOIN_SCREEN || screen_dim(dim), "MQ_JOIN_SCREEN serves dim 256, 512 or 768 (got %d)", dim);
  MQ_CHECK_ARG(n >= 0 && n < (1ll << 31), "the self-join serves fewer than 2^31 rows (got %lld)", (long long)n);
  MQ_CHECK_ARG(left_rows || n_left == n || n_left == 0, "n_left %lld must equal the index's %lld rows when left_rows is NULL",
               (long long)n_left, (long long)n);
  MQ_CHECK_ARG(out_info, "NULL out_info");
  if (n_left == 0 || n == 0) return MQ_OK;  // out_info alone: nothing else is read or written
  MQ_CHECK_ARG(out_counts && out_first && out_nearest && out_nearest_scores, "NULL output buffer");
  MQ_CHECK_ARG(scratch, "NULL scratch");
  MQ_CHECK_ARG((uintptr_t)scratch % 16 == 0, "scratch must be 16-byte aligned (got %p)", scratch);
  const int64_t need = join_layout(n, n_left).total;
  MQ_CHECK_ARG(scratch_bytes >= need, "scratch_bytes %lld is below the %lld bytes mq_join_scratch_bytes(%lld, %lld) asks",
               (long long)scratch_bytes, (long long)need, (long long)n, (long long)n_left);
  MQ_CHECK_ARG(!overlaps(scratch, scratch_bytes, out_counts, n_left * 8), "scratch overlaps out_counts (%p)",
               (const void*)out_counts);
  MQ_CHECK_ARG(!overlaps(scratch, scratch_bytes, out_first, n_left * 8), "scratch overlaps out_first (%p)",
               (const void*)out_first);
  MQ_CHECK_ARG(!overlaps(scratch, scratch_bytes, out_nearest, n_left * 8), "scratch overlaps out_nearest (%p)",
               (const void*)out_nearest);
  MQ_CHECK_ARG(!overlaps(scratch, scratch_bytes, out_nearest_scores, n_left * 4),
               "scratch overlaps out_nearest_scores (%p)", (const void*)out_nearest_scores);
  MQ_CHECK_ARG(!overlaps(scratch, scratch_bytes, out_info, 4 * 8), "scratch overlaps out_info (%p)",
               (const void*)out_info);
  if (left_rows)
    MQ_CHECK_ARG(!overlaps(scratch, scratch_bytes, left_rows, n_left * 8), "scratch overlaps left_rows (%p)",
                 (const void*)left_rows);
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

struct ExactArgs {
  const float* rows;
  int64_t n;
  int dim;
  const unsigned* bits;
  const int64_t* left;
  float min_score;
  JoinPartial* part;
  int blocks;
  int64_t *oc, *of, *on;
  float* os;
};

template <int NQ>
void launch_exact_nq(const ExactArgs& a, const int* pos_list, int64_t p0, int nq, hipStream_t s) {
  // the staged rows, then the workgroup's 4 KB fold; <= 64 KB: the default dynamic-LDS limit
  const size_t lds = std::max<size_t>((size_t)NQ * a.dim * sizeof(float), 256 * sizeof(JoinPartial));
  if (a.dim == 768)  // the BERT-base width, register arrays sized exactly
    hipLaunchKernelGGL((join_exact_kernel<NQ, 12>), dim3(a.blocks), dim3(256), lds, s, a.rows, a.n, a.dim, a.bits,
                       a.left, pos_list, p0, nq, a.min_score, a.part);
  else
    hipLaunchKernelGGL((join_exact_kernel<NQ, kJoinMaxNV>), dim3(a.blocks), dim3(256), lds, s, a.rows, a.n, a.dim,
                       a.bits, a.left, pos_list, p0, nq, a.min_score, a.part);
}

// One pass of the exact walk: lefts pos_list[p0 .. p0 + nq) (NULL: positions p0 ..), nq <= 16.
void launch_exact(const ExactArgs& a, const int* pos_list, int64_t p0, int nq, hipStream_t s) {
  if (nq <= 1)
    launch_exact_nq<1>(a, pos_list, p0, nq, s);
  else if (nq <= 2)
    launch_exact_nq<2>(a, pos_list, p0, nq, s);
  else if (nq <= 4)
    launch_exact_nq<4>(a, pos_list, p0, nq, s);
  else if (nq <= 8)
    launch_exact_nq<8>(a, pos_list, p0, nq, s);
  else
    launch_exact_nq<16>(a, pos_list, p0, nq, s);
  hipLaunchKernelGGL(join_finish_kernel, dim3(1), dim3(256), 0, s, a.part, a.blocks, pos_list, p0, nq, a.oc, a.of,
                     a.on, a.os);
}

}  // namespace

extern "C" {

int64_t mq_join_scratch_bytes(int64_t n_rows, int64_t n_left) { return join_layout(n_rows, n_left).total; }

int mq_debug_join_check(int dim, int64_t n_rows, float min_score, int mode, const int64_t* left_rows, int64_t n_left,
                        const int64_t* out_counts, const int64_t* out_first, const int64_t* out_nearest,
                        const float* out_nearest_scores, const int64_t* out_info, const void* scratch,
                        int64_t scratch_bytes) {
  clear_error();
  return check_join_args(dim, n_rows, min_score, mode, left_rows, n_left, out_counts, out_first, out_nearest,
                         out_nearest_scores, out_info, scratch, scratch_bytes);
}

int mq_index_self_join(mq_index* ix, float min_score, const uint32_t* bits, const int64_t* left_rows, int64_t n_left,
                       int mode, int64_t* out_counts, int64_t* out_first, int64_t* out_nearest,
                       float* out_nearest_scores, int64_t* out_info, int io_on_device, void* scratch,
                       int64_t scratch_bytes, void* stream) {
  clear_error();
  // the scalars first: they need no handle
  if (int rc = check_join_scalars(min_score, mode, n_left)) return rc;
  MQ_CHECK_ARG(ix, "NULL index");
  int64_t n = 0;
  int dim = 0;
  void* slab = nullptr;
  int rc = mq_index_size(ix, &n);
  if (!rc) rc = mq_index_dim(ix, &dim);
  if (!rc) rc = mq_index_data(ix, &slab);
  if (rc) return rc;
  rc = check_join_args(dim, n, min_score, mode, left_rows, n_left, out_counts, out_first, out_nearest,
                       out_nearest_scores, out_info, scratch, scratch_bytes);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;

  if (n == 0 || n_left == 0) {  // nothing to answer: out_info alone
    if (!io_on_device) {
      for (int i = 0; i < 4; ++i) out_info[i] = 0;
      return MQ_OK;
    }
    const int dev = pointer_device(out_info);
    MQ_CHECK_ARG(dev >= 0, "out_info must be device memory");
    DeviceGuard dg(dev);
    MQ_HIP(hipMemsetAsync(out_info, 0, 4 * 8, s));
    MQ_HIP(hipStreamSynchronize(s));
    return MQ_OK;
  }
  if (!io_on_device && left_rows)
    for (int64_t i = 0; i < n_left; ++i)
      MQ_CHECK_ARG(left_rows[i] >= 0 && left_rows[i] < n, "left_rows[%lld] = %lld is outside [0, %lld)", (long long)i,
                   (long long)left_rows[i], (long long)n);

  const int device = pointer_device(slab);
  if (device < 0) MQ_FAIL(MQ_ESTATE, "the index's row slab is not device memory");
  MQ_CHECK_ARG(!bits || pointer_device(bits) == device, "the mask must be device memory of the index's GPU %d", device);
  MQ_CHECK_ARG(pointer_device(scratch) == device, "scratch must be device memory of the index's GPU %d", device);
  if (io_on_device)
    MQ_CHECK_ARG((!left_rows || pointer_device(left_rows) == device) && pointer_device(out_counts) == device &&
                     pointer_device(out_first) == device && pointer_device(out_nearest) == device &&
                     pointer_device(out_nearest_scores) == device && pointer_device(out_info) == device,
                 "left_rows and outputs must be device memory of the index's GPU %d", device);
  DeviceGuard dg(device);

  const JoinLayout l = join_layout(n, n_left);
  char* base = static_cast<char*>(scratch);
  float* tau = reinterpret_cast<float*>(base + l.tau);
  int* count = reinterpret_cast<int*>(base + l.count);
  float* cs = reinterpret_cast<float*>(base + l.cs);
  int* ci = reinterpret_cast<int*>(base + l.ci);
  unsigned* redo_count = reinterpret_cast<unsigned*>(base + l.ctr);
  unsigned long long* verified = reinterpret_cast<unsigned long long*>(base + l.ctr + 8);
  int* redo = reinterpret_cast<int*>(base + l.redo);
  const float* rows = static_cast<const float*>(slab);

  const int64_t* d_left = left_rows;
  int64_t *oc = out_counts, *of = out_first, *on = out_nearest, *oi = out_info;
  float* os = out_nearest_scores;
  if (!io_on_device) {
    if (left_rows) {
      int64_t* st = reinterpret_cast<int64_t*>(base + l.st_left);
      MQ_HIP(hipMemcpyAsync(st, left_rows, (size_t)n_left * 8, hipMemcpyHostToDevice, s));
      d_left = st;
    }
    oc = reinterpret_cast<int64_t*>(base + l.st_counts);
    of = reinterpret_cast<int64_t*>(base + l.st_first);
    on = reinterpret_cast<int64_t*>(base + l.st_nearest);
    os = reinterpret_cast<float*>(base + l.st_scores);
    oi = reinterpret_cast<int64_t*>(base + l.st_info);
  }
  MQ_HIP(hipMemsetAsync(base + l.ctr, 0, 256, s));

  const int cus = num_cus(device);
  const int blocks = std::min(kJoinMaxBlocks, mq_range_scan_blocks(n, cus));
  const ExactArgs ea{rows, n, dim, bits, d_left, min_score, reinterpret_cast<JoinPartial*>(base + l.part), blocks,
                     oc, of, on, os};
  const bool screen = mode == MQ_JOIN_SCREEN || (mode == MQ_JOIN_AUTO && screen_dim(dim) && n >= kJoinAutoMinRows);
  int64_t n_exact = 0;
  if (screen) {
    ShadowView sv;
    rc = index_shadow(ix, s, &sv);
    if (rc) return rc;
    ThreshArgs ta{};
    ta.q16 = reinterpret_cast<const float*>(base + l.q16);
    ta.rows = sv.rows16;
    ta.n = n;
    ta.dim = dim;
    ta.num_cus = sv.num_cus;
    ta.tau = tau;
    ta.count = count;
    ta.cs = cs;
    ta.ci = ci;
    ta.mask = bits;
    for (int64_t p0 = 0; p0 < n_left; p0 += kJoinPanel) {
      const int pq = (int)std::min<int64_t>(kJoinPanel, n_left - p0);
      hipLaunchKernelGGL(join_tau_kernel, dim3((pq + 3) / 4), dim3(256), 0, s, sv.rows16, sv.stats16, n, dim, bits,
                         d_left, p0, pq, min_score, reinterpret_cast<uint2*>(base + l.q16), tau);
      MQ_HIP(hipGetLastError());
      ta.nq = pq;
      MQ_HIP(launch_thresh_append(ta, s));
      hipLaunchKernelGGL(join_verify_kernel, dim3(pq), dim3(256), (size_t)dim * sizeof(float), s, rows, n, dim, bits,
                         d_left, p0, min_score, count, ci, redo, redo_count, verified, oc, of, on, os);
      MQ_HIP(hipGetLastError());
    }
    // the one readback: how many left rows overflowed their survivor list
    unsigned n_redo = 0;
    MQ_HIP(hipMemcpyAsync(&n_redo, redo_count, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    MQ_HIP(hipStreamSynchronize(s));
    n_exact = std::min<int64_t>(n_redo, n_left);
    for (int64_t r0 = 0; r0 < n_exact; r0 += kJoinPassQ) {
      launch_exact(ea, redo, r0, (int)std::min<int64_t>(kJoinPassQ, n_exact - r0), s);
      MQ_HIP(hipGetLastError());
    }
  } else {
    n_exact = n_left;
    for (int64_t p0 = 0; p0 < n_left; p0 += kJoinPassQ) {
      launch_exact(ea, nullptr, p0, (int)std::min<int64_t>(kJoinPassQ, n_left - p0), s);
      MQ_HIP(hipGetLastError());
    }
  }
  hipLaunchKernelGGL(join_info_kernel, dim3(1), dim3(256), 0, s, oc, n_left, verified, n_exact, oi);
  MQ_HIP(hipGetLastError());
  if (!io_on_device) {
    MQ_HIP(hipMemcpyAsync(out_counts, oc, (size_t)n_left * 8, hipMemcpyDeviceToHost, s));
    MQ_HIP(hipMemcpyAsync(out_first, of, (size_t)n_left * 8, hipMemcpyDeviceToHost, s));
    MQ_HIP(hipMemcpyAsync(out_nearest, on, (size_t)n_left * 8, hipMemcpyDeviceToHost, s));
    MQ_HIP(hipMemcpyAsync(out_nearest_scores, os, (size_t)n_left * 4, hipMemcpyDeviceToHost, s));
    MQ_HIP(hipMemcpyAsync(out_info, oi, 4 * 8, hipMemcpyDeviceToHost, s));
  }
  MQ_HIP(hipStreamSynchronize(s));
  return MQ_OK;
}

}  // extern "C"
