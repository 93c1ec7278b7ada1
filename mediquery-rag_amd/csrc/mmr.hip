// mmr.hip - K11: maximal-marginal-relevance selection on the device (include/mq.h,
// mq_index_mmr_select / mq_index_search_mmr).
//
// One workgroup (4 waves) per query.  The candidate rows are gathered from the slab in
// 128-float K-slices (register staged, double-buffered LDS image of 528-B rows), the
// fetch_k x fetch_k Gram matrix is accumulated on v_mfma_f32_32x32x2_f32 (exact fp32), and
// wave 0 then runs LangChain's greedy loop with lane i owning candidate i.  Nothing
// row-sized leaves HBM.
//
// This file talks to the index through its public ABI only (mq_index_search*, _data, _size,
// _dim): the top-fetch_k lists of mq_index_search_mmr live in a grow-only workspace kept
// per index handle here.
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "common.hpp"

namespace mq {

constexpr int kMmrBK = 128;             // floats per staged K-slice (one 32-float chunk per wave)
constexpr int kMmrStride = kMmrBK + 4;  // 528-B LDS rows: 16 rows of a ds_read_b128 hit distinct 16-B slots

// NB = blocks of 32 candidates (fetch_k <= 32: one 32 x 32 Gram block; else the three
// blocks (0,0), (0,1), (1,1) of the 64 x 64 matrix; (1,0) is (0,1) read transposed)
template <int NB>
struct MmrGeom {
  static constexpr int ROWS = 32 * NB;
  static constexpr int STAGE = ROWS * kMmrStride;              // floats per staged slice
  static constexpr int LOADS = ROWS * (kMmrBK / 4) / 256;      // float4 per thread per slice
  static constexpr int NBLK = NB == 1 ? 1 : 3;                 // 32 x 32 accumulators per wave
  static constexpr size_t LDS = (size_t)(2 * STAGE + ROWS * ROWS) * 4 + 64 * 8 + 64 * 4;
};

// Gram phase: slice j holds k = 128 j .. 128 j + 127 of every candidate row (zeros for
// padding candidates and past dim).  Wave w multiplies the slice's chunk k = 32 w .. 32 w + 31
// (lane half h carries k = 16 h + 4 q + s at MFMA step (q, s), the same fragments as both
// operands), so each wave holds the fmaf chain over its own k; the four chains are then
// added in wave order ((w0 + w1) + w2) + w3.  Every step of a diagonal block takes its A and
// B values from the same registers, so G[i][j] and G[j][i] there see the same products in
// the same order; off the diagonal only block (0,1) exists and serves both: the matrix is
// symmetric bit for bit.  A chunk at or past dim is skipped whole (dim % 32 == 0), so a
// partial last slice adds nothing.
template <int NB>
__global__ __launch_bounds__(256) void mmr_select_kernel(const float* __restrict__ rows, int64_t n, int dim,
                                                         const int64_t* __restrict__ cand_ids,
                                                         const float* __restrict__ cand_scores, int fetch_k,
                                                         int k, float lambda, int64_t* __restrict__ out_ids,
                                                         float* __restrict__ out_scores) {
  using Gm = MmrGeom<NB>;
  constexpr int ROWS = Gm::ROWS;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* stage = smem;
  float* G = smem + 2 * Gm::STAGE;
  int64_t* sid = reinterpret_cast<int64_t*>(G + ROWS * ROWS);
  float* ssc = reinterpret_cast<float*>(sid + 64);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t q = blockIdx.x;

  // candidate list: an id outside [0, n) is padding (never read, never picked)
  if (tid < 64) {
    int64_t id = -1;
    float sc = -INFINITY;
    if (tid < fetch_k) {
      id = cand_ids[q * fetch_k + tid];
      sc = cand_scores[q * fetch_k + tid];
    }
    if (id < 0 || id >= n) id = -1;
    sid[tid] = id;
    ssc[tid] = sc;
  }
  __syncthreads();

  // thread (tid >> 5, tid & 31) stages float4 `ch` of rows (tid >> 5) + 8 i
  const int ch = tid & 31, r0 = tid >> 5;
  const float* rp[Gm::LOADS];
#pragma unroll
  for (int i = 0; i < Gm::LOADS; ++i) {
    const int64_t id = sid[r0 + 8 * i];
    rp[i] = id >= 0 ? rows + id * dim + ch * 4 : nullptr;
  }
  auto fetch = [&](floatx4(&r)[Gm::LOADS], int k0) {
    const bool in = k0 + ch * 4 < dim;
#pragma unroll
    for (int i = 0; i < Gm::LOADS; ++i) {
      r[i] = floatx4{0.f, 0.f, 0.f, 0.f};
      if (in && rp[i]) r[i] = *reinterpret_cast<const floatx4*>(rp[i] + k0);
    }
  };
  auto store = [&](const floatx4(&r)[Gm::LOADS], float* st) {
#pragma unroll
    for (int i = 0; i < Gm::LOADS; ++i)
      *reinterpret_cast<floatx4*>(st + (r0 + 8 * i) * kMmrStride + ch * 4) = r[i];
  };

  floatx16 acc[Gm::NBLK];
#pragma unroll
  for (int b = 0; b < Gm::NBLK; ++b)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[b][e] = 0.f;

  auto mma = [&](const float* st, int k0) {
    if (k0 + 32 * wave >= dim) return;  // wave-uniform: this chunk lies past the rows' end
    const float* ap = st + (lane & 31) * kMmrStride + 32 * wave + 16 * (lane >> 5);
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const floatx4 a0 = *reinterpret_cast<const floatx4*>(ap + 4 * qq);
      floatx4 a1 = a0;
      if constexpr (NB == 2) a1 = *reinterpret_cast<const floatx4*>(ap + 32 * kMmrStride + 4 * qq);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], a0[s], acc[0], 0, 0, 0);
        if constexpr (NB == 2) {
          acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], a1[s], acc[1], 0, 0, 0);
          acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], a1[s], acc[2], 0, 0, 0);
        }
      }
    }
  };

  const int ns = (dim + kMmrBK - 1) / kMmrBK;
  floatx4 r[Gm::LOADS];
  fetch(r, 0);
  store(r, stage);
  __syncthreads();
  for (int j = 0; j < ns; ++j) {
    const bool more = j + 1 < ns;
    if (more) fetch(r, (j + 1) * kMmrBK);  // in flight under this slice's MFMAs
    mma(stage + (j & 1) * Gm::STAGE, j * kMmrBK);
    if (more) store(r, stage + ((j + 1) & 1) * Gm::STAGE);
    __syncthreads();
  }

  // G = ((w0 + w1) + w2) + w3, one wave per round; accumulator register e of a lane is
  // row (e & 3) + 8 (e >> 2) + 4 (lane >> 5), column lane & 31 of its block
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
      auto put = [&](int i, int j, float v) {
        float* g = G + i * ROWS + j;
        *g = w ? *g + v : v;
      };
      const int col = lane & 31;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        put(row, col, acc[0][e]);
        if constexpr (NB == 2) {  // block (1,0) is never stored: its readers take (0,1) transposed
          put(row, 32 + col, acc[1][e]);
          put(32 + row, 32 + col, acc[2][e]);
        }
      }
    }
    __syncthreads();
  }

  // Greedy phase, wave 0: lane i owns candidate i, red_i lives in a register.
  if (wave != 0) return;
  const float s = ssc[lane];
  bool avail = sid[lane] >= 0;
  float red = -INFINITY;
  int t = 0;
  for (; t < k; ++t) {
    // the first pick is the most similar candidate; then MQ_MMR_SCORE, uncontracted
    float bv = t == 0 ? s : MQ_MMR_SCORE(__fmul_rn, __fsub_rn, lambda, s, red);
    int bi = avail ? lane : 64;
    // wave argmax on (score desc, list position asc); 64 = no candidate
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      if (oi < 64 && (bi >= 64 || ov > bv || (!(bv > ov) && oi < bi))) {
        bv = ov;
        bi = oi;
      }
    }
    bi = __shfl(bi, 0);
    if (bi >= 64) break;  // fewer than k valid candidates
    if (lane == 0) {
      out_ids[q * k + t] = sid[bi];
      out_scores[q * k + t] = ssc[bi];
    }
    if (lane == bi) avail = false;
    // G[lane][bi] = G[bi][lane] (one stored value serves both); row bi is contiguous, except
    // that block (1,0) is read as (0,1) transposed (a strided read of 32 lanes, k times in all)
    if (lane < ROWS) red = fmaxf(red, G[bi >= 32 && lane < 32 ? lane * ROWS + bi : bi * ROWS + lane]);
  }
  if (lane == 0)
    for (; t < k; ++t) {
      out_ids[q * k + t] = -1;
      out_scores[q * k + t] = -INFINITY;
    }
}

// (-inf, -1) into count result slots: what an empty index returns.
__global__ __launch_bounds__(256) void mmr_pad_kernel(float* __restrict__ out_scores, int64_t* __restrict__ out_ids,
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

// Grow-only device workspace of one index handle: the top-fetch_k lists of
// mq_index_search_mmr and the staging of the host-pointer calls.  Kept for the life of the
// process under the handle's address (the index's own struct is private to index.hip); a
// handle created later at the same address reuses it (re-created, pinned staging included,
// when that handle sits on another GPU).  `mu` is held for the whole of every
// mq_index_mmr_select / mq_index_search_mmr call on the handle, as the index's own mutex is
// by its neighbours: the calls serialise, and nobody grows or restages the workspace under
// a call that is using it.
struct MmrWork {
  std::mutex mu;
  int device = -1;
  void* p = nullptr;
  size_t bytes = 0;
  PinBuf pin;
  int ensure(int dev, size_t need) {
    if (dev == device && need <= bytes) return MQ_OK;
    if (p) {
      DeviceGuard dg(device);
      (void)hipFree(p);
    }
    if (dev != device) pin.release();
    p = nullptr;
    bytes = 0;
    device = dev;
    if (hipMalloc(&p, need) != hipSuccess) MQ_FAIL(MQ_ENOMEM, "hipMalloc(%zu bytes) failed", need);
    bytes = need;
    return MQ_OK;
  }
};

std::mutex g_work_mu;
std::unordered_map<const mq_index*, std::unique_ptr<MmrWork>> g_work;

MmrWork* work_of(const mq_index* ix) {
  std::lock_guard<std::mutex> lk(g_work_mu);
  auto& w = g_work[ix];
  if (!w) w = std::make_unique<MmrWork>();
  return w.get();
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// Device of a pointer (HIP device memory), or -1 (host / unknown).
int pointer_device(const void* p) {
  hipPointerAttribute_t a;
  if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  return a.type == hipMemoryTypeDevice ? a.device : -1;
}

int check_mmr_args(const mq_index* ix, int64_t nq, int fetch_k, int k, float lambda) {
  MQ_CHECK_ARG(ix, "NULL index");
  MQ_CHECK_ARG(nq >= 0 && nq <= (1ll << 24), "query count %lld out of range", (long long)nq);
  MQ_CHECK_ARG(fetch_k >= 1 && fetch_k <= MQ_MAX_K, "fetch_k must be in [1, %d] (got %d)", MQ_MAX_K, fetch_k);
  MQ_CHECK_ARG(k >= 1 && k <= fetch_k, "k must be in [1, fetch_k = %d] (got %d)", fetch_k, k);
  MQ_CHECK_ARG(std::isfinite(lambda) && lambda >= 0.f && lambda <= 1.f, "lambda must be finite and in [0, 1] (got %g)",
               (double)lambda);
  return MQ_OK;
}

constexpr int kMaxDevices = 64;
std::atomic<bool> g_lds_raised[kMaxDevices];  // mmr_select_kernel<2>'s LDS limit raised on that GPU

// The selection on device buffers, asynchronous on s (`device`, the index's GPU, is current).
int launch_select(int device, const float* rows, int64_t n, int dim, const float* cs, const int64_t* ci, int64_t nq, int fetch_k,
                  int k, float lambda, float* os, int64_t* oi, hipStream_t s) {
  if (fetch_k <= 32) {
    hipLaunchKernelGGL(mmr_select_kernel<1>, dim3((unsigned)nq), dim3(256), MmrGeom<1>::LDS, s, rows, n, dim, ci, cs,
                       fetch_k, k, lambda, oi, os);
  } else {
    // 83 KB of LDS: above the default dynamic-LDS limit, raised once per GPU
    const bool known = device >= 0 && device < kMaxDevices;
    if (!known || !g_lds_raised[device].load(std::memory_order_acquire)) {
      MQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mmr_select_kernel<2>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)MmrGeom<2>::LDS));
      if (known) g_lds_raised[device].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(mmr_select_kernel<2>, dim3((unsigned)nq), dim3(256), MmrGeom<2>::LDS, s, rows, n, dim, ci, cs,
                       fetch_k, k, lambda, oi, os);
  }
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

struct IndexView {
  const float* rows = nullptr;
  int64_t n = 0;
  int dim = 0;
  int device = -1;
};

int view_of(mq_index* ix, IndexView* v) {
  void* p = nullptr;
  int rc = mq_index_size(ix, &v->n);
  if (!rc) rc = mq_index_dim(ix, &v->dim);
  if (!rc) rc = mq_index_data(ix, &p);
  if (rc) return rc;
  v->rows = static_cast<const float*>(p);
  if (v->n > 0) {
    v->device = pointer_device(p);
    if (v->device < 0) MQ_FAIL(MQ_ESTATE, "the index's row slab is not device memory");
  }
  return MQ_OK;
}

void fill_padding_host(float* os, int64_t* oi, int64_t count) {
  for (int64_t i = 0; i < count; ++i) {
    os[i] = -INFINITY;
    oi[i] = -1;
  }
}

// An empty index: only padding.  Device buffers are filled by a kernel on their own GPU (an
// empty index may have no slab to tell the GPU by), asynchronous on s like every device call.
int fill_padding_any(float* os, int64_t* oi, int64_t count, int io_on_device, hipStream_t s) {
  if (!io_on_device) {
    fill_padding_host(os, oi, count);
    return MQ_OK;
  }
  const int dev = pointer_device(os);
  MQ_CHECK_ARG(dev >= 0 && pointer_device(oi) == dev, "the outputs must be device memory of one GPU");
  DeviceGuard dg(dev);
  hipLaunchKernelGGL(mmr_pad_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, os, oi, count);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

}  // namespace

extern "C" {

int mq_index_mmr_select(mq_index* ix, const float* cand_scores, const int64_t* cand_ids, int64_t nq, int fetch_k,
                        int k, float lambda, float* out_scores, int64_t* out_ids, int io_on_device, void* stream) {
  clear_error();
  int rc = check_mmr_args(ix, nq, fetch_k, k, lambda);
  if (rc) return rc;
  if (nq == 0) return MQ_OK;
  MQ_CHECK_ARG(cand_scores && cand_ids && out_scores && out_ids, "NULL buffer");
  MmrWork* w = work_of(ix);
  std::lock_guard<std::mutex> lk(w->mu);  // the whole call: one MMR call per handle at a time
  IndexView v;
  rc = view_of(ix, &v);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (v.n == 0) return fill_padding_any(out_scores, out_ids, nq * k, io_on_device, s);
  DeviceGuard dg(v.device);
  if (io_on_device)
    return launch_select(v.device, v.rows, v.n, v.dim, cand_scores, cand_ids, nq, fetch_k, k, lambda, out_scores,
                         out_ids, s);
  // host lists: staged through the handle's workspace (ids first: 8-byte aligned sections)
  const size_t cib = (size_t)nq * fetch_k * 8, csb = (size_t)nq * fetch_k * 4;
  const size_t oib = (size_t)nq * k * 8, osb = (size_t)nq * k * 4;
  rc = w->ensure(v.device, up256(cib) + up256(csb) + up256(oib) + up256(osb));
  if (rc) return rc;
  char* d = static_cast<char*>(w->p);
  int64_t* dci = reinterpret_cast<int64_t*>(d);
  float* dcs = reinterpret_cast<float*>(d + up256(cib));
  int64_t* doi = reinterpret_cast<int64_t*>(d + up256(cib) + up256(csb));
  float* dos = reinterpret_cast<float*>(d + up256(cib) + up256(csb) + up256(oib));
  MQ_HIP(hipMemcpyAsync(dci, cand_ids, cib, hipMemcpyHostToDevice, s));
  MQ_HIP(hipMemcpyAsync(dcs, cand_scores, csb, hipMemcpyHostToDevice, s));
  rc = launch_select(v.device, v.rows, v.n, v.dim, dcs, dci, nq, fetch_k, k, lambda, dos, doi, s);
  if (rc) return rc;
  MQ_HIP(hipMemcpyAsync(out_ids, doi, oib, hipMemcpyDeviceToHost, s));
  MQ_HIP(hipMemcpyAsync(out_scores, dos, osb, hipMemcpyDeviceToHost, s));
  MQ_HIP(hipStreamSynchronize(s));
  return MQ_OK;
}

int mq_index_search_mmr(mq_index* ix, const float* queries, int64_t nq, int k, int fetch_k, float lambda,
                        const uint32_t* bits, float* out_scores, int64_t* out_ids, int io_on_device, void* stream) {
  clear_error();
  int rc = check_mmr_args(ix, nq, fetch_k, k, lambda);
  if (rc) return rc;
  if (nq == 0) return MQ_OK;
  MQ_CHECK_ARG(queries && out_scores && out_ids, "NULL buffer");
  MmrWork* w = work_of(ix);
  std::lock_guard<std::mutex> lk(w->mu);  // the whole call; the searches below take the index's own mutex inside it
  IndexView v;
  rc = view_of(ix, &v);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (v.n == 0) return fill_padding_any(out_scores, out_ids, nq * k, io_on_device, s);
  DeviceGuard dg(v.device);
  const size_t cib = (size_t)nq * fetch_k * 8, csb = (size_t)nq * fetch_k * 4;
  const size_t oib = (size_t)nq * k * 8, osb = (size_t)nq * k * 4, qb = (size_t)nq * v.dim * 4;
  rc = w->ensure(v.device, up256(cib) + up256(csb) + (io_on_device ? 0 : up256(oib) + up256(osb) + up256(qb)));
  if (rc) return rc;
  char* d = static_cast<char*>(w->p);
  int64_t* dci = reinterpret_cast<int64_t*>(d);
  float* dcs = reinterpret_cast<float*>(d + up256(cib));
  int64_t* doi = out_ids;
  float* dos = out_scores;
  const float* dq = queries;
  unsigned char* hp = nullptr;
  // pinned staging for the few-query path only, as mq_index_search: a batch's bytes go
  // pageable (the copy dominates neither way, and the pinned buffer stays small)
  const bool pin = qb <= (1u << 20);
  if (!io_on_device) {
    doi = reinterpret_cast<int64_t*>(d + up256(cib) + up256(csb));
    dos = reinterpret_cast<float*>(d + up256(cib) + up256(csb) + up256(oib));
    float* stage = reinterpret_cast<float*>(d + up256(cib) + up256(csb) + up256(oib) + up256(osb));
    if (pin) {
      rc = w->pin.ensure(qb + oib + osb);
      if (rc) return rc;
      hp = w->pin.as<unsigned char>();
      memcpy(hp, queries, qb);
    }
    MQ_HIP(hipMemcpyAsync(stage, pin ? (const void*)hp : (const void*)queries, qb, hipMemcpyHostToDevice, s));
    dq = stage;
  }
  // the top min(fetch_k, n) of every query, padded with (-inf, -1), into the workspace
  rc = bits ? mq_index_search_masked_batch(ix, dq, nq, fetch_k, bits, dcs, dci, 1, stream)
            : mq_index_search(ix, dq, nq, fetch_k, dcs, dci, 1, stream);
  if (rc) return rc;
  rc = launch_select(v.device, v.rows, v.n, v.dim, dcs, dci, nq, fetch_k, k, lambda, dos, doi, s);
  if (rc || io_on_device) return rc;
  MQ_HIP(hipMemcpyAsync(pin ? (void*)(hp + qb) : (void*)out_ids, doi, oib, hipMemcpyDeviceToHost, s));
  MQ_HIP(hipMemcpyAsync(pin ? (void*)(hp + qb + oib) : (void*)out_scores, dos, osb, hipMemcpyDeviceToHost, s));
  MQ_HIP(hipStreamSynchronize(s));
  if (pin) {
    memcpy(out_ids, hp + qb, oib);
    memcpy(out_scores, hp + qb + oib, osb);
  }
  return MQ_OK;
}

}  // extern "C"
