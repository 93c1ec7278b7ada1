// encoder.hip - BERT-base encoder forward for gfx950 (K1..K7) and the mq_encoder_* ABI.
//
// Replaces the embedding model behind OllamaEmbeddings("shaw/dmeta-embedding-zh")
// (reference src/medical_engine.py:43, src/ingest_medical.py:104): token ids ->
// 12 x [self-attention + FFN] post-LN BERT layers -> CLS (or mean) pool -> L2 norm.
//
// Kernels (one forward = 1 + 7*layers + 1 launches):
//   K1 embed_ln_kernel      word + position + token-type embedding gather, LayerNorm
//   K2 gemm (EPI_BIAS)      fused QKV projection          [M,H] x [3H,H]^T
//   K3 attention_kernel     softmax(QK^T/sqrt(dh) + mask) V, online softmax, LDS tiles
//   K4 gemm (EPI_RESID)     output projection + bias + residual, then ln_kernel
//   K5 gemm (EPI_GELU)      FFN up + bias + GELU (erf or tanh)
//   K6 gemm (EPI_RESID)     FFN down + bias + residual, then ln_kernel
//   K7 pool_kernel          CLS / masked-mean pooling + L2 normalisation
// mq_encoder_score runs the same forward with the pairs' segment ids and a tail that leaves the
// CLS rows un-normalised, then K13 (cls_head.hip): the cross-encoder's pooler + classifier.
// All GEMMs run on the exact-fp32 MFMA core of gemm_f32.hpp (or its split-f32 form).
// Few token rows (a single query, B * L <= 64) take forward_rows instead: 5 launches per
// layer on the K2r / K3r kernels below, LayerNorm applied by the consuming GEMM.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "cls_head.hpp"
#include "common.hpp"
#include "gemm_epi.hpp"
#include "gemm_f32.hpp"
#include "gemm_x6p.hpp"

namespace mq {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// ------------------------------------------------------------------ GEMM -------
// out[M,N] = epi(A[M,K] . W[N,K]^T + bias[N] (+ resid[M,N])), K % 32 == 0.
// Row strides lda / ldr / ldo (in floats) let the CLS-only last layer run on every
// L-th row of the activations without a gather.
// Persistent: gridDim.x workgroups (a multiple of 8, two per CU) walk the tiles
// t = blockIdx.x, +gridDim.x, ...; the first K-slice of the next tile is fetched during
// the last slice of the current one, so the epilogue overlaps the next tile's loads.
// Within a round, the workgroups of one XCD (blockIdx % 8 equal) take consecutive
// tiles, i.e. share A row panels in their L2.
template <class T, int EPI>
__global__ __launch_bounds__(T::THREADS, T::WG_PER_CU) void gemm_nt_kernel(const float* __restrict__ A, int lda,
                                                         const float* __restrict__ W,
                                                         const float* __restrict__ bias,
                                                         const float* __restrict__ resid, int ldr,
                                                         float* __restrict__ out, int ldo, int M,
                                                         int N, int K, int rx, LnFold lf) {
  __shared__ __attribute__((aligned(16))) float lds[2 * T::STAGE_FLOATS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / T::WAVES_N, wn = wave % T::WAVES_N;
  const int tiles_n = (N + T::BN - 1) / T::BN, tiles_m = (M + T::BM - 1) / T::BM;
  const int G = gridDim.x, per_xcd = G >> 3;
  const int xslot = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  // rx > 0: region walk (gemm_x6p.hpp region_of): this XCD group's tiles, row-major in it
  Region rg{0, tiles_m, 0, tiles_n};
  int loc = xslot, wstep = G;
  if (rx > 0) {
    rg = region_of(rx, blockIdx.x & 7, tiles_m, tiles_n);
    loc = blockIdx.x >> 3;
    wstep = per_xcd;
  }
  const int rtiles = rg.rm * rg.rn;
  const int n_tiles = loc < rtiles ? (rtiles - loc + wstep - 1) / wstep : 0;
  const FastDiv tnd(rg.rn);
  auto coords = [&](int i, int& m0, int64_t& n0) {
    const int t = i * wstep + loc;
    const int tr = tnd.div(t);
    m0 = (rg.m_lo + tr) * T::BM;
    n0 = (int64_t)(rg.n_lo + t - tr * rg.rn) * T::BN;
  };
  auto epi = [&](int i, floatx16(&acc)[T::TM][T::TN], float*) {
    int m0;
    int64_t n0l;
    coords(i, m0, n0l);
    const int n0 = (int)n0l;
    if constexpr (T::M16) {  // 16x16 accumulator blocks (F32Tile::M16): K2p's store
      floatx4 a4[2 * T::TM][2 * T::TN];
#pragma unroll
      for (int m = 0; m < 2 * T::TM; ++m)
#pragma unroll
        for (int n = 0; n < 2 * T::TN; ++n)
#pragma unroll
          for (int e = 0; e < 4; ++e) a4[m][n][e] = acc[m >> 1][n >> 1][4 * (2 * (m & 1) + (n & 1)) + e];
      store_wave_tile16<EPI, 2 * T::TM, 2 * T::TN>(a4, m0 + wm * T::WM, n0 + wn * T::WN, M, N, bias, resid, ldr, out,
                                                   ldo, lane, lf);
      return;
    }
    static_assert(T::M16 || EPI < EPI_RESID_LN_STATS, "the LayerNorm-fold epilogues are on the 16x16 store");
    if (m0 + T::BM <= M && n0 + T::BN <= N) {
      // full tile: every bias / residual load goes out before the first use, so the
      // tile pays one memory round trip (the guarded loop below waits per element).
      // Residual loads and output stores are buffer ops off the wave tile's origin: one
      // lane offset (column, lane half's row quad) in a VGPR, each register's row offset
      // row(e) * ld a scalar soffset - no per-element address arithmetic.
      const int wr0 = m0 + wm * T::WM, wc0 = n0 + wn * T::WN;
      float bv[T::TN];
#pragma unroll
      for (int tn = 0; tn < T::TN; ++tn) bv[tn] = bias[wc0 + tn * 32 + (lane & 31)];
      float rv[T::TM][T::TN][16];
      if constexpr (EPI == EPI_RESID) {
        const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(resid + (int64_t)wr0 * ldr + wc0), (short)0, 0x7fffffff, 0x00020000);
        const int rl = (4 * (lane >> 5) * ldr + (lane & 31)) * 4;
#pragma unroll
        for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < T::TN; ++tn)
#pragma unroll
            for (int e = 0; e < 16; ++e)
              rv[tm][tn][e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                  rr, rl, (acc_row(tm, e, 0) * ldr + tn * 32) * 4, 0));
      }
      const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(out + (int64_t)wr0 * ldo + wc0), (short)0, 0x7fffffff, 0x00020000);
      const int ol = (4 * (lane >> 5) * ldo + (lane & 31)) * 4;
#pragma unroll
      for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < T::TN; ++tn)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            float v = acc[tm][tn][e] + bv[tn];
            if (EPI == EPI_GELU_ERF) v = gelu_erf(v);
            if (EPI == EPI_GELU_TANH) v = gelu_tanh(v);
            if (EPI == EPI_RESID) v += rv[tm][tn][e];
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ro, ol, (acc_row(tm, e, 0) * ldo + tn * 32) * 4, 0);
          }
      return;
    }
#pragma unroll
    for (int tn = 0; tn < T::TN; ++tn) {
      const int col = n0 + wn * T::WN + tn * 32 + (lane & 31);
      if (col >= N) continue;
      const float b = bias[col];
#pragma unroll
      for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = m0 + wm * T::WM + acc_row(tm, e, lane);
          if (row >= M) continue;
          float v = acc[tm][tn][e] + b;
          if (EPI == EPI_GELU_ERF) v = gelu_erf(v);
          if (EPI == EPI_GELU_TANH) v = gelu_tanh(v);
          if (EPI == EPI_RESID) v += resid[(int64_t)row * ldr + col];
          out[(int64_t)row * ldo + col] = v;
        }
    }
  };
  walk_tiles<T>(lds, n_tiles, TileOperands{A, lda, M, W, K, N, K}, coords, epi);
}

// ---------------------------------------------------------- split-K GEMM ------
// For few rows (single queries, the CLS-only last layer) the direct GEMM leaves most
// CUs idle.  Split K into S chunks: workgroup (tile, s) multiplies its tile over
// K-chunk s and stores an fp32 partial slab[s][M][N]; splitk_reduce_kernel then sums
// the S slabs IN ORDER (bitwise reproducible) and applies bias / GELU / residual.
template <class T>
__global__ __launch_bounds__(256, 2) void gemm_splitk_kernel(const float* __restrict__ A, int lda,
                                                             const float* __restrict__ W, int M,
                                                             int N, int K, int S,
                                                             float* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) float lds[2 * T::STAGE_FLOATS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / T::WAVES_N, wn = wave % T::WAVES_N;
  const int tiles_n = (N + T::BN - 1) / T::BN;
  const int tile = blockIdx.x / S, sidx = blockIdx.x % S;
  const int Kc = K / S;
  const int m0 = (tile / tiles_n) * T::BM;
  const int n0 = (tile % tiles_n) * T::BN;
  auto coords = [&](int, int& mm0, int64_t& nn0) {
    mm0 = m0;
    nn0 = n0;
  };
  float* dst = slab + (int64_t)sidx * M * N;
  auto epi = [&](int, floatx16(&acc)[T::TM][T::TN], float*) {
#pragma unroll
    for (int tn = 0; tn < T::TN; ++tn) {
      const int col = n0 + wn * T::WN + tn * 32 + (lane & 31);
      if (col >= N) continue;
#pragma unroll
      for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = m0 + wm * T::WM + acc_row(tm, e, lane);
          if (row < M) dst[(int64_t)row * N + col] = acc[tm][tn][e];
        }
    }
  };
  walk_tiles<T>(lds, 1, TileOperands{A + (int64_t)sidx * Kc, lda, M, W + (int64_t)sidx * Kc, K, N, Kc},
                coords, epi);
}

// sum_{s<S} p[s * plane] (float4), left to right; the loads go out 8, then 4 at a time
// so a deep split does not serialise on load latency (same additions, same order: the
// sum starts from -0.0f, the exact additive identity; S = 12 and 16, the split factors
// of K = 768 and 3072, take no single-load round trip).
__device__ __forceinline__ floatx4 sum_slabs(const float* __restrict__ p, int64_t plane, int S) {
  floatx4 v = {-0.f, -0.f, -0.f, -0.f};
  int s = 0;
  for (; s + 8 <= S; s += 8) {
    floatx4 t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = *reinterpret_cast<const floatx4*>(p + (s + u) * plane);
#pragma unroll
    for (int u = 0; u < 8; ++u) v += t[u];
  }
  if (s + 4 <= S) {
    floatx4 t[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) t[u] = *reinterpret_cast<const floatx4*>(p + (s + u) * plane);
#pragma unroll
    for (int u = 0; u < 4; ++u) v += t[u];
    s += 4;
  }
  for (; s < S; ++s) v += *reinterpret_cast<const floatx4*>(p + s * plane);
  return v;
}

template <int EPI>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ slab, int S,
                                                            int M, int N,
                                                            const float* __restrict__ bias,
                                                            const float* __restrict__ resid, int ldr,
                                                            float* __restrict__ out, int ldo) {
  const int64_t i4 = (int64_t)blockIdx.x * 256 + threadIdx.x;  // float4 index, N % 4 == 0
  const int64_t n4 = N / 4;
  if (i4 >= (int64_t)M * n4) return;
  const int row = (int)(i4 / n4), c = (int)(i4 % n4) * 4;
  const int64_t plane = (int64_t)M * N;
  floatx4 v = sum_slabs(slab + (int64_t)row * N + c, plane, S);
  v += *reinterpret_cast<const floatx4*>(bias + c);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (EPI == EPI_GELU_ERF) v[j] = gelu_erf(v[j]);
    if (EPI == EPI_GELU_TANH) v[j] = gelu_tanh(v[j]);
  }
  if (EPI == EPI_RESID) v += *reinterpret_cast<const floatx4*>(resid + (int64_t)row * ldr + c);
  *reinterpret_cast<floatx4*>(out + (int64_t)row * ldo + c) = v;
}

// ------------------------------------------------------- K1 / LayerNorm ------
// Token-type (segment) row of token `row`: types == nullptr (the embedding forward) is row 0;
// else the id clamped to [0, type_vocab), as the word ids are - never gather out of bounds.
__device__ __forceinline__ int type_row(const int* __restrict__ types, int row, int type_vocab) {
  if (!types) return 0;
  const int t = types[row];
  return t < 0 ? 0 : (t >= type_vocab ? type_vocab - 1 : t);
}

template <int VPL>
__device__ __forceinline__ void ln_row_store(floatx4 (&x)[VPL], const float* __restrict__ g,
                                             const float* __restrict__ b, float eps,
                                             float* __restrict__ dst, int lane) {
  constexpr int H = VPL * 256;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) s += x[i].x + x[i].y + x[i].z + x[i].w;
  const float mean = wave_sum(s) * (1.0f / H);
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    x[i] -= mean;
    v += x[i].x * x[i].x + x[i].y * x[i].y + x[i].z * x[i].z + x[i].w * x[i].w;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(v) * (1.0f / H) + eps);
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = (i * 64 + lane) * 4;
    const floatx4 gg = *reinterpret_cast<const floatx4*>(g + c);
    const floatx4 bb = *reinterpret_cast<const floatx4*>(b + c);
    *reinterpret_cast<floatx4*>(dst + c) = x[i] * rstd * gg + bb;
  }
}

// Split-K reduction of a residual projection fused with the LayerNorm after it (few-row
// path: saves a launch and the y round trip per LN): x = LN(sum_s slab[s] + bias +
// resid), slabs summed in order (the LN's reductions are block-wide, so the result
// matches splitk_reduce_kernel<EPI_RESID> + ln_kernel to rounding).  A block reads its
// whole row before writing it, so dst may alias resid row for row (stride H).
// POOL (the CLS-pooled last layer's FFN-down, MQ_ENC_OPT_CLS_KFREE): the rows are the
// sequences' CLS rows and this LayerNorm the encoder's last, so the row is L2-normalised here,
// v / max(||v||, 1e-12) as pool_kernel, and dst is the embedding - no pool launch.  raw != 0
// (scoring, mq_encoder_score): the LayerNorm output itself, not normalised.
template <int VPL, bool POOL = false>
__global__ __launch_bounds__(256) void splitk_reduce_ln_kernel(
    const float* __restrict__ slab, int S, int M, const float* __restrict__ bias,
    const float* resid, int ldr, const float* __restrict__ g, const float* __restrict__ b,
    float eps, float* dst, int raw) {
  // one 256-thread block per row (the few-row path has few rows: 4 waves per row keep
  // 4x more slab loads in flight than a wave per row); thread t owns columns t + 256 i
  constexpr int H = VPL * 256;
  __shared__ float part[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int row = blockIdx.x;
  const int64_t plane = (int64_t)M * H;
  float x[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = t + 256 * i;
    const float* p = slab + (int64_t)row * H + c;
    float v = -0.f;  // as sum_slabs: 8 then 4 loads in flight, same order
    int sl = 0;
    for (; sl + 8 <= S; sl += 8) {
      float u[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) u[j] = p[(sl + j) * plane];
#pragma unroll
      for (int j = 0; j < 8; ++j) v += u[j];
    }
    if (sl + 4 <= S) {
      float u[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) u[j] = p[(sl + j) * plane];
#pragma unroll
      for (int j = 0; j < 4; ++j) v += u[j];
      sl += 4;
    }
    for (; sl < S; ++sl) v += p[sl * plane];
    x[i] = v + bias[c] + resid[(int64_t)row * ldr + c];
  }
  auto block_sum = [&](float v) {
    v = wave_sum(v);
    if (lane == 0) part[wave] = v;
    __syncthreads();
    const float r = part[0] + part[1] + part[2] + part[3];
    __syncthreads();
    return r;
  };
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) sum += x[i];
  const float mean = block_sum(sum) * (1.0f / H);
  float var = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    x[i] -= mean;
    var += x[i] * x[i];
  }
  const float rstd = 1.0f / sqrtf(block_sum(var) * (1.0f / H) + eps);
  if constexpr (POOL) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = t + 256 * i;
      x[i] = x[i] * rstd * g[c] + b[c];
      ss += x[i] * x[i];
    }
    const float inv = raw ? 1.0f : 1.0f / fmaxf(sqrtf(block_sum(ss)), 1e-12f);
#pragma unroll
    for (int i = 0; i < VPL; ++i) dst[(int64_t)row * H + t + 256 * i] = x[i] * inv;
    return;
  }
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = t + 256 * i;
    dst[(int64_t)row * H + c] = x[i] * rstd * g[c] + b[c];
  }
}

// Row statistics of one LayerNorm row held as ln_row_store holds it (same sums in the
// same order, so mean / rstd are bitwise those of ln_kernel).
template <int VPL>
__device__ __forceinline__ void ln_row_stats(const floatx4 (&x)[VPL], float eps, float& mean,
                                             float& rstd) {
  constexpr int H = VPL * 256;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) s += x[i].x + x[i].y + x[i].z + x[i].w;
  mean = wave_sum(s) * (1.0f / H);
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const floatx4 d = x[i] - mean;
    v += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
  }
  rstd = 1.0f / sqrtf(wave_sum(v) * (1.0f / H) + eps);
}

// Wave sum with DPP lane moves inside each 16-lane row (xor 1, xor 2, half-row mirror, row
// mirror) and two cross-row shuffles: 2 LDS-crossbar round trips instead of wave_sum's 6
// (the few-row path's LayerNorm runs on the critical path of every launch).
__device__ __forceinline__ float dpp_add(float v, int ctrl_id) {
  int t;
  switch (ctrl_id) {  // dpp_ctrl must be an immediate
    case 0: t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false); break;   // quad xor 1
    case 1: t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false); break;   // quad xor 2
    case 2: t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false); break;  // row half mirror
    default: t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false); break; // row mirror
  }
  return v + __int_as_float(t);
}
__device__ __forceinline__ float wave_sum_fast(float v) {
  v = dpp_add(v, 0);
  v = dpp_add(v, 1);
  v = dpp_add(v, 2);
  v = dpp_add(v, 3);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

template <int VPL>
__device__ __forceinline__ void ln_row_stats_fast(const floatx4 (&x)[VPL], float eps, float& mean,
                                                  float& rstd) {
  constexpr int H = VPL * 256;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) s += x[i].x + x[i].y + x[i].z + x[i].w;
  mean = wave_sum_fast(s) * (1.0f / H);
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const floatx4 d = x[i] - mean;
    v += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
  }
  rstd = 1.0f / sqrtf(wave_sum_fast(v) * (1.0f / H) + eps);
}

// ------------------------------------------------------- few-row GEMM (K2r) ----
// A single query is M = L <= 64 token rows: the tiled GEMM leaves the chip idle and the
// split-K path pays a second launch for its ordered slab reduction (~5 us each, 4 per
// layer).  Here one 1024-thread workgroup owns a 16 x 16 output tile over the FULL depth:
// its 16 waves each multiply one contiguous K range (NB x 256 / 16 deep) on
// v_mfma_f32_16x16x4_f32 and the 16 partial tiles are summed in wave order through LDS
// (bitwise reproducible), then bias / GELU / residual.  Grid (N / 16, ceil(M / 16)):
// 288 workgroups for QKV, 384 for FFN-up, 96 for the two H-wide projections at M = 32.
// Lane (c = l & 15, kq = l >> 4) loads float4s of row c of the A and W tiles at
// k0 + 4 kq; MFMA step t multiplies element t, i.e. logical k index kq <-> k0 + 4 kq + t
// in both operands.
// LN_IN: A holds pre-LayerNorm rows (the last residual sum, K = H = 256 VPL); wave w
// first computes row r0 + w's mean / rstd (as ln_kernel) and A is normalised while it is
// loaded, so no LayerNorm launch sits between the GEMMs.  The column-0 workgroups also
// store the normalised rows to ln_out: the residual input of the next projection.
#ifndef MQ_ROWS_DBG
#define MQ_ROWS_DBG 0  // measurement builds only: 1 no weight loads, 2 no row loads, 4 no MFMA
#endif
#if MQ_ROWS_DBG != 0 && !defined(MQ_MEASUREMENT_BUILD)
#error "MQ_ROWS_DBG computes wrong results: only a measurement build (-DMQ_MEASUREMENT_BUILD) may set it"
#endif
// Measurement builds with -DMQ_KTRACE: thread 0 of each workgroup of the few-row kernels
// stamps the 100 MHz wall clock at phase boundaries into mq_ktrace[workgroup][slot]
// (read back by mq_debug_ktrace_read, tools/ktrace.py).  Compiled out otherwise.
#if defined(MQ_KTRACE) && !defined(MQ_MEASUREMENT_BUILD)
#error "MQ_KTRACE is a measurement build option (-DMQ_MEASUREMENT_BUILD)"
#endif
#ifdef MQ_KTRACE
// region 0 QKV, 1 FFN-up, 2 FFN-down / out-proj (rows_gemm_kernel by epilogue), 3 K3o
constexpr int kTraceSlots = 8, kTraceWgs = 1024, kTraceRegions = 4;
__device__ long long mq_ktrace[kTraceRegions * kTraceWgs * kTraceSlots];
#define KTRACE_R(region, slot)                                                                 \
  do {                                                                                        \
    if (threadIdx.x == 0) {                                                                   \
      const int wg_ = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);           \
      if (wg_ < kTraceWgs) mq_ktrace[((region) * kTraceWgs + wg_) * kTraceSlots + (slot)] = wall_clock64(); \
    }                                                                                         \
  } while (0)
#else
#define KTRACE_R(region, slot) \
  do {                         \
  } while (0)
#endif
// Measurement builds with -DMQ_ROWS_REPEAT: every few-row launch runs twice back to back
// (all five are idempotent), so a kernel trace shows each launch cold and with its
// weights warm in L2 / MALL - what a next-phase weight prefetch could at best recover.
#if defined(MQ_ROWS_REPEAT) && !defined(MQ_MEASUREMENT_BUILD)
#error "MQ_ROWS_REPEAT is a measurement build option (-DMQ_MEASUREMENT_BUILD)"
#endif
#ifdef MQ_ROWS_REPEAT
#define ROWS_REP for (int rep_ = 0; rep_ < 2; ++rep_)
#else
#define ROWS_REP
#endif
// A weight fragment of the few-row kernels: default cache policy, or non-temporal for the
// layers past the handle's `resident_layers` (MQ_ENC_OPT_RESIDENT_LAYERS), so that
// back-to-back single queries keep the first layers' weights in the 256 MB MALL instead
// of cycling all 340 MB through it (a cyclic sweep larger than the cache hits nothing).
// Buffer loads off the matrix base (byte offsets < 2^31): the policy is an immediate of the
// intrinsic, so the two forms stay two instructions (a plain load and a nontemporal-hinted
// one under a runtime branch get merged into one plain load).
__device__ __forceinline__ floatx4 load_w(__amdgpu_buffer_rsrc_t w, int byte_off, int nt) {
  return __builtin_bit_cast(floatx4, nt ? __builtin_amdgcn_raw_buffer_load_b128(w, byte_off, 0, 2)
                                        : __builtin_amdgcn_raw_buffer_load_b128(w, byte_off, 0, 0));
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t w_rsrc(const float* W) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)W, (short)0, 0x7fffffff, 0x00020000);
}
// Fragment image ("frag16") of a [R][C] fp32 matrix for the few-row kernels: per 16-row x
// 16-column block (block (rb, cb), cb fastest) 1 KB in the lane order of one
// v_mfma_f32_16x16x4_f32 operand load - lane l = c + 16 kq holds the float4 at row
// 16 rb + c, columns 16 cb + 4 kq .. + 3.  One wave-instruction then moves 1 KB of whole
// lines, where the row-major operand loads moved 16 rows x 64 B (16 half lines) each;
// profiles/r6/engine_probe.jsonl: 5.76 -> 3.37 us for FFN-down's per-workgroup bytes.
// The weights are imaged once at load (mq_encoder_load_weights); FFN-up writes its output
// in this layout for FFN-down (FL_O / FL_A).
// FL_OT (with FL_O): the blocks of the last third of the columns (QKV's V) are stored
// transposed - the frag16 of V^T - so attention's P V reads V^T fragments whole
// FL_ACC: the K splits add into ONE output plane (a no-return device-scope atomic add per
// element into a zeroed buffer) instead of writing a plane each.  With exactly two addends
// per element, 0 + a + b and 0 + b + a are the same float (addition commutes), so the result
// is bitwise the p0 + p1 the consumer summed before - and the consumer reads one plane.
enum RowsFlags { FL_A = 1, FL_O = 2, FL_OT = 4, FL_ACC = 8 };  // A / output in frag16 (weights always are)
__device__ __forceinline__ int64_t frag16_offset(int64_t row, int col, int cols) {  // in floats
  return ((row >> 4) * (cols >> 4) + (col >> 4)) * 256 + ((row & 15) + 16 * ((col & 15) >> 2)) * 4 + (col & 3);
}
__global__ __launch_bounds__(256) void frag16_image_kernel(const float* __restrict__ W, int R, int C,
                                                           floatx4* __restrict__ img) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;  // one float4 of the image
  if (idx >= (int64_t)R * C / 4) return;
  const int lane = (int)(idx & 63);
  const int64_t blk = idx >> 6;
  const int cbs = C >> 4;
  const int64_t rb = blk / cbs;
  const int cb = (int)(blk - rb * cbs);
  img[idx] = *reinterpret_cast<const floatx4*>(W + (rb * 16 + (lane & 15)) * C + cb * 16 + 4 * (lane >> 4));
}

constexpr int kRT = 16;      // rows = columns per output tile
constexpr int kRWaves = 16;  // waves per workgroup, one K range each
constexpr int kRowsMax = 256; // token rows up to which a forward may take this path
constexpr int kRowsDefault = 64;  // ... and does by default (MQ_ROWS_MAX overrides)

// W is the weights' frag16 image (ldw = the full depth); FL & FL_A: A (no LayerNorm input)
// in frag16 with lda columns; FL & FL_O: out in frag16 with ldo columns.
template <int EPI, bool LN_IN, int VPL, int NB, int S_IN, int RT, int FL = 0>
__global__ __launch_bounds__(1024) void rows_gemm_kernel(
    const float* __restrict__ A, int lda, int64_t a_plane, int M, const float* __restrict__ lng,
    const float* __restrict__ lnb, float eps, float* __restrict__ ln_out,
    const float* __restrict__ W, int ldw, const float* __restrict__ bias,
    const float* __restrict__ resid, int ldr, float* __restrict__ out, int ldo, int64_t o_plane,
    const int* __restrict__ ids, int L, int vocab, const float* __restrict__ pos,
    const float* __restrict__ typ, const int* __restrict__ types, int type_vocab, int nt_w,
    float* __restrict__ zbuf, int64_t zn) {
  static_assert(!(LN_IN && (FL & FL_A)), "a LayerNorm input is read row-major");
  static_assert(!((FL & FL_ACC) && (FL & FL_O)), "accumulated output is row-major");
  // zbuf: zn floats (a multiple of 4) this launch zeroes for a LATER launch's FL_ACC adds
  if (zbuf) {
    const int64_t nwg = (int64_t)gridDim.x * gridDim.y * gridDim.z;
    const int64_t wg = blockIdx.x + (int64_t)gridDim.x * (blockIdx.y + (int64_t)gridDim.y * blockIdx.z);
    for (int64_t i = wg * 1024 + threadIdx.x; i < zn / 4; i += nwg * 1024)
      reinterpret_cast<floatx4*>(zbuf)[i] = floatx4{0.f, 0.f, 0.f, 0.f};
  }
  constexpr int K = NB * 256;  // depth of this workgroup's K split (blockIdx.z)
  // 16-deep blocks per load batch: all of them while the operands fit the 128 VGPRs of a
  // 1024-thread workgroup (one memory round trip), else batches
  constexpr int CH = RT == 1 ? (NB <= 12 ? NB : 8) : (NB <= 6 ? NB : 4);
  static_assert(NB % CH == 0, "the load batch must divide NB");
  static_assert(!LN_IN || NB == VPL, "LayerNorm input needs K == H");
  static_assert(RT >= 1 && RT * kRT * kRT <= 1024, "one epilogue thread per output element");
  // LN_IN: the RT x 16 normalised rows, row stride K + 4 floats (a 16-lane ds_read_b128
  // group reads 16 rows at one k: 16 distinct 16-B bank groups)
  constexpr int AS = K + 4;
  __shared__ __attribute__((aligned(16))) float arows[LN_IN ? RT * kRT * AS : 4];
  __shared__ float part[kRWaves][RT][kRT * kRT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, kq = lane >> 4;
  const int n0 = blockIdx.x * kRT, r0 = blockIdx.y * kRT * RT;
  const int kb0 = wave * (K / kRWaves);  // this wave's K range
  const int ks = blockIdx.z;  // K split: columns [ks K, (ks + 1) K) of A and W
  const __amdgpu_buffer_rsrc_t wr = w_rsrc(W);
  // this lane's weight fragment: block (n0 / 16, (ks K + kb0) / 16 + j) of the image, 1 KB apart
  const int kblk0 = (ks * K + kb0) >> 4;
  const int wo4 = (((n0 >> 4) * (ldw >> 4) + kblk0) * 64 + lane) * 16;

  KTRACE_R(EPI == EPI_BIAS ? 0 : EPI == EPI_RESID ? 2 : 1, 0);
  floatx4 wv[CH], av[RT][CH];
  // the first batch of weights is in flight before anything else (the LayerNorm pass
  // below waits on its own row loads only).  All RT row tiles share each weight
  // fragment: the launch streams W once.
#pragma unroll
  for (int j = 0; j < CH; ++j)
    wv[j] = (MQ_ROWS_DBG & 1) ? floatx4{1e-3f, 1e-3f, 1e-3f, 1e-3f} : load_w(wr, wo4 + 1024 * j, nt_w);
  // Everything else this launch reads from memory goes out now too, under the weight
  // loads: the epilogue's bias / residual element (thread t < 256 RT finishes element
  // t % 256 of row tile t / 256) and the LayerNorm's gamma / beta.  Loaded where they are
  // used, each would add a dependent memory round trip to the launch's critical path
  // (after the partial-tile reduction, after the row statistics).  FL_O: thread t's element
  // is position t % 256 of the tile's frag16 block (lane (t % 256) / 4), so each wave
  // stores 256 contiguous bytes.
  const int et = threadIdx.x, ert = et / (kRT * kRT), ep = et % (kRT * kRT);
  const bool vt = (FL & FL_OT) && n0 >= 2 * (ldo / 3);  // a V block of QKV, stored as V^T
  const int ee = !(FL & FL_O) ? ep
                 : vt ? ((4 * (ep >> 6) + (ep & 3)) * kRT + ((ep >> 2) & 15))
                      : (((ep >> 2) & 15) * kRT + 4 * (ep >> 6) + (ep & 3));  // [row][col] in the tile
  const int erow = r0 + ert * kRT + ee / kRT, ecol = n0 + ee % kRT;
  float ebias = 0.f, eres = 0.f;
  if (ert < RT && ks == 0 && erow < M) {
    ebias = bias[ecol];
    if (EPI == EPI_RESID) eres = resid[(int64_t)erow * ldr + ecol];
  }
  floatx4 lgv[LN_IN ? VPL : 1], lbv[LN_IN ? VPL : 1];
  if (LN_IN) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      lgv[i] = *reinterpret_cast<const floatx4*>(lng + (i * 64 + lane) * 4);
      lbv[i] = *reinterpret_cast<const floatx4*>(lnb + (i * 64 + lane) * 4);
    }
  }
  if (LN_IN) {
    // wave w normalises rows r0 + w + 16 rt (one row per wave per row tile)
    floatx4 x[RT][VPL];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int rr = min(r0 + rt * kRT + wave, M - 1);
      const float* src = A + (int64_t)rr * lda;
      if constexpr (MQ_ROWS_DBG & 2) {
#pragma unroll
        for (int i = 0; i < VPL; ++i) x[rt][i] = floatx4{0.1f * lane, 0.2f, 0.3f, 0.4f * wave};
      } else if constexpr (S_IN == 0) {
        // layer 0: the row is the embedding sum word[id] + pos[p] + type[tt] (as
        // embed_ln_kernel; A = the word table), normalised with the embedding LayerNorm
        int id = ids[rr];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        const float* trow = typ + (int64_t)type_row(types, rr, type_vocab) * K;
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          const int cc = (i * 64 + lane) * 4;
          x[rt][i] = *reinterpret_cast<const floatx4*>(A + (int64_t)id * K + cc) +
                     *reinterpret_cast<const floatx4*>(pos + (int64_t)(rr % L) * K + cc) +
                     *reinterpret_cast<const floatx4*>(trow + cc);
        }
      } else {
        // the row is the sum of S_IN split-K planes of the producing GEMM, added in order
        floatx4 p[S_IN][VPL];
#pragma unroll
        for (int z = 0; z < S_IN; ++z)
#pragma unroll
          for (int i = 0; i < VPL; ++i)
            p[z][i] = *reinterpret_cast<const floatx4*>(src + z * a_plane + (i * 64 + lane) * 4);
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          x[rt][i] = p[0][i];
#pragma unroll
          for (int z = 1; z < S_IN; ++z) x[rt][i] += p[z][i];
        }
      }
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      float mu, rs;
      ln_row_stats_fast<VPL>(x[rt], eps, mu, rs);
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int cc = (i * 64 + lane) * 4;
        x[rt][i] = (x[rt][i] - mu) * rs * lgv[i] + lbv[i];
        *reinterpret_cast<floatx4*>(&arows[(rt * kRT + wave) * AS + cc]) = x[rt][i];
      }
    }
    KTRACE_R(EPI == EPI_BIAS ? 0 : EPI == EPI_RESID ? 2 : 1, 1);
    // LDS-only barrier: the weight loads stay in flight across it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    KTRACE_R(EPI == EPI_BIAS ? 0 : EPI == EPI_RESID ? 2 : 1, 2);
    // the normalised rows out, 16 columns per workgroup of this row group (not all of
    // them from one workgroup: the slowest workgroup sets the launch's duration)
    if (ln_out && ert < RT) {
      const int rr = ert * kRT + ee / kRT, cc = ee % kRT;
      if (r0 + rr < M)
        for (int c0 = blockIdx.x * kRT; c0 < K; c0 += gridDim.x * kRT)
          ln_out[(int64_t)(r0 + rr) * K + c0 + cc] = arows[rr * AS + c0 + cc];
    }
  }

  floatx4 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int b = 0; b < NB; b += CH) {
    if (b > 0) {
#pragma unroll
      for (int j = 0; j < CH; ++j) wv[j] = load_w(wr, wo4 + 1024 * (b + j), nt_w);
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const float* arow = A + (int64_t)min(r0 + rt * kRT + c, M - 1) * lda + ks * K + kb0 + 4 * kq;
      // frag16 A: row block (r0 / 16 + rt) (rows past M in the last block are never
      // written; they only feed output rows past M, which are not stored)
      const floatx4* afr = reinterpret_cast<const floatx4*>(A) +
                           ((int64_t)((r0 >> 4) + rt) * (lda >> 4) + kblk0) * 64 + lane;
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        if (LN_IN)
          av[rt][j] = *reinterpret_cast<const floatx4*>(&arows[(rt * kRT + c) * AS + kb0 + 16 * (b + j) + 4 * kq]);
        else if (MQ_ROWS_DBG & 2)
          av[rt][j] = floatx4{0.1f, 0.2f, 0.3f, 0.4f};
        else if (FL & FL_A)
          av[rt][j] = afr[(b + j) * 64];
        else
          av[rt][j] = *reinterpret_cast<const floatx4*>(arow + 16 * (b + j));
      }
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          if (MQ_ROWS_DBG & 4)
            acc[rt][t] += av[rt][j][t] * wv[j][t];
          else
            acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][j][t], wv[j][t], acc[rt], 0, 0, 0);
        }
      }
    }
  }
  KTRACE_R(EPI == EPI_BIAS ? 0 : EPI == EPI_RESID ? 2 : 1, 3);
  // accumulator element j is (row 4 kq + j, column c) of this wave's partial tile
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int j = 0; j < 4; ++j) part[wave][rt][(4 * kq + j) * kRT + c] = acc[rt][j];
  __syncthreads();
  KTRACE_R(EPI == EPI_BIAS ? 0 : EPI == EPI_RESID ? 2 : 1, 4);
  if (ert >= RT) return;
  float v = part[0][ert][ee];
#pragma unroll
  for (int w = 1; w < kRWaves; ++w) v += part[w][ert][ee];
  if (erow >= M) return;
  if (ks == 0) {  // split 0 carries bias / residual; GELU needs an unsplit K
    v += ebias;
    if (EPI == EPI_GELU_ERF) v = gelu_erf(v);
    if (EPI == EPI_GELU_TANH) v = gelu_tanh(v);
    if (EPI == EPI_RESID) v += eres;
  }
  if (FL & FL_O)
    out[ks * o_plane + (((int64_t)((r0 >> 4) + ert) * (ldo >> 4) + blockIdx.x) << 8) + ep] = v;
  else if (FL & FL_ACC)
    (void)atomicAdd(out + (int64_t)erow * ldo + ecol, v);
  else
    out[ks * o_plane + (int64_t)erow * ldo + ecol] = v;
  KTRACE_R(EPI == EPI_BIAS ? 0 : EPI == EPI_RESID ? 2 : 1, 5);
}

// One wave per row of H = 256*VPL floats held in registers (two-pass mean/variance).
template <int VPL>
__global__ __launch_bounds__(256) void embed_ln_kernel(
    const int* __restrict__ ids, int M, int L, int vocab, const float* __restrict__ word,
    const float* __restrict__ pos, const float* __restrict__ typ, const int* __restrict__ types,
    int type_vocab, const float* __restrict__ g, const float* __restrict__ b, float eps,
    float* __restrict__ out) {
  constexpr int H = VPL * 256;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  int id = ids[row];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);  // never gather out of bounds
  const int p = row % L;
  const float* trow = typ + (int64_t)type_row(types, row, type_vocab) * H;
  floatx4 x[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = (i * 64 + lane) * 4;
    x[i] = *reinterpret_cast<const floatx4*>(word + (int64_t)id * H + c) +
           *reinterpret_cast<const floatx4*>(pos + (int64_t)p * H + c) +
           *reinterpret_cast<const floatx4*>(trow + c);
  }
  ln_row_store<VPL>(x, g, b, eps, out + (int64_t)row * H, lane);
}

// RPW rows per wave, loaded together and reduced with interleaved shuffle chains (the
// per-row arithmetic is ln_row_store's, so results are bitwise those of one row per wave).
template <int VPL, int RPW>
__global__ __launch_bounds__(256) void ln_kernel(const float* __restrict__ src, int M,
                                                 const float* __restrict__ g,
                                                 const float* __restrict__ b, float eps,
                                                 float* __restrict__ dst) {
  constexpr int H = VPL * 256;
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW;
  if (row0 >= M) return;
  floatx4 x[RPW][VPL];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int i = 0; i < VPL; ++i)
      x[r][i] = *reinterpret_cast<const floatx4*>(src + (int64_t)min(row0 + r, M - 1) * H + (i * 64 + lane) * 4);
  float s[RPW], v[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    s[r] = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) s[r] += x[r][i].x + x[r][i].y + x[r][i].z + x[r][i].w;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int r = 0; r < RPW; ++r) s[r] += __shfl_xor(s[r], off);
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const float mean = s[r] * (1.0f / H);
    v[r] = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      x[r][i] -= mean;
      v[r] += x[r][i].x * x[r][i].x + x[r][i].y * x[r][i].y + x[r][i].z * x[r][i].z + x[r][i].w * x[r][i].w;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int r = 0; r < RPW; ++r) v[r] += __shfl_xor(v[r], off);
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    if (row0 + r >= M) break;
    const float rstd = 1.0f / sqrtf(v[r] * (1.0f / H) + eps);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = (i * 64 + lane) * 4;
      const floatx4 gg = *reinterpret_cast<const floatx4*>(g + c);
      const floatx4 bb = *reinterpret_cast<const floatx4*>(b + c);
      *reinterpret_cast<floatx4*>(dst + (int64_t)(row0 + r) * H + c) = x[r][i] * rstd * gg + bb;
    }
  }
}
// The forward's RPW (1 / 2 / 4 measured 0.38 / 0.31 / 0.30 ms per step: DESIGN.md section 4).
constexpr int kLnRowsPerWave = 4;

// LayerNorm of `rows` rows `stride` floats apart, in place (a wave holds its whole row before
// it writes): the B CLS rows of the raw y that the CLS-only last layer reads normalised when
// the LayerNorms are folded into the GEMMs.  ln_kernel's per-row arithmetic.
template <int VPL>
__global__ __launch_bounds__(256) void ln_rows_inplace_kernel(float* x, int rows, int64_t stride,
                                                              const float* __restrict__ g,
                                                              const float* __restrict__ b, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float* xr = x + (int64_t)row * stride;
  floatx4 v[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) v[i] = *reinterpret_cast<const floatx4*>(xr + (i * 64 + lane) * 4);
  ln_row_store<VPL>(v, g, b, eps, xr, lane);
}
// The same rows into a compact [rows][H] buffer, the source left as it is (the CLS_KFREE last
// layer: its pass over the raw rows still reads row b L raw, with the partials).
template <int VPL>
__global__ __launch_bounds__(256) void ln_rows_kernel(const float* __restrict__ x, int rows, int64_t stride,
                                                      const float* __restrict__ g, const float* __restrict__ b,
                                                      float eps, float* __restrict__ dst) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + (int64_t)row * stride;
  floatx4 v[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) v[i] = *reinterpret_cast<const floatx4*>(xr + (i * 64 + lane) * 4);
  ln_row_store<VPL>(v, g, b, eps, dst + (int64_t)row * (VPL * 256), lane);
}

// ------------------------------------------------------------ K3 attention ----
// One 64-thread workgroup (one wave) per (sequence, head, 32-query tile); dh = 64.
// Scores are computed TRANSPOSED on the f32 MFMA: S^T[key][query] = K . Q^T, so keys
// sit in the accumulator registers and queries on the lanes; the softmax over keys is
// then 16 in-register values + one cross-half exchange per query, and S^T is already
// the B operand of O^T[d][query] = V^T . P^T (no transpose, no LDS for P).
// Operand k-order: lane half h carries head dims 32h..32h+31 for QK^T (one contiguous
// 128-B read per row per lane), and key (s&3) + 8(s>>2) + 4h at PV step s (the
// accumulator row map).  Online softmax across 32-key tiles; masked keys weigh 0.
// NS > 1 (few (sequence, head, query tile) triples with many keys: a long single query, the
// CLS-only last layer): NS waves per workgroup split the key tiles (wave w takes tiles w,
// w + NS, ...), each with its own running max / sum / O^T, merged through LDS at the end in
// wave order: O = sum_w e^(m_w - m) O_w / sum_w e^(m_w - m) l_w (the same softmax; the
// rescaling order differs from one wave walking every tile, results agree to rounding).
constexpr int kDh = 64;

// HB > 1 (NS = 1): one workgroup per (sequence, query tile) with one wave per head, so a
// sequence's Q / K / V rows are read by waves issued together, whole 9 KB rows at a time
// (one wave per workgroup read 256-B head slices of rows 9 KB apart, ~4 TB/s).
template <int NS, int HB = 1>
__global__ __launch_bounds__(64 * NS * HB, NS == 1 && HB == 1 ? 3 : 1) void attention_kernel(const float* __restrict__ qkv,
                                                            const int* __restrict__ mask, int L,
                                                            int H, int heads, int q_tiles,
                                                            float scale, float* __restrict__ ctx) {
  // one LDS tile per wave, used in turn to stage Q, each key tile's K, and the output:
  // [32][68] rows for staging (a 16-lane ds_read_b128 group hits 16 distinct bank groups),
  // [32][65] for the output
  constexpr int kSt = kDh + 4;
  static_assert(HB == 1 || NS == 1, "heads per block or key splits");
  __shared__ __attribute__((aligned(16))) float tiles[NS * HB][32 * kSt];
  __shared__ float wmax[NS > 1 ? NS : 1][32], wsum[NS > 1 ? NS : 1][32];
  const int wv = NS > 1 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
  const int hw = HB > 1 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
  float* tile = tiles[NS > 1 ? wv : hw];
  float(*obuf)[kDh + 1] = reinterpret_cast<float(*)[kDh + 1]>(tile);
  const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
  const int hgroups = heads / HB;
  const int qt = blockIdx.x % q_tiles, h = ((blockIdx.x / q_tiles) % hgroups) * HB + hw;
  const int bseq = blockIdx.x / (q_tiles * hgroups);
  const int q0 = qt * 32;
  const int64_t row0 = (int64_t)bseq * L;
  const int ld = 3 * H;
  // Q / K tiles arrive by whole-line loads (4 rows x 256 B per wave-instruction) through
  // LDS; read lane-strided straight from HBM (64 lines per instruction) the tiles were
  // fetched ~2x (PMC), the lines evicted between the 8 instructions that share them.
  auto stage = [&](int row_base, int col) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int rr = 4 * i + (lane >> 4);
      const float* src = qkv + (row0 + min(row_base + rr, L - 1)) * ld + col + (lane & 15) * 4;
      *reinterpret_cast<floatx4*>(&tile[rr * kSt + (lane & 15) * 4]) = *reinterpret_cast<const floatx4*>(src);
    }
  };

  float qf[32];
  stage(q0, h * kDh);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const floatx4 v = *reinterpret_cast<const floatx4*>(&tile[r * kSt + hh * 32 + 4 * i]) * scale;
    qf[4 * i] = v.x;
    qf[4 * i + 1] = v.y;
    qf[4 * i + 2] = v.z;
    qf[4 * i + 3] = v.w;
  }
  float m_run = -INFINITY, l_run = 0.f;
  floatx16 o0, o1;
#pragma unroll
  for (int e = 0; e < 16; ++e) o0[e] = o1[e] = 0.f;

  for (int k0 = wv * 32; k0 < L; k0 += 32 * NS) {
    const int kr = min(k0 + r, L - 1);
    const bool kvalid = (k0 + r < L) && mask[row0 + kr] != 0;
    const unsigned long long kbits = __ballot(kvalid);  // bit j = key k0 + j usable
    float kf[32];
    stage(k0, H + h * kDh);  // (one wave per tile: its LDS reads of the last tile precede these writes)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const floatx4 v = *reinterpret_cast<const floatx4*>(&tile[r * kSt + hh * 32 + 4 * i]);
      kf[4 * i] = v.x;
      kf[4 * i + 1] = v.y;
      kf[4 * i + 2] = v.z;
      kf[4 * i + 3] = v.w;
    }
    floatx16 st;
#pragma unroll
    for (int e = 0; e < 16; ++e) st[e] = 0.f;
#pragma unroll
    for (int sidx = 0; sidx < 32; ++sidx) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[sidx], qf[sidx], st, 0, 0, 0);

    float tmax = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = (e & 3) + 8 * (e >> 2) + 4 * hh;
      st[e] = ((kbits >> key) & 1ull) ? st[e] : -INFINITY;
      tmax = fmaxf(tmax, st[e]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float m_new = fmaxf(m_run, tmax);
    const float alpha = (m_new == -INFINITY) ? 1.f : expf(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      st[e] = (st[e] == -INFINITY) ? 0.f : expf(st[e] - m_new);
      psum += st[e];
    }
    psum += __shfl_xor(psum, 32);
    l_run = l_run * alpha + psum;
    m_run = m_new;
    o0 *= alpha;
    o1 *= alpha;
    // (V staged through this LDS tile by whole-line loads instead, in flight under the
    // softmax, measured slower: attention 0.298 -> 0.327 ms per step, r6)
    const float* vbase = qkv + row0 * ld + 2 * H + h * kDh + r;
#pragma unroll
    for (int sidx = 0; sidx < 16; ++sidx) {
      const int key = min(k0 + (sidx & 3) + 8 * (sidx >> 2) + 4 * hh, L - 1);
      const float v0 = vbase[(int64_t)key * ld];
      const float v1 = vbase[(int64_t)key * ld + 32];
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0, st[sidx], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1, st[sidx], o1, 0, 0, 0);
    }
  }
  const int nrows = min(32, L - q0);
  if constexpr (NS == 1) {
    // O^T (d on registers, query on lanes) -> LDS [query][d] -> coalesced row stores
    const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int d = (e & 3) + 8 * (e >> 2) + 4 * hh;
      obuf[r][d] = o0[e] * inv;
      obuf[r][d + 32] = o1[e] * inv;
    }
    __syncthreads();
    for (int q = 0; q < nrows; ++q) ctx[(row0 + q0 + q) * H + h * kDh + lane] = obuf[q][lane];
  } else {
    if (hh == 0) wmax[wv][r] = m_run;
    __syncthreads();  // also: every wave is past its last K-tile reads of its own tile
    float m = -INFINITY;
#pragma unroll
    for (int w = 0; w < NS; ++w) m = fmaxf(m, wmax[w][r]);
    const float sc = m_run == -INFINITY ? 0.f : expf(m_run - m);
    if (hh == 0) wsum[wv][r] = l_run * sc;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int d = (e & 3) + 8 * (e >> 2) + 4 * hh;
      obuf[r][d] = o0[e] * sc;
      obuf[r][d + 32] = o1[e] * sc;
    }
    __syncthreads();
    // 32 x 64 outputs over 64 NS threads, partials summed in wave order
    for (int i = threadIdx.x; i < 32 * kDh; i += 64 * NS) {
      const int q = i / kDh, d = i % kDh;
      if (q >= nrows) break;
      float o = 0.f, l = 0.f;
#pragma unroll
      for (int w = 0; w < NS; ++w) {
        o += reinterpret_cast<const float(*)[kDh + 1]>(tiles[w])[q][d];
        l += wsum[w][q];
      }
      ctx[(row0 + q0 + q) * H + h * kDh + d] = l > 0.f ? o * (1.0f / l) : 0.f;
    }
  }
}

// K3 launch: one wave per (sequence, head, query tile) when those fill the chip, else NS
// waves per triple splitting the key tiles (a 256-token single query: 96 waves -> 768).
void launch_attention(int B, int L, int heads, int qt, int H, float scale, const float* qkv,
                      const int* mask, float* ctx, hipStream_t s) {
  const int triples = B * heads * qt, key_tiles = (L + 31) / 32;
  const dim3 grid(triples);
  // (6 or 4 heads per workgroup, 2-3 workgroups per CU: 0.386 / 0.337 vs 0.305 ms per step,
  // same box, r6)
  if (key_tiles == 1 && heads == 12 && triples >= 12 * 256)  // BERT-base batches: 12 heads per workgroup
    hipLaunchKernelGGL((attention_kernel<1, 12>), dim3(B * qt), dim3(768), 0, s, qkv, mask, L, H, heads, qt, scale,
                       ctx);
  else if (key_tiles >= 8 && triples <= 256)
    hipLaunchKernelGGL(attention_kernel<8>, grid, dim3(512), 0, s, qkv, mask, L, H, heads, qt, scale, ctx);
  else if (key_tiles >= 4 && triples <= 512)
    hipLaunchKernelGGL(attention_kernel<4>, grid, dim3(256), 0, s, qkv, mask, L, H, heads, qt, scale, ctx);
  else if (key_tiles >= 2 && triples <= 1024)
    hipLaunchKernelGGL(attention_kernel<2>, grid, dim3(128), 0, s, qkv, mask, L, H, heads, qt, scale, ctx);
  else
    hipLaunchKernelGGL(attention_kernel<1>, grid, dim3(64), 0, s, qkv, mask, L, H, heads, qt, scale, ctx);
}

// K3 for the few-row forward (L <= 64 keys, one sequence's latency): one 512-thread
// workgroup per (sequence, head, 32-query tile).  Wave w = (key quarter kw = w >> 1,
// query half qh = w & 1) computes its 16 x 16 block of S^T = K Q^T on
// v_mfma_f32_16x16x4_f32 (dh = 64 in two 8-step chains), the softmax max and sum over
// all keys are shared through LDS, and the wave multiplies its 16 keys' P^T (the S^T
// accumulator is already the B operand) by V^T into a partial O^T; the four key
// quarters' partials are summed in order.  Masking, scale and exp as attention_kernel;
// the MFMA chain per SIMD is a quarter of the one-wave kernel's.
__global__ __launch_bounds__(512) void attention_rows_kernel(const float* __restrict__ qkv,
                                                             const int* __restrict__ mask, int L,
                                                             int H, int heads, int q_tiles,
                                                             float scale, float* __restrict__ ctx) {
  __shared__ float smax[2][4][16], ssum[2][4][16];
  __shared__ float opart[2][4][16][kDh + 1];  // [qh][kw][query][d]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int kw = w >> 1, qh = w & 1;
  const int c = lane & 15, g = lane >> 4;
  const int qt = blockIdx.x % q_tiles, h = (blockIdx.x / q_tiles) % heads;
  const int bseq = blockIdx.x / (q_tiles * heads);
  const int64_t row0 = (int64_t)bseq * L;
  const int ld = 3 * H;
  const int q = qt * 32 + qh * 16 + c;  // this lane's query (B-operand column)
  const int key = kw * 16 + c;          // this lane's key (A-operand row)

  // operands: lane (c, g) holds d = 16 s + 4 g + t at MFMA step (s, t) in both
  floatx4 qf[4], kf[4];
  {
    const float* qs = qkv + (row0 + min(q, L - 1)) * ld + h * kDh + 4 * g;
    const float* ks = qkv + (row0 + min(key, L - 1)) * ld + H + h * kDh + 4 * g;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      qf[s] = *reinterpret_cast<const floatx4*>(qs + 16 * s) * scale;
      kf[s] = *reinterpret_cast<const floatx4*>(ks + 16 * s);
    }
  }
  // V^T operand of the PV step: d = 16 db + c, key = kw * 16 + 4 g + t
  float vf[4][4];
  {
    const float* vs = qkv + row0 * ld + 2 * H + h * kDh + c;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int kk = min(kw * 16 + 4 * g + t, L - 1);
#pragma unroll
      for (int db = 0; db < 4; ++db) vf[db][t] = vs[(int64_t)kk * ld + 16 * db];
    }
  }
  const bool kvalid = key < L && mask[row0 + min(key, L - 1)] != 0;
  const unsigned kbits = (unsigned)(__ballot(kvalid) & 0xFFFFull);  // bit k: key kw*16+k usable

  floatx4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s][t], qf[s][t], s0, 0, 0, 0);
      s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s + 2][t], qf[s + 2][t], s1, 0, 0, 0);
    }
  // accumulator j = S^T[key kw*16 + 4g + j][query c]
  floatx4 st = s0 + s1;
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    st[j] = ((kbits >> (4 * g + j)) & 1u) ? st[j] : -INFINITY;
    mx = fmaxf(mx, st[j]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  if (g == 0) smax[qh][kw][c] = mx;
  __syncthreads();
  const float m = fmaxf(fmaxf(smax[qh][0][c], smax[qh][1][c]), fmaxf(smax[qh][2][c], smax[qh][3][c]));
  float ls = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    st[j] = (st[j] == -INFINITY) ? 0.f : expf(st[j] - m);
    ls += st[j];
  }
  ls += __shfl_xor(ls, 16);
  ls += __shfl_xor(ls, 32);
  if (g == 0) ssum[qh][kw][c] = ls;
  floatx4 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    o[db] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) o[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[db][t], st[t], o[db], 0, 0, 0);
  }
  // o[db][j] = O^T[d = 16 db + 4 g + j][query c] over this wave's 16 keys
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int j = 0; j < 4; ++j) opart[qh][kw][c][16 * db + 4 * g + j] = o[db][j];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int idx = e * 512 + (int)threadIdx.x;  // (query of the tile, d), d fastest
    const int q32 = idx >> 6, d = idx & 63;
    const int qq = q32 >> 4, qc = q32 & 15;
    const float v = ((opart[qq][0][qc][d] + opart[qq][1][qc][d]) + opart[qq][2][qc][d]) + opart[qq][3][qc][d];
    const float l = ((ssum[qq][0][qc] + ssum[qq][1][qc]) + ssum[qq][2][qc]) + ssum[qq][3][qc];
    const int qrow = qt * 32 + q32;
    if (qrow < L) ctx[(row0 + qrow) * H + h * kDh + d] = v * (l > 0.f ? 1.0f / l : 0.f);
  }
}

// K3o: attention + output projection of the few-row forward in ONE launch (L <= 64 keys;
// one attention launch per layer fewer).  Workgroup (column tile, query tile, head group):
// 8 waves; waves 0..HG-1 each run one head of the group for the tile's <= 16 queries of
// one sequence (all its keys), as attention_rows_kernel does on v_mfma_f32_16x16x4_f32 but
// with the whole key range in one wave (softmax max / sum by two cross-lane-group
// shuffles, no LDS exchange), and leave ctx[query][head group's 64 HG dims] in LDS; then
// all 8 waves multiply it by the group's K slice of Wo^T for the tile's 32 output columns
// (2 column blocks x 4 K quarters, partial tiles summed in order through LDS).  Group g
// writes output plane g (planes = heads / HG; the next FFN-up sums them while it
// normalises, as QKV sums FFN-down's split-K planes); plane 0 carries bias + residual.
// The attention of a query tile is recomputed by each of the H / 32 column tiles: HG heads
// x 16 queries x L keys of f32 MFMA per workgroup (~1.5 us at L = 32), cheaper than the
// separate launch and its boundary it replaces.
// Rows: output row r of the projection is query position q = r % rps of sequence
// b = r / rps (rps = L, or 1 for the CLS-only last layer: query 0, compact rows).
constexpr int kOpCols = 32;  // output columns per workgroup

// QF: qkv in frag16 with V^T blocks (QKV's FL_O | FL_OT; needs L % 16 == 0, so every
// sequence starts a 16-row block): Q, K and V^T fragments load as whole 1 KB blocks.
// ACC: the head groups add into ONE zeroed output plane (two groups: FL_ACC's argument).
template <int HG, int NKB, bool QF = false, bool ACC = false>
__global__ __launch_bounds__(512) void attn_oproj_rows_kernel(
    const float* __restrict__ qkv, const int* __restrict__ mask, int L, int H, int rps, int qtiles,
    float scale, const float* __restrict__ Wo, const float* __restrict__ bo,
    const float* __restrict__ resid, int ldr, float* __restrict__ out, int64_t o_plane, int nt_w) {
  // NKB = ceil(L / 16) key blocks (compile time: every operand load below is issued before
  // the first MFMA, one memory round trip for the whole launch)
  constexpr int KG = HG * kDh;     // K depth of this group's slice of the projection
  constexpr int CS = KG + 4;       // LDS row stride of ctx (conflict-free ds_read_b128)
  constexpr int KQ = KG / 4;       // K per quarter
  constexpr int NJ = KQ / 16;      // float4 per lane per operand in a quarter
  __shared__ __attribute__((aligned(16))) float ctx[16 * CS];
  __shared__ float part[8][256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int b = blockIdx.y / qtiles, q0 = (blockIdx.y % qtiles) * 16;
  const int grp = blockIdx.z, h0 = grp * HG;
  const int n0 = blockIdx.x * kOpCols;
  const int64_t srow0 = (int64_t)b * L;  // first qkv row of the sequence
  const int ld = 3 * H;

  KTRACE_R(3, 0);
  // projection operands of phase B, in flight from the start: wave w = (column block cb,
  // K quarter kqr); lane (c, g) holds W[n0 + 16 cb + c][k] at k = kqr KQ + 16 j + 4 g + t
  const int cb = w & 1, kqr = w >> 1;
  floatx4 wv[NJ];
  {  // Wo's frag16 image: block ((n0 + 16 cb) / 16, (h0 kDh + kqr KQ) / 16 + j)
    const __amdgpu_buffer_rsrc_t wr = w_rsrc(Wo);
    const int wo4 = ((((n0 >> 4) + cb) * (H >> 4) + ((h0 * kDh + kqr * KQ) >> 4)) * 64 + lane) * 16;
#pragma unroll
    for (int j = 0; j < NJ; ++j) wv[j] = load_w(wr, wo4 + 1024 * j, nt_w);
  }
  // epilogue element of threads < 512: column block et >> 8, row (et & 255) / 16
  const int et = threadIdx.x, ecb = et >> 8, erow_t = (et & 255) >> 4, ecol = n0 + ecb * 16 + (et & 15);
  const int qrow = q0 + erow_t;  // query position of the element's row within the sequence
  const int64_t orow = (int64_t)b * rps + qrow;
  float ebias = 0.f, eres = 0.f;
  if (grp == 0 && qrow < rps) {
    ebias = bo[ecol];
    eres = resid[orow * ldr + ecol];
  }

  if (w < HG) {
    const int h = h0 + w;
    // operands, all requested up front: Q (d = 16 s + 4 g + t for query c; rps == 1:
    // query 0), K per key block (key 16 kb + c), V^T per key block (key 16 kb + 4 g + t,
    // d = 16 db + c), the key mask
    const int qpos = rps == 1 ? 0 : min(q0 + c, L - 1);
    floatx4 qf[4], kf[NKB][4];
    float vf[NKB][4][4];
    if constexpr (QF) {
      // block (row block, column block) of the [rows][3H] frag16 image; lane = (c, g)
      const floatx4* f4 = reinterpret_cast<const floatx4*>(qkv);
      const int cbs = ld >> 4;
      const int64_t rb0 = srow0 >> 4;
      auto blk = [&](int64_t rb, int cb) { return f4 + (rb * cbs + cb) * 64 + lane; };
      // (rps == 1: rows c of block 0 - query 0 is row c = 0, the only one stored)
#pragma unroll
      for (int sI = 0; sI < 4; ++sI) qf[sI] = *blk(rb0 + (q0 >> 4), ((h * kDh) >> 4) + sI);
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int sI = 0; sI < 4; ++sI) kf[kb][sI] = *blk(rb0 + kb, ((H + h * kDh) >> 4) + sI);
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int db = 0; db < 4; ++db) {  // V^T block: (d = 16 db + c, key = 16 kb + 4 g + t)
          const floatx4 v = *blk(rb0 + kb, ((2 * H + h * kDh) >> 4) + db);
#pragma unroll
          for (int t = 0; t < 4; ++t) vf[kb][db][t] = v[t];
        }
    } else {
      const float* qs = qkv + (srow0 + qpos) * ld + h * kDh + 4 * g;
#pragma unroll
      for (int sI = 0; sI < 4; ++sI) qf[sI] = *reinterpret_cast<const floatx4*>(qs + 16 * sI);
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        const float* ks = qkv + (srow0 + min(kb * 16 + c, L - 1)) * ld + H + h * kDh + 4 * g;
#pragma unroll
        for (int sI = 0; sI < 4; ++sI) kf[kb][sI] = *reinterpret_cast<const floatx4*>(ks + 16 * sI);
      }
      const float* vs = qkv + srow0 * ld + 2 * H + h * kDh + c;
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int64_t kk = min(kb * 16 + 4 * g + t, L - 1);
#pragma unroll
          for (int db = 0; db < 4; ++db) vf[kb][db][t] = vs[kk * ld + 16 * db];
        }
    }
    const bool kval = lane < L && mask[srow0 + min(lane, L - 1)] != 0;
    const unsigned long long kbits = __ballot(kval);  // bit k: key k usable
#pragma unroll
    for (int sI = 0; sI < 4; ++sI) qf[sI] *= scale;
    KTRACE_R(3, 1);  // operands landed
    floatx4 st[NKB];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      floatx4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kb][0][t], qf[0][t], a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kb][2][t], qf[2][t], a1, 0, 0, 0);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kb][1][t], qf[1][t], a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kb][3][t], qf[3][t], a1, 0, 0, 0);
      }
      st[kb] = a0 + a1;  // st[kb][j] = S^T[key 16 kb + 4 g + j][query c]
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int key = kb * 16 + 4 * g + j;
        st[kb][j] = ((kbits >> key) & 1ull) ? st[kb][j] : -INFINITY;
        mx = fmaxf(mx, st[kb][j]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float ls = 0.f;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        st[kb][j] = (st[kb][j] == -INFINITY) ? 0.f : expf(st[kb][j] - mx);
        ls += st[kb][j];
      }
    ls += __shfl_xor(ls, 16);
    ls += __shfl_xor(ls, 32);
    const float inv = ls > 0.f ? 1.0f / ls : 0.f;
    // O^T[d][query] = V^T P^T: A = V[key 16 kb + 4 g + t][d = 16 db + c], B = st[kb][t]
    floatx4 o[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      o[db] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int t = 0; t < 4; ++t) o[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[kb][db][t], st[kb][t], o[db], 0, 0, 0);
    }
    // o[db][j] = O^T[d = 16 db + 4 g + j][query c]
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int j = 0; j < 4; ++j) ctx[c * CS + w * kDh + 16 * db + 4 * g + j] = o[db][j] * inv;
    KTRACE_R(3, 2);  // attention done (wave 0)
  }
  __syncthreads();
  KTRACE_R(3, 3);
  // phase B: partial [16 rows][16 cols] of column block cb over K quarter kqr, as two
  // interleaved accumulation chains (one chain of NJ * 4 dependent MFMAs waits out each
  // one's latency)
  floatx4 acc2[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const floatx4 av = *reinterpret_cast<const floatx4*>(&ctx[c * CS + kqr * KQ + 16 * j + 4 * g]);
#pragma unroll
    for (int t = 0; t < 4; ++t) acc2[j & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], wv[j][t], acc2[j & 1], 0, 0, 0);
  }
  const floatx4 acc = acc2[0] + acc2[1];
  KTRACE_R(3, 4);
  // acc[j] = (row 4 g + j, column c) of the partial
#pragma unroll
  for (int j = 0; j < 4; ++j) part[w][(4 * g + j) * 16 + c] = acc[j];
  __syncthreads();
  KTRACE_R(3, 5);
  const int e = et & 255;
  float v = part[ecb][e];
#pragma unroll
  for (int q = 1; q < 4; ++q) v += part[ecb + 2 * q][e];
  if (qrow >= rps) return;
  if (grp == 0) v = (v + ebias) + eres;
  if (ACC)
    (void)atomicAdd(out + orow * H + ecol, v);
  else
    out[grp * o_plane + orow * H + ecol] = v;
  KTRACE_R(3, 6);
}

// --------------------------------------------------------------- K7 pool -----
// One wave per sequence: CLS row (or masked mean over rows), then x / max(||x||, 1e-12).
// raw != 0 (one uniform flag of every tail; scoring, mq_encoder_score): the pooled row as it
// is, the final LayerNorm's output - the cross-encoder head's input.  x * 1.0f is x, so the
// embedding path's arithmetic is what it was.
template <int VPL>
__global__ __launch_bounds__(256) void pool_kernel(const float* __restrict__ hs,
                                                   const int* __restrict__ mask, int B, int L,
                                                   int pooling, float* __restrict__ out, int raw) {
  constexpr int H = VPL * 256;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  floatx4 x[VPL];
  if (pooling == MQ_POOL_MEAN) {
    float cnt = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) x[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < L; ++r) {
      if (!mask[(int64_t)b * L + r]) continue;
      cnt += 1.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i)
        x[i] += *reinterpret_cast<const floatx4*>(hs + ((int64_t)b * L + r) * H + (i * 64 + lane) * 4);
    }
    const float inv = 1.0f / fmaxf(cnt, 1.f);
#pragma unroll
    for (int i = 0; i < VPL; ++i) x[i] *= inv;
  } else {
#pragma unroll
    for (int i = 0; i < VPL; ++i)
      x[i] = *reinterpret_cast<const floatx4*>(hs + (int64_t)b * L * H + (i * 64 + lane) * 4);
  }
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) ss += x[i].x * x[i].x + x[i].y * x[i].y + x[i].z * x[i].z + x[i].w * x[i].w;
  const float inv = raw ? 1.0f : 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
  for (int i = 0; i < VPL; ++i)
    *reinterpret_cast<floatx4*>(out + (int64_t)b * H + (i * 64 + lane) * 4) = x[i] * inv;
}

// K7 for the few-row path, whose last layer leaves pre-LayerNorm rows as `planes`
// split-K planes (`plane` floats apart, summed in order): LN (g, be) of the pooled rows,
// then pool and L2-normalise as pool_kernel.  `rows` = rows per sequence in hs (1: the
// compact CLS rows of the pruned last layer).
template <int VPL>
__global__ __launch_bounds__(256) void ln_pool_kernel(const float* __restrict__ hs, int planes,
                                                      int64_t plane, const int* __restrict__ mask,
                                                      int B, int L, int rows, int pooling,
                                                      const float* __restrict__ g,
                                                      const float* __restrict__ be, float eps,
                                                      float* __restrict__ out, int raw) {
  constexpr int H = VPL * 256;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  auto ln_row = [&](const float* src, floatx4 (&x)[VPL]) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) x[i] = *reinterpret_cast<const floatx4*>(src + (i * 64 + lane) * 4);
    for (int z = 1; z < planes; ++z)
#pragma unroll
      for (int i = 0; i < VPL; ++i) x[i] += *reinterpret_cast<const floatx4*>(src + z * plane + (i * 64 + lane) * 4);
    float mu, rs;
    ln_row_stats<VPL>(x, eps, mu, rs);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = (i * 64 + lane) * 4;
      x[i] = (x[i] - mu) * rs * *reinterpret_cast<const floatx4*>(g + c) +
             *reinterpret_cast<const floatx4*>(be + c);
    }
  };
  floatx4 x[VPL];
  if (pooling == MQ_POOL_MEAN) {
    float cnt = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) x[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < L; ++r) {
      if (!mask[(int64_t)b * L + r]) continue;
      cnt += 1.f;
      floatx4 y[VPL];
      ln_row(hs + ((int64_t)b * rows + r) * H, y);
#pragma unroll
      for (int i = 0; i < VPL; ++i) x[i] += y[i];
    }
    const float inv = 1.0f / fmaxf(cnt, 1.f);
#pragma unroll
    for (int i = 0; i < VPL; ++i) x[i] *= inv;
  } else {
    ln_row(hs + (int64_t)b * rows * H, x);
  }
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) ss += x[i].x * x[i].x + x[i].y * x[i].y + x[i].z * x[i].z + x[i].w * x[i].w;
  const float inv = raw ? 1.0f : 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
  for (int i = 0; i < VPL; ++i)
    *reinterpret_cast<floatx4*>(out + (int64_t)b * H + (i * 64 + lane) * 4) = x[i] * inv;
}

// ------------------------------------------- CLS attention without K and V ----
// With CLS pooling the last layer attends from ONE query per sequence, so neither K nor V of
// its tokens is needed (MQ_ENC_OPT_CLS_KFREE).  For head h of sequence b, with X the layer's
// input rows, q the CLS query and Wk_h / Wv_h the head's 64 rows of Wk / Wv:
//   score[t] = x_t . u / sqrt(dh) + q . bk_h      u = Wk_h^T q           (gemm_heads_kernel)
//   z        = sum_t softmax(score)[t] x_t                               (cls_pass_kernel)
//   ctx      = Wv_h z + bv_h                                             (gemm_heads_kernel)
// q . bk_h is the same for every key and drops out of the softmax; sum_t p[t] = 1 carries bv
// through.  The all-token [M, 2H] projection and the attention launch become two B-row GEMMs
// and one pass over X: the same sums re-associated, fp32 throughout.

// W [R][C] -> out [C][R] (Wk^T of the last layer, once per weight load).
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ W, int R, int C,
                                                        float* __restrict__ out) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  for (int j = ty; j < 32; j += 8)
    if (r0 + j < R && c0 + tx < C) tile[j][tx] = W[(int64_t)(r0 + j) * C + c0 + tx];
  __syncthreads();
  for (int j = ty; j < 32; j += 8)
    if (c0 + j < C && r0 + tx < R) out[(int64_t)(c0 + j) * R + r0 + tx] = tile[tx][j];
}

// One exact-f32 GEMM per head in one launch: for head h, out_h[M][N] = A_h[M][K] . W_h[N][K]^T
// (+ live[row] bias[h N + col]), with A_h = A + h a_head (row stride lda), W_h = W + h w_head
// (row stride ldw), out_h = out + h o_head (row stride ldo).  Workgroup (h, tile, s) runs its
// tile over K-chunk s of S and writes plane s (o_plane floats apart; S = 1: the bias goes in
// here) - every stored element is one k-ordered MFMA chain, whatever M is.  An exact-f32 MFMA
// chain is serial in k (64 cycles a step), so the deep product is cut into kClsCtxSplits
// chunks, a constant: the planes are summed in order by cls_ctx_reduce_kernel.
//   u   = Wk_h^T q:  A = q [B][H] (a_head 64), W = Wk^T [H][H] (w_head 64), K = 64, N = H
//   ctx = Wv_h z:    A = z [B][heads][H] (a_head H), W = Wv (w_head 64 H), K = H, N = 64, S = 4
constexpr int kClsCtxSplits = 4;
template <class T>
__global__ __launch_bounds__(256, 2) void gemm_heads_kernel(const float* __restrict__ A, int lda, int a_head,
                                                            const float* __restrict__ W, int ldw, int w_head,
                                                            const float* __restrict__ bias,
                                                            const float* __restrict__ live, int M, int N, int K,
                                                            float* __restrict__ out, int ldo, int o_head, int S,
                                                            int64_t o_plane) {
  __shared__ __attribute__((aligned(16))) float lds[2 * T::STAGE_FLOATS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / T::WAVES_N, wn = wave % T::WAVES_N;
  const int tiles_n = (N + T::BN - 1) / T::BN;
  const int per_head = ((M + T::BM - 1) / T::BM) * tiles_n;
  const int sidx = blockIdx.x % S, ht = blockIdx.x / S;
  const int head = ht / per_head, tile = ht % per_head;
  const int Kc = K / S;
  const int m0 = (tile / tiles_n) * T::BM;
  const int n0 = (tile % tiles_n) * T::BN;
  auto coords = [&](int, int& mm0, int64_t& nn0) {
    mm0 = m0;
    nn0 = n0;
  };
  float* dst = out + sidx * o_plane + (int64_t)head * o_head;
  auto epi = [&](int, floatx16(&acc)[T::TM][T::TN], float*) {
#pragma unroll
    for (int tn = 0; tn < T::TN; ++tn) {
      const int col = n0 + wn * T::WN + tn * 32 + (lane & 31);
      if (col >= N) continue;
      const float bv = bias ? bias[head * N + col] : 0.f;
#pragma unroll
      for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = m0 + wm * T::WM + acc_row(tm, e, lane);
          if (row < M) dst[(int64_t)row * ldo + col] = bias ? __fmaf_rn(live[row], bv, acc[tm][tn][e]) : acc[tm][tn][e];
        }
    }
  };
  walk_tiles<T>(lds, 1,
                TileOperands{A + (int64_t)head * a_head + sidx * Kc, lda, M, W + (int64_t)head * w_head + sidx * Kc, ldw,
                             N, Kc},
                coords, epi);
}

// ctx [B][H] = the kClsCtxSplits planes of Wv_h z summed in order + live[row] bv (float4 each).
__global__ __launch_bounds__(256) void cls_ctx_reduce_kernel(const float* __restrict__ part, int B, int H,
                                                             const float* __restrict__ bv,
                                                             const float* __restrict__ live,
                                                             float* __restrict__ ctx) {
  const int64_t i4 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n4 = H / 4;
  if (i4 >= (int64_t)B * n4) return;
  const int row = (int)(i4 / n4), c = (int)(i4 % n4) * 4;
  floatx4 v = sum_slabs(part + (int64_t)row * H + c, (int64_t)B * H, kClsCtxSplits);
  const float lv = live[row];
  const floatx4 b = *reinterpret_cast<const floatx4*>(bv + c);
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = __fmaf_rn(lv, b[j], v[j]);
  *reinterpret_cast<floatx4*>(ctx + (int64_t)row * H + c) = v;
}

// The pass over the last layer's input rows: one workgroup per sequence with one wave per head
// (H threads).  Rows arrive once, kClsChunk at a time, into LDS (the next chunk's loads in
// flight under this one's arithmetic).  Wave h keeps head h's u in registers, takes its dot
// products with the chunk's rows and advances the head's online softmax on lanes 0..15, one
// key each (running max / sum, the chunk's probabilities, the rescale alpha of what is
// accumulated); then thread c adds the chunk into column c of every head's z.  Any L: the
// state is O(1) in it.
// FOLD: x holds raw rows y with (mean, M2) partials (the LayerNorm-fold layers leave LN2
// unapplied): a row is staged as n_t = (y_t - mu_t) rho_t (ln_merge, as every other consumer) and
// gamma / beta are applied algebraically - score = n_t . (g o u) (+ beta . u, the same for every
// key: dropped with q . bk), z = g o sum_t p_t n_t + beta.
// A key with mask 0 gets probability exactly 0; a sequence with no live key gets z = 0, live = 0
// (ctx = 0 then, as attention_kernel gives).  Nothing here depends on B or on blockIdx beyond
// the sequence's own rows.
constexpr int kClsChunk = 16;
template <int VPL, bool FOLD>
__global__ __launch_bounds__(256 * VPL) void cls_pass_kernel(const float* __restrict__ x,
                                                             const float* __restrict__ stats,
                                                             const float* __restrict__ g,
                                                             const float* __restrict__ be, float eps,
                                                             const float* __restrict__ u,
                                                             const int* __restrict__ mask, int L, float scale,
                                                             float* __restrict__ z, float* __restrict__ live) {
  constexpr int H = VPL * 256, HEADS = H / kDh, CH = kClsChunk;
  constexpr int TPR = H / CH;  // threads per staged row: 4 float4 each
  static_assert(CH == 16 && (CH * H + CH * HEADS + 2 * HEADS) * 4 <= 64 * 1024, "LDS: one chunk of rows, scores");
  __shared__ __attribute__((aligned(16))) float xs[CH * H];
  __shared__ __attribute__((aligned(16))) float ps[CH * HEADS];  // [key][head] probabilities
  __shared__ __attribute__((aligned(16))) float alpha_s[HEADS];
  __shared__ float l_s[HEADS];
  const int t = threadIdx.x, lane = t & 63, h = t >> 6;
  const int b = blockIdx.x;
  const int64_t row0 = (int64_t)b * L;
  const int lrow = t / TPR, lc4 = t % TPR;  // this thread's row of a chunk and first float4 in it
  floatx4 ur[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    ur[i] = *reinterpret_cast<const floatx4*>(u + ((int64_t)b * HEADS + h) * H + (i * 64 + lane) * 4);
    if constexpr (FOLD) ur[i] *= *reinterpret_cast<const floatx4*>(g + (i * 64 + lane) * 4);
  }
  floatx4 xr[4], sr[kLnMaxParts / 2];
  int mk = 0;
  auto fetch = [&](int k0) {
    const int64_t row = row0 + min(k0 + lrow, L - 1);  // rows past L repeat the last (probability 0)
#pragma unroll
    for (int j = 0; j < 4; ++j) xr[j] = *reinterpret_cast<const floatx4*>(x + row * H + (lc4 + TPR * j) * 4);
    if constexpr (FOLD) {
      const floatx4* sp = reinterpret_cast<const floatx4*>(stats + row * (2 * kLnMaxParts));
#pragma unroll
      for (int i = 0; i < kLnMaxParts / 2; ++i) sr[i] = sp[i];
    }
    mk = lane < CH && k0 + lane < L ? mask[row0 + k0 + lane] : 0;
  };
  float zacc[HEADS];
#pragma unroll
  for (int hh = 0; hh < HEADS; ++hh) zacc[hh] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;  // head h's softmax state, the same on every lane of wave h
  fetch(0);
  for (int k0 = 0; k0 < L; k0 += CH) {
    if constexpr (FOLD) {
      float mu, rho;
      ln_merge(sr, eps, mu, rho);
#pragma unroll
      for (int j = 0; j < 4; ++j) xr[j] = (xr[j] - mu) * rho;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<floatx4*>(xs + lrow * H + (lc4 + TPR * j) * 4) = xr[j];
    const int live_key = mk;
    __syncthreads();
    if (k0 + CH < L) fetch(k0 + CH);
    // head h: the chunk's dot products, every lane ending with all of them
    float d[CH];
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const floatx4 v = *reinterpret_cast<const floatx4*>(xs + k * H + (i * 64 + lane) * 4);
        a = fmaf(v.x, ur[i].x, fmaf(v.y, ur[i].y, fmaf(v.z, ur[i].z, fmaf(v.w, ur[i].w, a))));
      }
      d[k] = a;
    }
#pragma unroll
    for (int k = 0; k < CH; ++k) d[k] = wave_sum_fast(d[k]);
    // lanes 0..15: key k0 + lane (the other lanes carry -inf / 0 through the 16-lane reductions)
    float sc = -INFINITY;
#pragma unroll
    for (int k = 0; k < CH; ++k) sc = lane == k ? d[k] : sc;
    sc = live_key != 0 ? sc * scale : -INFINITY;
    float tmax = sc;
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) tmax = fmaxf(tmax, __shfl_xor(tmax, off));
    tmax = __shfl(tmax, 0);
    const float m_new = fmaxf(m_run, tmax);
    const float alpha = m_new == -INFINITY ? 1.f : expf(m_run - m_new);
    const float p = sc == -INFINITY ? 0.f : expf(sc - m_new);
    float psum = p;
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) psum += __shfl_xor(psum, off);
    psum = __shfl(psum, 0);
    l_run = l_run * alpha + psum;
    m_run = m_new;
    if (lane < CH) ps[lane * HEADS + h] = p;
    if (lane == 0) alpha_s[h] = alpha;
    __syncthreads();
    // column t of every head's z
#pragma unroll
    for (int q4 = 0; q4 < HEADS / 4; ++q4) {
      const floatx4 a = *reinterpret_cast<const floatx4*>(alpha_s + 4 * q4);
#pragma unroll
      for (int e = 0; e < 4; ++e) zacc[4 * q4 + e] *= a[e];
    }
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const float xv = xs[k * H + t];
#pragma unroll
      for (int q4 = 0; q4 < HEADS / 4; ++q4) {
        const floatx4 pp = *reinterpret_cast<const floatx4*>(ps + k * HEADS + 4 * q4);
#pragma unroll
        for (int e = 0; e < 4; ++e) zacc[4 * q4 + e] = fmaf(pp[e], xv, zacc[4 * q4 + e]);
      }
    }
    __syncthreads();  // the next chunk overwrites xs / ps
  }
  if (lane == 0) l_s[h] = l_run;
  __syncthreads();
#pragma unroll
  for (int hh = 0; hh < HEADS; ++hh) {
    const float l = l_s[hh];
    float v = l > 0.f ? zacc[hh] * (1.0f / l) : 0.f;
    if constexpr (FOLD) v = l > 0.f ? fmaf(v, g[t], be[t]) : 0.f;
    z[((int64_t)b * HEADS + hh) * H + t] = v;
  }
  if (t == 0) live[b] = l_s[0] > 0.f ? 1.f : 0.f;
}

}  // namespace mq

// ================================================================ host side =====
using namespace mq;

namespace {

struct Buf {
  float* p = nullptr;
  size_t n = 0;  // floats
  int ensure(size_t need) {
    if (need <= n) return MQ_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    if (hipMalloc((void**)&p, need * sizeof(float)) != hipSuccess)
      MQ_FAIL(MQ_ENOMEM, "hipMalloc(%zu floats) failed", need);
    n = need;
    return MQ_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

struct LayerW {
  const float *wqkv, *bqkv, *wo, *bo, *ln1g, *ln1b, *w1, *b1, *w2, *b2, *ln2g, *ln2b;
  // W3 plane images of the four projection weights (gemm_x6p.hpp), built when the split-f32
  // precision is selected; null otherwise
  const unsigned char *wqkv3 = nullptr, *wo3 = nullptr, *w13 = nullptr, *w23 = nullptr;
  // frag16 images of the same four (the few-row kernels' weight operands)
  const float *wqkvf = nullptr, *wof = nullptr, *w1f = nullptr, *w2f = nullptr;
  // LayerNorm fold (build_fold): w1 scaled by this layer's ln1 gamma and wqkv by the PREVIOUS
  // layer's ln2 gamma (layers >= 1) as W3 images (x6_presplit) or fp32 (the re-split tiles),
  // and the fold's s / c vectors
  const unsigned char *w1g3 = nullptr, *wqkvg3 = nullptr;
  const float *w1gf = nullptr, *wqkvgf = nullptr;
  const float *w1s = nullptr, *w1c = nullptr, *wqkvs = nullptr, *wqkvc = nullptr;
};

int64_t weight_count(const mq_bert_config& c) {
  const int64_t H = c.hidden, F = c.ffn;
  const int64_t per_layer = 3 * H * H + 3 * H + H * H + H + 2 * H + F * H + F + H * F + H + 2 * H;
  return ((int64_t)c.vocab_size + c.max_positions + c.type_vocab) * H + 2 * H + c.layers * per_layer;
}

}  // namespace


namespace {

struct GemmArgs {
  float* slab;  // split-K workspace (may be null: never split)
  size_t slab_floats;
  const float* A;
  int lda;
  const float* W;
  const float* bias;
  const float* resid;
  int ldr;
  float* out;
  int ldo;
  int M, N, K;
  int nt = 0;  // few-row split-K launches: weights load non-temporally (layers past resident_layers)
  const void* W3 = nullptr;  // split-f32: W's W3 plane image (K2p, gemm_x6p.hip)
  LnFold lf{};               // the LayerNorm-fold epilogues (launch_gemm_fold)
  bool former_epi = false;   // K2p: the single-wave GELU epilogue (MQ_ENC_OPT_EPI_SPLIT 0)
};

template <class T, int EPI>
void launch_gemm_t(const GemmArgs& g, int num_cus, hipStream_t s) {
  const int tiles = ((g.M + T::BM - 1) / T::BM) * ((g.N + T::BN - 1) / T::BN);
  // persistent grid: the workgroups that fit the CUs at once, a multiple of 8
  const int grid = (std::min(tiles, T::WG_PER_CU * num_cus) + 7) / 8 * 8;
  const int tiles_m = (g.M + T::BM - 1) / T::BM, tiles_n = (g.N + T::BN - 1) / T::BN;
  const int rx = region_pick_rx(tiles_m, tiles_n, (double)T::BM * g.K * 4, (double)T::BN * g.K * 4, grid);
  hipLaunchKernelGGL((gemm_nt_kernel<T, EPI>), dim3(grid), dim3(T::THREADS), 0, s, g.A, g.lda, g.W,
                     g.bias, g.resid, g.ldr, g.out, g.ldo, g.M, g.N, g.K, rx, g.lf);
}

using GemmBig = F32Tile<2, 2, 2, 2>;    // 128 x 128
using GemmT96 = F32Tile<4, 1, 1, 3>;    // 128 x 96
using GemmMid = F32Tile<2, 2, 2, 1>;    // 128 x 64
using GemmSmall = F32Tile<1, 4, 1, 1>;  // 32 x 128  (few rows)

// Pick the tile whose launch wastes the least: every CU runs two workgroups at a time,
// so a grid that is not a multiple of 2*CUs idles part of the chip in its last round
// (M = 8192: N = 768 -> 128x96 gives exactly 512 tiles; 2304 -> 1536).  Cost model:
// rounds * tile area / relative tile efficiency.
// (the encoder's split-f32 tiles take K2p's arithmetic: the 16x16x32 MFMA, F32Tile::M16)
using X6Big = F32Tile<2, 2, 2, 2, true, 2, false, 0, false, true>;  // 128 x 128, split-f32
using X6T96 = F32Tile<4, 1, 1, 3, true, 2, false, 0, false, true>;  // 128 x 96
using X6Mid = F32Tile<2, 2, 2, 1, true, 2, false, 0, false, true>;  // 128 x 64
using X6W192 = F32Tile<4, 2, 1, 3, true, 2, false, 0, false, true>;  // 128 x 192, 8 waves

// Tile codes (also the mq_debug_gemm_f32 `tile` argument): 0-3 exact f32 128x128 /
// 128x96 / 128x64 / 32x128, 4 split-K (host path only), 5-7 split-f32 128x128 / 128x96
// / 128x64, 8 / 9 exact / split-f32 128x192 with 8-wave workgroups (one per CU; measured
// within run-to-run noise of the 4-wave tiles, kept as a test of the 8-wave walker).
template <int EPI>
void launch_gemm_tile(const GemmArgs& g, int tile, int num_cus, hipStream_t s) {
  switch (tile) {
    case 0: launch_gemm_t<GemmBig, EPI>(g, num_cus, s); return;
    case 1: launch_gemm_t<GemmT96, EPI>(g, num_cus, s); return;
    case 2: launch_gemm_t<GemmMid, EPI>(g, num_cus, s); return;
    case 5: launch_gemm_t<X6Big, EPI>(g, num_cus, s); return;
    case 6: launch_gemm_t<X6T96, EPI>(g, num_cus, s); return;
    case 7: launch_gemm_t<X6Mid, EPI>(g, num_cus, s); return;
    case 8: launch_gemm_t<F32Tile<4, 2, 1, 3>, EPI>(g, num_cus, s); return;         // 128x192, 8 waves
    case 9: launch_gemm_t<X6W192, EPI>(g, num_cus, s); return;                       // x6 128x192
    default: launch_gemm_t<GemmSmall, EPI>(g, num_cus, s); return;
  }
}

// Split-K factor for a GEMM that would under-fill the chip (0 = run it directly):
// enough chunks for ~2 workgroups per CU, each chunk a multiple of 32 deep.
int splitk_factor(const GemmArgs& g, int num_cus, int cap = 16, int tiles_max = 0) {
  if (!g.slab || g.N % 4 != 0) return 0;
  const int64_t tiles = (int64_t)((g.M + 31) / 32) * ((g.N + 127) / 128);  // 32 x 128 tiles
  const int64_t slots = 2 * (int64_t)num_cus;
  // split only grids of at most tiles_max direct tiles (0: one tile per CU)
  if (tiles > (tiles_max > 0 ? tiles_max : num_cus) || g.M > 256) return 0;
  const int slices = g.K / kBK;
  // At most 16 chunks: deeper splits fill more CUs but the slab traffic and the ordered
  // reduction grow with S (single query, L=32: encoder p50 0.74 ms at 16 vs 0.88 ms at
  // 64, 0.80 ms at 8).  MQ_ENC_OPT_SPLITK_MAX overrides it.
  int best = 1;
  for (int s = 1; s <= slices && s <= cap; ++s)
    if (slices % s == 0 && tiles * s <= slots && (size_t)s * g.M * g.N <= g.slab_floats) best = s;
  return best >= 2 ? best : 0;
}

// The split-K partial GEMM on the 32 x 128 tile (g.nt: non-temporal weight loads).
void launch_splitk_gemm(const GemmArgs& g, int S, hipStream_t s) {
  auto go = [&](auto tile) {
    using T = decltype(tile);
    const int tiles = ((g.M + T::BM - 1) / T::BM) * ((g.N + T::BN - 1) / T::BN);
    hipLaunchKernelGGL((gemm_splitk_kernel<T>), dim3(tiles * S), dim3(256), 0, s, g.A, g.lda, g.W, g.M, g.N, g.K,
                       S, g.slab);
  };
  if (g.nt)
    go(F32Tile<1, 4, 1, 1, false, 2, false, 0, true>{});
  else
    go(F32Tile<1, 4, 1, 1>{});
}

template <int EPI>
void launch_splitk(const GemmArgs& g, int S, hipStream_t s) {
  launch_splitk_gemm(g, S, s);
  const int64_t n4 = (int64_t)g.M * g.N / 4;
  hipLaunchKernelGGL((splitk_reduce_kernel<EPI>), dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0,
                     s, g.slab, S, g.M, g.N, g.bias, g.resid, g.ldr, g.out, g.ldo);
}

// the split-f32 tile (0 / 1 / 2 = 128 x 128 / 96 / 64) that wastes the least of its last round
int x6_tile_pick(const GemmArgs& g, int num_cus) {
  const int bns[3] = {128, 96, 64};
  const double effs[3] = {1.0, 0.96, 0.9};
  const int64_t slots = 2 * (int64_t)num_cus;
  int best = 0;
  double best_cost = 1e300;
  for (int i = 0; i < 3; ++i) {
    const int64_t tiles = (int64_t)((g.M + 127) / 128) * ((g.N + bns[i] - 1) / bns[i]);
    const double cost = (double)((tiles + slots - 1) / slots) * 128 * bns[i] / effs[i];
    if (cost < best_cost) {
      best_cost = cost;
      best = i;
    }
  }
  return best;
}

// A split-f32 GEMM with a LayerNorm-fold epilogue (g.lf; forward_vpl's gate has checked that
// it fills the chip).  K2p on the W3 image when there is one; else the split-f32 tiles that
// re-split both operands - the producer pinned to the 128 x 96 tile, whose wave tile is the
// partial width - with the same epilogue code on the same accumulators: the same bits.
template <int EPI>
void launch_gemm_fold(const GemmArgs& g, int num_cus, hipStream_t s) {
  if (g.W3) {
    X6pArgs a{g.A, g.lda, g.W3, g.bias, g.resid, g.ldr, g.out, g.ldo, g.M, g.N, g.K};
    a.lf = g.lf;
    a.former_epi = g.former_epi;
    launch_gemm_x6p(a, EPI, -1, num_cus, s);
    return;
  }
  if constexpr (EPI == EPI_RESID_LN_STATS) {
    launch_gemm_t<X6T96, EPI>(g, num_cus, s);
  } else {
    switch (x6_tile_pick(g, num_cus)) {
      case 0: launch_gemm_t<X6Big, EPI>(g, num_cus, s); return;
      case 1: launch_gemm_t<X6T96, EPI>(g, num_cus, s); return;
      default: launch_gemm_t<X6Mid, EPI>(g, num_cus, s); return;
    }
  }
}

template <int EPI>
void launch_gemm(const GemmArgs& g, int num_cus, hipStream_t s, bool x6 = false, int splitk_cap = 16,
                 int splitk_tiles = 0) {
  const int S = splitk_factor(g, num_cus, splitk_cap, splitk_tiles);
  if (S) {
    launch_splitk<EPI>(g, S, s);
    return;
  }
  // split-f32 pays where its tiles fill the chip; a GEMM of fewer rows (a long single
  // query: M = 512 is 48 K2p tiles on 256 CUs) runs the exact-f32 tiles instead - narrower
  // tiles spread further, and exact f32 is at least as accurate (L = 512 single query:
  // 3.09-3.16 ms p50 on either split-f32 path, 2.45 on exact f32)
  if (x6 && (int64_t)((g.M + 127) / 128) * ((g.N + 191) / 192) < num_cus) x6 = false;
  if (x6 && g.W3) {  // split-f32 on the pre-split weights (K2p)
    X6pArgs a{g.A, g.lda, g.W3, g.bias, g.resid, g.ldr, g.out, g.ldo, g.M, g.N, g.K};
    a.former_epi = g.former_epi;
    launch_gemm_x6p(a, EPI, -1, num_cus, s);
    return;
  }
  if (x6) {  // split-f32 tiles (both operands split while staged): same waste model over 128x{128,96,64}
    launch_gemm_tile<EPI>(g, 5 + x6_tile_pick(g, num_cus), num_cus, s);
    return;
  }
  struct Cand {
    int bm, bn;
    double eff;
  };
  const Cand cands[4] = {{128, 128, 1.0}, {128, 96, 0.96}, {128, 64, 0.9}, {32, 128, 0.55}};
  const int64_t slots = 2 * (int64_t)num_cus;
  int best = 0;
  double best_cost = 1e300;
  for (int i = 0; i < 4; ++i) {
    const int64_t tiles = (int64_t)((g.M + cands[i].bm - 1) / cands[i].bm) * ((g.N + cands[i].bn - 1) / cands[i].bn);
    const int64_t rounds = (tiles + slots - 1) / slots;
    const double cost = (double)rounds * cands[i].bm * cands[i].bn / cands[i].eff;
    if (cost < best_cost) {
      best_cost = cost;
      best = i;
    }
  }
  launch_gemm_tile<EPI>(g, best, num_cus, s);
}

// MQ_ENC_OPT_LN_FOLD's default (DESIGN.md section 4 has the A/B that decides it)
#ifndef MQ_LN_FOLD_DEFAULT
#define MQ_LN_FOLD_DEFAULT 1
#endif
constexpr bool kLnFoldDefault = MQ_LN_FOLD_DEFAULT != 0;
// MQ_ENC_OPT_CLS_KFREE's default (DESIGN.md section 4 has the A/B that decides it)
#ifndef MQ_CLS_KFREE_DEFAULT
#define MQ_CLS_KFREE_DEFAULT 1
#endif
constexpr bool kClsKfreeDefault = MQ_CLS_KFREE_DEFAULT != 0;
// MQ_ENC_OPT_QKV_ATTN's default (DESIGN.md section 4 has the A/B that decides it)
#ifndef MQ_QKV_ATTN_DEFAULT
#define MQ_QKV_ATTN_DEFAULT 1
#endif
constexpr bool kQkvAttnDefault = MQ_QKV_ATTN_DEFAULT != 0;
// MQ_ENC_OPT_EPI_SPLIT's default (DESIGN.md section 4 has the A/B that decides it)
#ifndef MQ_EPI_SPLIT_DEFAULT
#define MQ_EPI_SPLIT_DEFAULT 1
#endif
constexpr bool kEpiSplitDefault = MQ_EPI_SPLIT_DEFAULT != 0;

// Stage labels for the optional per-kernel-class event timeline.
enum Stage { ST_EMBED = 0, ST_QKV, ST_ATTN, ST_OPROJ, ST_LN, ST_FFN_UP, ST_FFN_DOWN, ST_POOL, ST_N };


}  // namespace

struct mq_encoder {
  int device = 0;
  PinBuf pin;  // pinned staging of the host-pointer embed path (few tokens)
  mq_bert_config cfg{};
  int precision = MQ_DTYPE_F32;
  bool loaded = false;
  Buf weights;
  const float *word = nullptr, *pos = nullptr, *typ = nullptr, *eg = nullptr, *eb = nullptr;
  std::vector<LayerW> layers;
  Buf x, y, qkv, ctx, ffn, io_out, slab;  // (+ lnst below)
  Buf w3;  // split-f32: every layer's W3 plane images (LayerW::*3 point into it)
  Buf wfrag;  // every layer's frag16 weight images (LayerW::*f point into it), built at load
  int* io_ids = nullptr;
  int* io_mask = nullptr;
  size_t io_tokens = 0;
  Timeline tl;
  int num_cus = 256;
  // Replayed forwards: one hipGraph per (B, L, precision, buffer set), captured on a
  // private stream from io_ids/io_mask to io_out and launched on the caller's stream.
  struct Graph {
    int B = 0, L = 0, precision = 0;
    std::vector<const void*> bufs;
    hipGraphExec_t exec = nullptr;
    uint64_t last_use = 0;
  };
  std::vector<Graph> graphs;
  // tuning options (mq_encoder_set_option)
  bool fuse_attn_oproj = true;  // few-row forward: K3o (attention + output projection)
  int rows_max = kRowsDefault;  // few-row forward up to this many token rows (0 = off)
  int rows_splits = 0;          // few-row FFN-down K splits (0 = automatic)
  int splitk_max = 16;          // deepest split-K of the tiled path's few-row GEMMs
  int splitk_tiles = 0;         // split-K only grids of <= this many 32x128 tiles (0 = num_cus)
  int resident_layers = 8;      // few-row forward: layers whose weights load with the default
                                // cache policy (8 x 28 MB of BERT-base fit the 256 MB MALL);
                                // later layers' loads are non-temporal
  bool x6_presplit = true;      // split-f32 batched GEMMs on the W3 images (K2p)
  bool ln_fold = kLnFoldDefault;  // split-f32 batched forward: LayerNorm folded into the GEMMs (LnFold)
  Buf lnst;                     // its per-row partials, two sets of [M][H / kLnPartW] (mean, M2)
  Buf wfold3, wfoldf, sfold;    // its gamma-scaled weights (W3 images / fp32) and s, c vectors
  bool rows_planes = false;     // few-row forward: keep the two-plane hand-offs (no FL_ACC merge)
  bool cls_kfree = kClsKfreeDefault;  // CLS pooling, batched forward: the last layer without K / V
  bool qkv_attn = kQkvAttnDefault;    // split-f32 batched forward, L = 32: attention in the QKV epilogue
  bool epi_split = kEpiSplitDefault;  // K2p's GELU epilogues shared out between both waves of each SIMD
  Buf wkt;                      // its Wk^T of the last layer [H][H], built at weight load
  Buf cls;                      // its [B] rows: normalised CLS rows, q (H each), u, z (heads H each), live
  // cross-encoder head (mq_encoder_load_head): Wp [H][H], bp [H], Wc [n_labels][H], bc [n_labels]
  Buf head;
  int n_labels = 0;             // 0 = no head loaded
  Buf cls_state;                // scoring: the raw tail's [B][H] CLS rows, K13's input
  int* io_types = nullptr;      // staged segment ids of the host-pointer score path
  size_t io_type_tokens = 0;
  bool use_graphs = false;  // eager measured faster for one query (0.628 vs 0.645 ms: the
                            // graph path stages ids / mask / out through its own buffers)
  uint64_t graph_clock = 0;
  hipStream_t cap_stream = nullptr;
  std::mutex mu;
};

namespace {

// Split-f32 precision: split every layer's four projection weights once into their W3
// plane images (gemm_x6p.hpp; 6 B per weight, 510 MB for BERT-base), which the batched
// GEMMs (K2p) multiply without re-splitting them.  No-op unless the precision is F32X6 and
// weights are loaded, or when the images exist.  Synchronous.
int build_w3(mq_encoder* e) {
  if (e->precision != MQ_DTYPE_F32X6 || !e->loaded || e->layers.empty() || e->layers[0].wqkv3) return MQ_OK;
  const mq_bert_config& c = e->cfg;
  const int H = c.hidden, F = c.ffn;
  const size_t per = w3_bytes(3 * H, H) + w3_bytes(H, H) + w3_bytes(F, H) + w3_bytes(H, F);
  DeviceGuard dg(e->device);
  int rc = e->w3.ensure((per * e->layers.size() + 3) / 4);
  if (rc) return rc;
  unsigned char* p = reinterpret_cast<unsigned char*>(e->w3.p);
  for (LayerW& w : e->layers) {
    auto one = [&](const float* W, int n, int k, const unsigned char*& dst) {
      launch_split_w3(W, n, k, p, nullptr);
      dst = p;
      p += w3_bytes(n, k);
    };
    one(w.wqkv, 3 * H, H, w.wqkv3);
    one(w.wo, H, H, w.wo3);
    one(w.w1, F, H, w.w13);
    one(w.w2, H, F, w.w23);
  }
  MQ_HIP(hipGetLastError());
  MQ_HIP(hipStreamSynchronize(nullptr));
  return MQ_OK;
}

// LayerNorm fold (MQ_ENC_OPT_LN_FOLD): Wg = gamma W for every layer's w1 (ln1) and, from layer
// 1 on, wqkv (the previous layer's ln2), with s[n] = sum_k Wg[n,k] and c[n] = b[n] + sum_k
// beta_k W[n,k] - as W3 images for K2p (x6_presplit; 287 MB for BERT-base beside the 510 MB
// of W3) or as fp32 for the re-split tiles (191 MB), whichever the current mode needs and
// does not have yet.  The unfolded weights stay: layer 0 and every shape outside the gate use
// them.  Synchronous; a no-op unless the option is on, the precision split-f32, H = 768.
int build_fold(mq_encoder* e) {
  const mq_bert_config& c = e->cfg;
  const int H = c.hidden, F = c.ffn;
  if (!e->ln_fold || e->precision != MQ_DTYPE_F32X6 || !e->loaded || e->layers.empty() ||
      H != kLnPartW * kLnMaxParts || F % 32 != 0)
    return MQ_OK;
  const bool img = e->x6_presplit;
  if (img ? e->layers[0].w1g3 != nullptr : e->layers[0].w1gf != nullptr) return MQ_OK;
  const size_t nl = e->layers.size();
  DeviceGuard dg(e->device);
  int rc = e->sfold.ensure(nl * 2 * ((size_t)F + 3 * H));
  if (rc) return rc;
  Buf tmp;  // one weight's fp32 Wg, the split's source
  if (img) {
    rc = e->wfold3.ensure((nl * w3_bytes(F, H) + (nl - 1) * w3_bytes(3 * H, H) + 3) / 4);
    if (!rc) rc = tmp.ensure((size_t)std::max(F, 3 * H) * H);
  } else {
    rc = e->wfoldf.ensure((nl * (size_t)F + (nl - 1) * (size_t)3 * H) * H);
  }
  if (rc) return rc;
  unsigned char* p3 = reinterpret_cast<unsigned char*>(e->wfold3.p);
  float* pf = e->wfoldf.p;
  float* ps = e->sfold.p;
  const LayerW* prev = nullptr;
  for (LayerW& w : e->layers) {
    auto one = [&](const float* W, const float* bias, const float* g, const float* b, int n, const unsigned char*& d3,
                   const float*& df, const float*& ds, const float*& dc) {
      float* wg = img ? tmp.p : pf;
      launch_ln_fold_weight(W, bias, g, b, n, H, wg, ps, ps + n, nullptr);
      ds = ps;
      dc = ps + n;
      ps += 2 * n;
      if (img) {
        launch_split_w3(wg, n, H, p3, nullptr);
        d3 = p3;
        p3 += w3_bytes(n, H);
      } else {
        df = pf;
        pf += (size_t)n * H;
      }
    };
    one(w.w1, w.b1, w.ln1g, w.ln1b, F, w.w1g3, w.w1gf, w.w1s, w.w1c);
    if (prev) one(w.wqkv, w.bqkv, prev->ln2g, prev->ln2b, 3 * H, w.wqkvg3, w.wqkvgf, w.wqkvs, w.wqkvc);
    prev = &w;
  }
  const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(nullptr);
  tmp.release();
  MQ_HIP(e1);
  MQ_HIP(e2);
  return MQ_OK;
}

// The frag16 images of every layer's four projection weights (the few-row kernels' layout,
// rows_gemm_kernel / attn_oproj_rows_kernel; 4 B per weight, 340 MB for BERT-base beside the
// row-major blob the batched GEMMs read).  Synchronous.
int build_frag16(mq_encoder* e) {
  const mq_bert_config& c = e->cfg;
  const int64_t H = c.hidden, F = c.ffn;
  const int64_t per = 3 * H * H + H * H + F * H + H * F;
  DeviceGuard dg(e->device);
  int rc = e->wfrag.ensure((size_t)(per * (int64_t)e->layers.size()));
  if (rc) return rc;
  float* p = e->wfrag.p;
  for (LayerW& w : e->layers) {
    auto one = [&](const float* W, int64_t r, int64_t k, const float*& dst) {
      const int64_t n4 = r * k / 4;
      hipLaunchKernelGGL(frag16_image_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, nullptr, W, (int)r,
                         (int)k, reinterpret_cast<floatx4*>(p));
      dst = p;
      p += r * k;
    };
    one(w.wqkv, 3 * H, H, w.wqkvf);
    one(w.wo, H, H, w.wof);
    one(w.w1, F, H, w.w1f);
    one(w.w2, H, F, w.w2f);
  }
  MQ_HIP(hipGetLastError());
  MQ_HIP(hipStreamSynchronize(nullptr));
  return MQ_OK;
}

// Wk^T of the last layer (MQ_ENC_OPT_CLS_KFREE: u = Wk_h^T q reads it K-contiguous), 4 H^2
// bytes, built with the other weight images at load when the pooling is CLS.  Synchronous.
int build_wkt(mq_encoder* e) {
  const int H = e->cfg.hidden;
  if (e->cfg.pooling != MQ_POOL_CLS || e->layers.empty()) return MQ_OK;
  DeviceGuard dg(e->device);
  int rc = e->wkt.ensure((size_t)H * H);
  if (rc) return rc;
  hipLaunchKernelGGL(transpose_kernel, dim3(H / 32, H / 32), dim3(256), 0, nullptr,
                     e->layers.back().wqkv + (int64_t)H * H, H, H, e->wkt.p);
  MQ_HIP(hipGetLastError());
  MQ_HIP(hipStreamSynchronize(nullptr));
  return MQ_OK;
}

template <int EPI>
void gemm(mq_encoder* e, const GemmArgs& g, int stage, hipStream_t s) {
  e->tl.mark(s, stage);
  GemmArgs a = g;
  if (!e->x6_presplit) a.W3 = nullptr;
  a.former_epi = !e->epi_split;
  launch_gemm<EPI>(a, e->num_cus, s, e->precision == MQ_DTYPE_F32X6, e->splitk_max, e->splitk_tiles);
}

// Residual projection + LayerNorm: x = LN(A W^T + b + resid), through y (g.out) on the
// tiled path; on the split-K (few-row) path the slab reduction, residual and LN run as
// one kernel writing x directly (bit-identical).  The fused form needs resid rows at
// stride H (a wave overwrites only the row it has read).
template <int VPL>
void gemm_resid_ln(mq_encoder* e, const GemmArgs& g, const float* lng, const float* lnb, float* x,
                   int stage, hipStream_t s) {
  const int H = VPL * 256;
  const int S = splitk_factor(g, e->num_cus, e->splitk_max, e->splitk_tiles);
  if (S && g.ldr == H && g.N == H) {
    e->tl.mark(s, stage);
    launch_splitk_gemm(g, S, s);
    e->tl.mark(s, ST_LN);
    hipLaunchKernelGGL((splitk_reduce_ln_kernel<VPL>), dim3((unsigned)g.M), dim3(256), 0, s, g.slab, S,
                       g.M, g.bias, g.resid, g.ldr, lng, lnb, e->cfg.ln_eps, x, 0);
    return;
  }
  gemm<EPI_RESID>(e, g, stage, s);
  e->tl.mark(s, ST_LN);
  constexpr int rows = 4 * kLnRowsPerWave;  // per 256-thread block
  hipLaunchKernelGGL((ln_kernel<VPL, kLnRowsPerWave>), dim3((unsigned)((g.M + rows - 1) / rows)), dim3(256), 0, s,
                     g.out, g.M, lng, lnb, e->cfg.ln_eps, x);
}

// The CLS_KFREE last layer's buffers inside mq_encoder::cls for B sequences.
struct ClsBufs {
  float *xc, *q, *u, *z, *part, *live;  // part: the ctx product's kClsCtxSplits planes [B][H]
  static size_t floats(int B, int H, int heads) {
    return (size_t)B * ((2 + kClsCtxSplits) * H + 2 * (size_t)heads * H + 1);
  }
  ClsBufs(float* p, int B, int H, int heads)
      : xc(p), q(xc + (size_t)B * H), u(q + (size_t)B * H), z(u + (size_t)B * heads * H),
        part(z + (size_t)B * heads * H), live(part + (size_t)kClsCtxSplits * B * H) {}
};

// u [B][heads][H] = Wk_h^T q for every head: 32 x 128 tiles, 64 deep.
void launch_cls_u(int B, int H, int heads, const float* q, const float* wkt, float* u, hipStream_t s) {
  using T = F32Tile<1, 4, 1, 1>;
  const int tiles = ((B + T::BM - 1) / T::BM) * ((H + T::BN - 1) / T::BN);
  hipLaunchKernelGGL((gemm_heads_kernel<T>), dim3(tiles * heads), dim3(256), 0, s, q, H, kDh, wkt, H, kDh, nullptr,
                     nullptr, B, H, kDh, u, heads * H, H, 1, (int64_t)0);
}

// z (the pass over the input rows: x normalised, or raw with stats / g / be) and ctx [B][H] =
// Wv_h z + live bv (64 x 64 tiles over H / kClsCtxSplits each into `part`, then the ordered
// sum).  H = 256 / 512 / 768.
void launch_cls_ctx(int B, int L, int H, int heads, float scale, const float* x, const float* stats,
                    const float* g, const float* be, float eps, const float* u, const int* mask, const float* wv,
                    const float* bv, float* z, float* part, float* live, float* ctx, hipStream_t s) {
  auto pass = [&](auto vpl) {
    constexpr int VPL = decltype(vpl)::value;
    if (stats)
      hipLaunchKernelGGL((cls_pass_kernel<VPL, true>), dim3(B), dim3(256 * VPL), 0, s, x, stats, g, be, eps, u, mask, L,
                         scale, z, live);
    else
      hipLaunchKernelGGL((cls_pass_kernel<VPL, false>), dim3(B), dim3(256 * VPL), 0, s, x, stats, g, be, eps, u, mask, L,
                         scale, z, live);
  };
  if (H == 256)
    pass(IC<1>{});
  else if (H == 512)
    pass(IC<2>{});
  else
    pass(IC<3>{});
  using T = F32Tile<2, 2, 1, 1>;
  const int tiles = (B + T::BM - 1) / T::BM;
  hipLaunchKernelGGL((gemm_heads_kernel<T>), dim3(tiles * heads * kClsCtxSplits), dim3(256), 0, s, z, heads * H, H, wv, H,
                     kDh * H, nullptr, nullptr, B, kDh, H, part, H, kDh, kClsCtxSplits, (int64_t)B * H);
  hipLaunchKernelGGL(cls_ctx_reduce_kernel, dim3((unsigned)(((int64_t)B * H / 4 + 255) / 256)), dim3(256), 0, s, part, B,
                     H, bv, live, ctx);
}

// The CLS-pooled last layer's FFN-down with the encoder's closing LayerNorm, pooling and L2
// normalisation (CLS_KFREE): out [M][H] = l2norm(LN(A W^T + b + resid)).  Split-K: the ordered
// slab reduction does all of it; else the GEMM through y (g.out) and ln_pool_kernel.
template <int VPL>
void gemm_resid_ln_pool(mq_encoder* e, const GemmArgs& g, const float* lng, const float* lnb, const int* mask,
                        float* out, int raw, int stage, hipStream_t s) {
  const int H = VPL * 256;
  const int S = splitk_factor(g, e->num_cus, e->splitk_max, e->splitk_tiles);
  if (S && g.ldr == H && g.N == H) {
    e->tl.mark(s, stage);
    launch_splitk_gemm(g, S, s);
    e->tl.mark(s, ST_POOL);
    hipLaunchKernelGGL((splitk_reduce_ln_kernel<VPL, true>), dim3((unsigned)g.M), dim3(256), 0, s, g.slab, S, g.M,
                       g.bias, g.resid, g.ldr, lng, lnb, e->cfg.ln_eps, out, raw);
    return;
  }
  gemm<EPI_RESID>(e, g, stage, s);
  e->tl.mark(s, ST_POOL);
  hipLaunchKernelGGL((ln_pool_kernel<VPL>), dim3((unsigned)((g.M + 3) / 4)), dim3(256), 0, s, g.out, 1, (int64_t)0, mask,
                     g.M, 1, 1, MQ_POOL_CLS, lng, lnb, e->cfg.ln_eps, out, raw);
}

// One forward.  With CLS pooling the last layer only needs the CLS rows after its
// attention: the output projection, LayerNorms and FFN run on the B CLS rows - identical CLS
// outputs, ~8% less work.  Its attention has one query per sequence, so (MQ_ENC_OPT_CLS_KFREE,
// the section above cls_pass_kernel) it projects neither K nor V: Q for the B CLS rows, u =
// Wk_h^T q, one pass over the layer's input rows, ctx = Wv_h z + bv, then the tail, whose
// FFN-down reduction also applies the closing LayerNorm, the pooling and the L2 norm.  With the
// option off: K and V for every token ([M, 2H]), attention on the first 32-query tile, the tail
// on strided views of the activations, and a pool launch.
// types: the tokens' segment ids (nullptr = all 0, the embedding forward); raw_cls: the tail
// writes the CLS rows' final LayerNorm output to `out` without the L2 normalisation (scoring).
template <int VPL>
int forward_vpl(mq_encoder* e, const int* ids, const int* types, const int* mask, int B, int L, float* out,
                int raw_cls, hipStream_t s) {
  const mq_bert_config& c = e->cfg;
  const int M = B * L, H = c.hidden, F = c.ffn;
  const unsigned row_blocks = (unsigned)((M + 3) / 4);
  const float scale = 1.0f / sqrtf((float)(H / c.heads));
  const int q_tiles = (L + 31) / 32;
  e->tl.mark(s, ST_EMBED);
  hipLaunchKernelGGL((embed_ln_kernel<VPL>), dim3(row_blocks), dim3(256), 0, s, ids, M, L,
                     c.vocab_size, e->word, e->pos, e->typ, types, c.type_vocab, e->eg, e->eb, c.ln_eps, e->x.p);
  const LayerW* prev = nullptr;
  // LayerNorm folded into the split-f32 GEMMs (LnFold) on the full-M layers: every one of
  // their GEMMs on the split-f32 tiles (launch_gemm's fill-the-chip test at the narrowest, N
  // = H), the folded weights built.  x and y are then the two raw-y buffers: out-proj writes
  // y (+ fst1), FFN-down x (+ fst2), each reading the other as its residual.
  const int nt = H / kLnPartW;  // partials per row
  const LayerW w0 = e->layers.empty() ? LayerW{} : e->layers[0];
  const bool fold = e->ln_fold && e->precision == MQ_DTYPE_F32X6 && M > 256 && H == kLnPartW * kLnMaxParts &&
                    F % 32 == 0 && (int64_t)((M + 127) / 128) * ((H + 191) / 192) >= e->num_cus &&
                    e->lnst.n >= (size_t)4 * M * nt && (e->x6_presplit ? w0.w1g3 != nullptr : w0.w1gf != nullptr);
  float* fst1 = e->lnst.p;
  float* fst2 = e->lnst.p + (size_t)2 * M * nt;
  bool raw = false;  // fold: x holds the previous layer's raw FFN-down sum (+ fst2), not LN2 of it
  bool pooled = false;  // CLS_KFREE: the last FFN-down's reduction has written the embeddings
  // MQ_ENC_OPT_QKV_ATTN: L = 32, 64-wide heads, whole 192-column tiles per head, and the QKV
  // GEMM one that launch_gemm runs on K2p's 128 x 192 tile (no split-K: M > 256; the split-f32
  // tiles fill the chip; x6p_pick_tile takes tile 0); the full-M QKV of every layer but a
  // CLS-only last one takes it, LN2 of the previous layer folded in or not as `fold` says.
  // On the re-split tiles (x6_presplit 0) the QKV GEMM runs as it did and the epilogue's
  // attention follows as a launch of its own (launch_attn32): x6_presplit 0 / 1 give the same bits.
  const bool attn_shape = e->qkv_attn && e->precision == MQ_DTYPE_F32X6 && L == 32 && H == 64 * c.heads &&
                          H % 192 == 0 && H % 32 == 0 && M > 256 &&
                          (int64_t)((M + 127) / 128) * ((3 * H + 191) / 192) >= e->num_cus &&
                          x6p_pick_tile(M, 3 * H, e->num_cus) == 0 && (int64_t)M * H < (1ll << 29);
  const bool qkv_attn = attn_shape && e->x6_presplit;
  auto fold_gemm = [&](auto epi, GemmArgs g, int stage) {
    e->tl.mark(s, stage);
    if (!e->x6_presplit) g.W3 = nullptr;
    g.former_epi = !e->epi_split;
    g.lf.eps = c.ln_eps;
    launch_gemm_fold<decltype(epi)::value>(g, e->num_cus, s);
  };
  for (size_t li = 0; li < e->layers.size(); ++li) {
    const LayerW& w = e->layers[li];
    const bool cls_only = c.pooling == MQ_POOL_CLS && li + 1 == e->layers.size();
    // rows this layer carries past attention: all M tokens, or the B CLS rows
    const int rows = cls_only ? B : M;
    int stride = cls_only ? L * H : H;  // row stride of the x / ctx views
    const float* resid = e->x.p;        // out-proj's residual rows (stride ldr)
    int ldr = stride;
    // the last layer without K / V (cls_pass_kernel holds hidden <= 768 in LDS)
    const bool kfree = cls_only && L > 1 && e->cls_kfree && VPL <= 3 && e->wkt.p != nullptr &&
                       e->cls.n >= ClsBufs::floats(B, H, c.heads);
    // few rows (single queries past the few-row limit): the layers past resident_layers
    // stream their weights non-temporally in the split-K GEMMs (as forward_rows does)
    const int lnt = M <= 256 && (int)li >= e->resident_layers ? 1 : 0;
    // the CLS-only tail (the B CLS rows past attention) runs unfolded
    const bool fold_layer = fold && !(cls_only && L > 1);
    bool attn_done = false;   // qkv_attn: this layer's QKV launch has written ctx
    bool attn_after = false;  // ... or the same attention follows the plain QKV launch
    // the folded QKV weights' rows [row0, ..): LN2 of the previous layer applied in the epilogue
    auto qkv_fold = [&](GemmArgs g, int row0) {
      g.W = w.wqkvgf ? w.wqkvgf + (int64_t)row0 * H : nullptr;
      g.W3 = w.wqkvg3 ? w.wqkvg3 + w3_row_offset(row0, H) : nullptr;
      g.bias = w.wqkvc + row0;
      g.lf.s = w.wqkvs + row0;
      g.lf.stats_in = fst2;
      fold_gemm(IC<EPI_BIAS_LNFOLD>{}, g, ST_QKV);
    };
    auto qkv_gemm = [&](GemmArgs g) {
      g.nt = lnt;
      if (raw)
        qkv_fold(g, (int)(g.W - w.wqkv) / H);
      else
        gemm<EPI_BIAS>(e, g, ST_QKV, s);
    };
    if (kfree) {
      const ClsBufs cb(e->cls.p, B, H, c.heads);
      // the layer's input as the pass reads it: normalised rows in x, or raw rows with their
      // partials and the previous layer's LN2 (the fold's x + fst2)
      const float* xin = e->x.p;
      const float* xst = raw ? fst2 : nullptr;
      if (xst) {
        // The normalised CLS rows go to a SEPARATE [B, H] buffer (the Q GEMM and the tail's
        // residual read that): row b L of the raw buffer stays raw for the pass below.
        e->tl.mark(s, ST_LN);
        hipLaunchKernelGGL((ln_rows_kernel<VPL>), dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, xin, B, (int64_t)L * H,
                           prev->ln2g, prev->ln2b, c.ln_eps, cb.xc);
        resid = cb.xc;
        ldr = H;
      }
      GemmArgs q{e->slab.p, e->slab.n, resid, ldr, w.wqkv, w.bqkv, nullptr, 0, cb.q, H, B, H, H, lnt};
      q.W3 = w.wqkv3;
      gemm<EPI_BIAS>(e, q, ST_QKV, s);
      launch_cls_u(B, H, c.heads, cb.q, e->wkt.p, cb.u, s);
      e->tl.mark(s, ST_ATTN);
      launch_cls_ctx(B, L, H, c.heads, scale, xin, xst, xst ? prev->ln2g : nullptr, xst ? prev->ln2b : nullptr,
                     c.ln_eps, cb.u, mask, w.wqkv + (int64_t)2 * H * H, w.bqkv + 2 * H, cb.z, cb.part, cb.live, e->ctx.p, s);
      stride = H;  // ctx is compact
    } else if (cls_only && L > 1) {
      // only the CLS rows need queries: K and V for every token ([M, 2H] into qkv columns
      // H..3H), Q for the B CLS rows (every L-th row of x into row b*L of qkv)
      GemmArgs kv{e->slab.p, e->slab.n, e->x.p, H, w.wqkv + (int64_t)H * H, w.bqkv + H, nullptr, 0, e->qkv.p + H,
                  3 * H, M, 2 * H, H};
      if (w.wqkv3) kv.W3 = w.wqkv3 + w3_row_offset(H, H);
      qkv_gemm(kv);
      if (raw) {  // the CLS rows of the raw y, normalised in place for the Q GEMM and the tail
        e->tl.mark(s, ST_LN);
        hipLaunchKernelGGL((ln_rows_inplace_kernel<VPL>), dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, e->x.p, B,
                           (int64_t)L * H, prev->ln2g, prev->ln2b, c.ln_eps);
      }
      GemmArgs q{e->slab.p, e->slab.n, e->x.p, L * H, w.wqkv, w.bqkv, nullptr, 0, e->qkv.p, L * 3 * H, B, H, H, lnt};
      q.W3 = w.wqkv3;
      gemm<EPI_BIAS>(e, q, ST_QKV, s);
    } else if (qkv_attn && (raw ? w.wqkvg3 != nullptr : w.wqkv3 != nullptr)) {
      // L = 32 attention in the QKV GEMM's epilogue (EPI_ATTN_*): ctx straight from the
      // accumulators, no qkv written and no attention launch; folded or not as the plain QKV is
      X6pArgs a{e->x.p, H, raw ? w.wqkvg3 : w.wqkv3, raw ? w.wqkvc : w.bqkv, nullptr, 0, e->ctx.p, H, M, 3 * H, H};
      if (raw) {
        a.lf.s = w.wqkvs;
        a.lf.stats_in = fst2;
        a.lf.eps = c.ln_eps;
      }
      a.at.mask = mask;
      a.at.scale = scale;
      e->tl.mark(s, ST_QKV);
      launch_gemm_x6p(a, raw ? EPI_ATTN_LNFOLD : EPI_ATTN_BIAS, 0, e->num_cus, s);
      attn_done = true;
    } else {
      GemmArgs qkv{e->slab.p, e->slab.n, e->x.p, H, w.wqkv, w.bqkv, nullptr, 0, e->qkv.p, 3 * H, M, 3 * H, H};
      qkv.W3 = w.wqkv3;
      qkv_gemm(qkv);
      attn_after = attn_shape;
    }
    const bool resid_raw = raw && fold_layer;  // (the tail's residual rows were normalised above)
    raw = false;
    if (!kfree && !attn_done) {
      e->tl.mark(s, ST_ATTN);
      const int qt = cls_only ? 1 : q_tiles;
      if (attn_after)
        launch_attn32(e->qkv.p, mask, e->ctx.p, M, H, scale, s);
      else
        launch_attention(B, L, c.heads, qt, H, scale, e->qkv.p, mask, e->ctx.p, s);
    }
    // x = LN1(x + ctx Wo^T + bo)  (compact [rows, H], through y)
    GemmArgs oproj{e->slab.p, e->slab.n, e->ctx.p, stride, w.wo, w.bo, resid, ldr, e->y.p, H, rows, H, H, lnt};
    oproj.W3 = w.wo3;
    if (fold_layer) {  // y = ctx Wo^T + bo + (LN2_prev(x) or x), raw, + its partials
      oproj.lf.stats_out = fst1;
      if (resid_raw) {
        oproj.lf.stats_in = fst2;
        oproj.lf.g = prev->ln2g;
        oproj.lf.b = prev->ln2b;
      }
      fold_gemm(IC<EPI_RESID_LN_STATS>{}, oproj, ST_OPROJ);
    } else {
      gemm_resid_ln<VPL>(e, oproj, w.ln1g, w.ln1b, e->x.p, ST_OPROJ, s);
    }
    GemmArgs up{e->slab.p, e->slab.n, e->x.p, H, w.w1, w.b1, nullptr, 0, e->ffn.p, F, rows, F, H, lnt};
    up.W3 = w.w13;
    if (fold_layer) {  // FFN-up on the raw y with LN1 folded in
      up.A = e->y.p;
      up.W = w.w1gf;
      up.W3 = w.w1g3;
      up.bias = w.w1c;
      up.lf.s = w.w1s;
      up.lf.stats_in = fst1;
      if (c.gelu == MQ_GELU_TANH)
        fold_gemm(IC<EPI_GELU_TANH_LNFOLD>{}, up, ST_FFN_UP);
      else
        fold_gemm(IC<EPI_GELU_ERF_LNFOLD>{}, up, ST_FFN_UP);
    } else if (c.gelu == MQ_GELU_TANH) {
      gemm<EPI_GELU_TANH>(e, up, ST_FFN_UP, s);
    } else {
      gemm<EPI_GELU_ERF>(e, up, ST_FFN_UP, s);
    }
    GemmArgs down{e->slab.p, e->slab.n, e->ffn.p, F, w.w2, w.b2, e->x.p, H, e->y.p, H, rows, H, F, lnt};
    down.W3 = w.w23;
    if (fold_layer) {  // x = ffn W2^T + b2 + LN1(y), raw, + its partials: LN2 is the next QKV's
      const bool last = li + 1 == e->layers.size();
      down.resid = e->y.p;
      down.lf.stats_in = fst1;
      down.lf.g = w.ln1g;
      down.lf.b = w.ln1b;
      down.lf.stats_out = fst2;
      down.out = last ? e->ctx.p : e->x.p;  // (last: the final LayerNorm stays a launch, ctx -> x)
      fold_gemm(IC<EPI_RESID_LN_STATS>{}, down, ST_FFN_DOWN);
      if (last) {
        e->tl.mark(s, ST_LN);
        constexpr int wg_rows = 4 * kLnRowsPerWave;
        hipLaunchKernelGGL((ln_kernel<VPL, kLnRowsPerWave>), dim3((unsigned)((M + wg_rows - 1) / wg_rows)), dim3(256),
                           0, s, e->ctx.p, M, w.ln2g, w.ln2b, c.ln_eps, e->x.p);
      } else {
        raw = true;
      }
    } else if (kfree) {  // the encoder's end: LN2, CLS pooling and the L2 norm with the reduction
      gemm_resid_ln_pool<VPL>(e, down, w.ln2g, w.ln2b, mask, out, raw_cls, ST_FFN_DOWN, s);
      pooled = true;
    } else {
      gemm_resid_ln<VPL>(e, down, w.ln2g, w.ln2b, e->x.p, ST_FFN_DOWN, s);
    }
    prev = &w;
  }
  if (!pooled) {
    e->tl.mark(s, ST_POOL);
    const bool pruned = c.pooling == MQ_POOL_CLS;  // x holds [B, H] CLS rows
    hipLaunchKernelGGL((pool_kernel<VPL>), dim3((B + 3) / 4), dim3(256), 0, s, e->x.p, mask, B,
                       pruned ? 1 : L, c.pooling, out, raw_cls);
  }
  e->tl.close(s);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

// ------------------------------------------------------- few-row forward ------
struct RowsArgs {
  const float* A;
  int lda;
  int64_t a_plane;  // LN_IN: floats between the summed input planes
  const float* W;
  int ldw;
  const float* bias;
  const float* resid;
  int ldr;
  float* out;
  int ldo;
  int64_t o_plane;  // floats between the output planes of a K split
  int M, N, K;      // K: full depth (ldw >= K)
  int splits;       // K splits (grid.z), each writing one output plane
  // LN_IN with s_in = 0: A is the word-embedding table, rows gathered by token id
  const int* ids = nullptr;
  int L = 1, vocab = 0;
  const float* pos = nullptr;
  const float* typ = nullptr;
  const int* types = nullptr;  // segment ids (nullptr = type row 0)
  int type_vocab = 1;
  int nt_w = 0;  // weights loaded non-temporally (layers past resident_layers)
  float* zbuf = nullptr;  // zn floats this launch zeroes for a later launch's FL_ACC adds
  int64_t zn = 0;
};

// Row tiles per workgroup: two for the LayerNorm-input GEMMs when M > 16 (the launch then
// streams each weight panel once instead of once per 16-row tile: QKV 10.5 -> 9.0 us,
// FFN-up 10.1 -> 8.6 us at M = 32), unless the normalised rows would not fit LDS (hidden
// 1024).  The plain GEMMs keep one: with half the workgroups their per-CU bytes, not the
// chip's, bound them (FFN-down 7.8 -> 10.9 us with two).
template <int EPI, bool LN_IN, int VPL, int NB, int S_IN, int RT, int FL>
void launch_rows_rt(const RowsArgs& g, const float* lng, const float* lnb, float eps, float* ln_out,
                    hipStream_t s) {
  hipLaunchKernelGGL((rows_gemm_kernel<EPI, LN_IN, VPL, NB, S_IN, RT, FL>),
                     dim3(g.N / kRT, (g.M + kRT * RT - 1) / (kRT * RT), g.splits), dim3(64 * kRWaves), 0, s,
                     g.A, g.lda, g.a_plane, g.M, lng, lnb, eps, ln_out, g.W, g.ldw, g.bias, g.resid, g.ldr,
                     g.out, g.ldo, g.o_plane, g.ids, g.L, g.vocab, g.pos, g.typ, g.types, g.type_vocab, g.nt_w, g.zbuf,
                     g.zn);
}

template <int EPI, bool LN_IN, int VPL, int NB, int S_IN, int FL = 0>
void launch_rows_nb(const RowsArgs& g, const float* lng, const float* lnb, float eps, float* ln_out,
                    hipStream_t s) {
  constexpr bool two_fit = LN_IN && (size_t)(2 * kRT * (NB * 256 + 4) + kRWaves * 2 * kRT * kRT) * 4 <= 160 * 1024;
  if constexpr (two_fit) {
    if (g.M > kRT) {
      launch_rows_rt<EPI, LN_IN, VPL, NB, S_IN, 2, FL>(g, lng, lnb, eps, ln_out, s);
      return;
    }
  }
  launch_rows_rt<EPI, LN_IN, VPL, NB, S_IN, 1, FL>(g, lng, lnb, eps, ln_out, s);
}

// Per-split depths the few-row kernel is instantiated for (K / 256 blocks per wave).
bool rows_nb_ok(int nb) { return nb >= 1 && (nb <= 4 || nb == 6 || nb == 8 || nb == 12 || nb == 16); }

// K splits for a depth-K projection: the fewest with per-split depth <= 1536, at most 4.
// More splits put more workgroups on the weights but add planes the consumer sums (at
// K = 3072, encoder p50: one split 13.9 us per FFN-down launch; two 0.474 ms, three 0.495,
// four 0.493 - FFN-down 8.9 / 9.2 / 7.1 us, the next QKV 9.2 / 10.0 / 11.0 us).
int rows_splits(int K, int forced = 0) {  // forced: MQ_ENC_OPT_ROWS_SPLITS, used when it divides K / 256
  const int nb = K / 256;
  if (forced >= 1 && forced <= 4 && nb % forced == 0 && rows_nb_ok(nb / forced)) return forced;
  for (int sp = 1; sp <= 4; ++sp)
    if (nb % sp == 0 && nb / sp <= 6 && rows_nb_ok(nb / sp)) return sp;
  return 1;
}

template <int EPI, int NB, int FL>
void launch_rows_plain(const RowsArgs& g, hipStream_t s) {
  launch_rows_nb<EPI, false, 1, NB, 1, FL>(g, nullptr, nullptr, 0.f, nullptr, s);
}

// No LayerNorm on A: any instantiated per-split depth; FL_A: A in frag16 (FFN-up's output).
template <int EPI, int FL = 0>
void launch_rows(const RowsArgs& g, hipStream_t s) {
  switch (g.K / g.splits / 256) {
    case 1: launch_rows_plain<EPI, 1, FL>(g, s); return;
    case 2: launch_rows_plain<EPI, 2, FL>(g, s); return;
    case 3: launch_rows_plain<EPI, 3, FL>(g, s); return;
    case 4: launch_rows_plain<EPI, 4, FL>(g, s); return;
    case 6: launch_rows_plain<EPI, 6, FL>(g, s); return;
    case 8: launch_rows_plain<EPI, 8, FL>(g, s); return;
    case 12: launch_rows_plain<EPI, 12, FL>(g, s); return;
    default: launch_rows_plain<EPI, 16, FL>(g, s); return;
  }
}

// A = LN(sum of s_in planes) with K == H, the normalised rows also to ln_out (may be null);
// s_in = 0: A = LN(embedding sum) gathered by token id (g.ids, g.pos, g.typ).
template <int EPI, int VPL, int FL = 0>
void launch_rows_ln(const RowsArgs& g, int s_in, const float* lng, const float* lnb, float eps,
                    float* ln_out, hipStream_t s) {
  switch (s_in) {
    case 0: launch_rows_nb<EPI, true, VPL, VPL, 0, FL>(g, lng, lnb, eps, ln_out, s); return;
    case 1: launch_rows_nb<EPI, true, VPL, VPL, 1, FL>(g, lng, lnb, eps, ln_out, s); return;
    case 2: launch_rows_nb<EPI, true, VPL, VPL, 2, FL>(g, lng, lnb, eps, ln_out, s); return;
    case 3: launch_rows_nb<EPI, true, VPL, VPL, 3, FL>(g, lng, lnb, eps, ln_out, s); return;
    default: launch_rows_nb<EPI, true, VPL, VPL, 4, FL>(g, lng, lnb, eps, ln_out, s); return;
  }
}

template <int HG, bool QF, bool ACC>
void launch_attn_oproj_hg(int nkb, dim3 grid, hipStream_t s, const float* qkv, const int* mask, int L, int H,
                          int rps, int qtiles, float scale, const float* wo, const float* bo, const float* resid,
                          int ldr, float* out, int64_t o_plane, int nt_w) {
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(512), 0, s, qkv, mask, L, H, rps, qtiles, scale, wo, bo, resid, ldr, out,
                       o_plane, nt_w);
  };
  switch (nkb) {
    case 1: go(attn_oproj_rows_kernel<HG, 1, QF, ACC>); break;
    case 2: go(attn_oproj_rows_kernel<HG, 2, QF, ACC>); break;
    case 3: go(attn_oproj_rows_kernel<HG, 3, QF, ACC>); break;
    default: go(attn_oproj_rows_kernel<HG, 4, QF, ACC>); break;
  }
}

// acc: the two head-group planes added into one zeroed plane (hg = heads / 2 only)
void launch_attn_oproj(int hg, bool qf, bool acc, int nkb, dim3 grid, hipStream_t s, const float* qkv,
                       const int* mask, int L, int H, int rps, int qtiles, float scale, const float* wo,
                       const float* bo, const float* resid, int ldr, float* out, int64_t o_plane, int nt_w) {
  auto go = [&](auto hgc, auto qfc, auto accc) {
    launch_attn_oproj_hg<decltype(hgc)::value, decltype(qfc)::value, decltype(accc)::value>(
        nkb, grid, s, qkv, mask, L, H, rps, qtiles, scale, wo, bo, resid, ldr, out, o_plane, nt_w);
  };
  if (hg == 6) {
    if (qf && acc) go(IC<6>{}, std::true_type{}, std::true_type{});
    else if (qf) go(IC<6>{}, std::true_type{}, std::false_type{});
    else if (acc) go(IC<6>{}, std::false_type{}, std::true_type{});
    else go(IC<6>{}, std::false_type{}, std::false_type{});
  } else {
    if (qf && acc) go(IC<4>{}, std::true_type{}, std::true_type{});
    else if (qf) go(IC<4>{}, std::true_type{}, std::false_type{});
    else if (acc) go(IC<4>{}, std::false_type{}, std::true_type{});
    else go(IC<4>{}, std::false_type{}, std::false_type{});
  }
}

// Heads per output plane of the fused attention + output projection (K3o), 0 = run
// attention and the projection as two launches (keys past 64, or a head count neither
// 6 nor 4 divides).  6 at BERT-base (12 heads: two planes).
int oproj_heads_per_plane(const mq_encoder* e, int L) {
  const mq_bert_config& c = e->cfg;
  if (!e->fuse_attn_oproj || L > 64 || c.hidden != c.heads * kDh || c.hidden % kOpCols) return 0;
  return c.heads % 6 == 0 ? 6 : c.heads % 4 == 0 ? 4 : 0;
}

// Few-row forward (B * L <= kRowsMax): 5 launches per layer instead of 9, 5 L + 1 in all.  Between
// layers the activations stay pre-LayerNorm, as the FFN-down's split-K planes in `slab`;
// the next GEMM sums and normalises them on load (K2r LN_IN) and materialises the
// normalised rows in x for the residual:
//   QKV   qkv = LN2'(sum slab) Wqkv^T + b  (x = LN2'(...); layer 0: LN of the gathered
//         embedding sum, so the forward has no separate embedding launch)
//   attn  ctx
//   oproj y = ctx Wo^T + bo + x
//   up    ffn = GELU(LN1(y) W1^T + b1)     (x = LN1(y))
//   down  slab[z] = ffn[:, Kz] W2[:, Kz]^T (+ b2 + x for z = 0)
// and ln_pool applies the last LN2 to the pooled rows.  The CLS-only last layer carries
// the B CLS rows past attention as forward_vpl does.
template <int VPL>
int forward_rows(mq_encoder* e, const int* ids, const int* types, const int* mask, int B, int L, float* out,
                 int raw, hipStream_t s) {
  const mq_bert_config& c = e->cfg;
  const int M = B * L, H = c.hidden, F = c.ffn;
  const float eps = c.ln_eps;
  const float scale = 1.0f / sqrtf((float)(H / c.heads));
  const int q_tiles = (L + 31) / 32;
  const int dsplit = rows_splits(F, e->rows_splits);
  const int hg = oproj_heads_per_plane(e, L);
  // QKV -> K3o through frag16 (Q, K, V^T blocks) when every sequence starts a 16-row block
  const bool qf = hg != 0 && L % 16 == 0 && (3 * H) % 48 == 0;
  // two-addend plane merges (FL_ACC): FFN-down's two K splits and K3o's two head groups add
  // into one zeroed plane, so QKV and FFN-up read one plane of rows instead of two (the
  // buffer each zeroes: the slab by FFN-up, y by QKV, a launch ahead of the adds)
  const bool dacc = dsplit == 2 && !e->rows_planes;
  const bool yacc = hg != 0 && c.heads / hg == 2 && !e->rows_planes;
  int prev_rows = M;
  for (size_t li = 0; li < e->layers.size(); ++li) {
    const LayerW& w = e->layers[li];
    const bool cls_only = c.pooling == MQ_POOL_CLS && li + 1 == e->layers.size();
    const int rows = cls_only ? B : M;
    const int stride = cls_only ? L * H : H;
    const int nt = (int)li >= e->resident_layers ? 1 : 0;  // this layer's weights bypass MALL
    e->tl.mark(s, ST_QKV);
    RowsArgs qkv{e->slab.p, H, (int64_t)prev_rows * H, w.wqkvf, H, w.bqkv, nullptr, 0, e->qkv.p, 3 * H, 0, M, 3 * H, H, 1};
    qkv.nt_w = nt;
    if (li == 0) {  // the embedding gather + LayerNorm run inside the first QKV launch
      qkv.A = e->word;
      qkv.a_plane = 0;
      qkv.ids = ids;
      qkv.L = L;
      qkv.vocab = c.vocab_size;
      qkv.pos = e->pos;
      qkv.typ = e->typ;
      qkv.types = types;
      qkv.type_vocab = c.type_vocab;
    }
    const LayerW* pl = li ? &e->layers[li - 1] : nullptr;
    const float* lg = pl ? pl->ln2g : e->eg;
    const float* lb = pl ? pl->ln2b : e->eb;
    const int s_in = pl ? (dacc ? 1 : dsplit) : 0;
    if (yacc) {  // K3o of this layer adds into y
      qkv.zbuf = e->y.p;
      qkv.zn = (int64_t)rows * H;
    }
    if (qf)  // K3o reads Q, K, V^T as whole frag16 blocks
      ROWS_REP launch_rows_ln<EPI_BIAS, VPL, FL_O | FL_OT>(qkv, s_in, lg, lb, eps, e->x.p, s);
    else
      ROWS_REP launch_rows_ln<EPI_BIAS, VPL>(qkv, s_in, lg, lb, eps, e->x.p, s);
    const int qt = cls_only ? 1 : q_tiles;
    int y_planes = 1;
    if (hg) {  // attention + output projection in one launch (K3o), hg heads per plane
      e->tl.mark(s, ST_OPROJ);
      const int rps = cls_only ? 1 : L, qtiles = (rps + 15) / 16;
      y_planes = c.heads / hg;
      const dim3 grid(H / kOpCols, B * qtiles, y_planes);
      if (yacc) y_planes = 1;
      ROWS_REP launch_attn_oproj(hg, qf, yacc, (L + 15) / 16, grid, s, e->qkv.p, mask, L, H, rps, qtiles, scale, w.wof, w.bo, e->x.p,
                                 stride, e->y.p, (int64_t)rows * H, nt);
    } else {
      e->tl.mark(s, ST_ATTN);
      if (L <= 64)
        hipLaunchKernelGGL(attention_rows_kernel, dim3(B * c.heads * qt), dim3(512), 0, s, e->qkv.p, mask, L,
                           H, c.heads, qt, scale, e->ctx.p);
      else
        launch_attention(B, L, c.heads, qt, H, scale, e->qkv.p, mask, e->ctx.p, s);
      e->tl.mark(s, ST_OPROJ);
      RowsArgs oproj{e->ctx.p, stride, 0, w.wof, H, w.bo, e->x.p, stride, e->y.p, H, 0, rows, H, H, 1};
      oproj.nt_w = nt;
      launch_rows<EPI_RESID>(oproj, s);
    }
    e->tl.mark(s, ST_FFN_UP);
    // FFN-up writes the GELU rows in frag16 for FFN-down's A operand
    RowsArgs up{e->y.p, H, (int64_t)rows * H, w.w1f, H, w.b1, nullptr, 0, e->ffn.p, F, 0, rows, F, H, 1};
    up.nt_w = nt;
    if (dacc) {  // FFN-down of this layer adds into the slab
      up.zbuf = e->slab.p;
      up.zn = (int64_t)rows * H;
    }
    if (c.gelu == MQ_GELU_TANH)
      ROWS_REP launch_rows_ln<EPI_GELU_TANH, VPL, FL_O>(up, y_planes, w.ln1g, w.ln1b, eps, e->x.p, s);
    else
      ROWS_REP launch_rows_ln<EPI_GELU_ERF, VPL, FL_O>(up, y_planes, w.ln1g, w.ln1b, eps, e->x.p, s);
    e->tl.mark(s, ST_FFN_DOWN);
    RowsArgs down{e->ffn.p, F, 0, w.w2f, F, w.b2, e->x.p, H, e->slab.p, H, (int64_t)rows * H, rows, H, F, dsplit};
    down.nt_w = nt;
    if (dacc)
      ROWS_REP launch_rows<EPI_RESID, FL_A | FL_ACC>(down, s);
    else
      ROWS_REP launch_rows<EPI_RESID, FL_A>(down, s);
    prev_rows = rows;
  }
  e->tl.mark(s, ST_POOL);
  const LayerW& last = e->layers.back();
  const int pool_rows = c.pooling == MQ_POOL_CLS ? 1 : L;  // slab holds [B, H] CLS rows or [M, H]
  hipLaunchKernelGGL((ln_pool_kernel<VPL>), dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, e->slab.p, dacc ? 1 : dsplit,
                     (int64_t)prev_rows * H, mask, B, L, pool_rows, c.pooling, last.ln2g, last.ln2b, eps, out, raw);
  e->tl.close(s);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

// The few-row forward serves B * L <= rows_max token rows (MQ_ENC_OPT_ROWS_MAX, default
// 64: a single query up to 64 tokens; 0 turns it off).
bool use_rows_path(const mq_encoder* e, int B, int L) {
  const mq_bert_config& c = e->cfg;
  const int sp = rows_splits(c.ffn, e->rows_splits);
  // slab holds the FFN-down planes: splits x rows x H floats
  return (int64_t)B * L <= e->rows_max && !e->layers.empty() && c.ffn % 256 == 0 &&
         rows_nb_ok(c.ffn / 256 / sp) && (size_t)sp * B * L * c.hidden <= e->slab.n &&
         e->layers[0].wqkvf != nullptr;  // (the frag16 weight images)
}

}  // namespace

namespace {

// The one forward of both entry points: mq_encoder_embed passes types = nullptr, raw = 0;
// mq_encoder_score the segment ids and raw = 1 (out = the handle's [B][H] CLS-state buffer).
int forward(mq_encoder* e, const int* ids, const int* types, const int* mask, int B, int L, float* out,
            int raw, hipStream_t s) {
  const bool rows = use_rows_path(e, B, L);
  auto go = [&](auto vpl) {
    constexpr int VPL = decltype(vpl)::value;
    return rows ? forward_rows<VPL>(e, ids, types, mask, B, L, out, raw, s)
                : forward_vpl<VPL>(e, ids, types, mask, B, L, out, raw, s);
  };
  switch (e->cfg.hidden) {
    case 256: return go(IC<1>{});
    case 512: return go(IC<2>{});
    case 768: return go(IC<3>{});
    default: return go(IC<4>{});
  }
}

constexpr size_t kMaxGraphs = 6;

// Replay the forward io_ids/io_mask -> io_out for (B, L) as one hipGraph launch on s,
// capturing it first if no cached graph matches the shape, precision and buffers.
int launch_graph(mq_encoder* e, int B, int L, hipStream_t s) {
  const std::vector<const void*> bufs = {e->weights.p, e->x.p,   e->y.p,      e->qkv.p,
                                         e->ctx.p,     e->ffn.p, e->slab.p,   e->io_out.p,
                                         e->io_ids,    e->io_mask,  e->w3.p,   e->wfrag.p,
                                         e->wkt.p,     e->cls.p};
  mq_encoder::Graph* hit = nullptr;
  for (auto& g : e->graphs)
    if (g.B == B && g.L == L && g.precision == e->precision && g.bufs == bufs) hit = &g;
  if (!hit) {
    if (!e->cap_stream) MQ_HIP(hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking));
    // drop graphs that reference freed buffers, then the least recently used
    for (size_t i = 0; i < e->graphs.size();) {
      if (e->graphs[i].bufs != bufs) {
        (void)hipGraphExecDestroy(e->graphs[i].exec);
        e->graphs.erase(e->graphs.begin() + i);
      } else {
        ++i;
      }
    }
    if (e->graphs.size() >= kMaxGraphs) {
      auto lru = std::min_element(e->graphs.begin(), e->graphs.end(),
                                  [](const auto& a, const auto& b) { return a.last_use < b.last_use; });
      (void)hipGraphExecDestroy(lru->exec);
      e->graphs.erase(lru);
    }
    hipGraph_t graph = nullptr;
    MQ_HIP(hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeThreadLocal));
    const int rc = forward(e, e->io_ids, nullptr, e->io_mask, B, L, e->io_out.p, 0, e->cap_stream);
    const hipError_t end = hipStreamEndCapture(e->cap_stream, &graph);
    if (rc) {
      if (graph) (void)hipGraphDestroy(graph);
      return rc;
    }
    if (end != hipSuccess) MQ_FAIL(MQ_EHIP, "graph capture failed: %s", hipGetErrorString(end));
    mq_encoder::Graph g;
    g.B = B;
    g.L = L;
    g.precision = e->precision;
    g.bufs = bufs;
    const hipError_t inst = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (inst != hipSuccess) MQ_FAIL(MQ_EHIP, "graph instantiate failed: %s", hipGetErrorString(inst));
    e->graphs.push_back(g);
    hit = &e->graphs.back();
  }
  hit->last_use = ++e->graph_clock;
  MQ_HIP(hipGraphLaunch(hit->exec, s));
  return MQ_OK;
}

// mq_debug_attn_oproj's QF operand: the image of a row-major qkv [rows][3H] that the QKV
// launch writes with FL_O | FL_OT - frag16, the V blocks (columns from 2H) transposed
// within their 16 x 16 block.  One element per thread.
__global__ __launch_bounds__(256) void frag16_qkv_image_kernel(const float* __restrict__ qkv, int rows, int H,
                                                               float* __restrict__ img) {
  const int ld = 3 * H;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)rows * ld) return;
  const int64_t row = idx / ld;
  const int col = (int)(idx - row * ld);
  const bool vt = col >= 2 * H;
  const int64_t irow = vt ? ((row & ~(int64_t)15) | (col & 15)) : row;
  const int icol = vt ? ((col & ~15) | (int)(row & 15)) : col;
  img[frag16_offset(irow, icol, ld)] = qkv[idx];
}

// mq_debug_rows_gemm's LayerNorm-input kinds: the launches of forward_rows, by hidden size
// (kind 0 QKV: variant 1 = frag16 output with V^T blocks; kind 1 FFN-up: variant 1 = tanh GELU)
template <int VPL>
void debug_rows_ln(int kind, int variant, const RowsArgs& g, int s_in, const float* lg, const float* lb, float eps,
                   float* ln_out, hipStream_t s) {
  if (kind == 0) {
    if (variant)
      launch_rows_ln<EPI_BIAS, VPL, FL_O | FL_OT>(g, s_in, lg, lb, eps, ln_out, s);
    else
      launch_rows_ln<EPI_BIAS, VPL>(g, s_in, lg, lb, eps, ln_out, s);
  } else if (variant) {
    launch_rows_ln<EPI_GELU_TANH, VPL, FL_O>(g, s_in, lg, lb, eps, ln_out, s);
  } else {
    launch_rows_ln<EPI_GELU_ERF, VPL, FL_O>(g, s_in, lg, lb, eps, ln_out, s);
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int64_t mq_encoder_weight_count(const mq_bert_config* cfg) {
  if (!cfg) return -1;
  return weight_count(*cfg);
}

int mq_encoder_create(int device, const mq_bert_config* cfg, mq_encoder** out) {
  clear_error();
  MQ_CHECK_ARG(out && cfg, "NULL argument");
  *out = nullptr;
  const mq_bert_config& c = *cfg;
  MQ_CHECK_ARG(c.hidden == 256 || c.hidden == 512 || c.hidden == 768 || c.hidden == 1024,
               "hidden must be 256/512/768/1024 (got %d)", c.hidden);
  MQ_CHECK_ARG(c.heads > 0 && c.hidden / c.heads == kDh && c.hidden % c.heads == 0,
               "head dim must be %d (hidden %d, heads %d)", kDh, c.hidden, c.heads);
  MQ_CHECK_ARG(c.ffn > 0 && c.ffn % kBK == 0, "ffn must be a positive multiple of %d", kBK);
  MQ_CHECK_ARG(c.layers >= 1 && c.vocab_size > 0 && c.max_positions > 0 && c.type_vocab > 0,
               "bad config");
  MQ_CHECK_ARG(c.gelu == MQ_GELU_ERF || c.gelu == MQ_GELU_TANH, "bad gelu variant");
  MQ_CHECK_ARG(c.pooling == MQ_POOL_CLS || c.pooling == MQ_POOL_MEAN, "bad pooling");
  DeviceGuard dg(device);
  if (!dg.ok) MQ_FAIL(MQ_EHIP, "hipSetDevice(%d) failed", device);
  auto e = std::make_unique<mq_encoder>();
  e->device = device;
  e->cfg = c;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
      cus > 0)
    e->num_cus = cus;
  *out = e.release();
  return MQ_OK;
}

int mq_encoder_destroy(mq_encoder* e) {
  clear_error();
  if (!e) return MQ_OK;
  {
    DeviceGuard dg(e->device);
    for (Buf* b : {&e->weights, &e->x, &e->y, &e->qkv, &e->ctx, &e->ffn, &e->io_out, &e->slab, &e->w3, &e->wfrag,
                   &e->lnst, &e->wkt, &e->cls, &e->head, &e->cls_state})
      b->release();
    if (e->io_types) (void)hipFree(e->io_types);
    if (e->io_ids) (void)hipFree(e->io_ids);
    if (e->io_mask) (void)hipFree(e->io_mask);
    e->pin.release();
    for (auto& g : e->graphs) (void)hipGraphExecDestroy(g.exec);
    if (e->cap_stream) (void)hipStreamDestroy(e->cap_stream);
  }
  delete e;
  return MQ_OK;
}

int mq_encoder_load_weights(mq_encoder* e, const float* blob, int64_t n_floats) {
  clear_error();
  MQ_CHECK_ARG(e && blob, "NULL argument");
  const mq_bert_config& c = e->cfg;
  const int64_t need = weight_count(c);
  MQ_CHECK_ARG(n_floats == need, "weight blob has %lld floats, config needs %lld",
               (long long)n_floats, (long long)need);
  std::lock_guard<std::mutex> lk(e->mu);
  DeviceGuard dg(e->device);
  int rc = e->weights.ensure((size_t)need);
  if (rc) return rc;
  MQ_HIP(hipMemcpy(e->weights.p, blob, (size_t)need * 4, hipMemcpyHostToDevice));
  const int64_t H = c.hidden, F = c.ffn;
  const float* p = e->weights.p;
  auto take = [&](int64_t n) {
    const float* r = p;
    p += n;
    return r;
  };
  e->word = take((int64_t)c.vocab_size * H);
  e->pos = take((int64_t)c.max_positions * H);
  e->typ = take((int64_t)c.type_vocab * H);
  e->eg = take(H);
  e->eb = take(H);
  e->layers.clear();
  for (int l = 0; l < c.layers; ++l) {
    LayerW w;
    w.wqkv = take(3 * H * H);
    w.bqkv = take(3 * H);
    w.wo = take(H * H);
    w.bo = take(H);
    w.ln1g = take(H);
    w.ln1b = take(H);
    w.w1 = take(F * H);
    w.b1 = take(F);
    w.w2 = take(H * F);
    w.b2 = take(H);
    w.ln2g = take(H);
    w.ln2b = take(H);
    e->layers.push_back(w);
  }
  e->loaded = true;
  if (H % 16 == 0 && F % 16 == 0) {  // (the few-row path needs them: use_rows_path checks)
    rc = build_frag16(e);
    if (rc) return rc;
  }
  rc = build_wkt(e);
  if (rc) return rc;
  return build_w3(e);  // (re)split the new weights when the split-f32 precision is selected
}

int mq_encoder_set_precision(mq_encoder* e, int dtype) {
  clear_error();
  MQ_CHECK_ARG(e, "NULL encoder");
  MQ_CHECK_ARG(dtype == MQ_DTYPE_F32 || dtype == MQ_DTYPE_F32X6,
               "encoder precision must be MQ_DTYPE_F32 or MQ_DTYPE_F32X6 (got %d)", dtype);
  std::lock_guard<std::mutex> lk(e->mu);
  e->precision = dtype;
  return build_w3(e);
}

int mq_debug_gemm_f32(const float* A, const float* W, const float* bias, const float* resid,
                      float* out, int M, int N, int K, int epi, int tile, void* stream) {
  clear_error();
  MQ_CHECK_ARG(A && W && bias && out && (epi != EPI_RESID || resid), "NULL buffer");
  MQ_CHECK_ARG(M > 0 && N > 0 && K > 0 && K % kBK == 0, "bad shape M=%d N=%d K=%d", M, N, K);
  MQ_CHECK_ARG(epi >= 0 && epi <= 3 && tile >= 0 && tile <= 9, "bad epi/tile");
  int dev = 0, cus = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  GemmArgs g{nullptr, 0, A, K, W, bias, resid, N, out, N, M, N, K};
  hipStream_t s = (hipStream_t)stream;
  if (tile == 4) {  // split-K path (test hook: allocates its own slab)
    MQ_CHECK_ARG(N % 4 == 0, "split-K needs N %% 4 == 0");
    const int slices = K / kBK;
    int S = 1;
    for (int c = 2; c <= slices && c <= 64; ++c)
      if (slices % c == 0) S = c;
    float* slab = nullptr;
    if (hipMalloc((void**)&slab, (size_t)S * M * N * 4) != hipSuccess)
      MQ_FAIL(MQ_ENOMEM, "slab allocation failed");
    g.slab = slab;
    g.slab_floats = (size_t)S * M * N;
    switch (epi) {
      case EPI_BIAS: launch_splitk<EPI_BIAS>(g, S, s); break;
      case EPI_GELU_ERF: launch_splitk<EPI_GELU_ERF>(g, S, s); break;
      case EPI_GELU_TANH: launch_splitk<EPI_GELU_TANH>(g, S, s); break;
      default: launch_splitk<EPI_RESID>(g, S, s); break;
    }
    const hipError_t err = hipStreamSynchronize(s);
    (void)hipFree(slab);
    if (err != hipSuccess) MQ_FAIL(MQ_EHIP, "split-K GEMM failed: %s", hipGetErrorString(err));
    return MQ_OK;
  }
  switch (epi) {
    case EPI_BIAS: launch_gemm_tile<EPI_BIAS>(g, tile, cus, s); break;
    case EPI_GELU_ERF: launch_gemm_tile<EPI_GELU_ERF>(g, tile, cus, s); break;
    case EPI_GELU_TANH: launch_gemm_tile<EPI_GELU_TANH>(g, tile, cus, s); break;
    default: launch_gemm_tile<EPI_RESID>(g, tile, cus, s); break;
  }
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mq_debug_attention(const float* qkv, const int* mask, int B, int L, int H, int heads, float scale,
                       int variant, float* ctx, void* stream) {
  clear_error();
  MQ_CHECK_ARG(qkv && mask && ctx, "NULL buffer");
  MQ_CHECK_ARG(B > 0 && L > 0 && heads > 0 && H == heads * kDh, "bad shape B=%d L=%d H=%d heads=%d", B, L, H, heads);
  hipStream_t s = (hipStream_t)stream;
  const int qt = (L + 31) / 32;
  const dim3 grid(B * heads * qt);
  switch (variant) {
    case -1: launch_attention(B, L, heads, qt, H, scale, qkv, mask, ctx, s); break;
    case 1: hipLaunchKernelGGL(attention_kernel<1>, grid, dim3(64), 0, s, qkv, mask, L, H, heads, qt, scale, ctx); break;
    case 2: hipLaunchKernelGGL(attention_kernel<2>, grid, dim3(128), 0, s, qkv, mask, L, H, heads, qt, scale, ctx); break;
    case 4: hipLaunchKernelGGL(attention_kernel<4>, grid, dim3(256), 0, s, qkv, mask, L, H, heads, qt, scale, ctx); break;
    case 8: hipLaunchKernelGGL(attention_kernel<8>, grid, dim3(512), 0, s, qkv, mask, L, H, heads, qt, scale, ctx); break;
    case 12:  // one wave per head: the dispatcher's condition on the shape
      MQ_CHECK_ARG(heads == 12 && L <= 32, "variant 12 needs heads == 12 and L <= 32 (heads %d, L %d)", heads, L);
      hipLaunchKernelGGL((attention_kernel<1, 12>), dim3(B * qt), dim3(768), 0, s, qkv, mask, L, H, heads, qt, scale,
                         ctx);
      break;
    case 16:
      MQ_CHECK_ARG(L <= 64, "variant 16 (attention_rows_kernel) needs L <= 64 (got %d)", L);
      hipLaunchKernelGGL(attention_rows_kernel, grid, dim3(512), 0, s, qkv, mask, L, H, heads, qt, scale, ctx);
      break;
    default: MQ_FAIL(MQ_EINVAL, "bad attention variant %d", variant);
  }
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mq_debug_attn_oproj(const float* qkv, const int* mask, int B, int L, int H, int heads, float scale,
                        const float* Wo, const float* bo, const float* resid, int cls_only, int hg, int qf,
                        int acc, float* out, void* stream) {
  clear_error();
  MQ_CHECK_ARG(qkv && mask && Wo && bo && resid && out, "NULL buffer");
  MQ_CHECK_ARG(B > 0 && L > 0 && heads > 0 && H == heads * kDh, "bad shape B=%d L=%d H=%d heads=%d", B, L, H, heads);
  MQ_CHECK_ARG((hg == 4 || hg == 6) && heads % hg == 0, "hg must be 4 or 6 and divide heads (hg %d, heads %d)", hg,
               heads);
  MQ_CHECK_ARG(L <= 64, "the fused kernel holds L <= 64 keys (got %d)", L);
  MQ_CHECK_ARG(!qf || L % 16 == 0, "qf needs L %% 16 == 0 (got %d)", L);
  const int planes = heads / hg;
  MQ_CHECK_ARG(!acc || planes == 2, "acc needs two head groups (got %d)", planes);
  hipStream_t s = (hipStream_t)stream;
  const int M = B * L, rows = cls_only ? B : M;
  float* scratch = nullptr;  // Wo's frag16 image, then (qf) the qkv image
  const size_t wo_floats = (size_t)H * H, qkv_floats = qf ? (size_t)M * 3 * H : 0;
  if (hipMalloc((void**)&scratch, (wo_floats + qkv_floats) * 4) != hipSuccess)
    MQ_FAIL(MQ_ENOMEM, "operand image allocation failed");
  hipLaunchKernelGGL(frag16_image_kernel, dim3((unsigned)((wo_floats / 4 + 255) / 256)), dim3(256), 0, s, Wo, H, H,
                     reinterpret_cast<floatx4*>(scratch));
  const float* qkv_in = qkv;
  if (qf) {
    float* img = scratch + wo_floats;
    hipLaunchKernelGGL(frag16_qkv_image_kernel, dim3((unsigned)((qkv_floats + 255) / 256)), dim3(256), 0, s, qkv, M,
                       H, img);
    qkv_in = img;
  }
  hipError_t err = hipSuccess;
  if (acc) err = hipMemsetAsync(out, 0, (size_t)rows * H * 4, s);
  if (err == hipSuccess) {  // rps, qtiles, ldr and the grid as forward_rows passes them
    const int rps = cls_only ? 1 : L, qtiles = (rps + 15) / 16;
    const dim3 grid(H / kOpCols, B * qtiles, planes);
    launch_attn_oproj(hg, qf != 0, acc != 0, (L + 15) / 16, grid, s, qkv_in, mask, L, H, rps, qtiles, scale, scratch,
                      bo, resid, cls_only ? L * H : H, out, (int64_t)rows * H, 0);
    err = hipGetLastError();
  }
  const hipError_t serr = hipStreamSynchronize(s);
  (void)hipFree(scratch);
  if (err == hipSuccess) err = serr;
  if (err != hipSuccess) MQ_FAIL(MQ_EHIP, "fused attention + output projection failed: %s", hipGetErrorString(err));
  return MQ_OK;
}

int mq_debug_rows_gemm(int kind, int variant, const float* A, int lda, int64_t a_plane, int s_in, const float* W,
                       const float* bias, const float* resid, int ldr, float* out, int64_t o_plane, int M, int N,
                       int K, int splits, const float* ln_g, const float* ln_b, float eps, float* ln_out,
                       const int* ids, const int* types, int L, int vocab, const float* pos, const float* typ,
                       int type_vocab, int nt_w, float* zbuf, int64_t zn, void* stream) {
  clear_error();
  MQ_CHECK_ARG(kind >= MQ_ROWS_QKV && kind <= MQ_ROWS_DOWN, "bad kind %d", kind);
  MQ_CHECK_ARG(variant == 0 || variant == 1, "variant must be 0 or 1 (got %d)", variant);
  MQ_CHECK_ARG(A && W && bias && out, "NULL buffer");
  MQ_CHECK_ARG(M >= 1 && M <= kRowsMax, "M must be in [1, %d] (got %d)", kRowsMax, M);
  const bool ln_kind = kind == MQ_ROWS_QKV || kind == MQ_ROWS_UP;
  const bool vt = kind == MQ_ROWS_QKV && variant;
  MQ_CHECK_ARG(N > 0 && N % kRT == 0 && (!vt || N % 48 == 0), "N must be a positive multiple of %d (got %d)",
               vt ? 48 : kRT, N);
  MQ_CHECK_ARG(splits >= 1 && splits <= 4, "splits must be in [1, 4] (got %d)", splits);
  MQ_CHECK_ARG(K > 0 && K % (256 * splits) == 0, "K must be a positive multiple of 256 * splits (K %d, splits %d)", K,
               splits);
  MQ_CHECK_ARG(rows_nb_ok(K / splits / 256), "no kernel for a per-split depth of %d (K %d, splits %d)", K / splits, K,
               splits);
  MQ_CHECK_ARG((int64_t)N * K * 4 < ((int64_t)1 << 31), "W is past the 2 GB a buffer load addresses");
  MQ_CHECK_ARG(nt_w == 0 || nt_w == 1, "nt_w must be 0 or 1 (got %d)", nt_w);
  MQ_CHECK_ARG(zn >= 0 && zn % 4 == 0 && (zn == 0 || zbuf) && aligned16(zbuf),
               "zbuf must be 16-byte aligned with zn %% 4 == 0 (zn %lld)", (long long)zn);
  MQ_CHECK_ARG(aligned16(A) && aligned16(W), "A and W must be 16-byte aligned");
  const bool acc = kind == MQ_ROWS_DOWN && variant;
  if (ln_kind) {
    MQ_CHECK_ARG(K == 256 || K == 512 || K == 768 || K == 1024,
                 "a LayerNorm input needs K = hidden in 256 / 512 / 768 / 1024 (got %d)", K);
    MQ_CHECK_ARG(splits == 1, "a LayerNorm input takes an unsplit K (splits %d)", splits);
    MQ_CHECK_ARG(ln_g && ln_b && aligned16(ln_g) && aligned16(ln_b), "NULL or unaligned LayerNorm weights");
    MQ_CHECK_ARG(!ln_out || aligned16(ln_out), "ln_out must be 16-byte aligned");
    MQ_CHECK_ARG(s_in >= (kind == MQ_ROWS_QKV ? 0 : 1) && s_in <= 4, "s_in out of range (kind %d, s_in %d)", kind,
                 s_in);
    if (s_in == 0) {
      MQ_CHECK_ARG(ids && pos && typ && aligned16(pos) && aligned16(typ), "the embedding gather needs ids, pos, typ");
      MQ_CHECK_ARG(L >= 1 && vocab >= 1 && type_vocab >= 1, "bad gather shape L=%d vocab=%d type_vocab=%d", L, vocab,
                   type_vocab);
    } else {
      MQ_CHECK_ARG(a_plane >= 0 && a_plane % 4 == 0, "a_plane must be a non-negative multiple of 4 (got %lld)",
                   (long long)a_plane);
    }
  } else {
    MQ_CHECK_ARG(resid && ldr >= N, "the residual kinds need resid with ldr >= N (ldr %d)", ldr);
    if (kind == MQ_ROWS_OPROJ) {
      MQ_CHECK_ARG(splits == 1, "oproj takes an unsplit K (splits %d)", splits);
      MQ_CHECK_ARG(lda >= K && lda % 4 == 0, "lda must be a multiple of 4, >= K (lda %d, K %d)", lda, K);
    } else {
      MQ_CHECK_ARG(!acc || splits == 2, "acc needs exactly two K splits (got %d)", splits);
      MQ_CHECK_ARG(acc || splits == 1 || o_plane >= (int64_t)M * N, "o_plane must hold a plane of M * N floats (got %lld)",
                   (long long)o_plane);
    }
  }
  hipStream_t s = (hipStream_t)stream;
  float* wimg = nullptr;  // W's frag16 image
  const size_t w_floats = (size_t)N * K;
  if (hipMalloc((void**)&wimg, w_floats * 4) != hipSuccess) MQ_FAIL(MQ_ENOMEM, "operand image allocation failed");
  hipLaunchKernelGGL(frag16_image_kernel, dim3((unsigned)((w_floats / 4 + 255) / 256)), dim3(256), 0, s, W, N, K,
                     reinterpret_cast<floatx4*>(wimg));
  hipError_t err = hipSuccess;
  if (acc) err = hipMemsetAsync(out, 0, (size_t)M * N * 4, s);
  if (err == hipSuccess) {  // lda / ldw / ldo as forward_rows passes them: K, K (oproj: the caller's lda), N
    RowsArgs g{A, kind == MQ_ROWS_OPROJ ? lda : K, ln_kind && s_in ? a_plane : 0, wimg, K, bias,
               ln_kind ? nullptr : resid, ln_kind ? 0 : ldr, out, N, kind == MQ_ROWS_DOWN ? o_plane : 0, M, N, K, splits};
    g.nt_w = nt_w;
    g.zbuf = zn ? zbuf : nullptr;
    g.zn = zn;
    if (ln_kind && s_in == 0) {
      g.ids = ids;
      g.L = L;
      g.vocab = vocab;
      g.pos = pos;
      g.typ = typ;
      g.types = types;
      g.type_vocab = type_vocab;
    }
    if (ln_kind) {
      switch (K) {
        case 256: debug_rows_ln<1>(kind, variant, g, s_in, ln_g, ln_b, eps, ln_out, s); break;
        case 512: debug_rows_ln<2>(kind, variant, g, s_in, ln_g, ln_b, eps, ln_out, s); break;
        case 768: debug_rows_ln<3>(kind, variant, g, s_in, ln_g, ln_b, eps, ln_out, s); break;
        default: debug_rows_ln<4>(kind, variant, g, s_in, ln_g, ln_b, eps, ln_out, s); break;
      }
    } else if (kind == MQ_ROWS_OPROJ) {
      launch_rows<EPI_RESID>(g, s);
    } else if (acc) {
      launch_rows<EPI_RESID, FL_A | FL_ACC>(g, s);
    } else {
      launch_rows<EPI_RESID, FL_A>(g, s);
    }
    err = hipGetLastError();
  }
  const hipError_t serr = hipStreamSynchronize(s);
  (void)hipFree(wimg);
  if (err == hipSuccess) err = serr;
  if (err != hipSuccess) MQ_FAIL(MQ_EHIP, "few-row GEMM failed: %s", hipGetErrorString(err));
  return MQ_OK;
}

int mq_debug_ln_pool(const float* hs, int planes, int64_t plane, const int* mask, int B, int L, int rows, int pooling,
                     const float* ln_g, const float* ln_b, float eps, int H, float* out, int raw, void* stream) {
  clear_error();
  MQ_CHECK_ARG(hs && ln_g && ln_b && out, "NULL buffer");
  MQ_CHECK_ARG(H == 256 || H == 512 || H == 768 || H == 1024, "hidden must be 256/512/768/1024 (got %d)", H);
  MQ_CHECK_ARG(B >= 1 && L >= 1, "bad shape B=%d L=%d", B, L);
  MQ_CHECK_ARG(planes >= 1 && planes <= 4, "planes must be in [1, 4] (got %d)", planes);
  MQ_CHECK_ARG(planes == 1 || (plane > 0 && plane % 4 == 0), "plane must be a positive multiple of 4 (got %lld)",
               (long long)plane);
  MQ_CHECK_ARG(pooling == MQ_POOL_CLS || pooling == MQ_POOL_MEAN, "bad pooling %d", pooling);
  MQ_CHECK_ARG(rows == L || (rows == 1 && pooling == MQ_POOL_CLS),
               "rows per sequence must be L, or 1 with CLS pooling (rows %d, L %d)", rows, L);
  MQ_CHECK_ARG(pooling == MQ_POOL_CLS || mask, "mean pooling needs the mask");
  MQ_CHECK_ARG(raw == 0 || raw == 1, "raw must be 0 or 1 (got %d)", raw);
  MQ_CHECK_ARG(aligned16(hs) && aligned16(ln_g) && aligned16(ln_b) && aligned16(out), "buffers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((B + 3) / 4));
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, hs, planes, plane, mask, B, L, rows, pooling, ln_g, ln_b, eps, out,
                       raw);
  };
  switch (H) {
    case 256: go(ln_pool_kernel<1>); break;
    case 512: go(ln_pool_kernel<2>); break;
    case 768: go(ln_pool_kernel<3>); break;
    default: go(ln_pool_kernel<4>); break;
  }
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mq_debug_cls_attention(const float* q, const float* x, const float* stats, const float* ln_g,
                           const float* ln_b, float eps, const int* mask, int B, int L, int H, int heads,
                           float scale, const float* Wk, const float* Wv, const float* bv, float* ctx,
                           void* stream) {
  clear_error();
  MQ_CHECK_ARG(q && x && mask && Wk && Wv && bv && ctx, "NULL buffer");
  MQ_CHECK_ARG(B > 0 && L > 0 && heads > 0 && H == heads * kDh, "bad shape B=%d L=%d H=%d heads=%d", B, L, H, heads);
  MQ_CHECK_ARG(H == 256 || H == 512 || H == 768, "hidden must be 256 / 512 / 768 (got %d)", H);
  MQ_CHECK_ARG(!stats || (ln_g && ln_b && H == kLnPartW * kLnMaxParts), "stats need ln_g, ln_b and H = %d",
               kLnPartW * kLnMaxParts);
  hipStream_t s = (hipStream_t)stream;
  float* scratch = nullptr;  // Wk^T, then the forward's CLS buffers
  const size_t wkt_floats = (size_t)H * H;
  if (hipMalloc((void**)&scratch, (wkt_floats + ClsBufs::floats(B, H, heads)) * 4) != hipSuccess)
    MQ_FAIL(MQ_ENOMEM, "scratch allocation failed");
  const ClsBufs cb(scratch + wkt_floats, B, H, heads);
  hipLaunchKernelGGL(transpose_kernel, dim3(H / 32, H / 32), dim3(256), 0, s, Wk, H, H, scratch);
  launch_cls_u(B, H, heads, q, scratch, cb.u, s);
  launch_cls_ctx(B, L, H, heads, scale, x, stats, ln_g, ln_b, eps, cb.u, mask, Wv, bv, cb.z, cb.part, cb.live, ctx, s);
  hipError_t err = hipGetLastError();
  const hipError_t serr = hipStreamSynchronize(s);
  (void)hipFree(scratch);
  if (err == hipSuccess) err = serr;
  if (err != hipSuccess) MQ_FAIL(MQ_EHIP, "CLS attention failed: %s", hipGetErrorString(err));
  return MQ_OK;
}

int mq_encoder_set_graphs(mq_encoder* e, int enabled) {
  clear_error();
  MQ_CHECK_ARG(e, "NULL encoder");
  std::lock_guard<std::mutex> lk(e->mu);
  e->use_graphs = enabled != 0;
  return MQ_OK;
}

int mq_encoder_set_option(mq_encoder* e, int option, int value) {
  clear_error();
  MQ_CHECK_ARG(e, "NULL encoder");
  std::lock_guard<std::mutex> lk(e->mu);
  switch (option) {
    case MQ_ENC_OPT_ROWS_MAX:
      MQ_CHECK_ARG(value >= 0 && value <= kRowsMax, "rows_max must be in [0, %d] (got %d)", kRowsMax, value);
      e->rows_max = value;
      break;
    case MQ_ENC_OPT_ROWS_SPLITS:
      MQ_CHECK_ARG(value >= 0 && value <= 4, "rows_splits must be in [0, 4] (got %d)", value);
      e->rows_splits = value;
      break;
    case MQ_ENC_OPT_SPLITK_MAX:
      MQ_CHECK_ARG(value >= 2 && value <= 64, "splitk_max must be in [2, 64] (got %d)", value);
      e->splitk_max = value;
      break;
    case MQ_ENC_OPT_FUSE_ATTN_OPROJ:
      MQ_CHECK_ARG(value == 0 || value == 1, "fuse_attn_oproj must be 0 or 1 (got %d)", value);
      e->fuse_attn_oproj = value != 0;
      break;
    case MQ_ENC_OPT_RESIDENT_LAYERS:
      MQ_CHECK_ARG(value >= 0 && value <= 1024, "resident_layers must be in [0, 1024] (got %d)", value);
      e->resident_layers = value;
      break;
    case MQ_ENC_OPT_SPLITK_TILES:
      MQ_CHECK_ARG(value >= 0 && value <= 4096, "splitk_tiles must be in [0, 4096] (got %d)", value);
      e->splitk_tiles = value;
      break;
    case MQ_ENC_OPT_X6_PRESPLIT:
      MQ_CHECK_ARG(value == 0 || value == 1, "x6_presplit must be 0 or 1 (got %d)", value);
      e->x6_presplit = value != 0;
      break;
    case MQ_ENC_OPT_ROWS_PLANES:
      MQ_CHECK_ARG(value == 0 || value == 1, "rows_planes must be 0 or 1 (got %d)", value);
      e->rows_planes = value != 0;
      break;
    case MQ_ENC_OPT_LN_FOLD:
      MQ_CHECK_ARG(value == 0 || value == 1, "ln_fold must be 0 or 1 (got %d)", value);
      e->ln_fold = value != 0;
      break;
    case MQ_ENC_OPT_CLS_KFREE:
      MQ_CHECK_ARG(value == 0 || value == 1, "cls_kfree must be 0 or 1 (got %d)", value);
      e->cls_kfree = value != 0;
      break;
    case MQ_ENC_OPT_QKV_ATTN:
      MQ_CHECK_ARG(value == 0 || value == 1, "qkv_attn must be 0 or 1 (got %d)", value);
      e->qkv_attn = value != 0;
      break;
    case MQ_ENC_OPT_EPI_SPLIT:
      MQ_CHECK_ARG(value == 0 || value == 1, "epi_split must be 0 or 1 (got %d)", value);
      e->epi_split = value != 0;
      break;
    default:
      MQ_FAIL(MQ_EINVAL, "unknown encoder option %d", option);
  }
  // captured forwards bake the old choices in
  for (auto& g : e->graphs) (void)hipGraphExecDestroy(g.exec);
  e->graphs.clear();
  return MQ_OK;
}

int mq_encoder_get_option(const mq_encoder* e, int option, int* value) {
  clear_error();
  MQ_CHECK_ARG(e && value, "NULL argument");
  switch (option) {
    case MQ_ENC_OPT_ROWS_MAX: *value = e->rows_max; break;
    case MQ_ENC_OPT_ROWS_SPLITS: *value = e->rows_splits; break;
    case MQ_ENC_OPT_SPLITK_MAX: *value = e->splitk_max; break;
    case MQ_ENC_OPT_FUSE_ATTN_OPROJ: *value = e->fuse_attn_oproj ? 1 : 0; break;
    case MQ_ENC_OPT_RESIDENT_LAYERS: *value = e->resident_layers; break;
    case MQ_ENC_OPT_SPLITK_TILES: *value = e->splitk_tiles; break;
    case MQ_ENC_OPT_X6_PRESPLIT: *value = e->x6_presplit ? 1 : 0; break;
    case MQ_ENC_OPT_ROWS_PLANES: *value = e->rows_planes ? 1 : 0; break;
    case MQ_ENC_OPT_LN_FOLD: *value = e->ln_fold ? 1 : 0; break;
    case MQ_ENC_OPT_CLS_KFREE: *value = e->cls_kfree ? 1 : 0; break;
    case MQ_ENC_OPT_QKV_ATTN: *value = e->qkv_attn ? 1 : 0; break;
    case MQ_ENC_OPT_EPI_SPLIT: *value = e->epi_split ? 1 : 0; break;
    default: MQ_FAIL(MQ_EINVAL, "unknown encoder option %d", option);
  }
  return MQ_OK;
}

int mq_encoder_set_timing(mq_encoder* e, int enabled) {
  clear_error();
  MQ_CHECK_ARG(e, "NULL encoder");
  std::lock_guard<std::mutex> lk(e->mu);
  DeviceGuard dg(e->device);
  e->tl.drain();
  e->tl.on = enabled != 0;
  return MQ_OK;
}

int mq_encoder_read_timing(mq_encoder* e, float* ms, int n) {
  clear_error();
  MQ_CHECK_ARG(e && ms && n >= 0, "bad argument");
  std::lock_guard<std::mutex> lk(e->mu);
  DeviceGuard dg(e->device);
  e->tl.read(ms, n);
  return MQ_OK;
}

}  // extern "C"

namespace {

// The activation buffers of one forward of B x L tokens (grown on demand, never shrunk).
int ensure_forward_bufs(mq_encoder* e, int B, int L) {
  const mq_bert_config& c = e->cfg;
  const size_t M = (size_t)B * L;
  if (e->tl.used > 4096) e->tl.drain();  // bound the event pool while timing
  int rc = MQ_OK;
  // split-K slabs: up to 2*CUs partial tiles of 32 x 128 floats
  rc = e->slab.ensure((size_t)2 * e->num_cus * 32 * 128);
  if (rc) return rc;
  // y also holds the few-row forward's output-projection planes (<= 4 of M rows)
  rc = build_fold(e);  // (MQ_ENC_OPT_LN_FOLD: the folded weights of the current mode, once)
  if (rc) return rc;
  const size_t ln_parts = e->ln_fold && M > 256 ? (size_t)4 * M * std::max(1, c.hidden / kLnPartW) : 0;
  // (MQ_ENC_OPT_CLS_KFREE: the last layer's CLS-row buffers)
  const size_t cls_floats = e->cls_kfree && c.pooling == MQ_POOL_CLS && L > 1 ? ClsBufs::floats(B, c.hidden, c.heads) : 0;
  for (auto bn : {std::make_pair(&e->x, M * c.hidden), std::make_pair(&e->y, (M <= (size_t)kRowsMax ? 4 : 1) * M * c.hidden),
                  std::make_pair(&e->ctx, M * c.hidden), std::make_pair(&e->qkv, M * 3 * c.hidden),
                  // (the few-row FFN output is frag16: whole 16-row blocks)
                  std::make_pair(&e->ffn, (M + 15) / 16 * 16 * c.ffn), std::make_pair(&e->lnst, ln_parts),
                  std::make_pair(&e->cls, cls_floats)}) {
    rc = bn.first->ensure(bn.second);
    if (rc) return rc;
  }
  return MQ_OK;
}

// The handle's own io buffers for M tokens and B output rows of `hidden` floats.
int ensure_io(mq_encoder* e, size_t M, int B) {
  if (e->io_tokens < M) {
    if (e->io_ids) (void)hipFree(e->io_ids);
    if (e->io_mask) (void)hipFree(e->io_mask);
    e->io_ids = e->io_mask = nullptr;
    e->io_tokens = 0;
    if (hipMalloc((void**)&e->io_ids, M * 4) != hipSuccess ||
        hipMalloc((void**)&e->io_mask, M * 4) != hipSuccess)
      MQ_FAIL(MQ_ENOMEM, "hipMalloc(io) failed");
    e->io_tokens = M;
  }
  return e->io_out.ensure((size_t)B * e->cfg.hidden);
}

}  // namespace

extern "C" {

int mq_encoder_embed(mq_encoder* e, const int32_t* ids, const int32_t* mask, int B, int L,
                     float* out, int io_on_device, void* stream) {
  clear_error();
  MQ_CHECK_ARG(e, "NULL encoder");
  MQ_CHECK_ARG(B >= 0 && L >= 1, "bad shape B=%d L=%d", B, L);
  MQ_CHECK_ARG(L <= e->cfg.max_positions, "L=%d exceeds max_positions %d", L, e->cfg.max_positions);
  if (B == 0) return MQ_OK;
  MQ_CHECK_ARG(ids && mask && out, "NULL buffer");
  MQ_CHECK_ARG((int64_t)B * L < (1ll << 31) / 4096, "batch too large");
  if (!e->loaded) MQ_FAIL(MQ_ESTATE, "encoder weights not loaded");
  std::lock_guard<std::mutex> lk(e->mu);
  DeviceGuard dg(e->device);
  hipStream_t s = (hipStream_t)stream;
  const mq_bert_config& c = e->cfg;
  const size_t M = (size_t)B * L;
  int rc = ensure_forward_bufs(e, B, L);
  if (rc) return rc;
  const bool graph = e->use_graphs && !e->tl.on;
  const int* dids = ids;
  const int* dmask = mask;
  float* dout = out;
  if (!io_on_device || graph) {  // stage through the encoder's own io buffers
    rc = ensure_io(e, M, B);
    if (rc) return rc;
    const hipMemcpyKind kind = io_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (!io_on_device && M * 8 + (size_t)B * c.hidden * 4 <= (1u << 20)) {
      // few tokens (single queries): ids and mask through pinned staging, one DMA each
      rc = e->pin.ensure(M * 8 + (size_t)B * c.hidden * 4);
      if (rc) return rc;
      memcpy(e->pin.as<unsigned char>(), ids, M * 4);
      memcpy(e->pin.as<unsigned char>() + M * 4, mask, M * 4);
      MQ_HIP(hipMemcpyAsync(e->io_ids, e->pin.p, M * 4, kind, s));
      MQ_HIP(hipMemcpyAsync(e->io_mask, e->pin.as<unsigned char>() + M * 4, M * 4, kind, s));
    } else {
      MQ_HIP(hipMemcpyAsync(e->io_ids, ids, M * 4, kind, s));
      MQ_HIP(hipMemcpyAsync(e->io_mask, mask, M * 4, kind, s));
    }
    dids = e->io_ids;
    dmask = e->io_mask;
    dout = e->io_out.p;
  }
  if (graph) {
    rc = launch_graph(e, B, L, s);
  } else {
    rc = forward(e, dids, nullptr, dmask, B, L, dout, 0, s);
  }
  if (rc) return rc;
  if (io_on_device && dout != out)
    MQ_HIP(hipMemcpyAsync(out, dout, (size_t)B * c.hidden * 4, hipMemcpyDeviceToDevice, s));
  if (!io_on_device) {
    const size_t ob = (size_t)B * c.hidden * 4;
    if (M * 8 + ob <= (1u << 20)) {  // (the pinned staging above)
      unsigned char* hp = e->pin.as<unsigned char>() + M * 8;
      MQ_HIP(hipMemcpyAsync(hp, dout, ob, hipMemcpyDeviceToHost, s));
      MQ_HIP(hipStreamSynchronize(s));
      memcpy(out, hp, ob);
    } else {
      MQ_HIP(hipMemcpyAsync(out, dout, ob, hipMemcpyDeviceToHost, s));
      MQ_HIP(hipStreamSynchronize(s));
    }
  }
  return MQ_OK;
}

int mq_encoder_load_head(mq_encoder* e, const float* pooler_w, const float* pooler_b, const float* cls_w,
                         const float* cls_b, int n_labels) {
  clear_error();
  MQ_CHECK_ARG(n_labels >= 1 && n_labels <= MQ_HEAD_MAX_LABELS, "n_labels must be in [1, %d] (got %d)",
               MQ_HEAD_MAX_LABELS, n_labels);
  MQ_CHECK_ARG(e, "NULL encoder");
  MQ_CHECK_ARG(pooler_w && pooler_b && cls_w && cls_b, "NULL argument");
  if (!e->loaded) MQ_FAIL(MQ_ESTATE, "encoder weights not loaded");
  std::lock_guard<std::mutex> lk(e->mu);
  DeviceGuard dg(e->device);
  const size_t H = (size_t)e->cfg.hidden;
  e->n_labels = 0;  // (no half-replaced head after a failure)
  const int rc = e->head.ensure(H * H + H + (size_t)MQ_HEAD_MAX_LABELS * (H + 1));
  if (rc) return rc;
  float* p = e->head.p;
  MQ_HIP(hipMemcpy(p, pooler_w, H * H * 4, hipMemcpyHostToDevice));
  MQ_HIP(hipMemcpy(p + H * H, pooler_b, H * 4, hipMemcpyHostToDevice));
  MQ_HIP(hipMemcpy(p + H * H + H, cls_w, (size_t)n_labels * H * 4, hipMemcpyHostToDevice));
  MQ_HIP(hipMemcpy(p + H * H + H + (size_t)MQ_HEAD_MAX_LABELS * H, cls_b, (size_t)n_labels * 4, hipMemcpyHostToDevice));
  e->n_labels = n_labels;
  return MQ_OK;
}

int mq_encoder_score(mq_encoder* e, const int32_t* ids, const int32_t* types, const int32_t* mask, int B, int L,
                     float* logits, int io_on_device, void* stream) {
  clear_error();
  MQ_CHECK_ARG(e, "NULL encoder");
  MQ_CHECK_ARG(B >= 0 && L >= 1, "bad shape B=%d L=%d", B, L);
  MQ_CHECK_ARG(L <= e->cfg.max_positions, "L=%d exceeds max_positions %d", L, e->cfg.max_positions);
  if (!e->loaded) MQ_FAIL(MQ_ESTATE, "encoder weights not loaded");
  if (e->cfg.pooling != MQ_POOL_CLS) MQ_FAIL(MQ_ESTATE, "scoring needs CLS pooling (the head reads the CLS state)");
  if (B == 0) return MQ_OK;
  MQ_CHECK_ARG(ids && types && mask && logits, "NULL buffer");
  MQ_CHECK_ARG((int64_t)B * L < (1ll << 31) / 4096, "batch too large");
  std::lock_guard<std::mutex> lk(e->mu);
  if (e->n_labels < 1) MQ_FAIL(MQ_ESTATE, "no cross-encoder head loaded (mq_encoder_load_head)");
  DeviceGuard dg(e->device);
  hipStream_t s = (hipStream_t)stream;
  const mq_bert_config& c = e->cfg;
  const size_t M = (size_t)B * L, H = (size_t)c.hidden, nl = (size_t)e->n_labels;
  int rc = ensure_forward_bufs(e, B, L);
  if (!rc) rc = e->cls_state.ensure((size_t)B * H);
  if (rc) return rc;
  const int* dids = ids;
  const int* dtypes = types;
  const int* dmask = mask;
  float* dlogits = logits;
  // host io: ids | types | mask | logits through one pinned block, one DMA each way per array
  const size_t ob = (size_t)B * nl * 4;
  if (!io_on_device) {
    rc = ensure_io(e, M, B);  // (io_out's B x hidden floats hold the B x n_labels logits)
    if (rc) return rc;
    if (e->io_type_tokens < M) {
      if (e->io_types) (void)hipFree(e->io_types);
      e->io_types = nullptr;
      e->io_type_tokens = 0;
      if (hipMalloc((void**)&e->io_types, M * 4) != hipSuccess) MQ_FAIL(MQ_ENOMEM, "hipMalloc(io) failed");
      e->io_type_tokens = M;
    }
    rc = e->pin.ensure(M * 12 + ob);
    if (rc) return rc;
    unsigned char* hp = e->pin.as<unsigned char>();
    memcpy(hp, ids, M * 4);
    memcpy(hp + M * 4, types, M * 4);
    memcpy(hp + M * 8, mask, M * 4);
    MQ_HIP(hipMemcpyAsync(e->io_ids, hp, M * 4, hipMemcpyHostToDevice, s));
    MQ_HIP(hipMemcpyAsync(e->io_types, hp + M * 4, M * 4, hipMemcpyHostToDevice, s));
    MQ_HIP(hipMemcpyAsync(e->io_mask, hp + M * 8, M * 4, hipMemcpyHostToDevice, s));
    dids = e->io_ids;
    dtypes = e->io_types;
    dmask = e->io_mask;
    dlogits = e->io_out.p;
  }
  // always eager: captured graphs are the embedding forward's (launch_graph), never replayed here
  rc = forward(e, dids, dtypes, dmask, B, L, e->cls_state.p, 1, s);
  if (rc) return rc;
  const float* hp = e->head.p;
  e->tl.mark(s, ST_POOL);
  launch_cls_head(e->cls_state.p, B, c.hidden, hp, hp + H * H, hp + H * H + H,
                  hp + H * H + H + (size_t)MQ_HEAD_MAX_LABELS * H, e->n_labels, dlogits, s);
  e->tl.close(s);
  MQ_HIP(hipGetLastError());
  if (!io_on_device) {
    unsigned char* out_pin = e->pin.as<unsigned char>() + M * 12;
    MQ_HIP(hipMemcpyAsync(out_pin, dlogits, ob, hipMemcpyDeviceToHost, s));
    MQ_HIP(hipStreamSynchronize(s));
    memcpy(logits, out_pin, ob);
  }
  return MQ_OK;
}

#ifdef MQ_KTRACE
// Measurement builds: copy (and clear) the few-row kernels' phase stamps, [4][1024][8] int64.
int mq_debug_ktrace_read(long long* out, int n) {
  const int total = kTraceRegions * kTraceWgs * kTraceSlots;
  if (!out || n < total) return MQ_EINVAL;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mq_ktrace), total * sizeof(long long)) != hipSuccess) return MQ_EHIP;
  std::vector<long long> zero(total, 0);
  if (hipMemcpyToSymbol(HIP_SYMBOL(mq_ktrace), zero.data(), total * sizeof(long long)) != hipSuccess) return MQ_EHIP;
  return MQ_OK;
}
#endif

}  // extern "C"
