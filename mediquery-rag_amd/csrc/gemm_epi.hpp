// gemm_epi.hpp - epilogue pieces shared by the encoder GEMMs (encoder.hip) and the
// pre-split split-f32 GEMM (gemm_x6p.hip): the epilogue kinds, the branch-free GELU
// forms, and a wave-tile store of 32x32 MFMA accumulators with bias / GELU / residual.
#pragma once

#include "gemm_f32.hpp"
#include "gemm_x6p.hpp"

namespace mq {

// EPI_RESID_STATS: EPI_RESID that also leaves per-row LayerNorm partials of its output
// (encoder.hip, LnArgs: the LayerNorm is then applied by the consuming GEMM).
// LayerNorm folded into the split-f32 GEMMs (LnFold, gemm_x6p.hpp; 16x16 store only):
// EPI_RESID_LN_STATS is the producer, out = acc + bias + LN(resid) plus the partials of out;
// the *_LNFOLD kinds are the consumers, out = epi(rho_r (acc - mu_r s[col]) + c[col]) with
// c passed as `bias`.
enum Epi {
  EPI_BIAS = 0,
  EPI_GELU_ERF = 1,
  EPI_GELU_TANH = 2,
  EPI_RESID = 3,
  EPI_RESID_STATS = 4,
  EPI_RESID_LN_STATS = 5,
  EPI_BIAS_LNFOLD = 6,
  EPI_GELU_ERF_LNFOLD = 7,
  EPI_GELU_TANH_LNFOLD = 8
};
constexpr bool epi_is_lnfold(int epi) { return epi >= EPI_BIAS_LNFOLD && epi <= EPI_GELU_TANH_LNFOLD; }

// GELU, branch-free (it runs 64 times per lane in every FFN-up tile epilogue; ocml's erff
// is ~50 VALU + a divergent branch per element and measured as the FFN-up epilogue's cost).
// erf form: x * Phi(x), Phi(x) = 0.5 erfc(-x / sqrt 2), with erfc(z) for z = |x| / sqrt 2 from
// the Chebyshev fit t * exp(-z^2 + P(t)), t = 1 / (1 + z / 2) (Numerical Recipes erfcc,
// |relative error| < 1.2e-7 for all z >= 0): Phi = 1 - e / 2 for x >= 0, e / 2 below.  No
// 1 + erf cancellation for negative x: max |error| vs float64 3.8e-7 over [-12, 12], relative
// 1.7e-6 where |gelu| > 1e-3 (0.5 x (1 + erff) in fp32: 4.5e-7 and 5.1e-5).  v_rcp / v_exp
// are the hardware 1-ulp forms.
__device__ __forceinline__ float gelu_erf(float x) {
  const float z = fabsf(x) * 0.70710678118654752f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.5f, z, 1.0f));
  float p = 0.17087277f;
  p = fmaf(p, t, -0.82215223f);
  p = fmaf(p, t, 1.48851587f);
  p = fmaf(p, t, -1.13520398f);
  p = fmaf(p, t, 0.27886807f);
  p = fmaf(p, t, -0.18628806f);
  p = fmaf(p, t, 0.09678418f);
  p = fmaf(p, t, 0.37409196f);
  p = fmaf(p, t, 1.00002368f);
  p = fmaf(p, t, -1.26551223f);
  const float e = t * __builtin_amdgcn_exp2f(fmaf(-z, z, p) * 1.4426950408889634f);  // erfc(z)
  return x * (x >= 0.f ? fmaf(-0.5f, e, 1.0f) : 0.5f * e);
}
// tanh form (llama.cpp's): 0.5 x (1 + tanh u) = x / (1 + exp(-2u)), u = sqrt(2/pi)(x + 0.044715 x^3)
__device__ __forceinline__ float gelu_tanh(float x) {
  const float u = 0.7978845608028654f * fmaf(0.044715f * x, x * x, x);
  return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(u * -2.8853900817779268f));
}

template <int EPI>
__device__ __forceinline__ float epi_apply(float v) {
  if constexpr (EPI == EPI_GELU_ERF || EPI == EPI_GELU_ERF_LNFOLD) return gelu_erf(v);
  if constexpr (EPI == EPI_GELU_TANH || EPI == EPI_GELU_TANH_LNFOLD) return gelu_tanh(v);
  return v;
}

// A row's kLnMaxParts (mean, M2) partials over kLnPartW columns each, p[i] = (mean_2i, M2_2i,
// mean_2i+1, M2_2i+1), merged into the row's mean and 1 / sqrt(var + eps) (Chan, equal
// counts).  Every operation is spelled out (no contraction left to the compiler): the
// producer's residual path and the consumers call this one function and get the same bits.
__device__ __forceinline__ void ln_merge(const floatx4 (&p)[kLnMaxParts / 2], float eps, float& mean, float& rstd) {
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < kLnMaxParts / 2; ++i) {
    sum += p[i].x;
    sum += p[i].z;
  }
  mean = sum * (1.0f / (float)kLnMaxParts);
  float m2 = 0.f;
#pragma unroll
  for (int i = 0; i < kLnMaxParts / 2; ++i) {
    const float d0 = p[i].x - mean, d1 = p[i].z - mean;
    m2 = __fmaf_rn((float)kLnPartW * d0, d0, m2 + p[i].y);
    m2 = __fmaf_rn((float)kLnPartW * d1, d1, m2 + p[i].w);
  }
  rstd = 1.0f / sqrtf(__fmaf_rn(m2, 1.0f / (float)(kLnPartW * kLnMaxParts), eps));
}
// (mean, rstd) of one row per lane from stats [M][kLnMaxParts] pairs: lane (c = lane & 15, g =
// lane >> 4) of a wave tile whose origin row is wr0 takes row wr0 + 16 (c >> 2) + 4 g + (c & 3)
// (clamped to M - 1; block rows past MB repeat the last), i.e. lane 4 m + e of a 16-lane row
// group holds the group's row e of block row m: ln_row_bcast hands it to the group's lanes.
template <int MB>
__device__ __forceinline__ void ln_row_own(const float* __restrict__ stats, int wr0, int M, float eps, int lane,
                                           float& mean, float& rstd) {
  const int c = lane & 15;
  const int row = min(wr0 + 16 * min(c >> 2, MB - 1) + 4 * (lane >> 4) + (c & 3), M - 1);
  const floatx4* src = reinterpret_cast<const floatx4*>(stats + (int64_t)row * (2 * kLnMaxParts));
  floatx4 p[kLnMaxParts / 2];
#pragma unroll
  for (int i = 0; i < kLnMaxParts / 2; ++i) p[i] = src[i];
  ln_merge(p, eps, mean, rstd);
}
__device__ __forceinline__ float ln_row_bcast(float v, int lane, int m, int e) {
  return __shfl(v, (lane & 48) + 4 * m + e);
}
// sum over the 16 lanes of a row group, every lane ending with the same bits (quad xor 1, quad
// xor 2, then the mirrors: the lanes they pair hold equal quad / half sums)
__device__ __forceinline__ float row16_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));
  return v;
}

// Store one wave's TM x TN grid of 32x32 accumulators whose origin is (wr0, wc0):
// out = epi(acc + bias[col]) (+ resid for EPI_RESID).  A wave tile inside [M, N] takes
// buffer loads / stores off its origin (one lane offset in a VGPR, each register's row
// offset a scalar soffset: no per-element address arithmetic) with every bias / residual
// load issued before the first use; a ragged edge tile takes guarded plain accesses.
template <int EPI, int TM, int TN>
__device__ __forceinline__ void store_wave_tile(floatx16 (&acc)[TM][TN], int wr0, int wc0, int M, int N,
                                                const float* __restrict__ bias, const float* __restrict__ resid,
                                                int ldr, float* __restrict__ out, int ldo, int lane) {
  if (wr0 + TM * 32 <= M && wc0 + TN * 32 <= N) {
    float bv[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) bv[tn] = bias[wc0 + tn * 32 + (lane & 31)];
    float rv[TM][TN][16];
    if constexpr (EPI == EPI_RESID) {
      const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(resid + (int64_t)wr0 * ldr + wc0), (short)0, 0x7fffffff, 0x00020000);
      const int rl = (4 * (lane >> 5) * ldr + (lane & 31)) * 4;
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
          for (int e = 0; e < 16; ++e)
            rv[tm][tn][e] = __uint_as_float(
                __builtin_amdgcn_raw_buffer_load_b32(rr, rl, (acc_row(tm, e, 0) * ldr + tn * 32) * 4, 0));
    }
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(out + (int64_t)wr0 * ldo + wc0), (short)0, 0x7fffffff, 0x00020000);
    const int ol = (4 * (lane >> 5) * ldo + (lane & 31)) * 4;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float v = epi_apply<EPI>(acc[tm][tn][e] + bv[tn]);
          if constexpr (EPI == EPI_RESID) v += rv[tm][tn][e];
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ro, ol, (acc_row(tm, e, 0) * ldo + tn * 32) * 4, 0);
        }
    return;
  }
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    const int col = wc0 + tn * 32 + (lane & 31);
    if (col >= N) continue;
    const float b = bias[col];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = wr0 + acc_row(tm, e, lane);
        if (row >= M) continue;
        float v = epi_apply<EPI>(acc[tm][tn][e] + b);
        if constexpr (EPI == EPI_RESID) v += resid[(int64_t)row * ldr + col];
        out[(int64_t)row * ldo + col] = v;
      }
  }
}

// The same store for a wave's MB x NB grid of 16x16 accumulators (v_mfma_f32_16x16x32_*:
// register e of lane l is row 4 (l >> 4) + e, column l & 15 of its block).  The residual
// is loaded one block row at a time (the caller's operand fragments stay live across it).
//
// EPI_RESID_LN_STATS (the wave tile is NB 16 = kLnPartW columns wide, N a multiple of it):
// the residual is the previous raw y, normalised on the fly - (r - mu_r) rho_r gamma + beta
// with (mu, rho) merged from lf.stats_in (null: the residual is taken as it is) - and the
// (mean, M2) partial of each output row over the wave tile's columns goes to lf.stats_out
// [row][wc0 / kLnPartW]: the lane's NB columns summed in-lane, then a 4-step reduce over the
// 16 lanes of the row group, two passes (mean, then sum (v - mean)^2).  Rows past M are
// loaded clamped and neither stored nor given partials.
// Loads and stores are buffer ops off column wc0 with a per-row lane offset (rows clamped to M -
// 1 for the loads, stores predicated on row < M: one path for whole and ragged tiles; byte
// offsets are 32-bit, M ld < 2^29); ER rows of a block row are loaded, finished and stored at
// a time.
//
// HAND (K2p's loader-wave hand-off, gemm_x6p.hip): the normalised residual t = (r - mu) rho (r
// itself without stats_in) of the wave tile already lies in LDS at `tl`, written by the
// partner loader wave in accumulator order (ln_tile_write below) - one ds_read_b128 per block,
// no residual or stats_in traffic here; the same v = fma(t, gamma, acc + bias + beta) and the
// same partials, bit for bit.
typedef unsigned uint2v_t __attribute__((ext_vector_type(2)));
// byte offset of lane l's four rows 4 (l >> 4) + e of column l & 15 inside a block's 1 KB of t:
// the 16-B slot of column c of row group g is c ^ g, so that the writer's ds_write_b32 (lanes
// that differ in g hold the same column) and this read are both free of bank conflicts
__device__ __forceinline__ unsigned ln_t_slot(int lane) { return 16u * (unsigned)(lane ^ (lane >> 4)); }
template <int ER, int MB, int NB, bool HAND = false>
__device__ __forceinline__ void store_wave_tile16_ln_stats(floatx4 (&acc)[MB][NB], int wr0, int wc0, int M,
                                                           const float* __restrict__ bias,
                                                           const float* __restrict__ resid, int ldr,
                                                           float* __restrict__ out, int ldo, int lane,
                                                           const LnFold& lf, const unsigned char* tl = nullptr) {
  static_assert(NB * 16 == kLnPartW && MB <= 4, "partials are per kLnPartW-column wave tile");
  static_assert(!HAND || ER == 1, "the hand-off form finishes a row at a time");
  const int c = lane & 15, g = lane >> 4;
  const bool ln_r = lf.stats_in != nullptr;  // (kernel-uniform)
  float own_mu = 0.f, own_rho = 1.0f;        // this lane's row of the residual (ln_row_own)
  if constexpr (!HAND) {
    if (ln_r) ln_row_own<MB>(lf.stats_in, wr0, M, lf.eps, lane, own_mu, own_rho);
  }
  // bias + beta goes into the accumulators in place and only gamma stays live (the kernels
  // around this store sit at the register limit)
  float gv[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int col = wc0 + n * 16 + c;
    const float bb = bias[col] + (ln_r ? lf.b[col] : 0.f);
    gv[n] = ln_r ? lf.g[col] : 1.0f;
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[m][n][e] += bb;
  }
  const __amdgpu_buffer_rsrc_t rr =
      __builtin_amdgcn_make_buffer_rsrc((void*)(resid + wc0), (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t ro =
      __builtin_amdgcn_make_buffer_rsrc((void*)(out + wc0), (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(lf.stats_out + 2 * (wc0 / kLnPartW)), (short)0, 0x7fffffff, 0x00020000);
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    floatx4 tv[NB];
    if constexpr (HAND) {
#pragma unroll
      for (int n = 0; n < NB; ++n)
        tv[n] = *reinterpret_cast<const floatx4*>(tl + (m * NB + n) * 1024 + ln_t_slot(lane));
    }
#pragma unroll
    for (int eh = 0; eh < 4; eh += ER) {
      float v[ER][NB];
      if constexpr (!HAND) {
#pragma unroll
        for (int e2 = 0; e2 < ER; ++e2) {
          const int lo = (min(wr0 + m * 16 + 4 * g + eh + e2, M - 1) * ldr + c) * 4;
#pragma unroll
          for (int n = 0; n < NB; ++n)
            v[e2][n] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rr, lo, n * 64, 0));
        }
      }
#pragma unroll
      for (int e2 = 0; e2 < ER; ++e2) {
        const int e = eh + e2, row = wr0 + m * 16 + 4 * g + e;
        float mu = 0.f, rho = 1.0f;
        if constexpr (!HAND) {
          mu = ln_row_bcast(own_mu, lane, m, e);
          rho = ln_row_bcast(own_rho, lane, m, e);
        }
        const int so = (row * ldo + c) * 4;
        float sum = 0.f;
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          if constexpr (HAND)
            v[e2][n] = __fmaf_rn(tv[n][e], gv[n], acc[m][n][e]);
          else
            v[e2][n] = __fmaf_rn((v[e2][n] - mu) * rho, gv[n], acc[m][n][e]);
          sum += v[e2][n];
          if (row < M) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[e2][n]), ro, so, n * 64, 0);
        }
        const float mean = row16_sum(sum) * (1.0f / (float)kLnPartW);  // the partial's mean
        float m2 = 0.f;
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          const float d = v[e2][n] - mean;
          m2 = __fmaf_rn(d, d, m2);
        }
        m2 = row16_sum(m2);
        if (c == 0 && row < M) {
          uint2v_t pr;
          pr.x = __float_as_uint(mean);
          pr.y = __float_as_uint(m2);
          __builtin_amdgcn_raw_buffer_store_b64(pr, rs, row * (kLnMaxParts * 8), 0, 0);
        }
      }
    }
  }
}

// The loader wave's side of the hand-off: the residual of an MB x NB block wave tile, one
// 16x16 block per 16-byte row-major load instruction (lane -> row lane >> 2, columns 4 (lane &
// 3) .. + 3; rows clamped to M - 1 as the epilogue's loads are; N is a multiple of the wave
// tile's width), and the (mean, M2) partials of one of the lane's MB = 4 rows, that of block
// row lane & 3 (the four lanes of a quad hold the same row of every block row: each merges one
// and a quad broadcast hands it round); then t = (r - mu) rho, with (mu, rho) from the same
// ln_merge as every other user (mu = 0, rho = 1 without stats_in: t is r, as in the global-load
// epilogue), written in accumulator order (ln_t_slot).
template <int MB, int NB>
struct LnTileRegs {
  floatx4 r[MB][NB];
  floatx4 p[kLnMaxParts / 2];
};
template <int Q>
__device__ __forceinline__ float quad_bcast(float v) {  // lane Q of each quad
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), Q * 0x55, 0xF, 0xF, false));
}
template <int MB, int NB>
__device__ __forceinline__ void ln_tile_load(LnTileRegs<MB, NB>& q, const float* __restrict__ resid, int ldr,
                                             int wr0, int wc0, int M, const LnFold& lf, int lane) {
  const __amdgpu_buffer_rsrc_t rr =
      __builtin_amdgcn_make_buffer_rsrc((void*)(resid + wc0), (short)0, 0x7fffffff, 0x00020000);
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    const int row = min(wr0 + m * 16 + (lane >> 2), M - 1);
    const int lo = (row * ldr + 4 * (lane & 3)) * 4;
#pragma unroll
    for (int n = 0; n < NB; ++n)
      q.r[m][n] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rr, lo, n * 64, 0));
  }
  if (lf.stats_in != nullptr) {
    const int row = min(wr0 + (lane & 3) * 16 + (lane >> 2), M - 1);
    const floatx4* src = reinterpret_cast<const floatx4*>(lf.stats_in + (int64_t)row * (2 * kLnMaxParts));
#pragma unroll
    for (int i = 0; i < kLnMaxParts / 2; ++i) q.p[i] = src[i];
  }
}
template <int MB, int NB>
__device__ __forceinline__ void ln_tile_write(const LnTileRegs<MB, NB>& q, unsigned char* tl, const LnFold& lf,
                                              int lane) {
  static_assert(MB == 4, "a quad's lanes share out the block rows");
  const int g = lane >> 4, e = (lane >> 2) & 3;
  unsigned off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) off[i] = (unsigned)(256 * g + 16 * ((4 * (lane & 3) + i) ^ g) + 4 * e);
  float own_mu = 0.f, own_rho = 1.0f;
  if (lf.stats_in != nullptr) ln_merge(q.p, lf.eps, own_mu, own_rho);
  const float mus[4] = {quad_bcast<0>(own_mu), quad_bcast<1>(own_mu), quad_bcast<2>(own_mu), quad_bcast<3>(own_mu)};
  const float rhos[4] = {quad_bcast<0>(own_rho), quad_bcast<1>(own_rho), quad_bcast<2>(own_rho),
                         quad_bcast<3>(own_rho)};
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    const float mu = mus[m], rho = rhos[m];
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float*>(tl + (m * NB + n) * 1024 + off[i]) = (q.r[m][n][i] - mu) * rho;
  }
}

template <int EPI, int MB, int NB>
__device__ __forceinline__ void store_wave_tile16(floatx4 (&acc)[MB][NB], int wr0, int wc0, int M, int N,
                                                  const float* __restrict__ bias, const float* __restrict__ resid,
                                                  int ldr, float* __restrict__ out, int ldo, int lane,
                                                  const LnFold& lf = LnFold{}) {
  const int c = lane & 15, g = lane >> 4;
  if constexpr (EPI == EPI_RESID_LN_STATS) {
    // one row at a time: K2p's default tiles spill 4 VGPRs at two rows, 32 at four (tools/spill_audit.py)
    store_wave_tile16_ln_stats<1>(acc, wr0, wc0, M, bias, resid, ldr, out, ldo, lane, lf);
    return;
  }
  // the consumers of a folded LayerNorm: v = rho_r (acc - mu_r s[col]) + c[col] (c as `bias`)
  constexpr bool FOLD = epi_is_lnfold(EPI);
  static_assert(!FOLD || MB <= 4, "one lane of a 16-lane row group per row of the wave tile");
  float own_mu = 0.f, own_rho = 0.f;  // this lane's row of A (ln_row_own)
  if constexpr (FOLD) ln_row_own<MB>(lf.stats_in, wr0, M, lf.eps, lane, own_mu, own_rho);
  if (wr0 + MB * 16 <= M && wc0 + NB * 16 <= N) {
    float bv[NB], sv[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n) bv[n] = bias[wc0 + n * 16 + c];
    if constexpr (FOLD) {
#pragma unroll
      for (int n = 0; n < NB; ++n) sv[n] = lf.s[wc0 + n * 16 + c];
    }
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(resid + (EPI == EPI_RESID ? (int64_t)wr0 * ldr + wc0 : 0)), (short)0, 0x7fffffff, 0x00020000);
    const int rl = (4 * g * ldr + c) * 4;
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(out + (int64_t)wr0 * ldo + wc0), (short)0, 0x7fffffff, 0x00020000);
    const int ol = (4 * g * ldo + c) * 4;
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      float rv[NB][4];
      if constexpr (EPI == EPI_RESID) {
#pragma unroll
        for (int n = 0; n < NB; ++n)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            rv[n][e] = __uint_as_float(
                __builtin_amdgcn_raw_buffer_load_b32(rr, rl, ((m * 16 + e) * ldr + n * 16) * 4, 0));
      }
      if constexpr (FOLD) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float mu = ln_row_bcast(own_mu, lane, m, e), rho = ln_row_bcast(own_rho, lane, m, e);
#pragma unroll
          for (int n = 0; n < NB; ++n) {
            const float v = epi_apply<EPI>(__fmaf_rn(rho, __fmaf_rn(-mu, sv[n], acc[m][n][e]), bv[n]));
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ro, ol, ((m * 16 + e) * ldo + n * 16) * 4, 0);
          }
        }
      } else {
#pragma unroll
        for (int n = 0; n < NB; ++n)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float v = epi_apply<EPI>(acc[m][n][e] + bv[n]);
            if constexpr (EPI == EPI_RESID) v += rv[n][e];
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ro, ol, ((m * 16 + e) * ldo + n * 16) * 4, 0);
          }
      }
    }
    return;
  }
  if constexpr (FOLD) {  // ragged edge (the row statistics are shared by shuffle: no lane may have left)
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      float mu[4], rho[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        mu[e] = ln_row_bcast(own_mu, lane, m, e);
        rho[e] = ln_row_bcast(own_rho, lane, m, e);
      }
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        const int col = wc0 + n * 16 + c;
        if (col < N) {
          const float b = bias[col], sn = lf.s[col];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int row = wr0 + m * 16 + 4 * g + e;
            if (row < M)
              out[(int64_t)row * ldo + col] = epi_apply<EPI>(__fmaf_rn(rho[e], __fmaf_rn(-mu[e], sn, acc[m][n][e]), b));
          }
        }
      }
    }
    return;
  }
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int col = wc0 + n * 16 + c;
    if (col >= N) continue;
    const float b = bias[col];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = wr0 + m * 16 + 4 * g + e;
        if (row >= M) continue;
        float v = epi_apply<EPI>(acc[m][n][e] + b);
        if constexpr (EPI == EPI_RESID) v += resid[(int64_t)row * ldr + col];
        out[(int64_t)row * ldo + col] = v;
      }
  }
}

}  // namespace mq
