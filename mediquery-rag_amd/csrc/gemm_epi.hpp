// gemm_epi.hpp - epilogue pieces shared by the encoder GEMMs (encoder.hip) and the
// pre-split split-f32 GEMM (gemm_x6p.hip): the epilogue kinds, the branch-free GELU
// forms, and a wave-tile store of 32x32 MFMA accumulators with bias / GELU / residual.
#pragma once

#include "gemm_f32.hpp"
#include "gemm_x6p.hpp"

namespace mq {

// LayerNorm folded into the split-f32 GEMMs (LnFold, gemm_x6p.hpp; 16x16 store only):
// EPI_RESID_LN_STATS is the producer, out = acc + bias + LN(resid) plus the partials of out;
// the *_LNFOLD kinds are the consumers, out = epi(rho_r (acc - mu_r s[col]) + c[col]) with
// c passed as `bias`.
enum Epi {
  EPI_BIAS = 0,
  EPI_GELU_ERF = 1,
  EPI_GELU_TANH = 2,
  EPI_RESID = 3,
  // 4: retired, never reuse
  EPI_RESID_LN_STATS = 5,
  EPI_BIAS_LNFOLD = 6,
  EPI_GELU_ERF_LNFOLD = 7,
  EPI_GELU_TANH_LNFOLD = 8,
  // L = 32 attention in the QKV epilogue (K2p's 128 x 192 loader-wave tile only, attn_wave_tile
  // below): EPI_BIAS / EPI_BIAS_LNFOLD whose Q, K, V never leave the registers; out is ctx [M, H]
  EPI_ATTN_BIAS = 9,
  EPI_ATTN_LNFOLD = 10
};
constexpr bool epi_is_lnfold(int epi) { return epi >= EPI_BIAS_LNFOLD && epi <= EPI_GELU_TANH_LNFOLD; }
constexpr bool epi_is_attn(int epi) { return epi == EPI_ATTN_BIAS || epi == EPI_ATTN_LNFOLD; }

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

// [M_LO, M_HI): the block rows this call finishes (K2p's split epilogue, gemm_x6p.hip: a wave tile's
// block rows shared out between two waves; the block rows outside the range are not read).  Which
// path a wave tile takes - whole or ragged - is decided on the whole wave tile, and ln_row_own is
// taken over all MB block rows (lane 4 m + e of a row group holds row e of block row m whatever
// the range): a block row's values do not depend on the range it is finished in.
//
// EpiPre / epi_pre_load: what the bias / GELU / fold kinds read from memory besides the
// accumulators - the lane's bias (and s) of each block column, columns clamped to N - 1 (a clamped
// column is never stored), and its row statistics - loaded ahead of time, so that a wave that
// receives its block rows late (the split epilogue's loader wave) has them when the rows arrive.
// With `pre` the store reads none of them itself: the same values, so the same bits.
template <int NB>
struct EpiPre {
  float bv[NB], sv[NB];
  float own_mu = 0.f, own_rho = 0.f;
};
template <int EPI, int MB, int NB>
__device__ __forceinline__ void epi_pre_load(EpiPre<NB>& p, int wr0, int wc0, int M, int N,
                                             const float* __restrict__ bias, const LnFold& lf, int lane) {
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int col = min(wc0 + n * 16 + (lane & 15), N - 1);
    p.bv[n] = bias[col];
    p.sv[n] = epi_is_lnfold(EPI) ? lf.s[col] : 0.f;
  }
  if constexpr (epi_is_lnfold(EPI)) ln_row_own<MB>(lf.stats_in, wr0, M, lf.eps, lane, p.own_mu, p.own_rho);
}
template <int EPI, int MB, int NB, int M_LO = 0, int M_HI = MB, bool PRE = false>
__device__ __forceinline__ void store_wave_tile16(floatx4 (&acc)[MB][NB], int wr0, int wc0, int M, int N,
                                                  const float* __restrict__ bias, const float* __restrict__ resid,
                                                  int ldr, float* __restrict__ out, int ldo, int lane,
                                                  const LnFold& lf = LnFold{}, const EpiPre<NB>* pre = nullptr) {
  static_assert(!PRE || (EPI != EPI_RESID && EPI != EPI_RESID_LN_STATS), "preloads: the kinds without a residual");
  static_assert(0 <= M_LO && M_LO < M_HI && M_HI <= MB, "block-row range");
  static_assert(EPI != EPI_RESID_LN_STATS || (M_LO == 0 && M_HI == MB), "the producer finishes whole wave tiles");
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
  if constexpr (PRE) {
    own_mu = pre->own_mu;
    own_rho = pre->own_rho;
  } else if constexpr (FOLD) {
    ln_row_own<MB>(lf.stats_in, wr0, M, lf.eps, lane, own_mu, own_rho);
  }
  if (wr0 + MB * 16 <= M && wc0 + NB * 16 <= N) {
    float bv[NB], sv[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      if constexpr (PRE)
        bv[n] = pre->bv[n];
      else
        bv[n] = bias[wc0 + n * 16 + c];
    }
    if constexpr (FOLD) {
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        if constexpr (PRE)
          sv[n] = pre->sv[n];
        else
          sv[n] = lf.s[wc0 + n * 16 + c];
      }
    }
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(resid + (EPI == EPI_RESID ? (int64_t)wr0 * ldr + wc0 : 0)), (short)0, 0x7fffffff, 0x00020000);
    const int rl = (4 * g * ldr + c) * 4;
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(out + (int64_t)wr0 * ldo + wc0), (short)0, 0x7fffffff, 0x00020000);
    const int ol = (4 * g * ldo + c) * 4;
#pragma unroll
    for (int m = M_LO; m < M_HI; ++m) {
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
    for (int m = M_LO; m < M_HI; ++m) {
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
          float b, sn;
          if constexpr (PRE) {
            b = pre->bv[n];
            sn = pre->sv[n];
          } else {
            b = bias[col];
            sn = lf.s[col];
          }
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
    float b;
    if constexpr (PRE)
      b = pre->bv[n];
    else
      b = bias[col];
#pragma unroll
    for (int m = M_LO; m < M_HI; ++m)
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

// L = 32 attention as the epilogue of the QKV GEMM (EPI_ATTN_BIAS / EPI_ATTN_LNFOLD; K2p's
// 128 x 192 tile with its W3 column blocks gathered per head, gemm_x6p.hip).  The wave (wm, wn)
// holds, for head `head` and the 64 rows from wr0 - two whole sequences - the 16-column blocks
// n = 0, 1: Q, 2, 3: K, 4, 5: V of head dims 32 wn .. + 31.  Per sequence:
//   1  Q, K, V are finished in the registers exactly as EPI_BIAS / EPI_BIAS_LNFOLD store them,
//      Q times `scale`;
//   2  the Q and K halves (32 x 32) go through the wave's private staging `stg` ([64][kAttnSt]
//      floats, Q rows then K rows) and come back rows-on-lanes: lane (c, g) reads dims 4 g + i
//      and 16 + 4 g + i of row c, step i of the 8-step v_mfma_f32_16x16x4_f32 chain taking
//      k-slot g <-> dim 4 g + i (16 (i >> 2) + 4 g + (i & 3)), the same for Q and K: the partial
//      S^T[key][query] over the wave's 32 head dims, four 16 x 16 blocks;
//   3  both sequences' partials overwrite the staging (the wave's own reads have returned: one
//      wave's LDS operations execute in order), ONE workgroup barrier - which the loader waves
//      execute too - and the partner's (same wm, other wn) partials are added: a + b is
//      commutative, so both waves hold the same bits;
//   4  softmax over keys in registers: the 8 keys 16 kb + 4 g + e of a lane, then the lane
//      groups g by two xor shuffles; masked keys weigh exactly 0, no live key gives l = 0 and
//      ctx exactly 0; expf and o (1 / l) as attention_kernel;
//   5  O[q][d] = sum P V: register e of the S^T block (kb, qb) is operand A (query c, key 16 kb +
//      4 g + e) and register e of V's accumulator block is operand B (the same key, dim c): no
//      data movement.  Rows >= M are not stored.
// Every wave executes the barrier exactly once, whatever M.
// PRE (attn32_kernel, gemm_x6p.hip: the same attention as a launch of its own): acc already
// holds the finished Q, K, V as an unfused QKV launch stored them; only Q's scale is applied.
// Everything after step 1 is this one function: the same bits as the epilogue.
constexpr int kAttnSt = 36;                     // staging row stride in floats (32 + 4)
constexpr int kAttnStage = 64 * kAttnSt * 4;    // bytes of staging per wave (>= the 8 KB of partials)
template <bool FOLD, bool PRE = false>
__device__ __forceinline__ void attn_wave_tile(floatx4 (&acc)[4][6], int wr0, int head, int wn, int M, int H,
                                               const float* __restrict__ bias, const LnFold& lf,
                                               const int* __restrict__ mask, float scale,
                                               float* __restrict__ ctx, int lane, unsigned char* stg,
                                               const unsigned char* partner) {
  static_assert(kAttnStage >= 8 * 1024, "the partials of two sequences fit the staging");
  const int c = lane & 15, g = lane >> 4;
  // key-live bits: bit 32 s + k = key k of sequence s (rows past M: clamped, never stored)
  const unsigned long long kbits = __ballot(mask[min(wr0 + lane, M - 1)] != 0);
  float own_mu = 0.f, own_rho = 0.f;
  if constexpr (FOLD) ln_row_own<4>(lf.stats_in, wr0, M, lf.eps, lane, own_mu, own_rho);
  if constexpr (PRE) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[m][n][e] = acc[m][n][e] * scale;
  } else {
    float bv[6], sv[6];
#pragma unroll
    for (int n = 0; n < 6; ++n) {
      const int col = (n >> 1) * H + 64 * head + 32 * wn + 16 * (n & 1) + c;
      bv[n] = bias[col];
      if constexpr (FOLD) sv[n] = lf.s[col];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float mu = 0.f, rho = 0.f;
        if constexpr (FOLD) {
          mu = ln_row_bcast(own_mu, lane, m, e);
          rho = ln_row_bcast(own_rho, lane, m, e);
        }
#pragma unroll
        for (int n = 0; n < 6; ++n) {
          float v;
          if constexpr (FOLD)
            v = __fmaf_rn(rho, __fmaf_rn(-mu, sv[n], acc[m][n][e]), bv[n]);
          else
            v = acc[m][n][e] + bv[n];
          acc[m][n][e] = n < 2 ? v * scale : v;
        }
      }
  }
  float* sf = reinterpret_cast<float*>(stg);
  floatx4 sp[2][2][2];  // [sequence][key block][query block]
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int t = 0; t < 2; ++t)  // Q rows 0-31, K rows 32-63
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nd = 0; nd < 2; ++nd)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            sf[(32 * t + 16 * mb + 4 * g + e) * kAttnSt + 16 * nd + c] = acc[2 * s + mb][2 * t + nd][e];
    floatx4 qf[2][2], kf[2][2];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        qf[blk][hf] = *reinterpret_cast<const floatx4*>(&sf[(16 * blk + c) * kAttnSt + 16 * hf + 4 * g]);
        kf[blk][hf] = *reinterpret_cast<const floatx4*>(&sf[(32 + 16 * blk + c) * kAttnSt + 16 * hf + 4 * g]);
      }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        floatx4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 8; ++i)
          st = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kb][i >> 2][i & 3], qf[qb][i >> 2][i & 3], st, 0, 0, 0);
        sp[s][kb][qb] = st;
      }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i)
    *reinterpret_cast<floatx4*>(stg + i * 1024 + lane * 16) = sp[i >> 2][(i >> 1) & 1][i & 1];
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // the exchange barrier
#pragma unroll
  for (int i = 0; i < 8; ++i)
    sp[i >> 2][(i >> 1) & 1][i & 1] += *reinterpret_cast<const floatx4*>(partner + i * 1024 + lane * 16);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const unsigned kb32 = (unsigned)(kbits >> (32 * s));
    float inv[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool live = (kb32 >> (16 * kb + 4 * g + e)) & 1u;
          sp[s][kb][qb][e] = live ? sp[s][kb][qb][e] : -INFINITY;
          mx = fmaxf(mx, sp[s][kb][qb][e]);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      float l = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = sp[s][kb][qb][e];
          const float p = v == -INFINITY ? 0.f : expf(v - mx);
          sp[s][kb][qb][e] = p;
          l += p;
        }
      l += __shfl_xor(l, 16);
      l += __shfl_xor(l, 32);
      inv[qb] = l > 0.f ? 1.0f / l : 0.f;  // of query 16 qb + c, in every lane group
    }
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      floatx4 o[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int nd = 0; nd < 2; ++nd)
            o[nd] = __builtin_amdgcn_mfma_f32_16x16x4f32(sp[s][kb][qb][e], acc[2 * s + kb][4 + nd][e], o[nd], 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float iq = __shfl(inv[qb], 4 * g + e);  // of query 16 qb + 4 g + e
        const int row = wr0 + 32 * s + 16 * qb + 4 * g + e;
        if (row < M) {
          float* dst = ctx + (int64_t)row * H + 64 * head + 32 * wn + c;
          dst[0] = o[0][e] * iq;
          dst[16] = o[1][e] * iq;
        }
      }
    }
  }
}

}  // namespace mq
