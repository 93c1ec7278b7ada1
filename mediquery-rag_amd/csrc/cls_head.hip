// cls_head.hip - K13: the cross-encoder head (include/mq.h, mq_encoder_score /
// mq_debug_cls_head): logits[b] = Wc tanh(Wp h_b + bp) + bc on the un-normalised CLS states
// h [B][H] the encoder's tail leaves - BertPooler + the classifier of
// BertForSequenceClassification.
//
// One launch.  A workgroup (16 waves) owns a block of 16 rows and computes ALL H pooled values
// of them, so the classifier runs in the same workgroup on the pooled rows it holds in LDS:
//   1. the 16 CLS rows -> LDS, a row per wave (row stride H + 4 floats: a 16-lane ds_read_b128
//      group reads 16 rows at one k, 16 distinct 16-byte bank groups);
//   2. wave w owns the H / 16 pooled columns from w H / 16, as H / 256 tiles of 16.
//      v_mfma_f32_16x16x4_f32, fp32 operands and accumulators: lane (c = l & 15, kq = l >> 4)
//      loads the float4 at k0 + 4 kq of row c of the LDS rows and of row n0 + c of Wp (row-major
//      [out][in]: B^T as it lies in memory), MFMA step t multiplies element t.  Wp is read from
//      memory once per row block - 16 rows share every fragment - and stays in L2 for the other
//      row blocks (2.4 MB at H = 768).  Four waves per SIMD: one wave's weight loads fly under
//      the others' MFMAs (a 16-row block is 16 H^2 MACs whatever B is: 31 us of fp32 MFMA on one
//      CU at H = 768, the kernel's floor for B <= 16);
//   3. each tile sums over four accumulator chains (16-deep k blocks 0, 1, 2, 3 mod 4), added
//      ((a0 + a1) + (a2 + a3)): a quarter of the rounding-error growth of one chain, and
//      independent MFMAs in flight per tile;
//   4. tanhf(acc + bp) overwrites the LDS rows (after a barrier: every wave has read them);
//   5. wave w's row w: for each label a dot product over H - the lane's float4s in order, then
//      the xor-shuffle tree - + bc.
// The summation order is fixed and nothing is accumulated with atomics: repeated calls are
// bit-identical.  Rows past B in the last block read row B - 1 and are never stored.
#include "cls_head.hpp"

#include "common.hpp"

namespace mq {

namespace {

constexpr int kHeadRows = 16;  // rows per workgroup (the MFMA's M)

__device__ __forceinline__ float head_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

constexpr int kHeadWaves = 16;

template <int VPL>
__global__ __launch_bounds__(64 * kHeadWaves) void cls_head_kernel(const float* __restrict__ cls, int B,
                                                                   const float* __restrict__ Wp,
                                                                   const float* __restrict__ bp,
                                                                   const float* __restrict__ Wc,
                                                                   const float* __restrict__ bc, int n_labels,
                                                                   float* __restrict__ logits) {
  constexpr int H = VPL * 256;
  constexpr int AS = H + 4;
  static_assert(kHeadRows == kHeadWaves, "a row per wave");
  __shared__ __attribute__((aligned(16))) float rows[kHeadRows * AS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, kq = lane >> 4;
  const int r0 = blockIdx.x * kHeadRows;
  // 1. wave w stages row w
  {
    const float* src = cls + (int64_t)min(r0 + wave, B - 1) * H;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int cc = (i * 64 + lane) * 4;
      *reinterpret_cast<floatx4*>(&rows[wave * AS + cc]) = *reinterpret_cast<const floatx4*>(src + cc);
    }
  }
  __syncthreads();
  // 2./3. pooled pre-activations of this wave's VPL 16-column tiles
  const int wn0 = wave * (H / kHeadWaves);
  floatx4 acc[VPL][4];  // [tile][chain]
#pragma unroll
  for (int p = 0; p < VPL; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = floatx4{0.f, 0.f, 0.f, 0.f};
  const float* arow = &rows[c * AS + 4 * kq];
  const float* wrow = Wp + (int64_t)(wn0 + c) * H + 4 * kq;  // tile p: + 16 p rows
#pragma unroll 1
  for (int k0 = 0; k0 < H; k0 += 64) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // chains 2 h, 2 h + 1: 2 VPL weight fragments in flight
      floatx4 av[2], wv[VPL][2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        av[q] = *reinterpret_cast<const floatx4*>(arow + k0 + 16 * (2 * h + q));
#pragma unroll
        for (int p = 0; p < VPL; ++p)
          wv[p][q] = *reinterpret_cast<const floatx4*>(wrow + (int64_t)16 * p * H + k0 + 16 * (2 * h + q));
      }
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int p = 0; p < VPL; ++p)
            acc[p][2 * h + q] =
                __builtin_amdgcn_mfma_f32_16x16x4f32(av[q][t], wv[p][q][t], acc[p][2 * h + q], 0, 0, 0);
    }
  }
  __syncthreads();  // every wave has read the CLS rows: the pooled rows take their place
  // 4. accumulator element e of tile p is (row 4 kq + e, column wn0 + 16 p + c)
#pragma unroll
  for (int p = 0; p < VPL; ++p) {
    const floatx4 pre = (acc[p][0] + acc[p][1]) + (acc[p][2] + acc[p][3]);
    const int col = wn0 + p * 16 + c;
    const float bias = bp[col];
#pragma unroll
    for (int e = 0; e < 4; ++e) rows[(4 * kq + e) * AS + col] = tanhf(pre[e] + bias);
  }
  __syncthreads();
  // 5. the classifier on row w
  if (r0 + wave >= B) return;  // (wave-uniform, past the last barrier)
  for (int lab = 0; lab < n_labels; ++lab) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int cc = (i * 64 + lane) * 4;
      const floatx4 x = *reinterpret_cast<const floatx4*>(&rows[wave * AS + cc]);
      const floatx4 w = *reinterpret_cast<const floatx4*>(Wc + (int64_t)lab * H + cc);
      s += (x.x * w.x + x.y * w.y) + (x.z * w.z + x.w * w.w);
    }
    s = head_wave_sum(s);
    if (lane == 0) logits[(int64_t)(r0 + wave) * n_labels + lab] = s + bc[lab];
  }
}

}  // namespace

bool launch_cls_head(const float* cls, int B, int H, const float* pooler_w, const float* pooler_b,
                     const float* cls_w, const float* cls_b, int n_labels, float* logits, hipStream_t s) {
  const dim3 grid((unsigned)((B + kHeadRows - 1) / kHeadRows));
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(64 * kHeadWaves), 0, s, cls, B, pooler_w, pooler_b, cls_w, cls_b, n_labels, logits);
  };
  switch (H) {
    case 256: go(cls_head_kernel<1>); return true;
    case 512: go(cls_head_kernel<2>); return true;
    case 768: go(cls_head_kernel<3>); return true;
    case 1024: go(cls_head_kernel<4>); return true;
    default: return false;
  }
}

}  // namespace mq

extern "C" int mq_debug_cls_head(const float* cls, int B, int H, const float* pooler_w, const float* pooler_b,
                                 const float* cls_w, const float* cls_b, int n_labels, float* logits, void* stream) {
  mq::clear_error();
  MQ_CHECK_ARG(B >= 0 && (H == 256 || H == 512 || H == 768 || H == 1024), "bad head shape B=%d H=%d", B, H);
  MQ_CHECK_ARG(n_labels >= 1 && n_labels <= MQ_HEAD_MAX_LABELS, "n_labels must be in [1, %d] (got %d)",
               MQ_HEAD_MAX_LABELS, n_labels);
  if (B == 0) return MQ_OK;
  MQ_CHECK_ARG(cls && pooler_w && pooler_b && cls_w && cls_b && logits, "NULL buffer");
  mq::launch_cls_head(cls, B, H, pooler_w, pooler_b, cls_w, cls_b, n_labels, logits, (hipStream_t)stream);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}
