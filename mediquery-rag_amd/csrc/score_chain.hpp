// score_chain.hpp - the exact fp32 score of a stored row against a vector held in LDS, as the
// 16-lane row walks compute it (range.hip's range_score_kernel, grouped.hip's
// group_scan_kernel), for the kernels of join.hip that must return those bits.
//
// Lane gl of a row's 16-lane group holds the 16-byte pieces gl, gl + 16, gl + 32, ... of the row
// (coordinates 64 it + 4 gl .. + 3 for it = 0 .. dim / 64 - 1) and multiplies each with the same
// coordinates of the other vector: one FMA chain per lane, it ascending, inside a piece the
// coordinates w, z, y, x in that order; then a butterfly over the 16 lanes (xor 8, 4, 2, 1), after
// which every lane holds the sum.  The order depends on the coordinate index alone and both
// the product and the butterfly's addition commute, so score(a, b) and score(b, a) have the
// same bits.
#pragma once

#include "common.hpp"

namespace mq {

__device__ __forceinline__ float chain_step(float acc, floatx4 v, floatx4 q) {
  return fmaf(v.x, q.x, fmaf(v.y, q.y, fmaf(v.z, q.z, fmaf(v.w, q.w, acc))));
}

__device__ __forceinline__ float chain_reduce16(float acc) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 16);
  return acc;
}

// The score as an order-preserving unsigned (the high word of grouped.hip's group_key: sign
// bit flipped for non-negative scores, every bit inverted for negative ones); never 0 for a
// finite score.
__device__ __forceinline__ unsigned chain_score_word(float score) {
  const unsigned b = __float_as_uint(score);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float chain_word_score(unsigned hi) {
  return __uint_as_float((hi & 0x80000000u) ? (hi ^ 0x80000000u) : ~hi);
}
// group_key: the score word, then the inverted row - descending keys rank (score desc, row asc).
__device__ __forceinline__ unsigned long long chain_key(unsigned word, int64_t row) {
  return ((unsigned long long)word << 32) | (0xFFFFFFFFu - (unsigned)row);
}

}  // namespace mq
