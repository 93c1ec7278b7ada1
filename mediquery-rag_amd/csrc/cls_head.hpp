// cls_head.hpp - launcher of K13 (cls_head.hip), the cross-encoder head behind the encoder's
// raw CLS tail (mq_encoder_score) and mq_debug_cls_head.
#pragma once

#include <hip/hip_runtime.h>

namespace mq {

// logits [B][n_labels] = Wc tanh(Wp cls_b + bp) + bc for B rows of H = 256 / 512 / 768 / 1024
// floats; one launch on `s`, device buffers, no allocation.  False for another H.
bool launch_cls_head(const float* cls, int B, int H, const float* pooler_w, const float* pooler_b,
                     const float* cls_w, const float* cls_b, int n_labels, float* logits, hipStream_t s);

}  // namespace mq
