// Per-anchor score of the detection head, shared by the post-processing kernels (postproc.hip, detect_wide.hip) and by ConvDet's key-writing
// epilogue (conv_wino_vs.hip): both must produce the same bits, so there is one copy of the arithmetic.  Every translation unit
// that includes this is built with -ffp-contract=off and IEEE division (the Makefile's common flags): the expressions mirror the
// fp32 reference op for op.
#pragma once
#include "sqd_common.h"
#include <math.h>

#define SQD_MAX_CLASSES 16

// score / class of one anchor row.  p points at C+5 floats.
__device__ __forceinline__ void anchor_score(const float* __restrict__ p, int C, float& score, int& cls) {
  float l[SQD_MAX_CLASSES];
  float conf_logit;
  if (C == 3) {
    const f32x4 v = *(const f32x4*)p;
    l[0] = v.x; l[1] = v.y; l[2] = v.z; conf_logit = v.w;
  } else {
    for (int c = 0; c < C; ++c) l[c] = p[c];
    conf_logit = p[C];
  }
  float m = l[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, l[c]);
  float sum = 0.f;
  for (int c = 0; c < C; ++c) { l[c] = expf(l[c] - m); sum += l[c]; }
  const float conf = 1.f / (1.f + expf(-conf_logit));
  float best = -1.f; int bc = 0;
  for (int c = 0; c < C; ++c) {
    const float v = (l[c] / sum) * conf;
    if (v > best) { best = v; bc = c; }
  }
  score = best; cls = bc;
}

// Candidate key of a three-class anchor whose (l0, l1, l2, conf_logit) a lane holds in registers: the fp32 score bits (scores are
// >= 0: the bit patterns order like the floats) if score > score_thresh, else 0.  Confidence first, as detect_kernel's phases 1a / 1b:
// score = max_c softmax_c * conf <= conf (softmax_c <= 1 and the product rounds monotonically), so conf <= threshold already decides
// key = 0 -- exactly -- and only the anchors that pass pay for the softmax.
__device__ __forceinline__ unsigned anchor_key3(f32x4 v, float score_thresh) {
  const float conf = 1.f / (1.f + expf(-v.w));
  if (!(conf > score_thresh)) return 0u;
  float s; int c;
  anchor_score((const float*)&v, 3, s, c);
  return (s > score_thresh) ? __float_as_uint(s) : 0u;
}
