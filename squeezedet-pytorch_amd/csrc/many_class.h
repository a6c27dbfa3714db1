// Lane-group access to one anchor row for the many-class head (1 <= C <= 256 classes).
//
// The <= 16-class kernels keep a row's logits in one lane's registers (float l[16]).  Past 16 classes that would need up to 256
// registers per lane, and at C = 80 one lane per 340-byte row is uncoalesced as well.  Here a fixed group of MC_LANES = 16
// consecutive lanes owns a row: lane j holds classes j, j + 16, j + 32, ... in at most MC_REGS = 16 registers, so consecutive lanes
// read consecutive floats, and the row's max / sum / arg-max meet in a fixed xor-shuffle tree inside the group (four steps: 8, 4, 2,
// 1).  The class limit is therefore MC_LANES x MC_REGS = 16 x 16 = 256.
//
// The kernels are instantiated for R = 2, 5, 8, 16 registers per lane (C <= 32, 80, 128, 256); a slot past C holds -inf and adds an
// exact +0 to the sum, and the per-lane order (ascending r) and the tree are the same for every R, so a row's results do not depend
// on the instantiation that computed them.  Every lane of the group ends with the same bits (a + b == b + a, fmaxf likewise).
#pragma once
#include "sqd_common.h"
#include <math.h>

#define MC_LANES 16
#define MC_REGS 16
#define SQD_MANY_MAX_CLASSES (MC_LANES * MC_REGS)      // 16 lanes x 16 registers
#define MC_THREADS 256
#define MC_GROUPS (MC_THREADS / MC_LANES)              // rows in flight per workgroup

// registers per lane for C classes -> instantiate CALL(R) for the smallest of 2, 5, 8, 16 that holds ceil(C / 16)
#define MC_DISPATCH(C, CALL) do { const int r_ = ((C) + MC_LANES - 1) / MC_LANES; \
    if (r_ <= 2) { CALL(2); } else if (r_ <= 5) { CALL(5); } else if (r_ <= 8) { CALL(8); } else { CALL(16); } } while (0)

__device__ __forceinline__ float mc_group_max(float v) {
#pragma unroll
  for (int off = MC_LANES / 2; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, MC_LANES));
  return v;
}

__device__ __forceinline__ float mc_group_sum(float v) {
#pragma unroll
  for (int off = MC_LANES / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, MC_LANES);
  return v;
}

// lane j's slice of the row's class logits (-inf past C) and the row maximum
template <int R>
__device__ __forceinline__ float mc_load_logits(const float* __restrict__ p, int C, int j, float (&l)[R]) {
  float m = -INFINITY;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int c = j + MC_LANES * r;
    l[r] = (c < C) ? p[c] : -INFINITY;
    m = fmaxf(m, l[r]);
  }
  return mc_group_max(m);
}

// e[r] = exp(l[r] - m) (0 past C); returns the row sum
template <int R>
__device__ __forceinline__ float mc_exp_sum(int C, int j, float m, const float (&l)[R], float (&e)[R]) {
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    e[r] = (j + MC_LANES * r < C) ? expf(l[r] - m) : 0.f;
    s += e[r];
  }
  return mc_group_sum(s);
}

// The one scoring routine of the many-class head (dense decode, the detect scoring kernel and the rank-r re-decode all call it, so
// the fused detect agrees with the dense decode bit for bit).  Oracle order: e_c = exp(l_c - max), p_c = e_c / sum,
// v_c = p_c * sigmoid(conf), score = max_c v_c, class = the LOWEST index attaining that maximum (torch's first-max rule, applied to
// the products v_c, not to the logits: two unequal logits can round to the same product).  p: the row's C + 5 floats; j: lane in group.
template <int R>
__device__ __forceinline__ void mc_anchor_score(const float* __restrict__ p, int C, int j, float& score, int& cls) {
  float l[R], e[R];
  const float m = mc_load_logits<R>(p, C, j, l);
  const float sum = mc_exp_sum<R>(C, j, m, l, e);
  const float conf = 1.f / (1.f + expf(-p[C]));
  float best = -1.f; int bc = 0x7fffffff;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int c = j + MC_LANES * r;
    const float v = (e[r] / sum) * conf;
    if (c < C && v > best) { best = v; bc = c; }        // ascending c inside the lane: the first maximum stays
  }
#pragma unroll
  for (int off = MC_LANES / 2; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(best, off, MC_LANES);
    const int oc = __shfl_xor(bc, off, MC_LANES);
    if (ov > best || (ov == best && oc < bc)) { best = ov; bc = oc; }
  }
  score = best; cls = (bc == 0x7fffffff) ? 0 : bc;    // (no v compared greater than -1: a NaN row; class 0 like the narrow kernels)
}
