// Multi-task detection loss, forward and analytic backward.
//
// Reference: Loss.forward src/model/squeezedet.py:133-174, compute_overlaps src/model/modules.py:48-63,
// PredictionResolver (log_softmax branch) src/model/squeezedet.py:109-120, deltas_to_boxes
// src/model/modules.py:27-45.  The reference runs ~40 elementwise/reduction launches forward and an
// autograd graph backward; here: one reduction kernel (+ a tiny finalise) forward, one elementwise
// kernel backward.
//
//   class  = sum_a  w_c * mask * sum_c onehot_c * (-log_softmax_c)        / n_obj
//   pos    = sum_a  w_p * mask     * (iou - sigmoid(conf))^2              / n_obj
//   neg    = sum_a  w_n * (1-mask) * (iou - sigmoid(conf))^2              / (A - n_obj)
//   bbox   = sum_a  w_b * mask * sum_j (delta_j - gt_delta_j)^2           / n_obj
//   iou    = IoU(gt_box, decode(delta)) * mask, IoU = inter / (union + 1e-10)   -- NOT detached:
// the positive-score term back-propagates through iou -> predicted box -> clamp -> exp -> deltas
// (SURVEY.md section 8a row L).  All per-image ([B] vectors); n_obj = 0 gives NaN like the reference.
//
// LossBoxArgs::box (SQD_BOX_IOU .. SQD_BOX_CIOU, the sqd_loss_box_* entries) replaces the bbox term by an IoU-family regression on the
// same operands as the confidence target, gt columns 5..8 unread:
//   bbox   = sum_a  w_b * [mask != 0] * (1 - q)                           / n_obj
//   iou : q = iou          giou: q = iou - (cw*ch - union) / (cw*ch + eps)          diou: q = iou - rho2 / (cw^2 + ch^2 + eps)
//   ciou: q = diou's - alpha * v,  v = 4/pi^2 (atan(gw / (gh + eps)) - atan(pw / (ph + eps)))^2,  alpha = v / (1 - iou + v + eps)
// (cw, ch: the enclosing box; rho2: the squared centre distance; alpha: a constant in the backward).  Both the value and the gradient
// are float64 work on the rows with a box only (box_loss_value, the positive-row branch of anchor_geom_grad_nneg); the BOX = false
// instantiations of every kernel are the L2 code as it was.  'iou' has no box gradient where the boxes are disjoint.
#include "sqd_common.h"
#include "many_class.h"
#include <math.h>

#define LOSS_MAX_CLASSES 16
#define LOSS_NPART 16          // partial-sum blocks per image (deterministic two-stage reduction)
#define LOSS_THREADS 256
#define LOSS_EPS 1e-10f
// the box regression kinds (include/sqd_hip.h)
#define SQD_BOX_L2 0
#define SQD_BOX_IOU 1
#define SQD_BOX_GIOU 2
#define SQD_BOX_DIOU 3
#define SQD_BOX_CIOU 4

struct LossArgs {
  const float* pred; const float* gt; const float* anchors;
  int B, A, C;
  float wmax, hmax;
  float w_class, w_pos, w_neg, w_bbox;
};
struct LossBoxArgs : LossArgs { int box; };      // + SQD_BOX_*: what the loss_box_* kernels take (the L2 kernels keep LossArgs)

struct AnchorGeom {           // the class-independent part: confidence, box decode, IoU, delta regression
  float mask, conf, iou_raw, e;          // e = iou*mask - conf
  float bb;                              // sum_j (delta_j - gt_j)^2; BOX: [mask != 0] * (1 - q)
  // box decode intermediates for the backward
  float w, h, ax, ay, aw, ah;
  float x1u, y1u, x2u, y2u;              // unclamped
  float px1, py1, px2, py2;              // clamped
  float gx1, gy1, gx2, gy2;
  float lr_raw, tb_raw, inter, uni;
};

struct AnchorTerms : AnchorGeom {        // everything both passes need about one anchor
  float ce;                              // sum_c onehot_c * (-logp_c)
  float prob[LOSS_MAX_CLASSES];
  float onehot_sum;
};

// ---- IoU-family box regression: float64, rows with a box only -------------------------------------------------------------------------
// The clamped predicted box, the gt box and their IoU pieces in float64 (den = uni + eps).
struct Box64 {
  double px1, py1, px2, py2, gx1, gy1, gx2, gy2;
  double lr_raw, tb_raw, lr, tb, inter, uni, den;
};

// sub-gradients of minimum / maximum toward `mine`: ties split evenly (torch.minimum / maximum backward)
__device__ __forceinline__ double tie_min(double mine, double other) { return mine < other ? 1.0 : (mine == other ? 0.5 : 0.0); }
__device__ __forceinline__ double tie_max(double mine, double other) { return mine > other ? 1.0 : (mine == other ? 0.5 : 0.0); }

// pen = iou - q of kind `box`; GRAD: dp = d pen / d (px1, py1, px2, py2), before the clamp rule.  The enclosing box's max / min compare
// the pairs the intersection's min / max compare, with the same tie rule; alpha is a constant of the derivative.
template <bool GRAD>
__device__ __forceinline__ double box_penalty(int box, const Box64& b, double (&dp)[4]) {
  if (GRAD) dp[0] = dp[1] = dp[2] = dp[3] = 0.0;
  if (box == SQD_BOX_IOU) return 0.0;
  const double eps = (double)LOSS_EPS;
  const double pw = b.px2 - b.px1, ph = b.py2 - b.py1;
  const double cw = fmax(b.gx2, b.px2) - fmin(b.gx1, b.px1), ch = fmax(b.gy2, b.py2) - fmin(b.gy1, b.py1);
  // d cw / d (px1, px2), d ch / d (py1, py2)
  const double cx1 = -tie_min(b.px1, b.gx1), cx2 = tie_max(b.px2, b.gx2), cy1 = -tie_min(b.py1, b.gy1), cy2 = tie_max(b.py2, b.gy2);
  if (box == SQD_BOX_GIOU) {
    const double ce = cw * ch + eps;
    if (GRAD) {
      const double dix = b.lr_raw >= 0.0 ? b.tb : 0.0, diy = b.tb_raw >= 0.0 ? b.lr : 0.0;       // d inter / d (lr_raw, tb_raw)
      const double du[4] = {-ph + dix * tie_max(b.px1, b.gx1), -pw + diy * tie_max(b.py1, b.gy1),
                            ph - dix * tie_min(b.px2, b.gx2), pw - diy * tie_min(b.py2, b.gy2)};   // d uni
      const double dc[4] = {ch * cx1, cw * cy1, ch * cx2, cw * cy2};                                 // d (cw * ch)
      const double k1 = b.den / (ce * ce), k2 = 1.0 / ce;
      for (int j = 0; j < 4; ++j) dp[j] = dc[j] * k1 - du[j] * k2;
    }
    return (cw * ch - b.uni) / ce;
  }
  const double sx = b.gx1 + b.gx2 - b.px1 - b.px2, sy = b.gy1 + b.gy2 - b.py1 - b.py2;
  const double rho2 = (sx * sx + sy * sy) * 0.25, c2e = cw * cw + ch * ch + eps;
  double pen = rho2 / c2e;
  if (GRAD) {
    const double k1 = 1.0 / c2e, k2 = 2.0 * rho2 / (c2e * c2e);
    dp[0] = -0.5 * sx * k1 - cw * cx1 * k2; dp[1] = -0.5 * sy * k1 - ch * cy1 * k2;
    dp[2] = -0.5 * sx * k1 - cw * cx2 * k2; dp[3] = -0.5 * sy * k1 - ch * cy2 * k2;
  }
  if (box == SQD_BOX_CIOU) {
    const double c4pi2 = 4.0 / (M_PI * M_PI);
    const double hp = ph + eps, rp = pw / hp;
    const double da = atan((b.gx2 - b.gx1) / (b.gy2 - b.gy1 + eps)) - atan(rp);
    const double v = c4pi2 * da * da;
    const double alpha = v / (1.0 - b.inter / b.den + v + eps);
    pen += alpha * v;
    if (GRAD) {
      const double dpw = alpha * (-2.0 * c4pi2 * da) / ((1.0 + rp * rp) * hp), dph = -dpw * rp;     // alpha * d v / d (pw, ph)
      dp[0] -= dpw; dp[2] += dpw; dp[1] -= dph; dp[3] += dph;
    }
  }
  return pen;
}

// [mask != 0] * (1 - q) of a row with a box: the decode and the IoU again in float64 from the row's own operands, rounded once.
__device__ __forceinline__ float box_loss_value(const LossBoxArgs& a, const float* __restrict__ d, float ax, float ay, float aw_, float ah_,
                                                float gx1, float gy1, float gx2, float gy2) {
  const double aw = aw_, ah = ah_, wmax = a.wmax, hmax = a.hmax;
  const double cx = (double)ax + aw * (double)d[0], cy = (double)ay + ah * (double)d[1];
  const double w = aw * exp((double)d[2]), h = ah * exp((double)d[3]);
  Box64 b;
  b.px1 = fmin(fmax(cx - 0.5 * (w - 1.0), 0.0), wmax); b.py1 = fmin(fmax(cy - 0.5 * (h - 1.0), 0.0), hmax);
  b.px2 = fmin(fmax(cx + 0.5 * (w - 1.0), 0.0), wmax); b.py2 = fmin(fmax(cy + 0.5 * (h - 1.0), 0.0), hmax);
  b.gx1 = gx1; b.gy1 = gy1; b.gx2 = gx2; b.gy2 = gy2;
  b.lr_raw = fmin(b.gx2, b.px2) - fmax(b.gx1, b.px1); b.tb_raw = fmin(b.gy2, b.py2) - fmax(b.gy1, b.py1);
  b.lr = fmax(b.lr_raw, 0.0); b.tb = fmax(b.tb_raw, 0.0);
  b.inter = b.lr * b.tb;
  b.uni = (b.gx2 - b.gx1) * (b.gy2 - b.gy1) + (b.px2 - b.px1) * (b.py2 - b.py1) - b.inter;
  b.den = b.uni + (double)LOSS_EPS;
  double unused[4];
  return (float)(1.0 - (b.inter / b.den - box_penalty<false>(a.box, b, unused)));
}

// p: the row's C + 5 floats, g: its C + 9 ground-truth floats.  Shared by the <= 16-class and the many-class kernels.
template <bool BOX = false, class Args>
__device__ __forceinline__ void anchor_geom(const Args& a, const float* __restrict__ p, const float* __restrict__ g,
                                            const float* __restrict__ anc, AnchorGeom& t) {
  const int C = a.C;
  t.mask = g[0];
  t.gx1 = g[1]; t.gy1 = g[2]; t.gx2 = g[3]; t.gy2 = g[4];
  t.conf = 1.f / (1.f + expf(-p[C]));
  // box decode (deltas_to_boxes)
  const float* d = p + C + 1;
  const float ax = anc[0], ay = anc[1];
  t.ax = ax; t.ay = ay; t.aw = anc[2]; t.ah = anc[3];
  const float cx = ax + t.aw * d[0], cy = ay + t.ah * d[1];
  t.w = t.aw * expf(d[2]); t.h = t.ah * expf(d[3]);
  t.x1u = cx - 0.5f * (t.w - 1.f); t.y1u = cy - 0.5f * (t.h - 1.f);
  t.x2u = cx + 0.5f * (t.w - 1.f); t.y2u = cy + 0.5f * (t.h - 1.f);
  t.px1 = fminf(fmaxf(t.x1u, 0.f), a.wmax); t.py1 = fminf(fmaxf(t.y1u, 0.f), a.hmax);
  t.px2 = fminf(fmaxf(t.x2u, 0.f), a.wmax); t.py2 = fminf(fmaxf(t.y2u, 0.f), a.hmax);
  // IoU(gt, pred)
  t.lr_raw = fminf(t.gx2, t.px2) - fmaxf(t.gx1, t.px1);
  t.tb_raw = fminf(t.gy2, t.py2) - fmaxf(t.gy1, t.py1);
  const float lr = fmaxf(t.lr_raw, 0.f), tb = fmaxf(t.tb_raw, 0.f);
  t.inter = lr * tb;
  t.uni = (t.gx2 - t.gx1) * (t.gy2 - t.gy1) + (t.px2 - t.px1) * (t.py2 - t.py1) - t.inter;
  t.iou_raw = t.inter / (t.uni + LOSS_EPS);
  t.e = t.iou_raw * t.mask - t.conf;
  if constexpr (BOX) {
    t.bb = t.mask != 0.f ? box_loss_value(a, d, ax, ay, t.aw, t.ah, t.gx1, t.gy1, t.gx2, t.gy2) : 0.f;
  } else {
    float bb = 0.f;
    for (int j = 0; j < 4; ++j) { const float df = d[j] - g[5 + j]; bb += df * df; }
    t.bb = bb;
  }
}

template <bool BOX = false, class Args>
__device__ __forceinline__ void anchor_terms(const Args& a, const float* __restrict__ p, const float* __restrict__ g,
                                             const float* __restrict__ anc, AnchorTerms& t) {
  const int C = a.C;
  // log-softmax over the class logits
  float m = p[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, p[c]);
  float sum = 0.f;
  for (int c = 0; c < C; ++c) { t.prob[c] = expf(p[c] - m); sum += t.prob[c]; }
  const float lse = logf(sum);
  float ce = 0.f, ohs = 0.f;
  for (int c = 0; c < C; ++c) {
    const float oh = g[9 + c];
    ce += oh * (-((p[c] - m) - lse));
    ohs += oh;
    t.prob[c] = t.prob[c] / sum;
  }
  t.ce = ce; t.onehot_sum = ohs;
  anchor_geom<BOX>(a, p, g, anc, t);
}

// The anchors [lo, hi) of an image that block blk of LOSS_NPART sums.
__device__ __forceinline__ void loss_slice(int A, int blk, int& lo, int& hi) {
  const int per = (A + LOSS_NPART - 1) / LOSS_NPART;
  lo = blk * per;
  hi = min(A, lo + per);
}

// The first stage of every forward: each thread's NS sums meet in a fixed order (wave shuffle tree, then the waves one after the
// other), so the same operands give the same bits; partial[b][blk][NS] is what the finalize kernels add up.
template <int NS, int THREADS>
__device__ __forceinline__ void block_reduce_store(const float (&s)[NS], float* partial, int b, int blk) {
  __shared__ float red[NS][THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    float v = s[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0) red[k][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    float v = 0.f;
    for (int w = 0; w < THREADS / 64; ++w) v += red[threadIdx.x][w];
    partial[((long long)b * LOSS_NPART + blk) * NS + threadIdx.x] = v;
  }
}

// partial[b][blk][5] = (n_obj, S_class, S_pos, S_neg, S_bbox) over the block's anchors.  Every kernel below is a body with a BOX
// parameter and two entries: the L2 kernel under the name it always had, and its loss_box_* twin.
template <bool BOX, class Args>
__device__ __forceinline__ void loss_partial_body(const Args a, float* __restrict__ partial) {
  const int b = blockIdx.y, blk = blockIdx.x;
  int lo, hi;
  loss_slice(a.A, blk, lo, hi);
  float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = lo + threadIdx.x; i < hi; i += LOSS_THREADS) {
    const long long row = (long long)b * a.A + i;
    AnchorTerms t;
    anchor_terms<BOX>(a, a.pred + row * (a.C + 5), a.gt + row * (a.C + 9), a.anchors + 4 * i, t);
    s[0] += t.mask;
    s[1] += t.mask * t.ce;
    s[2] += t.mask * (t.e * t.e);
    s[3] += (1.f - t.mask) * (t.e * t.e);
    s[4] += BOX ? t.bb : t.mask * t.bb;
  }
  block_reduce_store<5, LOSS_THREADS>(s, partial, b, blk);
}

__global__ __launch_bounds__(LOSS_THREADS) void loss_partial_kernel(LossArgs a, float* __restrict__ partial) {
  loss_partial_body<false>(a, partial);
}
__global__ __launch_bounds__(LOSS_THREADS) void loss_box_partial_kernel(LossBoxArgs a, float* __restrict__ partial) {
  loss_partial_body<true>(a, partial);
}

// The second stage, one image: its LOSS_NPART partials -> v = (class, score = pos+neg, bbox, total) and the counts the backward
// takes.  PlainImage: n_obj = 0 gives NaN like the reference.
struct PlainImage {
  static __device__ __forceinline__ void losses(const float* partial, int b, int A, float w_class, float w_pos, float w_neg,
                                                float w_bbox, float (&v)[4], float& n, float&) {
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < LOSS_NPART; ++k)
      for (int j = 0; j < 5; ++j) s[j] += partial[((long long)b * LOSS_NPART + k) * 5 + j];
    n = s[0];
    const float cls = w_class * s[1] / n, pos = w_pos * s[2] / n, neg = w_neg * s[3] / ((float)A - n), bbx = w_bbox * s[4] / n;
    v[0] = cls; v[1] = pos + neg; v[2] = bbx; v[3] = cls + pos + neg + bbx;     // same association as the reference (:166)
  }
  static __device__ __forceinline__ void store_counts(float* nobj, int, int b, float n, float) { nobj[b] = n; }      // nobj [B]
};

// MaskedImage: partial [B][LOSS_NPART][6] with n_neg = A - n_obj - n_ign and the zero-denominator conventions: class, pos and bbox
// are 0 where n_obj = 0, neg is 0 where n_neg = 0.  With n_ign = 0 and n_obj > 0 every operation is PlainImage's, in its order: the
// same bits.
struct MaskedImage {
  static __device__ __forceinline__ void losses(const float* partial, int b, int A, float w_class, float w_pos, float w_neg,
                                                float w_bbox, float (&v)[4], float& n, float& nneg) {
    float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < LOSS_NPART; ++k)
      for (int j = 0; j < 6; ++j) s[j] += partial[((long long)b * LOSS_NPART + k) * 6 + j];
    n = s[0];
    nneg = (float)A - n - s[5];
    const float cls = n > 0.f ? w_class * s[1] / n : 0.f, pos = n > 0.f ? w_pos * s[2] / n : 0.f;
    const float neg = nneg > 0.f ? w_neg * s[3] / nneg : 0.f, bbx = n > 0.f ? w_bbox * s[4] / n : 0.f;
    v[0] = cls; v[1] = pos + neg; v[2] = bbx; v[3] = cls + pos + neg + bbx;
  }
  static __device__ __forceinline__ void store_counts(float* counts, int B, int b, float n, float nneg) {       // counts [2][B]
    counts[b] = n; counts[B + b] = nneg;
  }
};

// losses[4][B] and the image rule's counts.  mean4 (or null): the four batch means, loss.mean() of src/engine/trainer.py:43 without
// a torch reduction kernel -- ONE block then walks the images (thread t takes b = t, t + 64, ...: a fixed order) and the 64 partial
// sums meet in a fixed shuffle tree.  Without mean4: one thread per image.  Both forms run the same per-image body, so the plain and
// the mean forward give the same per-image bits.
template <class Image>
__device__ __forceinline__ void finalize_walk(const float* partial, float* losses, float* counts, int B, int A, float w_class,
                                              float w_pos, float w_neg, float w_bbox, float* mean4) {
  if (mean4) {
    float m[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = threadIdx.x; b < B; b += 64) {
      float v[4], n, nneg;
      Image::losses(partial, b, A, w_class, w_pos, w_neg, w_bbox, v, n, nneg);
      for (int j = 0; j < 4; ++j) { losses[j * B + b] = v[j]; m[j] += v[j]; }
      Image::store_counts(counts, B, b, n, nneg);
    }
    for (int j = 0; j < 4; ++j) {
      float v = m[j];
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
      if (threadIdx.x == 0) mean4[j] = v / (float)B;
    }
    return;
  }
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float v[4], n, nneg;
  Image::losses(partial, b, A, w_class, w_pos, w_neg, w_bbox, v, n, nneg);
  for (int j = 0; j < 4; ++j) losses[j * B + b] = v[j];
  Image::store_counts(counts, B, b, n, nneg);
}

__global__ void loss_finalize_kernel(const float* __restrict__ partial, float* __restrict__ losses, float* __restrict__ nobj,
                                     int B, int A, float w_class, float w_pos, float w_neg, float w_bbox, float* __restrict__ mean4) {
  finalize_walk<PlainImage>(partial, losses, nobj, B, A, w_class, w_pos, w_neg, w_bbox, mean4);
}

// upstream gradients of image b's (class, score, bbox): per image and component (coef [3][B]), or (gmean: d / d mean(total)) the
// same gmean[0] / B for all
struct Upstream { float uc, us, ub; };
__device__ __forceinline__ Upstream upstream_grads(const LossArgs& a, const float* coef, const float* gmean, int b) {
  const float gm = gmean ? gmean[0] / (float)a.B : 0.f;
  return {gmean ? gm : coef[0 * a.B + b], gmean ? gm : coef[1 * a.B + b], gmean ? gm : coef[2 * a.B + b]};
}

// d loss / d (conf logit, 4 deltas) of one anchor: the score terms incl. the un-detached IoU path, and the delta regression.
// us / ub: upstream gradients of the image's score and bbox components; n = n_obj.  Shared by both backward kernels.
// nneg: the denominator of the negative score term, A - n_obj (the masked launches: a count that left the ignored anchors out).
// BOX: the delta regression is gone; a row with a box always takes the float64 branch, where the box term adds kq = -ub * w_b / n
// to d / d iou and -kq * d pen to the clamped box's gradient, ahead of the clamp rule.
template <bool BOX = false, class Args>
__device__ __forceinline__ void anchor_geom_grad_nneg(const Args& a, const AnchorGeom& t, const float* __restrict__ d,
                                                      const float* __restrict__ g, float n, float nneg, float us, float ub,
                                                      float (&out)[5]) {
  // score terms: k*(iou*mask - conf)^2, k = w_p*mask/n + w_n*(1-mask)/(A-n)
  const float k = us * (a.w_pos * t.mask / n + a.w_neg * (1.f - t.mask) / nneg);
  const float dL_de = 2.f * k * t.e;
  out[0] = -dL_de * t.conf * (1.f - t.conf);
  // IoU path: d e / d iou_raw = mask.  Only the rows with a box take it (about 0.1 % of a batch), and there the gradient is a
  // difference of two products of areas that cancel about 3:1 for a well-fitting box: every float32 evaluation of it lands a few ulp
  // to either side.  Those rows redo the decode and the IoU in float64 from the row's own operands and round once at the end; the
  // branch rules are the forward's (clamp passes inclusively, min / max ties split, clamp_min passes at 0).
  const float dL_dov = dL_de * t.mask;
  if (dL_dov != 0.f || (BOX && t.mask != 0.f)) {
    const double aw = t.aw, ah = t.ah, wmax = a.wmax, hmax = a.hmax;
    const double cx = (double)t.ax + aw * (double)d[0], cy = (double)t.ay + ah * (double)d[1];
    const double w = aw * exp((double)d[2]), h = ah * exp((double)d[3]);
    const double x1u = cx - 0.5 * (w - 1.0), y1u = cy - 0.5 * (h - 1.0), x2u = cx + 0.5 * (w - 1.0), y2u = cy + 0.5 * (h - 1.0);
    const double px1 = fmin(fmax(x1u, 0.0), wmax), py1 = fmin(fmax(y1u, 0.0), hmax);
    const double px2 = fmin(fmax(x2u, 0.0), wmax), py2 = fmin(fmax(y2u, 0.0), hmax);
    const double gx1 = t.gx1, gy1 = t.gy1, gx2 = t.gx2, gy2 = t.gy2;
    const double lr_raw = fmin(gx2, px2) - fmax(gx1, px1), tb_raw = fmin(gy2, py2) - fmax(gy1, py1);
    const double lr = fmax(lr_raw, 0.0), tb = fmax(tb_raw, 0.0);
    const double inter = lr * tb;
    const double den = (gx2 - gx1) * (gy2 - gy1) + (px2 - px1) * (py2 - py1) - inter + (double)LOSS_EPS;
    const double e = inter / den * (double)t.mask - (double)t.conf;
    double dov = 2.0 * (double)k * e * (double)t.mask;
    double kq = 0.0;
    if constexpr (BOX) {
      if (t.mask != 0.f) { kq = -(double)ub * (double)a.w_bbox / (double)n; dov += kq; }
    }
    const double dov_dinter = 1.0 / den + inter / (den * den);      // union contains -inter
    const double dov_dap = -inter / (den * den);                    // pred-box area
    const double dlr = (lr_raw >= 0.0) ? dov * dov_dinter * tb : 0.0;
    const double dtb = (tb_raw >= 0.0) ? dov * dov_dinter * lr : 0.0;
    // min/max sub-gradients: ties split evenly (torch.minimum/maximum backward)
    auto wmin = [](double mine, double other) { return tie_min(mine, other); };
    auto wmaxf = [](double mine, double other) { return tie_max(mine, other); };
    const double pw = px2 - px1, ph = py2 - py1;
    const double dap = dov * dov_dap;
    double dpx2 = dlr * wmin(px2, gx2) + dap * ph;
    double dpx1 = -dlr * wmaxf(px1, gx1) - dap * ph;
    double dpy2 = dtb * wmin(py2, gy2) + dap * pw;
    double dpy1 = -dtb * wmaxf(py1, gy1) - dap * pw;
    if constexpr (BOX) {
      if (kq != 0.0 && a.box != SQD_BOX_IOU) {
        const Box64 bx = {px1, py1, px2, py2, gx1, gy1, gx2, gy2, lr_raw, tb_raw, lr, tb, inter, den - (double)LOSS_EPS, den};
        double dpen[4];
        box_penalty<true>(a.box, bx, dpen);
        dpx1 -= kq * dpen[0]; dpy1 -= kq * dpen[1]; dpx2 -= kq * dpen[2]; dpy2 -= kq * dpen[3];
      }
    }
    // clamp backward: passes where the unclamped value is inside [0, max] (inclusive)
    if (!(x1u >= 0.0 && x1u <= wmax)) dpx1 = 0.0;
    if (!(x2u >= 0.0 && x2u <= wmax)) dpx2 = 0.0;
    if (!(y1u >= 0.0 && y1u <= hmax)) dpy1 = 0.0;
    if (!(y2u >= 0.0 && y2u <= hmax)) dpy2 = 0.0;
    const double gd[4] = {(dpx1 + dpx2) * aw,                    // d x{1,2}u / d dx = aw
                          (dpy1 + dpy2) * ah,
                          (dpx2 - dpx1) * 0.5 * w,               // d x2u/d dw = +w/2, d x1u/d dw = -w/2
                          (dpy2 - dpy1) * 0.5 * h};
    if constexpr (BOX) {
      for (int j = 0; j < 4; ++j) out[1 + j] = (float)gd[j];
    } else {
      const double kb = (double)ub * (double)a.w_bbox * (double)t.mask / (double)n * 2.0;
      for (int j = 0; j < 4; ++j) out[1 + j] = (float)(gd[j] + kb * ((double)d[j] - (double)g[5 + j]));
    }
    return;
  }
  if constexpr (BOX) {
    for (int j = 0; j < 4; ++j) out[1 + j] = 0.f;
    return;
  }
  const float kb = ub * a.w_bbox * t.mask / n * 2.f;
  for (int j = 0; j < 4; ++j) out[1 + j] = 0.f + kb * (d[j] - g[5 + j]);      // (0.f +: a row without a box never holds -0)
}

template <bool BOX = false, class Args>
__device__ __forceinline__ void anchor_geom_grad(const Args& a, const AnchorGeom& t, const float* __restrict__ d,
                                                 const float* __restrict__ g, float n, float us, float ub, float (&out)[5]) {
  anchor_geom_grad_nneg<BOX>(a, t, d, g, n, (float)a.A - n, us, ub, out);
}

// dpred[b][a][:] = u_class[b]*d(class_b) + u_score[b]*d(score_b) + u_bbox[b]*d(bbox_b), coef[3][B]
template <bool BOX, class Args>
__device__ __forceinline__ void loss_bwd_body(const Args a, const float* __restrict__ nobj, const float* __restrict__ coef,
                                              float* __restrict__ dpred, const float* __restrict__ gmean) {
  const long long total = (long long)a.B * a.A;
  const int C = a.C;
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < total; row += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(row / a.A), i = (int)(row - (long long)b * a.A);
    const float* p = a.pred + row * (C + 5);
    const float* g = a.gt + row * (C + 9);
    AnchorTerms t;
    anchor_terms<BOX>(a, p, g, a.anchors + 4 * i, t);
    const float n = nobj[b];
    const Upstream u = upstream_grads(a, coef, gmean, b);
    const float uc = u.uc, us = u.us, ub = u.ub;
    float* o = dpred + row * (C + 5);
    // class logits: w_c*mask/n * (sum(onehot)*softmax_j - onehot_j)
    const float kc = uc * a.w_class * t.mask / n;
    for (int c = 0; c < C; ++c) o[c] = kc * (t.onehot_sum * t.prob[c] - g[9 + c]);
    float og[5];
    anchor_geom_grad<BOX>(a, t, p + C + 1, g, n, us, ub, og);
    for (int j = 0; j < 5; ++j) o[C + j] = og[j];
  }
}

__global__ __launch_bounds__(LOSS_THREADS) void loss_bwd_kernel(LossArgs a, const float* __restrict__ nobj,
                                                                const float* __restrict__ coef, float* __restrict__ dpred,
                                                                const float* __restrict__ gmean) {
  loss_bwd_body<false>(a, nobj, coef, dpred, gmean);
}
__global__ __launch_bounds__(LOSS_THREADS) void loss_box_bwd_kernel(LossBoxArgs a, const float* __restrict__ nobj,
                                                                    const float* __restrict__ coef, float* __restrict__ dpred,
                                                                    const float* __restrict__ gmean) {
  loss_bwd_body<true>(a, nobj, coef, dpred, gmean);
}

// ---- many-class loss: 1 <= num_classes <= 256 = 16 lanes x 16 registers (many_class.h) ------------------------------------------------
// The same four launches with a 16-lane group per anchor row.  The class terms (log-softmax, cross entropy, softmax for the backward)
// are spread over the group and meet in its fixed shuffle tree; the class-independent chain (anchor_geom / anchor_geom_grad) is the
// <= 16-class kernels' own, evaluated by every lane of the group (16 lanes issue it at the cost of one) and taken from lane 0.  The
// partial sums keep the two-stage reduction over LOSS_NPART blocks per image and share loss_finalize_kernel, so a result does not
// change from run to run and the plain and the mean forward give the same per-image bits.
template <int R, bool BOX, class Args>
__device__ __forceinline__ void loss_many_partial_body(const Args a, float* __restrict__ partial) {
  const int b = blockIdx.y, blk = blockIdx.x, C = a.C;
  int lo, hi;
  loss_slice(a.A, blk, lo, hi);
  const int j = threadIdx.x & (MC_LANES - 1), grp = threadIdx.x / MC_LANES;
  float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = lo + grp; i < hi; i += MC_GROUPS) {            // (group-uniform)
    const long long row = (long long)b * a.A + i;
    const float* p = a.pred + row * (C + 5);
    const float* g = a.gt + row * (C + 9);
    float l[R], e[R];
    const float m = mc_load_logits<R>(p, C, j, l);
    const float lse = logf(mc_exp_sum<R>(C, j, m, l, e));
    float ce = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int c = j + MC_LANES * r;
      if (c < C) ce += g[9 + c] * (-((l[r] - m) - lse));
    }
    ce = mc_group_sum(ce);
    AnchorGeom t;
    anchor_geom<BOX>(a, p, g, a.anchors + 4 * i, t);
    if (j == 0) {                                              // one lane of the group carries the row into the block's sums
      s[0] += t.mask;
      s[1] += t.mask * ce;
      s[2] += t.mask * (t.e * t.e);
      s[3] += (1.f - t.mask) * (t.e * t.e);
      s[4] += BOX ? t.bb : t.mask * t.bb;
    }
  }
  block_reduce_store<5, MC_THREADS>(s, partial, b, blk);
}

template <int R>
__global__ __launch_bounds__(MC_THREADS) void loss_many_partial_kernel(LossArgs a, float* __restrict__ partial) {
  loss_many_partial_body<R, false>(a, partial);
}
template <int R>
__global__ __launch_bounds__(MC_THREADS) void loss_box_many_partial_kernel(LossBoxArgs a, float* __restrict__ partial) {
  loss_many_partial_body<R, true>(a, partial);
}

// A positive dpred row is written by its 16-lane group: lane j stores classes c = j, j + 16, ... as
// kc * (sum(onehot) * softmax_c - onehot_c), onehot(r, c) being the row's one-hot at c = j + 16 r (a register of the dense gt row,
// or a comparison with the sparse class id); lanes 0..4 store the confidence and the four deltas, geom_grad(og) being the kernel's
// anchor_geom_grad call (every lane evaluates it, as it does anchor_geom).
template <int R, class OneHot, class GeomGrad>
__device__ __forceinline__ void store_positive_row(float* o, int C, int j, float kc, float ohs, const float (&e)[R], float sum,
                                                   OneHot onehot, GeomGrad geom_grad) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int c = j + MC_LANES * r;
    if (c < C) o[c] = kc * (ohs * (e[r] / sum) - onehot(r, c));
  }
  float og[5];
  geom_grad(og);
  if (j < 5) o[C + j] = (j == 0) ? og[0] : (j == 1) ? og[1] : (j == 2) ? og[2] : (j == 3) ? og[3] : og[4];
}

template <int R, bool BOX, class Args>
__device__ __forceinline__ void loss_many_bwd_body(const Args a, const float* __restrict__ nobj, const float* __restrict__ coef,
                                                   float* __restrict__ dpred, const float* __restrict__ gmean) {
  const long long total = (long long)a.B * a.A;
  const int C = a.C, j = threadIdx.x & (MC_LANES - 1);
  for (long long row = (long long)blockIdx.x * MC_GROUPS + threadIdx.x / MC_LANES; row < total; row += (long long)gridDim.x * MC_GROUPS) {
    const int b = (int)(row / a.A), i = (int)(row - (long long)b * a.A);
    const float* p = a.pred + row * (C + 5);
    const float* g = a.gt + row * (C + 9);
    float l[R], e[R], oh[R];
    const float m = mc_load_logits<R>(p, C, j, l);
    const float sum = mc_exp_sum<R>(C, j, m, l, e);
    float ohs = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      oh[r] = (j + MC_LANES * r < C) ? g[9 + j + MC_LANES * r] : 0.f;
      ohs += oh[r];
    }
    ohs = mc_group_sum(ohs);
    AnchorGeom t;
    anchor_geom<BOX>(a, p, g, a.anchors + 4 * i, t);
    const float n = nobj[b];
    const Upstream u = upstream_grads(a, coef, gmean, b);
    const float uc = u.uc, us = u.us, ub = u.ub;
    // class logits: w_c*mask/n * (sum(onehot)*softmax_c - onehot_c)
    store_positive_row<R>(dpred + row * (C + 5), C, j, uc * a.w_class * t.mask / n, ohs, e, sum,
                          [&](int r, int) { return oh[r]; },
                          [&](float (&og)[5]) { anchor_geom_grad<BOX>(a, t, p + C + 1, g, n, us, ub, og); });
  }
}

template <int R>
__global__ __launch_bounds__(MC_THREADS) void loss_many_bwd_kernel(LossArgs a, const float* __restrict__ nobj,
                                                                   const float* __restrict__ coef, float* __restrict__ dpred,
                                                                   const float* __restrict__ gmean) {
  loss_many_bwd_body<R, false>(a, nobj, coef, dpred, gmean);
}
template <int R>
__global__ __launch_bounds__(MC_THREADS) void loss_box_many_bwd_kernel(LossBoxArgs a, const float* __restrict__ nobj,
                                                                       const float* __restrict__ coef, float* __restrict__ dpred,
                                                                       const float* __restrict__ gmean) {
  loss_many_bwd_body<R, true>(a, nobj, coef, dpred, gmean);
}

// ---- host side of the dense launches ---------------------------------------------------------------------------------------------------
static void fill_common(LossArgs& a, const float* pred, const float* gt, const float* anchors, int B, int A, int C, int input_h,
                        int input_w, float w_class, float w_pos, float w_neg, float w_bbox) {
  a.pred = pred; a.gt = gt; a.anchors = anchors; a.B = B; a.A = A; a.C = C;
  a.wmax = (float)(input_w - 1); a.hmax = (float)(input_h - 1);
  a.w_class = w_class; a.w_pos = w_pos; a.w_neg = w_neg; a.w_bbox = w_bbox;
}

// what a launch hands its kernel: LossArgs, or (BOX) LossBoxArgs with the kind
template <bool BOX> static auto kernel_args(const LossArgs& a, int box) {
  if constexpr (BOX) {
    LossBoxArgs b;
    static_cast<LossArgs&>(b) = a;
    b.box = box;
    return b;
  } else {
    return a;
  }
}
// launch K (BOX: its loss_box_ twin) with the kernel arguments ka in front of the rest
#define LOSS_T2(A_, B_) <A_, B_>
#define LOSS_LAUNCH(K, TARGS, GRID, BLOCK, ...) do { \
    if constexpr (BOX) hipLaunchKernelGGL(HIP_KERNEL_NAME(loss_box_##K TARGS), GRID, BLOCK, 0, s, ka, __VA_ARGS__); \
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(loss_##K TARGS), GRID, BLOCK, 0, s, ka, __VA_ARGS__); } while (0)

// the <= 16-class kernels: status 1 for anything malformed, a class count past 16 included
static int fill_args(LossArgs& a, const float* pred, const float* gt, const float* anchors, int B, int A, int C,
                     int input_h, int input_w, float w_class, float w_pos, float w_neg, float w_bbox) {
  SQD_CHECK_ARG(pred && gt && anchors && B > 0 && A > 0 && C >= 1 && C <= LOSS_MAX_CLASSES);
  fill_common(a, pred, gt, anchors, B, A, C, input_h, input_w, w_class, w_pos, w_neg, w_bbox);
  return SQD_OK;
}

// the many-class kernels: status 1 for anything malformed, 2 for num_classes > 256
static int fill_args_many(LossArgs& a, const float* pred, const float* gt, const float* anchors, int B, int A, int C,
                          int input_h, int input_w, float w_class, float w_pos, float w_neg, float w_bbox) {
  SQD_CHECK_ARG(pred && gt && anchors && B > 0 && A > 0 && C >= 1);
  if (C > SQD_MANY_MAX_CLASSES) return SQD_ERR_UNSUPPORTED;
  fill_common(a, pred, gt, anchors, B, A, C, input_h, input_w, w_class, w_pos, w_neg, w_bbox);
  return SQD_OK;
}

// The second launch of every forward.  mean4 (or null) selects the grid: ONE block that also writes the batch means, or a thread per
// image.
template <class Kernel>
static void launch_finalize(Kernel kernel, const LossArgs& a, const float* workspace, float* losses, float* counts, float* mean4,
                            hipStream_t s) {
  hipLaunchKernelGGL(kernel, dim3(mean4 ? 1u : (unsigned)sqd_cdiv(a.B, 64)), dim3(64), 0, s, workspace, losses, counts, a.B, a.A,
                     a.w_class, a.w_pos, a.w_neg, a.w_bbox, mean4);
}

// Forward on a dense gt; MANY: the 16-lane-group kernels (1 <= num_classes <= 256), else the <= 16-class ones.  workspace:
// float[B * 16 * 5]; losses: float[4][B] = (class, score, bbox, total); nobj: float[B]; mean (the *_mean_fwd entries): mean4 [4] = the
// batch means of the four, `loss.mean()` of the training step (src/engine/trainer.py:43) computed by the finalize launch itself.
// BOX (the sqd_loss_box_* entries with a kind other than L2): the loss_box_* kernels with a.box = box.
template <bool MANY, bool BOX = false>
static int loss_dense_fwd(const float* pred, const float* gt, const float* anchors, float* workspace, float* losses, float* nobj,
                          float* mean4, bool mean, int B, int A, int C, int input_h, int input_w, float w_class, float w_pos,
                          float w_neg, float w_bbox, void* stream, int box = SQD_BOX_L2) {
  LossArgs a;
  if (int rc = (MANY ? fill_args_many : fill_args)(a, pred, gt, anchors, B, A, C, input_h, input_w, w_class, w_pos, w_neg, w_bbox)) return rc;
  SQD_CHECK_ARG(workspace && losses && nobj && (mean4 || !mean));
  const auto ka = kernel_args<BOX>(a, box);
  hipStream_t s = (hipStream_t)stream;
  if constexpr (MANY) {
#define CALL(R) LOSS_LAUNCH(many_partial_kernel, <R>, dim3(LOSS_NPART, (unsigned)a.B), dim3(MC_THREADS), workspace)
    MC_DISPATCH(a.C, CALL);
#undef CALL
  } else {
    LOSS_LAUNCH(partial_kernel, , dim3(LOSS_NPART, (unsigned)B), dim3(LOSS_THREADS), workspace);
  }
  launch_finalize(loss_finalize_kernel, a, workspace, losses, nobj, mean4, s);
  return sqd_launch_status();
}

// Backward on a dense gt, exactly one of coef / gmean.  coef: float[3][B] upstream gradients of (class, score, bbox) per image
// (total's gradient already added to each).  gmean (backward of mean(total)): a DEVICE float, the gradient arriving at the mean (1 for
// `loss.mean().backward()`); every image's three components get gmean / B.
template <bool MANY, bool BOX = false>
static int loss_dense_bwd(const float* pred, const float* gt, const float* anchors, const float* nobj, const float* coef,
                          const float* gmean, float* dpred, int B, int A, int C, int input_h, int input_w, float w_class, float w_pos,
                          float w_neg, float w_bbox, void* stream, int box = SQD_BOX_L2) {
  LossArgs a;
  if (int rc = (MANY ? fill_args_many : fill_args)(a, pred, gt, anchors, B, A, C, input_h, input_w, w_class, w_pos, w_neg, w_bbox)) return rc;
  SQD_CHECK_ARG(nobj && (coef || gmean) && dpred);
  const auto ka = kernel_args<BOX>(a, box);
  hipStream_t s = (hipStream_t)stream;
  const long long rows = (long long)B * A;
  if constexpr (MANY) {
    const long long blocks64 = (rows + MC_GROUPS - 1) / MC_GROUPS;
    const unsigned blocks = (unsigned)(blocks64 < (1 << 20) ? blocks64 : (1 << 20));
#define CALL(R) LOSS_LAUNCH(many_bwd_kernel, <R>, dim3(blocks), dim3(MC_THREADS), nobj, coef, dpred, gmean)
    MC_DISPATCH(a.C, CALL);
#undef CALL
  } else {
    const int blocks = (int)((rows + LOSS_THREADS - 1) / LOSS_THREADS);
    LOSS_LAUNCH(bwd_kernel, , dim3((unsigned)blocks), dim3(LOSS_THREADS), nobj, coef, dpred, gmean);
  }
  return sqd_launch_status();
}

// The sixteen entries: each forwards to its pass and family; what all of them end in, and what the sparse ones begin with.
#define LOSS_TAIL B, A, num_classes, input_h, input_w, w_class, w_pos, w_neg, w_bbox, stream
extern "C" int sqd_loss_fwd(const float* pred, const float* gt, const float* anchors, float* workspace, float* losses,
                            float* nobj, int B, int A, int num_classes, int input_h, int input_w, float w_class,
                            float w_pos, float w_neg, float w_bbox, void* stream) {
  return loss_dense_fwd<false>(pred, gt, anchors, workspace, losses, nobj, nullptr, false, LOSS_TAIL);
}

extern "C" int sqd_loss_mean_fwd(const float* pred, const float* gt, const float* anchors, float* workspace, float* losses,
                                 float* nobj, float* mean4, int B, int A, int num_classes, int input_h, int input_w, float w_class,
                                 float w_pos, float w_neg, float w_bbox, void* stream) {
  return loss_dense_fwd<false>(pred, gt, anchors, workspace, losses, nobj, mean4, true, LOSS_TAIL);
}

extern "C" int sqd_loss_bwd(const float* pred, const float* gt, const float* anchors, const float* nobj, const float* coef,
                            float* dpred, int B, int A, int num_classes, int input_h, int input_w, float w_class,
                            float w_pos, float w_neg, float w_bbox, void* stream) {
  return loss_dense_bwd<false>(pred, gt, anchors, nobj, coef, nullptr, dpred, LOSS_TAIL);
}

extern "C" int sqd_loss_mean_bwd(const float* pred, const float* gt, const float* anchors, const float* nobj, const float* gmean,
                                 float* dpred, int B, int A, int num_classes, int input_h, int input_w, float w_class,
                                 float w_pos, float w_neg, float w_bbox, void* stream) {
  return loss_dense_bwd<false>(pred, gt, anchors, nobj, nullptr, gmean, dpred, LOSS_TAIL);
}

// sqd_loss_fwd / sqd_loss_mean_fwd / sqd_loss_bwd / sqd_loss_mean_bwd for 1 <= num_classes <= 256: same arguments, same workspace.
extern "C" int sqd_loss_many_fwd(const float* pred, const float* gt, const float* anchors, float* workspace, float* losses,
                                 float* nobj, int B, int A, int num_classes, int input_h, int input_w, float w_class,
                                 float w_pos, float w_neg, float w_bbox, void* stream) {
  return loss_dense_fwd<true>(pred, gt, anchors, workspace, losses, nobj, nullptr, false, LOSS_TAIL);
}

extern "C" int sqd_loss_many_mean_fwd(const float* pred, const float* gt, const float* anchors, float* workspace, float* losses,
                                      float* nobj, float* mean4, int B, int A, int num_classes, int input_h, int input_w, float w_class,
                                      float w_pos, float w_neg, float w_bbox, void* stream) {
  return loss_dense_fwd<true>(pred, gt, anchors, workspace, losses, nobj, mean4, true, LOSS_TAIL);
}

extern "C" int sqd_loss_many_bwd(const float* pred, const float* gt, const float* anchors, const float* nobj, const float* coef,
                                 float* dpred, int B, int A, int num_classes, int input_h, int input_w, float w_class,
                                 float w_pos, float w_neg, float w_bbox, void* stream) {
  return loss_dense_bwd<true>(pred, gt, anchors, nobj, coef, nullptr, dpred, LOSS_TAIL);
}

extern "C" int sqd_loss_many_mean_bwd(const float* pred, const float* gt, const float* anchors, const float* nobj, const float* gmean,
                                      float* dpred, int B, int A, int num_classes, int input_h, int input_w, float w_class,
                                      float w_pos, float w_neg, float w_bbox, void* stream) {
  return loss_dense_bwd<true>(pred, gt, anchors, nobj, nullptr, gmean, dpred, LOSS_TAIL);
}

// ---- sparse ground truth: the positives as a list, 1 <= num_classes <= 256 -----------------------------------------------------------
// The dense gt [B][A][C+9] is zero except for the ~0.1 % rows the encoder assigned a box (csrc/gt_encode.hip), and the encoder already
// returns those rows as a list.  These launches take the list: anchor_idx / boxes / deltas / class_ids [total] and offsets [B+1]
// (image b owns entries offsets[b] .. offsets[b+1] - 1), meaning the dense gt with mask = 1, the box, the deltas and a one-hot class at
// anchor_idx and zeros elsewhere.  Contract: the anchor indices of one image are distinct (the encoder's greedy assignment); their order
// is free; an entry with anchor_idx outside [0, A) (the encoder's "unassigned" value A) is ignored; a class id outside [0, C) gives a row
// without a class term (as the dense encoder leaves the one-hot empty); total = 0 and images without entries are legal (n_obj = 0: NaN).
//
// A negative row costs ONE float of pred, its confidence logit: with mask = 0 the dense kernels' e is -sigmoid(conf) and every other
// term is multiplied by the mask.  A positive row gets a 16-lane group (many_class.h) that synthesises the row's nine gt floats in
// registers, so the class-independent chain is anchor_geom / anchor_geom_grad, the dense kernels' own.  The forward keeps the
// [B][LOSS_NPART][5] partial layout and loss_finalize_kernel; no floating-point atomics anywhere (the LDS atomics are integer or / max,
// which do not depend on the order they arrive in), so the same operands give the same bits and the plain and the mean forward agree.
#define LS_MAX_ANCHORS (1 << 20)
#define LS_BITMAP_WORDS (LS_MAX_ANCHORS / LOSS_NPART / 32)      // one bit per anchor of a block's slice: 8 KB
#define LS_ROWS MC_THREADS                                       // dpred rows per workgroup of the backward

struct SparseGT {
  const int* anchor_idx; const float* boxes; const float* deltas; const int* class_ids; const int* offsets;
  int total;
};

// What a sparse kernel takes: the list, and in the MASKED form the ignore bitmap [B][ceil(A / 32)] (anchor a of image b: word a >> 5,
// bit a & 31).  SparseArgs<false> is SparseGT itself, so the unmasked kernels keep their arguments.
template <bool MASKED> struct SparseArgs : SparseGT {
  SparseArgs(const SparseGT& s, const unsigned*) : SparseGT(s) {}
};
template <> struct SparseArgs<true> : SparseGT {
  const unsigned* ignore;
  SparseArgs(const SparseGT& s, const unsigned* ig) : SparseGT(s), ignore(ig) {}
};

__device__ __forceinline__ bool ignore_bit(const SparseArgs<true>& sg, int b, int A, int i) {
  return (sg.ignore[(long long)b * ((A + 31) >> 5) + (i >> 5)] >> (i & 31)) & 1u;
}
__device__ __forceinline__ bool ignore_bit(const SparseArgs<false>&, int, int, int) { return false; }

// image b's entries [beg, end), cut to the list (a malformed offsets table reads nothing out of bounds)
__device__ __forceinline__ void sparse_range(const SparseGT& sg, int b, int& beg, int& end) {
  beg = max(0, sg.offsets[b]);
  end = min(sg.total, sg.offsets[b + 1]);
}

// the first nine floats of the dense gt row that entry e stands for: mask, xyxy, deltas
__device__ __forceinline__ void sparse_gt_row(const SparseGT& sg, int e, float (&g)[9]) {
  g[0] = 1.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) { g[1 + k] = sg.boxes[4 * (long long)e + k]; g[5 + k] = sg.deltas[4 * (long long)e + k]; }
}

// MASKED: a row that is no positive and whose ignore bit is set adds nothing but a count, the sixth partial sum n_ign
// (partial [B][LOSS_NPART][6]); the words are read from global memory by the global anchor index (a slice's lo is no multiple of 32).
template <int R, bool MASKED, bool BOX, class Args>
__device__ __forceinline__ void loss_sparse_partial_body(const Args a, const SparseArgs<MASKED>& sg, float* __restrict__ partial) {
  constexpr int NS = MASKED ? 6 : 5;
  __shared__ unsigned bitmap[LS_BITMAP_WORDS];
  const int b = blockIdx.y, blk = blockIdx.x, C = a.C, tid = threadIdx.x;
  int lo, hi;
  loss_slice(a.A, blk, lo, hi);
  // 1. mark the slice's positives (integer atomic-or: the result does not depend on the list's order)
  for (int w = tid; w < (hi - lo + 31) / 32; w += MC_THREADS) bitmap[w] = 0u;
  __syncthreads();
  int beg, end;
  sparse_range(sg, b, beg, end);
  for (int e = beg + tid; e < end; e += MC_THREADS) {
    const int i = sg.anchor_idx[e];
    if (i >= lo && i < hi) atomicOr(&bitmap[(i - lo) >> 5], 1u << ((i - lo) & 31));
  }
  __syncthreads();
  float s[NS] = {};
  // 2. every row of the slice: a marked row counts toward n_obj, any other adds sigmoid(conf)^2 (the dense e * e at mask = 0)
  for (int i = lo + tid; i < hi; i += MC_THREADS) {
    if ((bitmap[(i - lo) >> 5] >> ((i - lo) & 31)) & 1u) {
      s[0] += 1.f;
    } else if (MASKED && ignore_bit(sg, b, a.A, i)) {
      s[NS - 1] += 1.f;
    } else {
      const float conf = 1.f / (1.f + expf(-a.pred[((long long)b * a.A + i) * (C + 5) + C]));
      const float e = 0.f - conf;
      s[3] += e * e;
    }
  }
  // 3. the positives: group g takes the image's entries g, g + MC_GROUPS, ... that fall in the slice (a fixed assignment)
  const int j = tid & (MC_LANES - 1), grp = tid / MC_LANES;
  for (int e = beg + grp; e < end; e += MC_GROUPS) {          // (group-uniform)
    const int i = sg.anchor_idx[e];
    if (i < lo || i >= hi) continue;
    const float* p = a.pred + ((long long)b * a.A + i) * (C + 5);
    float g[9];
    sparse_gt_row(sg, e, g);
    const int cls = sg.class_ids[e];
    float l[R], ex[R];
    const float m = mc_load_logits<R>(p, C, j, l);
    const float lse = logf(mc_exp_sum<R>(C, j, m, l, ex));
    float ce = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (j + MC_LANES * r == cls && cls < C) ce += -((l[r] - m) - lse);
    ce = mc_group_sum(ce);
    AnchorGeom t;
    anchor_geom<BOX>(a, p, g, a.anchors + 4 * i, t);
    if (j == 0) {
      s[1] += ce;
      s[2] += t.e * t.e;
      s[4] += t.bb;
    }
  }
  block_reduce_store<NS, MC_THREADS>(s, partial, b, blk);
}

template <int R, bool MASKED = false>
__global__ __launch_bounds__(MC_THREADS) void loss_sparse_partial_kernel(LossArgs a, SparseArgs<MASKED> sg, float* __restrict__ partial) {
  loss_sparse_partial_body<R, MASKED, false>(a, sg, partial);
}
template <int R, bool MASKED>
__global__ __launch_bounds__(MC_THREADS) void loss_box_sparse_partial_kernel(LossBoxArgs a, SparseArgs<MASKED> sg, float* __restrict__ partial) {
  loss_sparse_partial_body<R, MASKED, true>(a, sg, partial);
}

// The masked forward's second stage: counts [2][B] = (n_obj, n_neg).
__global__ void loss_masked_finalize_kernel(const float* __restrict__ partial, float* __restrict__ losses, float* __restrict__ counts,
                                            int B, int A, float w_class, float w_pos, float w_neg, float w_bbox, float* __restrict__ mean4) {
  finalize_walk<MaskedImage>(partial, losses, counts, B, A, w_class, w_pos, w_neg, w_bbox, mean4);
}

// One launch writes all of dpred.  Workgroup (x, b) owns rows x * LS_ROWS .. of image b: it looks its rows up in the image's list
// (slot[row] = entry + 1), writes every negative row as zeros with the confidence gradient in column C (anchor_geom_grad at mask = 0),
// consecutive lanes storing consecutive 16-byte pieces, and hands each positive row to a lane group as loss_many_bwd_kernel does.
// MASKED: ``nobj`` is counts [2][B] = (n_obj, n_neg) of the masked forward.  A positive row is what the unmasked kernel writes (the
// negative denominator reaches it only as w_neg * 0 / n_neg); a row that is no positive and whose ignore bit is set is all +0; every
// other row carries the confidence gradient with 1 / n_neg, and nothing is NaN because a count is 0.
template <int R, bool MASKED, bool BOX, class Args>
__device__ __forceinline__ void loss_sparse_bwd_body(const Args a, const SparseArgs<MASKED>& sg, const float* __restrict__ nobj,
                                                     const float* __restrict__ coef, float* __restrict__ dpred,
                                                     const float* __restrict__ gmean) {
  __shared__ int slot[LS_ROWS];
  __shared__ float cgrad[LS_ROWS];
  __shared__ unsigned char ign[MASKED ? LS_ROWS : 1];
  const int b = blockIdx.y, row0 = blockIdx.x * LS_ROWS, C = a.C, W = C + 5, tid = threadIdx.x;
  const int nrows = min(LS_ROWS, a.A - row0);
  slot[tid] = 0;
  __syncthreads();
  int beg, end;
  sparse_range(sg, b, beg, end);
  for (int e = beg + tid; e < end; e += MC_THREADS) {
    const int i = sg.anchor_idx[e];
    if (i >= row0 && i < row0 + nrows) atomicMax(&slot[i - row0], e - beg + 1);      // (distinct by contract; max: defined anyway)
  }
  const float n = nobj[b];
  const Upstream u = upstream_grads(a, coef, gmean, b);
  const float uc = u.uc, us = u.us, ub = u.ub;
  // mask = 0 in the dense formulas: the score coefficient, and what the class / delta columns hold (0, or NaN where n_obj = 0)
  // MASKED: the same expressions where their denominator is a count > 0 (so a zero keeps the sign it has there), else 0; for
  // n > 0 the dropped w_pos * 0 / n is an exact zero added in front
  float nneg = 0.f, kneg, zc, zd;
  if constexpr (MASKED) {
    nneg = nobj[a.B + b];
    kneg = nneg > 0.f ? us * (0.f + a.w_neg * (1.f - 0.f) / nneg) : 0.f;
    zc = n > 0.f ? (uc * a.w_class * 0.f / n) * 0.f : 0.f;
    zd = n > 0.f ? kneg * 0.f + (ub * a.w_bbox * 0.f / n * 2.f) * 0.f : 0.f;
  } else {
    kneg = us * (a.w_pos * 0.f / n + a.w_neg * (1.f - 0.f) / ((float)a.A - n));
    zc = (uc * a.w_class * 0.f / n) * 0.f;
    zd = kneg * 0.f + (ub * a.w_bbox * 0.f / n * 2.f) * 0.f;
  }
  __syncthreads();
  const long long base = (long long)b * a.A + row0;
  if (MASKED && tid < nrows) ign[tid] = slot[tid] == 0 && ignore_bit(sg, b, a.A, row0 + tid);
  if (tid < nrows && slot[tid] == 0) {
    const float conf = 1.f / (1.f + expf(-a.pred[(base + tid) * W + C]));
    const float dL_de = 2.f * kneg * (0.f - conf);
    cgrad[tid] = -dL_de * conf * (1.f - conf);
    if (MASKED && ign[tid]) cgrad[tid] = 0.f;                                     // (ign[tid]: this thread's own write)
  }
  // an ignored row differs from a negative one outside column C only where zc / zd are not +0 (a negative upstream gradient gives
  // -0): only then does a store have to look the row up
  const bool zplain = MASKED && __float_as_uint(zc) == 0u && __float_as_uint(zd) == 0u;
  __syncthreads();
  float* __restrict__ o = dpred + base * W;
  {
    // the workgroup's nrows * W floats are contiguous: up to three floats to the first 16-byte boundary, 16-byte stores, a tail.  A
    // vector covers at most two rows (W >= 6); one that touches a positive row stores its other floats one by one.
    const int nfl = nrows * W;
    const auto val = [&](int r, int col) {
      if constexpr (MASKED) {
        if (col == C) return cgrad[r];
        if (!zplain && ign[r]) return 0.f;
        return col < C ? zc : zd;
      } else {
        return col < C ? zc : (col == C ? cgrad[r] : zd);
      }
    };
    int head = (int)((4 - ((base * W) & 3)) & 3);
    if ((reinterpret_cast<uintptr_t>(dpred) & 15) != 0 || head > nfl) head = nfl;          // (an unaligned dpred: all of it one by one)
    const int nv = (nfl - head) / 4;
    const auto put = [&](int f) {
      const int r = f / W, col = f - r * W;
      if (slot[r] == 0) o[f] = val(r, col);
    };
    for (int f = tid; f < head; f += MC_THREADS) put(f);
    for (int f = head + 4 * nv + tid; f < nfl; f += MC_THREADS) put(f);
    f32x4* __restrict__ o4 = reinterpret_cast<f32x4*>(o + head);
    const int q = (4 * MC_THREADS) / W, rem = (4 * MC_THREADS) % W;      // (row, column) advance by 4 * MC_THREADS floats: no division
    int r = (head + 4 * tid) / W, col = head + 4 * tid - r * W;
    for (int v = tid; v < nv; v += MC_THREADS) {
      float x[4]; int rk[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int ck = col + k >= W ? col + k - W : col + k;
        rk[k] = col + k >= W ? r + 1 : r;
        x[k] = val(rk[k], ck);
      }
      if (slot[r] == 0 && slot[rk[3]] == 0) {
        o4[v] = (f32x4){x[0], x[1], x[2], x[3]};
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (slot[rk[k]] == 0) o[head + 4 * v + k] = x[k];
      }
      r += q; col += rem;
      if (col >= W) { col -= W; ++r; }
    }
  }
  const int j = tid & (MC_LANES - 1);
  for (int r = tid / MC_LANES; r < nrows; r += MC_GROUPS) {     // (group-uniform)
    const int sl = slot[r];
    if (sl == 0) continue;
    const int e = beg + sl - 1;
    const float* p = a.pred + (base + r) * W;
    float g[9];
    sparse_gt_row(sg, e, g);
    const int cls = sg.class_ids[e];
    const float ohs = (cls >= 0 && cls < C) ? 1.f : 0.f;
    float l[R], ex[R];
    const float m = mc_load_logits<R>(p, C, j, l);
    const float sum = mc_exp_sum<R>(C, j, m, l, ex);
    AnchorGeom t;
    anchor_geom<BOX>(a, p, g, a.anchors + 4 * (row0 + r), t);
    store_positive_row<R>(o + (long long)r * W, C, j, uc * a.w_class * t.mask / n, ohs, ex, sum,
                          [&](int, int c) { return c == cls ? 1.f : 0.f; },
                          [&](float (&og)[5]) {
                            if (MASKED) anchor_geom_grad_nneg<BOX>(a, t, p + C + 1, g, n, nneg > 0.f ? nneg : 1.f, us, ub, og);      // (mask = 1: w_neg * 0 / n_neg)
                            else anchor_geom_grad<BOX>(a, t, p + C + 1, g, n, us, ub, og);
                          });
  }
}

template <int R, bool MASKED = false>
__global__ __launch_bounds__(MC_THREADS) void loss_sparse_bwd_kernel(LossArgs a, SparseArgs<MASKED> sg, const float* __restrict__ nobj,
                                                                     const float* __restrict__ coef, float* __restrict__ dpred,
                                                                     const float* __restrict__ gmean) {
  loss_sparse_bwd_body<R, MASKED, false>(a, sg, nobj, coef, dpred, gmean);
}
template <int R, bool MASKED>
__global__ __launch_bounds__(MC_THREADS) void loss_box_sparse_bwd_kernel(LossBoxArgs a, SparseArgs<MASKED> sg, const float* __restrict__ nobj,
                                                                         const float* __restrict__ coef, float* __restrict__ dpred,
                                                                         const float* __restrict__ gmean) {
  loss_sparse_bwd_body<R, MASKED, true>(a, sg, nobj, coef, dpred, gmean);
}

// ---- host side of the sparse and the masked launches -----------------------------------------------------------------------------------
// status 1 for anything malformed (the list pointers may be null when total = 0), 2 for num_classes > 256 or A > 2^20
static int fill_args_sparse(LossArgs& a, SparseGT& sg, const float* pred, const int* anchor_idx, const float* boxes, const float* deltas,
                            const int* class_ids, const int* offsets, const float* anchors, int total, int B, int A, int C,
                            int input_h, int input_w, float w_class, float w_pos, float w_neg, float w_bbox) {
  SQD_CHECK_ARG(pred && anchors && offsets && B > 0 && B <= 65535 && A > 0 && C >= 1 && total >= 0);
  SQD_CHECK_ARG(total == 0 || (anchor_idx && boxes && deltas && class_ids));
  if (C > SQD_MANY_MAX_CLASSES || A > LS_MAX_ANCHORS) return SQD_ERR_UNSUPPORTED;
  fill_common(a, pred, nullptr, anchors, B, A, C, input_h, input_w, w_class, w_pos, w_neg, w_bbox);
  sg.anchor_idx = anchor_idx; sg.boxes = boxes; sg.deltas = deltas; sg.class_ids = class_ids; sg.offsets = offsets; sg.total = total;
  return SQD_OK;
}

// Forward on the sparse ground truth (all device pointers).  Workspace (MASKED: float[B * 16 * 6]), losses, mean4 and mean as for
// loss_dense_fwd; counts: nobj float[B], MASKED: float[2][B] = (n_obj, n_neg), what the backward takes in nobj's place.
template <bool MASKED, bool BOX = false>
static int loss_sparse_fwd(const float* pred, const int* anchor_idx, const float* boxes, const float* deltas, const int* class_ids,
                           const int* offsets, const unsigned* ignore, const float* anchors, float* workspace, float* losses,
                           float* counts, float* mean4, bool mean, int total, int B, int A, int C, int input_h, int input_w,
                           float w_class, float w_pos, float w_neg, float w_bbox, void* stream, int box = SQD_BOX_L2) {
  LossArgs a; SparseGT sg;
  if (int rc = fill_args_sparse(a, sg, pred, anchor_idx, boxes, deltas, class_ids, offsets, anchors, total, B, A, C, input_h, input_w,
                                w_class, w_pos, w_neg, w_bbox)) return rc;
  SQD_CHECK_ARG((ignore || !MASKED) && workspace && losses && counts && (mean4 || !mean));
  const auto ka = kernel_args<BOX>(a, box);
  hipStream_t s = (hipStream_t)stream;
  const SparseArgs<MASKED> sa(sg, ignore);
#define CALL(R) LOSS_LAUNCH(sparse_partial_kernel, LOSS_T2(R, MASKED), dim3(LOSS_NPART, (unsigned)a.B), dim3(MC_THREADS), sa, workspace)
  MC_DISPATCH(a.C, CALL);
#undef CALL
  if constexpr (MASKED) launch_finalize(loss_masked_finalize_kernel, a, workspace, losses, counts, mean4, s);
  else launch_finalize(loss_finalize_kernel, a, workspace, losses, counts, mean4, s);
  return sqd_launch_status();
}

// Backward on the sparse ground truth, exactly one of coef / gmean (loss_dense_bwd); counts: the forward's.
template <bool MASKED, bool BOX = false>
static int loss_sparse_bwd(const float* pred, const int* anchor_idx, const float* boxes, const float* deltas, const int* class_ids,
                           const int* offsets, const unsigned* ignore, const float* anchors, const float* counts, const float* coef,
                           const float* gmean, float* dpred, int total, int B, int A, int C, int input_h, int input_w, float w_class,
                           float w_pos, float w_neg, float w_bbox, void* stream, int box = SQD_BOX_L2) {
  LossArgs a; SparseGT sg;
  if (int rc = fill_args_sparse(a, sg, pred, anchor_idx, boxes, deltas, class_ids, offsets, anchors, total, B, A, C, input_h, input_w,
                                w_class, w_pos, w_neg, w_bbox)) return rc;
  SQD_CHECK_ARG((ignore || !MASKED) && counts && (coef || gmean) && dpred);
  const auto ka = kernel_args<BOX>(a, box);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)sqd_cdiv(a.A, LS_ROWS), (unsigned)a.B);
  const SparseArgs<MASKED> sa(sg, ignore);
#define CALL(R) LOSS_LAUNCH(sparse_bwd_kernel, LOSS_T2(R, MASKED), grid, dim3(MC_THREADS), sa, counts, coef, dpred, gmean)
  MC_DISPATCH(a.C, CALL);
#undef CALL
  return sqd_launch_status();
}

#define SPARSE_LIST pred, anchor_idx, boxes, deltas, class_ids, offsets
extern "C" int sqd_loss_sparse_fwd(const float* pred, const int* anchor_idx, const float* boxes, const float* deltas, const int* class_ids,
                                   const int* offsets, const float* anchors, float* workspace, float* losses, float* nobj, int total,
                                   int B, int A, int num_classes, int input_h, int input_w, float w_class, float w_pos, float w_neg,
                                   float w_bbox, void* stream) {
  return loss_sparse_fwd<false>(SPARSE_LIST, nullptr, anchors, workspace, losses, nobj, nullptr, false, total, LOSS_TAIL);
}

extern "C" int sqd_loss_sparse_mean_fwd(const float* pred, const int* anchor_idx, const float* boxes, const float* deltas,
                                        const int* class_ids, const int* offsets, const float* anchors, float* workspace, float* losses,
                                        float* nobj, float* mean4, int total, int B, int A, int num_classes, int input_h, int input_w,
                                        float w_class, float w_pos, float w_neg, float w_bbox, void* stream) {
  return loss_sparse_fwd<false>(SPARSE_LIST, nullptr, anchors, workspace, losses, nobj, mean4, true, total, LOSS_TAIL);
}

extern "C" int sqd_loss_sparse_bwd(const float* pred, const int* anchor_idx, const float* boxes, const float* deltas, const int* class_ids,
                                   const int* offsets, const float* anchors, const float* nobj, const float* coef, float* dpred, int total,
                                   int B, int A, int num_classes, int input_h, int input_w, float w_class, float w_pos, float w_neg,
                                   float w_bbox, void* stream) {
  return loss_sparse_bwd<false>(SPARSE_LIST, nullptr, anchors, nobj, coef, nullptr, dpred, total, LOSS_TAIL);
}

extern "C" int sqd_loss_sparse_mean_bwd(const float* pred, const int* anchor_idx, const float* boxes, const float* deltas,
                                        const int* class_ids, const int* offsets, const float* anchors, const float* nobj,
                                        const float* gmean, float* dpred, int total, int B, int A, int num_classes, int input_h,
                                        int input_w, float w_class, float w_pos, float w_neg, float w_bbox, void* stream) {
  return loss_sparse_bwd<false>(SPARSE_LIST, nullptr, anchors, nobj, nullptr, gmean, dpred, total, LOSS_TAIL);
}

// ---- masked sparse loss: ignore regions and object-free images ---------------------------------------------------------------------------
// The sparse launches + ignore [B][ceil(A / 32)] uint32 (sqd_anchor_ignore_fwd's bitmap).  Per image: pos = the list's valid entries,
// ign = the anchors whose bit is set and that are no positives (a positive wins over its own bit), n_obj = |pos|, n_ign = |ign|,
// n_neg = A - n_obj - n_ign.  class, pos-score and bbox are the sparse launches' sums / n_obj, each 0 where n_obj = 0; neg =
// w_neg * sum over the rows outside pos and ign of sigmoid(conf)^2 / n_neg, 0 where n_neg = 0.  dpred: a positive row as the
// unmasked launch writes it, a row of ign all zeros, any other row zeros and the confidence gradient with 1 / n_neg.  An all-zero
// bitmap on images that all have positives gives the unmasked launches' bits.
extern "C" int sqd_loss_masked_fwd(const float* pred, const int* anchor_idx, const float* boxes, const float* deltas, const int* class_ids,
                                   const int* offsets, const unsigned* ignore, const float* anchors, float* workspace, float* losses,
                                   float* counts, int total, int B, int A, int num_classes, int input_h, int input_w, float w_class,
                                   float w_pos, float w_neg, float w_bbox, void* stream) {
  return loss_sparse_fwd<true>(SPARSE_LIST, ignore, anchors, workspace, losses, counts, nullptr, false, total, LOSS_TAIL);
}

extern "C" int sqd_loss_masked_mean_fwd(const float* pred, const int* anchor_idx, const float* boxes, const float* deltas,
                                        const int* class_ids, const int* offsets, const unsigned* ignore, const float* anchors,
                                        float* workspace, float* losses, float* counts, float* mean4, int total, int B, int A,
                                        int num_classes, int input_h, int input_w, float w_class, float w_pos, float w_neg,
                                        float w_bbox, void* stream) {
  return loss_sparse_fwd<true>(SPARSE_LIST, ignore, anchors, workspace, losses, counts, mean4, true, total, LOSS_TAIL);
}

extern "C" int sqd_loss_masked_bwd(const float* pred, const int* anchor_idx, const float* boxes, const float* deltas, const int* class_ids,
                                   const int* offsets, const unsigned* ignore, const float* anchors, const float* counts,
                                   const float* coef, float* dpred, int total, int B, int A, int num_classes, int input_h, int input_w,
                                   float w_class, float w_pos, float w_neg, float w_bbox, void* stream) {
  return loss_sparse_bwd<true>(SPARSE_LIST, ignore, anchors, counts, coef, nullptr, dpred, total, LOSS_TAIL);
}

extern "C" int sqd_loss_masked_mean_bwd(const float* pred, const int* anchor_idx, const float* boxes, const float* deltas,
                                        const int* class_ids, const int* offsets, const unsigned* ignore, const float* anchors,
                                        const float* counts, const float* gmean, float* dpred, int total, int B, int A,
                                        int num_classes, int input_h, int input_w, float w_class, float w_pos, float w_neg,
                                        float w_bbox, void* stream) {
  return loss_sparse_bwd<true>(SPARSE_LIST, ignore, anchors, counts, nullptr, gmean, dpred, total, LOSS_TAIL);
}

// ---- any box regression kind: six entries, {dense, sparse, masked} x {fwd, bwd} ---------------------------------------------------------
// box_loss: SQD_BOX_L2 .. SQD_BOX_CIOU (anything else: status 1).  SQD_BOX_L2 runs the launches of the sixteen entries above, so it
// gives their bits; the other kinds run the loss_box_* kernels.  mean4: null for the plain forward; backward: exactly one of coef /
// gmean.  The dense pair serves 1 <= num_classes <= 256: the <= 16-class kernels up to 16 classes, the many-class ones past it.
#define BOX_DISPATCH(FN, ...) (box_loss == SQD_BOX_L2 ? FN<false>(__VA_ARGS__) : FN<true>(__VA_ARGS__, box_loss))
#define BOX_KIND_OK(k) ((k) >= SQD_BOX_L2 && (k) <= SQD_BOX_CIOU)
template <bool BOX> static int box_dense_fwd(const float* pred, const float* gt, const float* anchors, float* workspace, float* losses,
                                             float* nobj, float* mean4, int B, int A, int num_classes, int input_h, int input_w,
                                             float w_class, float w_pos, float w_neg, float w_bbox, void* stream, int box = SQD_BOX_L2) {
  if (num_classes <= LOSS_MAX_CLASSES) return loss_dense_fwd<false, BOX>(pred, gt, anchors, workspace, losses, nobj, mean4, mean4 != nullptr, LOSS_TAIL, box);
  return loss_dense_fwd<true, BOX>(pred, gt, anchors, workspace, losses, nobj, mean4, mean4 != nullptr, LOSS_TAIL, box);
}
template <bool BOX> static int box_dense_bwd(const float* pred, const float* gt, const float* anchors, const float* nobj,
                                             const float* coef, const float* gmean, float* dpred, int B, int A, int num_classes,
                                             int input_h, int input_w, float w_class, float w_pos, float w_neg, float w_bbox,
                                             void* stream, int box = SQD_BOX_L2) {
  if (num_classes <= LOSS_MAX_CLASSES) return loss_dense_bwd<false, BOX>(pred, gt, anchors, nobj, coef, gmean, dpred, LOSS_TAIL, box);
  return loss_dense_bwd<true, BOX>(pred, gt, anchors, nobj, coef, gmean, dpred, LOSS_TAIL, box);
}
template <bool BOX> static int box_sparse_fwd(const float* pred, const int* anchor_idx, const float* boxes, const float* deltas,
                                              const int* class_ids, const int* offsets, const unsigned* ignore, bool masked,
                                              const float* anchors, float* workspace, float* losses, float* counts, float* mean4,
                                              int total, int B, int A, int num_classes, int input_h, int input_w, float w_class,
                                              float w_pos, float w_neg, float w_bbox, void* stream, int box = SQD_BOX_L2) {
  if (masked) return loss_sparse_fwd<true, BOX>(SPARSE_LIST, ignore, anchors, workspace, losses, counts, mean4, mean4 != nullptr, total, LOSS_TAIL, box);
  return loss_sparse_fwd<false, BOX>(SPARSE_LIST, nullptr, anchors, workspace, losses, counts, mean4, mean4 != nullptr, total, LOSS_TAIL, box);
}
template <bool BOX> static int box_sparse_bwd(const float* pred, const int* anchor_idx, const float* boxes, const float* deltas,
                                              const int* class_ids, const int* offsets, const unsigned* ignore, bool masked,
                                              const float* anchors, const float* counts, const float* coef, const float* gmean,
                                              float* dpred, int total, int B, int A, int num_classes, int input_h, int input_w,
                                              float w_class, float w_pos, float w_neg, float w_bbox, void* stream, int box = SQD_BOX_L2) {
  if (masked) return loss_sparse_bwd<true, BOX>(SPARSE_LIST, ignore, anchors, counts, coef, gmean, dpred, total, LOSS_TAIL, box);
  return loss_sparse_bwd<false, BOX>(SPARSE_LIST, nullptr, anchors, counts, coef, gmean, dpred, total, LOSS_TAIL, box);
}

extern "C" int sqd_loss_box_fwd(const float* pred, const float* gt, const float* anchors, float* workspace, float* losses, float* nobj,
                                float* mean4, int box_loss, int B, int A, int num_classes, int input_h, int input_w, float w_class,
                                float w_pos, float w_neg, float w_bbox, void* stream) {
  SQD_CHECK_ARG(BOX_KIND_OK(box_loss));
  return BOX_DISPATCH(box_dense_fwd, pred, gt, anchors, workspace, losses, nobj, mean4, LOSS_TAIL);
}

extern "C" int sqd_loss_box_bwd(const float* pred, const float* gt, const float* anchors, const float* nobj, const float* coef,
                                const float* gmean, float* dpred, int box_loss, int B, int A, int num_classes, int input_h, int input_w,
                                float w_class, float w_pos, float w_neg, float w_bbox, void* stream) {
  SQD_CHECK_ARG(BOX_KIND_OK(box_loss) && (coef != nullptr) != (gmean != nullptr));
  return BOX_DISPATCH(box_dense_bwd, pred, gt, anchors, nobj, coef, gmean, dpred, LOSS_TAIL);
}

extern "C" int sqd_loss_box_sparse_fwd(const float* pred, const int* anchor_idx, const float* boxes, const float* deltas,
                                       const int* class_ids, const int* offsets, const float* anchors, float* workspace, float* losses,
                                       float* nobj, float* mean4, int box_loss, int total, int B, int A, int num_classes, int input_h,
                                       int input_w, float w_class, float w_pos, float w_neg, float w_bbox, void* stream) {
  SQD_CHECK_ARG(BOX_KIND_OK(box_loss));
  return BOX_DISPATCH(box_sparse_fwd, SPARSE_LIST, nullptr, false, anchors, workspace, losses, nobj, mean4, total, LOSS_TAIL);
}

extern "C" int sqd_loss_box_sparse_bwd(const float* pred, const int* anchor_idx, const float* boxes, const float* deltas,
                                       const int* class_ids, const int* offsets, const float* anchors, const float* nobj,
                                       const float* coef, const float* gmean, float* dpred, int box_loss, int total, int B, int A,
                                       int num_classes, int input_h, int input_w, float w_class, float w_pos, float w_neg, float w_bbox,
                                       void* stream) {
  SQD_CHECK_ARG(BOX_KIND_OK(box_loss) && (coef != nullptr) != (gmean != nullptr));
  return BOX_DISPATCH(box_sparse_bwd, SPARSE_LIST, nullptr, false, anchors, nobj, coef, gmean, dpred, total, LOSS_TAIL);
}

extern "C" int sqd_loss_box_masked_fwd(const float* pred, const int* anchor_idx, const float* boxes, const float* deltas,
                                       const int* class_ids, const int* offsets, const unsigned* ignore, const float* anchors,
                                       float* workspace, float* losses, float* counts, float* mean4, int box_loss, int total, int B,
                                       int A, int num_classes, int input_h, int input_w, float w_class, float w_pos, float w_neg,
                                       float w_bbox, void* stream) {
  SQD_CHECK_ARG(BOX_KIND_OK(box_loss));
  return BOX_DISPATCH(box_sparse_fwd, SPARSE_LIST, ignore, true, anchors, workspace, losses, counts, mean4, total, LOSS_TAIL);
}

extern "C" int sqd_loss_box_masked_bwd(const float* pred, const int* anchor_idx, const float* boxes, const float* deltas,
                                       const int* class_ids, const int* offsets, const unsigned* ignore, const float* anchors,
                                       const float* counts, const float* coef, const float* gmean, float* dpred, int box_loss, int total,
                                       int B, int A, int num_classes, int input_h, int input_w, float w_class, float w_pos, float w_neg,
                                       float w_bbox, void* stream) {
  SQD_CHECK_ARG(BOX_KIND_OK(box_loss) && (coef != nullptr) != (gmean != nullptr));
  return BOX_DISPATCH(box_sparse_bwd, SPARSE_LIST, ignore, true, anchors, counts, coef, gmean, dpred, total, LOSS_TAIL);
}
