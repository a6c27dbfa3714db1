// What the narrow fused detect (postproc.hip) and the wide family (detect_wide.hip) share: the decoded box, the argument block of every
// detect kernel and its two host-side builders.
#pragma once
#include "sqd_common.h"
#include <math.h>

struct BoxF { float x1, y1, x2, y2; };

__device__ __forceinline__ BoxF anchor_box(const float* __restrict__ d, const float* __restrict__ anc, float wmax, float hmax) {
  const float ax = anc[0], ay = anc[1], aw = anc[2], ah = anc[3];
  const float cx = ax + aw * d[0];
  const float cy = ay + ah * d[1];
  const float w = aw * expf(d[2]);
  const float h = ah * expf(d[3]);
  BoxF b;
  b.x1 = fminf(fmaxf(cx - 0.5f * (w - 1.f), 0.f), wmax);
  b.y1 = fminf(fmaxf(cy - 0.5f * (h - 1.f), 0.f), hmax);
  b.x2 = fminf(fmaxf(cx + 0.5f * (w - 1.f), 0.f), wmax);
  b.y2 = fminf(fmaxf(cy + 0.5f * (h - 1.f), 0.f), hmax);
  return b;
}

struct DetArgs {
  const float* pred = nullptr; const float* anchors = nullptr; const float* scales = nullptr;   // scales [B][2] = (sy, sx) or null
  const float* shifts = nullptr;                                  // [B][2] = (dy, dx) added after the scale division, or null
  const long long* in_class = nullptr; const float* in_score = nullptr; const float* in_box = nullptr;   // dense inputs (filter mode) or null
  unsigned* keys = nullptr;                                       // workspace [B][ceil4(A)] keys + [B] arrival counters, or null (one workgroup per image)
  int keys_ready = 0;                                             // the workspace already holds every key of the batch (words A .. ceil4(A)-1 of an image: any)
  int S = 1, per = 0;                                             // detect_kernel's scoring split (launch_detect sets them); the wide kernels read neither
  int* det_count = nullptr; long long* det_class = nullptr; float* det_score = nullptr; float* det_box = nullptr; int* det_anchor = nullptr;
  int B = 0, A = 0, C = 0, K = 0;
  float wmax = 0.f, hmax = 0.f, nms_thresh = 0.f, score_thresh = 0.f;
};

// the part every entry point fills the same way: workspace, result buffers, sizes, thresholds
static inline DetArgs det_args_common(unsigned* keys_ws, int* det_count, long long* det_class, float* det_score, float* det_box,
                                      int* det_anchor, int B, int A, int num_classes, int keep_top_k, float nms_thresh, float score_thresh) {
  DetArgs a;
  a.keys = keys_ws;
  a.det_count = det_count; a.det_class = det_class; a.det_score = det_score; a.det_box = det_box; a.det_anchor = det_anchor;
  a.B = B; a.A = A; a.C = num_classes; a.K = keep_top_k;
  a.nms_thresh = nms_thresh; a.score_thresh = score_thresh;
  return a;
}

// pred inputs: pred [B][A][C+5], anchors [A][4], optional scales / shifts; boxes are clamped to the input_h x input_w canvas
static inline DetArgs det_args_pred(const float* pred, const float* anchors, const float* scales, const float* shifts, unsigned* keys_ws,
                                    int* det_count, long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                    int num_classes, int input_h, int input_w, int keep_top_k, float nms_thresh, float score_thresh) {
  DetArgs a = det_args_common(keys_ws, det_count, det_class, det_score, det_box, det_anchor, B, A, num_classes, keep_top_k, nms_thresh, score_thresh);
  a.pred = pred; a.anchors = anchors; a.scales = scales; a.shifts = shifts;
  a.wmax = (float)(input_w - 1); a.hmax = (float)(input_h - 1);
  return a;
}

// dense inputs: class_ids int64 [B][A], scores [B][A], boxes [B][A][4]
static inline DetArgs det_args_dense(const long long* class_ids, const float* scores, const float* boxes, unsigned* keys_ws, int* det_count,
                                     long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                     int num_classes, int keep_top_k, float nms_thresh, float score_thresh) {
  DetArgs a = det_args_common(keys_ws, det_count, det_class, det_score, det_box, det_anchor, B, A, num_classes, keep_top_k, nms_thresh, score_thresh);
  a.in_class = class_ids; a.in_score = scores; a.in_box = boxes;
  return a;
}

// status-1 checks of the pointers: every input of the form and the five result buffers are there, det_box (and the dense boxes) take
// 16-byte accesses.  pred's own alignment differs by entry point (the one-lane decode reads it in 16-byte pieces, the 16-lane one does not)
static inline bool det_ptrs_ok(const DetArgs& a) {
  const bool in = a.in_score ? (a.in_class && a.in_box && ((uintptr_t)a.in_box & 15) == 0) : (a.pred && a.anchors);
  return in && a.det_count && a.det_class && a.det_score && a.det_box && a.det_anchor && ((uintptr_t)a.det_box & 15) == 0;
}
static inline bool det_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
