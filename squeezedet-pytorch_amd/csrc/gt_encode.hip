// On-device GT encoding: greedy unique anchor assignment + regression targets +
// the dense [A][C+9] gt tensor, one workgroup per image.
//
// Reference (CPU, Python double loop with an argsort over all anchors per box, inside DataLoader workers):
// compute_deltas src/utils/boxes.py:84-135 (compute_overlaps :70-81, xyxy_to_xywh :12-23, xywh_to_xyxy :26-34),
// BaseDataset.prepare_annotations src/datasets/base.py:61-76.
//
// Arithmetic mirrors numpy's promotion in the reference exactly: boxes are float32 (KITTI.load_annotations +
// resize, float32 in place), anchors float64 (generate_anchors).  So
//   boxes_xywh   = float32 arithmetic ((x1+x2)/2, x2-x1+1)                                   boxes.py:17-22
//   anchors_xyxy = float64                                                                    boxes.py:29-34
//   overlaps     = float64, except the box area (box[2]-box[0])*(box[3]-box[1]) which is a float32 scalar product
//   dist         = float64 sum over (cx,cy,w,h) of squares, left to right (numpy's order for 4 addends)
//   deltas       = float64 expression, rounded to float32 when stored (np.array(..., dtype=float32))
// Built with -ffp-contract=off, so no fma contraction changes a result bit.
//
// Selection rule: for box i (in input order) the free anchor with the largest overlap if that overlap is > 0, else
// the free anchor with the smallest distance; an anchor is taken once.  Ties -> lowest anchor index (the reference
// leaves ties to numpy's unstable argsort; see tests/golden/make_golden_gt.py).
#include "sqd_common.h"

struct GtArgs {
  const float* boxes;        // [total][4] xyxy float32
  const int* class_ids;      // [total]
  const int* box_offsets;    // [B+1]
  const double* anchors;     // [A][4] cx,cy,w,h float64
  float* gt;                 // [B][A][C+9] or null
  int* anchor_idx;           // [total] or null
  float* deltas;             // [total][4] or null
  int B, A, C;
  const void* cand;          // GtCand [total] from gt_candidates_kernel, or null (every box scans with the taken mask)
};

struct Cand { double ov; double dist; int ov_idx; int dist_idx; };

__device__ __forceinline__ void cand_merge(Cand& c, double ov, int oi, double d, int di) {
  if (ov > c.ov || (ov == c.ov && oi < c.ov_idx)) { c.ov = ov; c.ov_idx = oi; }
  if (d < c.dist || (d == c.dist && di < c.dist_idx)) { c.dist = d; c.dist_idx = di; }
}

constexpr int GT_THREADS = 1024;

// First-choice pass (fully parallel, one workgroup per box): best overlap / nearest anchor over ALL anchors, ignoring the
// taken set.  The serial pass below accepts a box's first choice whenever that anchor is still free (masked arg-max =
// unmasked arg-max then) and only re-scans with the mask on a conflict, which is rare in real annotations.
struct GtCand { double ov; int ov_idx; int dist_idx; };

__global__ __launch_bounds__(256) void gt_candidates_kernel(const float* __restrict__ boxes, const double* __restrict__ anchors,
                                                            GtCand* __restrict__ cand, int A) {
  __shared__ Cand wave_c[4];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float b0 = boxes[4 * i], b1 = boxes[4 * i + 1], b2 = boxes[4 * i + 2], b3 = boxes[4 * i + 3];
  const float bcx = (b0 + b2) / 2.f, bcy = (b1 + b3) / 2.f, bw = b2 - b0 + 1.f, bh = b3 - b1 + 1.f;
  const double barea = (double)((b2 - b0) * (b3 - b1));
  Cand c; c.ov = -1.0; c.ov_idx = 0x7fffffff; c.dist = __builtin_inf(); c.dist_idx = 0x7fffffff;
  for (int j = tid; j < A; j += 256) {
    const double ax = anchors[4 * j], ay = anchors[4 * j + 1], aw = anchors[4 * j + 2], ah = anchors[4 * j + 3];
    const double x0 = ax - 0.5 * (aw - 1.0), y0 = ay - 0.5 * (ah - 1.0);
    const double x1 = ax + 0.5 * (aw - 1.0), y1 = ay + 0.5 * (ah - 1.0);
    const double lr = fmax(fmin(x1, (double)b2) - fmax(x0, (double)b0), 0.0);
    const double tb = fmax(fmin(y1, (double)b3) - fmax(y0, (double)b1), 0.0);
    const double inter = lr * tb;
    const double uni = (x1 - x0) * (y1 - y0) + barea - inter;
    const double ov = inter / (uni + 1e-10);
    const double d0 = (double)bcx - ax, d1 = (double)bcy - ay, d2 = (double)bw - aw, d3 = (double)bh - ah;
    const double dist = ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
    cand_merge(c, ov, j, dist, j);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(c.ov, off), d = __shfl_xor(c.dist, off);
    const int oi = __shfl_xor(c.ov_idx, off), di = __shfl_xor(c.dist_idx, off);
    cand_merge(c, ov, oi, d, di);
  }
  if (lane == 0) wave_c[wv] = c;
  __syncthreads();
  if (tid == 0) {
    Cand r = wave_c[0];
    for (int w = 1; w < 4; ++w) cand_merge(r, wave_c[w].ov, wave_c[w].ov_idx, wave_c[w].dist, wave_c[w].dist_idx);
    GtCand o; o.ov = r.ov; o.ov_idx = r.ov_idx; o.dist_idx = r.dist_idx;
    cand[i] = o;
  }
}

__global__ __launch_bounds__(GT_THREADS) void encode_gt_kernel(GtArgs a) {
  extern __shared__ unsigned taken[];                  // A bits
  __shared__ Cand wave_c[GT_THREADS / 64];
  constexpr int MAXB = 256;                            // boxes / first choices of the image staged in LDS
  __shared__ float s_box[MAXB][4];
  __shared__ GtCand s_cand[MAXB];
  __shared__ int s_next;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int row = a.C + 9;
  const int nwords = (a.A + 31) >> 5;
  const int beg = a.box_offsets[b], end = a.box_offsets[b + 1];
  for (int i = tid; i < nwords; i += GT_THREADS) taken[i] = 0u;
  for (int i = tid; i < MAXB && beg + i < end; i += GT_THREADS) {
    s_box[i][0] = a.boxes[4 * (beg + i)]; s_box[i][1] = a.boxes[4 * (beg + i) + 1];
    s_box[i][2] = a.boxes[4 * (beg + i) + 2]; s_box[i][3] = a.boxes[4 * (beg + i) + 3];
    if (a.cand) s_cand[i] = ((const GtCand*)a.cand)[beg + i];
  }
  if (a.gt) {                                          // zero the image's dense gt (16-B stores)
    float* g = a.gt + (long long)b * a.A * row;
    const long long n = (long long)a.A * row;
    const long long n4 = ((reinterpret_cast<uintptr_t>(g) & 15) == 0) ? n / 4 : 0;
    for (long long i = tid; i < n4; i += GT_THREADS) reinterpret_cast<f32x4*>(g)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (long long i = n4 * 4 + tid; i < n; i += GT_THREADS) g[i] = 0.f;
  }
  __syncthreads();
  auto box_of = [&](int i, float (&bx)[4]) {
    if (i - beg < MAXB) { bx[0] = s_box[i - beg][0]; bx[1] = s_box[i - beg][1]; bx[2] = s_box[i - beg][2]; bx[3] = s_box[i - beg][3]; }
    else { bx[0] = a.boxes[4 * i]; bx[1] = a.boxes[4 * i + 1]; bx[2] = a.boxes[4 * i + 2]; bx[3] = a.boxes[4 * i + 3]; }
  };
  // thread 0 only: anchor `pick` goes to box i -- taken bit, regression targets, dense row, index
  auto commit = [&](int i, int pick, const float (&bx)[4]) {
    if (pick >= 0) {
      taken[pick >> 5] |= 1u << (pick & 31);
      const float bcx = (bx[0] + bx[2]) / 2.f, bcy = (bx[1] + bx[3]) / 2.f, bw = bx[2] - bx[0] + 1.f, bh = bx[3] - bx[1] + 1.f;
      const double ax = a.anchors[4 * pick], ay = a.anchors[4 * pick + 1], aw = a.anchors[4 * pick + 2], ah = a.anchors[4 * pick + 3];
      const float dx = (float)(((double)bcx - ax) / aw), dy = (float)(((double)bcy - ay) / ah);
      const float dw = (float)log((double)bw / aw), dh = (float)log((double)bh / ah);
      if (a.deltas) { float* d = a.deltas + 4 * (long long)i; d[0] = dx; d[1] = dy; d[2] = dw; d[3] = dh; }
      if (a.gt) {
        float* g = a.gt + ((long long)b * a.A + pick) * row;
        g[0] = 1.f; g[1] = bx[0]; g[2] = bx[1]; g[3] = bx[2]; g[4] = bx[3]; g[5] = dx; g[6] = dy; g[7] = dw; g[8] = dh;
        const int cls = a.class_ids[i];
        if (cls >= 0 && cls < a.C) g[9 + cls] = 1.f;
      }
    }
    if (a.anchor_idx) a.anchor_idx[i] = pick >= 0 ? pick : a.A;     // reference's "unassigned" value is num_anchors
  };
  int i = beg;
  while (i < end) {
    if (a.cand) {
      // thread 0 walks the boxes whose first choice is still free (no scan, no barrier per box) up to the first conflict
      if (tid == 0) {
        int k = i;
        for (; k < end; ++k) {
          const GtCand fc = (k - beg < MAXB) ? s_cand[k - beg] : ((const GtCand*)a.cand)[k];
          const int want = fc.ov > 0.0 ? fc.ov_idx : fc.dist_idx;
          if (want < 0 || want >= a.A || (taken[want >> 5] & (1u << (want & 31)))) break;
          float bx[4]; box_of(k, bx);
          commit(k, want, bx);
        }
        s_next = k;
      }
      __syncthreads();
      i = s_next;
      if (i >= end) break;
    }
    // ---- box i: scan all anchors with the taken mask (every box when there is no first-choice pass, else a conflict) ----
    float bx[4]; box_of(i, bx);
    const float b0 = bx[0], b1 = bx[1], b2 = bx[2], b3 = bx[3];
    const float bcx = (b0 + b2) / 2.f, bcy = (b1 + b3) / 2.f, bw = b2 - b0 + 1.f, bh = b3 - b1 + 1.f;
    const double barea = (double)((b2 - b0) * (b3 - b1));
    Cand c; c.ov = -1.0; c.ov_idx = 0x7fffffff; c.dist = __builtin_inf(); c.dist_idx = 0x7fffffff;
    for (int j = tid; j < a.A; j += GT_THREADS) {
      if (taken[j >> 5] & (1u << (j & 31))) continue;
      const double ax = a.anchors[4 * j], ay = a.anchors[4 * j + 1], aw = a.anchors[4 * j + 2], ah = a.anchors[4 * j + 3];
      const double x0 = ax - 0.5 * (aw - 1.0), y0 = ay - 0.5 * (ah - 1.0);
      const double x1 = ax + 0.5 * (aw - 1.0), y1 = ay + 0.5 * (ah - 1.0);
      const double lr = fmax(fmin(x1, (double)b2) - fmax(x0, (double)b0), 0.0);
      const double tb = fmax(fmin(y1, (double)b3) - fmax(y0, (double)b1), 0.0);
      const double inter = lr * tb;
      const double uni = (x1 - x0) * (y1 - y0) + barea - inter;
      const double ov = inter / (uni + 1e-10);
      const double d0 = (double)bcx - ax, d1 = (double)bcy - ay, d2 = (double)bw - aw, d3 = (double)bh - ah;
      const double dist = ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
      cand_merge(c, ov, j, dist, j);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double ov = __shfl_xor(c.ov, off), d = __shfl_xor(c.dist, off);
      const int oi = __shfl_xor(c.ov_idx, off), di = __shfl_xor(c.dist_idx, off);
      cand_merge(c, ov, oi, d, di);
    }
    if (lane == 0) wave_c[wv] = c;
    __syncthreads();
    if (tid == 0) {
      Cand r = wave_c[0];
      for (int w = 1; w < GT_THREADS / 64; ++w) cand_merge(r, wave_c[w].ov, wave_c[w].ov_idx, wave_c[w].dist, wave_c[w].dist_idx);
      int pick = (r.ov > 0.0) ? r.ov_idx : r.dist_idx;
      if (pick == 0x7fffffff) pick = -1;               // more boxes than anchors: nothing free
      commit(i, pick, bx);
    }
    __syncthreads();
    ++i;
  }
}

// boxes [total][4] xyxy fp32 (network-input coordinates), class_ids [total] int32, box_offsets [B+1] int32 (image b
// owns boxes box_offsets[b] .. box_offsets[b+1]-1, in the order the reference would iterate them), anchors [A][4]
// float64 (cx,cy,w,h).  Outputs (each may be NULL): gt [B][A][C+9] dense (fully overwritten), anchor_idx [total]
// int32, deltas [total][4] fp32.  All pointers are device pointers.
// workspace: 16 * total_boxes bytes of device memory (total_boxes given by the caller) or NULL; with it a fully parallel
// first-choice pass runs first and the serial pass only re-scans on conflicts (same results, several times faster).
extern "C" int sqd_encode_gt_fwd(const float* boxes, const int* class_ids, const int* box_offsets, const double* anchors,
                                 float* gt, int* anchor_idx, float* deltas, void* workspace, int total_boxes, int B, int A,
                                 int num_classes, void* stream) {
  SQD_CHECK_ARG(box_offsets && anchors && B > 0 && A > 0 && A <= (1 << 20) && num_classes > 0);
  SQD_CHECK_ARG(gt || anchor_idx || deltas);
  SQD_CHECK_ARG(!gt || class_ids);
  GtArgs a;
  a.boxes = boxes; a.class_ids = class_ids; a.box_offsets = box_offsets; a.anchors = anchors;
  a.gt = gt; a.anchor_idx = anchor_idx; a.deltas = deltas; a.B = B; a.A = A; a.C = num_classes;
  a.cand = nullptr;
  if (workspace && total_boxes > 0 && boxes) {
    SQD_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && total_boxes <= (1 << 24));
    hipLaunchKernelGGL(gt_candidates_kernel, dim3((unsigned)total_boxes), dim3(256), 0, (hipStream_t)stream, boxes, anchors,
                       (GtCand*)workspace, A);
    a.cand = workspace;
  }
  const size_t lds = (size_t)((A + 31) / 32) * sizeof(unsigned);
  if (lds > 48 * 1024 &&
      hipFuncSetAttribute((const void*)encode_gt_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return SQD_ERR_LAUNCH;
  hipLaunchKernelGGL(encode_gt_kernel, dim3((unsigned)B), dim3(GT_THREADS), lds, (hipStream_t)stream, a);
  return sqd_launch_status();
}

// ---- anchor ignore bitmap: which anchors lie on an ignore region (KITTI DontCare, VOC difficult, COCO crowd) ---------------------------
// Bit a of image b is set iff area > 0 and inter >= overlap * area for SOME ignore box of the image, with the anchor corners the
// encoder above uses, inter the intersection with the box and area the ANCHOR's area: intersection over anchor area, the per-box
// maximum.  (An IoU would never fire for a small anchor inside a large region.)  All float64 and no division, so a numpy float64
// restatement gives the same bits (boxes.anchor_ignore_mask).  One thread per anchor, grid (ceil(A / 256), B); the image's boxes pass
// through LDS in chunks of IGN_THREADS; a wave's 64 results leave as two ballot words, so every word of mask [B][ceil(A / 32)] is
// written (bits at and past A are 0) and the caller needs no memset.
constexpr int IGN_THREADS = 256;
constexpr int IGN_MAX_BOXES = 65535;                   // ignore boxes per image

__global__ __launch_bounds__(IGN_THREADS) void anchor_ignore_kernel(const float* __restrict__ boxes, const int* __restrict__ offsets,
                                                                    const double* __restrict__ anchors, unsigned* __restrict__ mask,
                                                                    double overlap, int total, int A) {
  __shared__ float s_box[IGN_THREADS][4];
  const int b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * IGN_THREADS + tid;
  const int beg = max(0, offsets[b]), end = min(total, offsets[b + 1]);      // (a malformed table reads nothing out of bounds)
  double x0 = 0.0, y0 = 0.0, x1 = 0.0, y1 = 0.0, area = 0.0;
  if (i < A) {
    const double ax = anchors[4 * i], ay = anchors[4 * i + 1], aw = anchors[4 * i + 2], ah = anchors[4 * i + 3];
    x0 = ax - 0.5 * (aw - 1.0); y0 = ay - 0.5 * (ah - 1.0);
    x1 = ax + 0.5 * (aw - 1.0); y1 = ay + 0.5 * (ah - 1.0);
    area = (x1 - x0) * (y1 - y0);
  }
  const bool live = i < A && area > 0.0;
  bool hit = false;
  for (int c = beg; c < end; c += IGN_THREADS) {        // (block-uniform)
    const int n = min(IGN_THREADS, end - c);
    __syncthreads();
    if (tid < n) {
      const float* bx = boxes + 4 * (long long)(c + tid);
      s_box[tid][0] = bx[0]; s_box[tid][1] = bx[1]; s_box[tid][2] = bx[2]; s_box[tid][3] = bx[3];
    }
    __syncthreads();
    if (live && !hit) {
      for (int k = 0; k < n; ++k) {
        const double lr = fmax(fmin(x1, (double)s_box[k][2]) - fmax(x0, (double)s_box[k][0]), 0.0);
        const double tb = fmax(fmin(y1, (double)s_box[k][3]) - fmax(y0, (double)s_box[k][1]), 0.0);
        if (lr * tb >= overlap * area) hit = true;
      }
    }
  }
  const unsigned long long bal = __ballot(hit);
  const int lane = tid & 63, nwords = (A + 31) >> 5;
  const int w0 = (blockIdx.x * IGN_THREADS + (tid & ~63)) >> 5;
  unsigned* row = mask + (long long)b * nwords;
  if (lane == 0 && w0 < nwords) row[w0] = (unsigned)(bal & 0xffffffffull);
  if (lane == 32 && w0 + 1 < nwords) row[w0 + 1] = (unsigned)(bal >> 32);
}

// ign_boxes [total][4] xyxy fp32 (network-input coordinates), ign_offsets [B+1] int32, anchors [A][4] float64 (cx,cy,w,h), mask
// uint32 [B][ceil(A/32)] (anchor a: word a >> 5, bit a & 31) -- device pointers; overlap: HOST pointer to one double in (0, 1].
// total = 0 (ign_boxes may then be NULL) and images without boxes are legal and give zero words.  Status 1 for anything malformed, 2
// for A > 2^20, B > 65535 or more boxes than 65535 per image can hold.
extern "C" int sqd_anchor_ignore_fwd(const float* ign_boxes, const int* ign_offsets, const double* anchors, unsigned* mask,
                                     const double* overlap, int total, int B, int A, void* stream) {
  SQD_CHECK_ARG(ign_offsets && anchors && mask && overlap && B > 0 && A > 0 && total >= 0);
  SQD_CHECK_ARG(total == 0 || ign_boxes);
  SQD_CHECK_ARG(*overlap > 0.0 && *overlap <= 1.0);
  if (A > (1 << 20) || B > 65535 || (long long)total > (long long)IGN_MAX_BOXES * B) return SQD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(anchor_ignore_kernel, dim3((unsigned)sqd_cdiv(A, IGN_THREADS), (unsigned)B), dim3(IGN_THREADS), 0,
                     (hipStream_t)stream, ign_boxes, ign_offsets, anchors, mask, *overlap, total, A);
  return sqd_launch_status();
}

// ---- IoU-threshold matching: extra positives and an ignore band on top of the greedy assignment -----------------------------------------
// The encoder above gives every box ONE anchor (its primary).  Here every other anchor j of the image is scored against the image's boxes
// with the encoder's own overlap expression (float64; the box area a float32 product, widened afterwards; inter / (union + 1e-10)):
//   m = max_i ov(i, j), i* = the LOWEST box index that attains it;  m >= pos_iou: j is an EXTRA positive of box i*;  else m >= ign_iou: j
//   is a BAND anchor (left out of the loss);  else a negative.  A primary is never re-assigned; an image without boxes has neither.
// The first max_extra extras of an image by ascending anchor index are kept, the rest are OVERFLOW and leave the loss with the band.
// Output list, a fixed total + B * max_extra entries, image b at out_offsets[b] = box_offsets[b] + b * max_extra: its primaries in box
// order (index, box, deltas, class copied; an unassigned one keeps A and gets zero deltas, which the encoder leaves unwritten), the kept
// extras in ascending anchor order (deltas by commit's arithmetic above), then padding (index A, zeros).  ignore_out = ignore_in | band |
// overflow, every word written, bits at and past A zero; overflow [B] = the overflow anchors per image.
//
// Two launches after the encoder's (one workgroup per image would leave most CUs idle at B = 20, and the scoring is the A x n part):
//   anchor_match_score_kernel    grid (ceil(A / 256), B), one thread per anchor: the image's boxes pass through LDS in chunks, the slice's
//                                primaries are marked in an LDS bitmap from anchor_idx; out: the best box per extra anchor (-1 otherwise),
//                                the band bits by wave ballot, the extras of the block in a count table.
//   anchor_match_compact_kernel  one workgroup per image: wave 0 scans the count table, then every wave walks whole 256-anchor blocks
//                                (skipping those without extras) and ranks its extras by ballot + popcount -- no barrier in the walk, no
//                                atomics anywhere: each ignore word is touched by one lane, each list entry written by one thread.
constexpr int AM_THREADS = 256;                        // anchors per scoring block = the granule of the count table
constexpr int AM_CHUNK = 256;                          // boxes staged per LDS pass
constexpr int AM_CTHREADS = 1024;
constexpr int AM_MAX_BLOCKS = (1 << 20) / AM_THREADS;  // A <= 2^20

struct MatchArgs {
  const float* boxes; const int* class_ids; const int* box_offsets; const int* anchor_idx; const float* deltas;
  const double* anchors; const unsigned* ignore_in;
  int* best; int* counts;                              // workspace: [B][A], [B][nblk]
  int* out_idx; float* out_boxes; float* out_deltas; int* out_cls; int* out_offsets;
  unsigned* ignore_out; int* overflow;
  double pos_iou, ign_iou;
  int total, B, A, max_extra, nblk;
};

__global__ __launch_bounds__(AM_THREADS) void anchor_match_score_kernel(MatchArgs a) {
  __shared__ double s_box[AM_CHUNK][5];                // x1, y1, x2, y2 widened, and the float32 area widened
  __shared__ unsigned s_prim[AM_THREADS / 32];
  __shared__ int s_cnt[AM_THREADS / 64];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, base = blockIdx.x * AM_THREADS, j = base + tid;
  const int beg = max(0, a.box_offsets[b]), end = min(a.total, a.box_offsets[b + 1]);      // (a malformed table reads nothing out of bounds)
  if (tid < AM_THREADS / 32) s_prim[tid] = 0u;
  __syncthreads();
  for (int i = beg + tid; i < end; i += AM_THREADS) {
    const int p = a.anchor_idx[i] - base;
    if (p >= 0 && p < AM_THREADS) atomicOr(&s_prim[p >> 5], 1u << (p & 31));               // (integer: order-free)
  }
  double x0 = 0.0, y0 = 0.0, x1 = 0.0, y1 = 0.0, aarea = 0.0;
  if (j < a.A) {
    const double ax = a.anchors[4 * j], ay = a.anchors[4 * j + 1], aw = a.anchors[4 * j + 2], ah = a.anchors[4 * j + 3];
    x0 = ax - 0.5 * (aw - 1.0); y0 = ay - 0.5 * (ah - 1.0);
    x1 = ax + 0.5 * (aw - 1.0); y1 = ay + 0.5 * (ah - 1.0);
    aarea = (x1 - x0) * (y1 - y0);
  }
  double m = -1.0;
  int bi = -1;
  for (int c = beg; c < end; c += AM_CHUNK) {           // (block-uniform)
    const int n = min(AM_CHUNK, end - c);
    __syncthreads();
    if (tid < n) {
      const float* bx = a.boxes + 4 * (long long)(c + tid);
      const float b0 = bx[0], b1 = bx[1], b2 = bx[2], b3 = bx[3];
      s_box[tid][0] = (double)b0; s_box[tid][1] = (double)b1; s_box[tid][2] = (double)b2; s_box[tid][3] = (double)b3;
      s_box[tid][4] = (double)((b2 - b0) * (b3 - b1));
    }
    __syncthreads();
    if (j < a.A) {
      for (int k = 0; k < n; ++k) {
        const double lr = fmax(fmin(x1, s_box[k][2]) - fmax(x0, s_box[k][0]), 0.0);
        const double tb = fmax(fmin(y1, s_box[k][3]) - fmax(y0, s_box[k][1]), 0.0);
        const double inter = lr * tb;
        const double uni = aarea + s_box[k][4] - inter;
        const double ov = inter / (uni + 1e-10);
        if (ov > m) { m = ov; bi = c + k; }             // strict: ties stay with the lowest box index
      }
    }
  }
  __syncthreads();                                      // (s_prim complete also for an image whose boxes skipped the loop's barriers)
  const bool scored = j < a.A && bi >= 0 && !(s_prim[tid >> 5] & (1u << (tid & 31)));
  const bool extra = scored && m >= a.pos_iou;
  const bool band = scored && !extra && m >= a.ign_iou;
  if (j < a.A) a.best[(long long)b * a.A + j] = extra ? bi : -1;
  const unsigned long long bal = __ballot(band), ebal = __ballot(extra);
  const int nwords = (a.A + 31) >> 5, w0 = (base + (tid & ~63)) >> 5;
  const long long row = (long long)b * nwords;
  if (lane == 0 && w0 < nwords) a.ignore_out[row + w0] = (unsigned)(bal & 0xffffffffull) | (a.ignore_in ? a.ignore_in[row + w0] : 0u);
  if (lane == 32 && w0 + 1 < nwords) a.ignore_out[row + w0 + 1] = (unsigned)(bal >> 32) | (a.ignore_in ? a.ignore_in[row + w0 + 1] : 0u);
  if (lane == 0) s_cnt[tid >> 6] = __popcll(ebal);
  __syncthreads();
  if (tid == 0) a.counts[(long long)b * a.nblk + blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ __launch_bounds__(AM_CTHREADS) void anchor_match_compact_kernel(MatchArgs a) {
  __shared__ int s_pref[AM_MAX_BLOCKS + 1];            // exclusive prefix of the image's block counts, [nblk] = the image's extras
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int beg = max(0, a.box_offsets[b]), end = max(beg, min(a.total, a.box_offsets[b + 1]));
  const int nb = end - beg;
  const long long out0 = (long long)beg + (long long)b * a.max_extra;     // (beg <= total: a malformed table writes nothing out of bounds)
  const int* cnt = a.counts + (long long)b * a.nblk;
  if (wv == 0) {                                        // the scan: a contiguous run of the table per lane, then across the lanes
    const int per = (a.nblk + 63) / 64, q0 = min(a.nblk, lane * per), q1 = min(a.nblk, q0 + per);
    int s = 0;
    for (int q = q0; q < q1; ++q) s += cnt[q];
    int inc = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int v = __shfl_up(inc, off);
      if (lane >= off) inc += v;
    }
    int run = inc - s;
    for (int q = q0; q < q1; ++q) { s_pref[q] = run; run += cnt[q]; }
    if (lane == 63) s_pref[a.nblk] = inc;
  }
  __syncthreads();
  const int E = s_pref[a.nblk], kept = min(E, a.max_extra);
  if (tid == 0) {
    a.overflow[b] = E - kept;
    a.out_offsets[b] = (int)out0;
    if (b == a.B - 1) a.out_offsets[a.B] = a.total + a.B * a.max_extra;
  }
  // the primaries, in box order
  for (int i = tid; i < nb; i += AM_CTHREADS) {
    const long long src = beg + i, dst = out0 + i;
    const int idx = a.anchor_idx[src];
    const bool assigned = idx >= 0 && idx < a.A;
    a.out_idx[dst] = idx;
    a.out_cls[dst] = a.class_ids[src];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a.out_boxes[4 * dst + k] = a.boxes[4 * src + k];
      a.out_deltas[4 * dst + k] = assigned ? a.deltas[4 * src + k] : 0.f;
    }
  }
  // padding
  for (int i = kept + tid; i < a.max_extra; i += AM_CTHREADS) {
    const long long dst = out0 + nb + i;
    a.out_idx[dst] = a.A; a.out_cls[dst] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { a.out_boxes[4 * dst + k] = 0.f; a.out_deltas[4 * dst + k] = 0.f; }
  }
  if (E == 0) return;                                   // (block-uniform)
  // the extras: wave wv takes the 256-anchor blocks wv, wv + 16, ...; rank = the block's prefix + the extras before it in the block
  const int nwords = (a.A + 31) >> 5;
  unsigned* irow = a.ignore_out + (long long)b * nwords;
  const int* best = a.best + (long long)b * a.A;
  for (int q = wv; q < a.nblk; q += AM_CTHREADS / 64) {
    int run = s_pref[q];
    if (s_pref[q + 1] == run) continue;                 // (wave-uniform)
    for (int s = 0; s < AM_THREADS / 64; ++s) {
      const int j = q * AM_THREADS + s * 64 + lane;
      const int bi = j < a.A ? best[j] : -1;
      const bool ex = bi >= 0 && bi < a.total;
      const unsigned long long bal = __ballot(ex);
      const int r = run + __popcll(bal & ((1ull << lane) - 1ull));
      const bool over = ex && r >= a.max_extra;
      if (ex && !over) {
        const long long dst = out0 + nb + r;
        const float b0 = a.boxes[4 * (long long)bi], b1 = a.boxes[4 * (long long)bi + 1];
        const float b2 = a.boxes[4 * (long long)bi + 2], b3 = a.boxes[4 * (long long)bi + 3];
        const float bcx = (b0 + b2) / 2.f, bcy = (b1 + b3) / 2.f, bw = b2 - b0 + 1.f, bh = b3 - b1 + 1.f;
        const double ax = a.anchors[4 * j], ay = a.anchors[4 * j + 1], aw = a.anchors[4 * j + 2], ah = a.anchors[4 * j + 3];
        a.out_idx[dst] = j; a.out_cls[dst] = a.class_ids[bi];
        a.out_boxes[4 * dst] = b0; a.out_boxes[4 * dst + 1] = b1; a.out_boxes[4 * dst + 2] = b2; a.out_boxes[4 * dst + 3] = b3;
        a.out_deltas[4 * dst] = (float)(((double)bcx - ax) / aw); a.out_deltas[4 * dst + 1] = (float)(((double)bcy - ay) / ah);
        a.out_deltas[4 * dst + 2] = (float)log((double)bw / aw); a.out_deltas[4 * dst + 3] = (float)log((double)bh / ah);
      }
      const unsigned long long obal = __ballot(over);
      const int w0 = (q * AM_THREADS + s * 64) >> 5;    // this wave step's two words: no other lane of the launch touches them
      if (lane == 0 && w0 < nwords && (unsigned)(obal & 0xffffffffull)) irow[w0] |= (unsigned)(obal & 0xffffffffull);
      if (lane == 32 && w0 + 1 < nwords && (unsigned)(obal >> 32)) irow[w0 + 1] |= (unsigned)(obal >> 32);
      run += __popcll(bal);
    }
  }
}

// boxes [total][4] fp32 xyxy, class_ids [total], box_offsets [B+1] and the encoder's anchor_idx [total] / deltas [total][4] for them;
// anchors [A][4] float64; ignore_in uint32 [B][ceil(A/32)] or NULL -- device pointers.  thresholds: HOST pointer to two doubles
// (pos_iou, ign_iou), 0 < ign_iou <= pos_iou <= 1.  workspace: 4 * B * (A + ceil(A / 256)) bytes of device memory.  Outputs (device):
// out_anchor_idx / out_class_ids [total + B * max_extra], out_boxes / out_deltas [..][4], out_offsets [B+1], ignore_out uint32
// [B][ceil(A/32)] (may be ignore_in itself: a word is read and written by one lane of the first launch), overflow int32 [B].  Everything
// is written.  Status 1 for anything malformed, 2 for A > 2^20, B > 65535 or total + B * max_extra >= 2^31 (include/sqd_hip.h).
extern "C" int sqd_anchor_match_fwd(const float* boxes, const int* class_ids, const int* box_offsets, const int* anchor_idx,
                                    const float* deltas, const double* anchors, const unsigned* ignore_in, const double* thresholds,
                                    void* workspace, int* out_anchor_idx, float* out_boxes, float* out_deltas, int* out_class_ids,
                                    int* out_offsets, unsigned* ignore_out, int* overflow, int total, int B, int A, int max_extra,
                                    void* stream) {
  SQD_CHECK_ARG(box_offsets && anchors && thresholds && workspace && out_offsets && ignore_out && overflow);
  SQD_CHECK_ARG(B > 0 && A > 0 && total >= 0 && max_extra >= 0);
  SQD_CHECK_ARG(total == 0 || (boxes && class_ids && anchor_idx && deltas));
  SQD_CHECK_ARG(thresholds[1] > 0.0 && thresholds[1] <= thresholds[0] && thresholds[0] <= 1.0);     // (NaN fails)
  if (A > (1 << 20) || B > 65535 || (long long)total + (long long)B * max_extra >= (1ll << 31)) return SQD_ERR_UNSUPPORTED;
  SQD_CHECK_ARG((total == 0 && max_extra == 0) || (out_anchor_idx && out_boxes && out_deltas && out_class_ids));
  SQD_CHECK_ARG(((uintptr_t)workspace & 3) == 0);
  MatchArgs a;
  a.boxes = boxes; a.class_ids = class_ids; a.box_offsets = box_offsets; a.anchor_idx = anchor_idx; a.deltas = deltas;
  a.anchors = anchors; a.ignore_in = ignore_in;
  a.nblk = sqd_cdiv(A, AM_THREADS);
  a.best = (int*)workspace; a.counts = a.best + (long long)B * A;
  a.out_idx = out_anchor_idx; a.out_boxes = out_boxes; a.out_deltas = out_deltas; a.out_cls = out_class_ids; a.out_offsets = out_offsets;
  a.ignore_out = ignore_out; a.overflow = overflow;
  a.pos_iou = thresholds[0]; a.ign_iou = thresholds[1];
  a.total = total; a.B = B; a.A = A; a.max_extra = max_extra;
  hipLaunchKernelGGL(anchor_match_score_kernel, dim3((unsigned)a.nblk, (unsigned)B), dim3(AM_THREADS), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(anchor_match_compact_kernel, dim3((unsigned)B), dim3(AM_CTHREADS), 0, (hipStream_t)stream, a);
  return sqd_launch_status();
}
