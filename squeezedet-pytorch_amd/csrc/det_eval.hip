// Detection AP on the device for any class count (DESIGN.md "Detection AP on the device"): the VOC / COCO style metric computed from
// the packed output of the fused detect launches and the ground truth that is already on the device.  Two kernels: the MATCH kernel
// labels every detection slot of a batch as true positive / false positive / ignored / empty at each IoU threshold; the AP kernel turns
// the accumulated, ordered labels of a whole dataset into per class and threshold average precision.
//
// Matching rule (pycocotools' greedy rule, with every ignored GT allowed to absorb any number of detections), per image b, class c and
// threshold t:
//   * the detections of class c are visited in descending score; among equal scores the lower slot k goes first (the detect output
//     is not assumed to be sorted; scores are compared as floats with -0 = +0 and a NaN below everything);
//   * a detection takes the UNCLAIMED, NON-IGNORED GT of class c in image b with the highest IoU (equal IoU: the lowest GT index);
//     if that IoU >= t it is a true positive and the GT is claimed at this t;
//   * otherwise, if some IGNORED GT of class c has IoU >= t, the detection is ignored and matched_gt names that GT (highest IoU,
//     lowest index); an ignored GT is never claimed;
//   * otherwise it is a false positive.
// A detection whose class id lies outside [0, num_classes) is a false positive at every t; a GT whose class id lies outside that
// range is matched by nothing and not counted.  IoU in float64 from the fp32 coordinates, no "+1" pixel convention, in this order
// (the Makefile's -ffp-contract=off keeps it free of fused multiply-adds, so a numpy float64 restatement gives the same bits):
//   area = (x2 - x1) * (y2 - y1);  iw = max(0, min(x2a, x2b) - max(x1a, x1b)), ih likewise;  inter = iw * ih;
//   uni = (area_a + area_b) - inter;  iou = uni > 0 ? inter / uni : 0.
//
// Match kernel: one workgroup of 1024 threads per image; all sizes below are constants, the result does not depend on a launch
// geometry.
//   1. The detections are ordered by (class, score descending, slot) by counting, in LDS; a histogram gives each class its segment.
//   2. Phase A, every detection on its own (a wave per detection, rounds of 16): the lanes stride over the image's GT -- staged
//      through LDS in chunks of 256, any number of GT up to 65 535 -- and reduce to the detection's FIRST candidate (the best
//      non-ignored GT of its class) and its best ignored GT.  Neither depends on claims.
//   3. Phase B, the claim walk, serial along a class's segment and parallel over classes and thresholds: step s settles the s-th
//      detection of every class that has one, a wave per detection, lane t < T owning threshold t.  Claims are not kept per GT (nothing
//      here is sized by the GT count): the GT a detection claimed at threshold t is stored with the DETECTION, mt[position][t] (uint16
//      index within the image: hence 65 535).  The order "IoU descending, index ascending" of the GT of one detection is the same at
//      every t, so candidates are taken in that order, and a lane settles as soon as the candidate's IoU falls below its threshold
//      (not a true positive) or the candidate is not among the claims of the class's earlier detections (true positive).  The first
//      candidate settles every lane unless it was already claimed (a duplicate detection); only then the waves that still have
//      unsettled lanes sweep the GT again for the best candidate strictly after the previous one.  Whether such a sweep is needed is
//      agreed on by the whole workgroup (__syncthreads_or), because chunk staging is shared: one barrier per round in the usual case.
//   4. npos: a per-image histogram in LDS, then one integer atomic add per class with GT.
//
// AP kernel: one workgroup per (class, threshold) over the class's segment of the ordered pool, in chunks of 1024 entries with carries:
// a forward scan of TP / FP counts (ballots; ignored and empty entries count as neither), precision = tp / (tp + fp) and recall =
// tp / npos in float64, a backward running max for the precision envelope, and the integration: mode 0 sums the envelope at every true
// positive and divides by npos (area under the monotone envelope, VOC2010+); modes 1 / 2 sample the envelope at the first position
// whose recall reaches k / 10 (k = 0..10, VOC2007) or k / 100 (k = 0..100, COCO), 0 where none does, and one lane sums the samples in
// index order.  Every thread reads back only the counts it wrote itself.
#include "sqd_common.h"
#include <limits.h>
#include <math.h>

constexpr int DM_THREADS = 1024;
constexpr int DM_WAVES = DM_THREADS / 64;
constexpr int DM_MAX_K = 1024;
constexpr int DM_MAX_T = 16;
constexpr int DM_MAX_C = 256;
constexpr int DM_CHUNK = 256;            // GT per LDS chunk
constexpr int DM_MAX_GT = 65535;         // per image: mt holds uint16 indices, 0xffff = none

__device__ __forceinline__ double dm_iou(double ax1, double ay1, double ax2, double ay2, double area_a, float4 g) {
  const double bx1 = (double)g.x, by1 = (double)g.y, bx2 = (double)g.z, by2 = (double)g.w;
  const double area_b = (bx2 - bx1) * (by2 - by1);
  const double iw = fmax(0.0, fmin(ax2, bx2) - fmax(ax1, bx1));
  const double ih = fmax(0.0, fmin(ay2, by2) - fmax(ay1, by1));
  const double inter = iw * ih;
  const double uni = (area_a + area_b) - inter;
  return uni > 0.0 ? inter / uni : 0.0;
}

// (iou, idx) ranks before (biou, bidx): higher IoU, then lower index
__device__ __forceinline__ bool dm_better(double iou, int idx, double biou, int bidx) {
  return iou > biou || (iou == biou && idx < bidx);
}

__device__ __forceinline__ void dm_wave_best(double& iou, int& idx) {
  for (int off = 32; off > 0; off >>= 1) {
    const double oi = __shfl_xor(iou, off);
    const int ox = __shfl_xor(idx, off);
    if (dm_better(oi, ox, iou, idx)) { iou = oi; idx = ox; }
  }
}

// One wave's sweep over the image's GT for the detection (ax1 .. area_a) of class c: the best non-ignored GT strictly after
// (prev_iou, prev_idx) in the order "IoU descending, index ascending" and, with FIRST, the best ignored GT.  The chunk loop and its
// staging barriers are uniform over the workgroup (waves without work pass active = false); every lane returns the wave's result.
struct DmSweep { double best_iou, ig_iou; int best_idx, ig_idx; };

template <bool FIRST>
__device__ __forceinline__ DmSweep dm_sweep(bool active, int c, double ax1, double ay1, double ax2, double ay2, double area_a,
                                            double prev_iou, int prev_idx, float4* s_gbox, int* s_gcode, const float* __restrict__ gbox,
                                            const int* __restrict__ gcls, const unsigned char* __restrict__ gign, int g0, int ng,
                                            int nchunks, int C) {
  const int tid = threadIdx.x, lane = tid & 63;
  double best_iou = -1.0, ig_iou = -1.0;
  int best_idx = INT_MAX, ig_idx = INT_MAX;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int cn = min(DM_CHUNK, ng - ch * DM_CHUNK);
    if (nchunks > 1) {                                     // (uniform over the workgroup; a single chunk stays staged)
      __syncthreads();
      if (tid < cn) {
        const int gi = g0 + ch * DM_CHUNK + tid, gc = gcls[gi];
        s_gbox[tid] = ((const float4*)gbox)[gi];
        s_gcode[tid] = gc >= 0 && gc < C ? (gc | ((gign && gign[gi]) ? 0x10000 : 0)) : -1;
      }
      __syncthreads();
    }
    if (active) {
      for (int i = lane; i < cn; i += 64) {
        const int code = s_gcode[i];
        if (code < 0 || (code & 0xffff) != c) continue;
        const int gi = ch * DM_CHUNK + i;
        const double iou = dm_iou(ax1, ay1, ax2, ay2, area_a, s_gbox[i]);
        if (code >> 16) {
          if (FIRST && dm_better(iou, gi, ig_iou, ig_idx)) { ig_iou = iou; ig_idx = gi; }
        } else if ((iou < prev_iou || (iou == prev_iou && gi > prev_idx)) && dm_better(iou, gi, best_iou, best_idx)) {
          best_iou = iou; best_idx = gi;
        }
      }
    }
  }
  if (active) {
    dm_wave_best(best_iou, best_idx);
    if (FIRST) dm_wave_best(ig_iou, ig_idx);
  }
  DmSweep r;
  r.best_iou = best_iou; r.ig_iou = ig_iou; r.best_idx = best_idx; r.ig_idx = ig_idx;
  return r;
}

__global__ __launch_bounds__(DM_THREADS) void det_match_kernel(const int* __restrict__ count, const long long* __restrict__ dcls,
                                                               const float* __restrict__ dsc, const float* __restrict__ dbox,
                                                               const float* __restrict__ gbox, const int* __restrict__ gcls,
                                                               const int* __restrict__ goff, const unsigned char* __restrict__ gign,
                                                               const double* __restrict__ thr, unsigned char* __restrict__ flags,
                                                               int* __restrict__ matched, int* __restrict__ npos, int K, int total,
                                                               int T, int C) {
  __shared__ unsigned long long s_key[DM_MAX_K];          // (class << 32) | inverted score key, per slot
  __shared__ unsigned short s_list[DM_MAX_K];             // ordered position -> slot
  __shared__ unsigned short s_bidx[DM_MAX_K], s_iidx[DM_MAX_K];      // ordered position -> first candidate / best ignored GT, 0xffff = none
  extern __shared__ __attribute__((aligned(16))) unsigned char dm_dyn[];
  float4* s_dbox = (float4*)dm_dyn;                                   // slot -> box: K entries
  unsigned short* s_mt = (unsigned short*)(dm_dyn + 16 * (size_t)K);  // (ordered position, t) -> claimed GT (index within the image) or 0xffff
  __shared__ int s_hist[DM_MAX_C + 1], s_start[DM_MAX_C + 2], s_gpos[DM_MAX_C], s_act[DM_MAX_C];
  __shared__ int s_nact;
  __shared__ float4 s_gbox[DM_CHUNK];
  __shared__ int s_gcode[DM_CHUNK];                       // class | ignored << 16, or -1: no valid class
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(max(count[b], 0), K);
  const int g0 = min(max(goff[b], 0), total), g1 = min(max(goff[b + 1], g0), total);
  const int ng = min(g1 - g0, DM_MAX_GT);
  const long long row0 = (long long)b * K;
  const double mythr = lane < T ? thr[lane] : 0.0;

  for (int i = tid; i <= C; i += DM_THREADS) s_hist[i] = 0;
  for (int i = tid; i < C; i += DM_THREADS) s_gpos[i] = 0;
  if (tid == 0) s_nact = 0;
  __syncthreads();
  for (int k = tid; k < K; k += DM_THREADS) {
    if (k < n) {
      const long long cl = dcls[row0 + k];
      const int c = cl >= 0 && cl < C ? (int)cl : C;
      const float s = dsc[row0 + k] + 0.0f;                // -0 -> +0
      const unsigned u = __float_as_uint(s);
      const unsigned skey = s != s ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));      // ascending with the score, NaN lowest
      s_key[k] = ((unsigned long long)c << 32) | (unsigned long long)(0xffffffffu - skey);
      s_dbox[k] = ((const float4*)dbox)[row0 + k];
      atomicAdd(&s_hist[c], 1);
      if (c == C || ng == 0)                               // no valid class, or nothing to match: a false positive
        for (int t = 0; t < T; ++t) { flags[(row0 + k) * T + t] = 0; matched[(row0 + k) * T + t] = -1; }
    } else {
      for (int t = 0; t < T; ++t) { flags[(row0 + k) * T + t] = 3; matched[(row0 + k) * T + t] = -1; }
    }
  }
  for (int i = tid; i < ng; i += DM_THREADS) {
    const int c = gcls[g0 + i];
    if (c >= 0 && c < C && !(gign && gign[g0 + i])) atomicAdd(&s_gpos[c], 1);
  }
  const int nchunks = (ng + DM_CHUNK - 1) / DM_CHUNK;
  if (nchunks == 1 && tid < ng) {                          // the usual case: the image's GT stay in LDS for the whole kernel
    const int c = gcls[g0 + tid];
    s_gbox[tid] = ((const float4*)gbox)[g0 + tid];
    s_gcode[tid] = c >= 0 && c < C ? (c | ((gign && gign[g0 + tid]) ? 0x10000 : 0)) : -1;
  }
  __syncthreads();
  for (int c = tid; c < C; c += DM_THREADS)
    if (s_gpos[c]) atomicAdd(&npos[c], s_gpos[c]);
  if (ng == 0) return;                                     // (uniform)
  for (int k = tid; k < n; k += DM_THREADS) {
    const unsigned long long kk = s_key[k];
    int pos = 0;
    for (int j = 0; j < n; ++j) {
      const unsigned long long kj = s_key[j];
      pos += (kj < kk || (kj == kk && j < k)) ? 1 : 0;
    }
    s_list[pos] = (unsigned short)k;
  }
  // the classes that have detections, by falling count (equal counts: rising class): at step s the ones with a detection left are a
  // prefix of this list
  for (int c = tid; c < C; c += DM_THREADS) {
    const int h = s_hist[c];
    if (h > 0) {
      int r = 0;
      for (int j = 0; j < C; ++j) {
        const int hj = s_hist[j];
        r += (hj > h || (hj == h && j < c)) ? 1 : 0;
      }
      s_act[r] = c;
      atomicAdd(&s_nact, 1);
    }
  }
  if (tid == 0) {
    int acc = 0;
    for (int c = 0; c <= C; ++c) { s_start[c] = acc; acc += s_hist[c]; }
    s_start[C + 1] = acc;
  }
  __syncthreads();
  const int nvalid = s_start[C], nact = s_nact;

  // phase A, every detection on its own: its first candidate and its best ignored GT (neither depends on claims)
  for (int base = 0; base < nvalid; base += DM_WAVES) {
    const int pos = base + wave;
    const bool has = pos < nvalid;
    const int k = has ? (int)s_list[pos] : 0;
    const int c = has ? (int)(s_key[k] >> 32) : -2;
    double ax1 = 0.0, ay1 = 0.0, ax2 = 0.0, ay2 = 0.0;
    if (has) {
      const float4 d = s_dbox[k];
      ax1 = (double)d.x; ay1 = (double)d.y; ax2 = (double)d.z; ay2 = (double)d.w;
    }
    const DmSweep r = dm_sweep<true>(has, c, ax1, ay1, ax2, ay2, (ax2 - ax1) * (ay2 - ay1), HUGE_VAL, -1, s_gbox, s_gcode, gbox, gcls,
                                     gign, g0, ng, nchunks, C);
    if (has && lane == 0) {
      s_bidx[pos] = r.best_idx == INT_MAX ? (unsigned short)0xffff : (unsigned short)r.best_idx;
      s_iidx[pos] = r.ig_idx == INT_MAX ? (unsigned short)0xffff : (unsigned short)r.ig_idx;
    }
  }
  __syncthreads();

  // phase B, the claim walk: step s settles the s-th detection of every class that has one, a wave per detection, lane t = threshold t
  const int maxcnt = nact > 0 ? s_hist[s_act[0]] : 0;
  for (int s = 0; s < maxcnt; ++s) {
    for (int base = 0; base < nact && s_hist[s_act[base]] > s; base += DM_WAVES) {       // (uniform)
      const int ai = base + wave;
      const int c = ai < nact ? s_act[ai] : 0;
      const bool has = ai < nact && s_hist[c] > s;
      const int pos = has ? s_start[c] + s : 0;
      const int k = has ? (int)s_list[pos] : 0;
      double ax1 = 0.0, ay1 = 0.0, ax2 = 0.0, ay2 = 0.0;
      if (has) {
        const float4 d = s_dbox[k];
        ax1 = (double)d.x; ay1 = (double)d.y; ax2 = (double)d.z; ay2 = (double)d.w;
      }
      const double area_a = (ax2 - ax1) * (ay2 - ay1);
      // the stored indices name GT of class c; their IoUs are computed again (the same operations: the same bits)
      int best_idx = INT_MAX, ig_idx = INT_MAX;
      double best_iou = -1.0, ig_iou = -1.0;
      if (has) {
        const int bi = s_bidx[pos], ii = s_iidx[pos];
        if (bi != 0xffff) { best_idx = bi; best_iou = dm_iou(ax1, ay1, ax2, ay2, area_a, nchunks == 1 ? s_gbox[bi] : ((const float4*)gbox)[g0 + bi]); }
        if (ii != 0xffff) { ig_idx = ii; ig_iou = dm_iou(ax1, ay1, ax2, ay2, area_a, nchunks == 1 ? s_gbox[ii] : ((const float4*)gbox)[g0 + ii]); }
      }
      bool pending = has && lane < T, tp = false;
      int tp_idx = 0;
      for (;;) {
        if (__ballot(pending) != 0ull) {                   // (uniform over the wave) settle what the candidate settles
          if (best_idx == INT_MAX) {
            pending = false;                               // no candidate left: not a true positive
          } else {
            const bool reach = pending && best_iou >= mythr;
            unsigned cm = 0u;
            if (__ballot(reach) != 0ull) {                 // is the candidate among the claims of the class's earlier detections?
              const int p0 = s_start[c], cnt = (pos - p0) * T;
              for (int e = lane; e < cnt; e += 64) {
                const int j = p0 + e / T, t = e - (e / T) * T;
                if ((int)s_mt[j * T + t] == best_idx) cm |= 1u << t;
              }
              for (int off = 32; off > 0; off >>= 1) cm |= __shfl_xor(cm, off);
            }
            if (pending) {
              if (!reach) pending = false;                 // every later candidate has a lower IoU still
              else if (!((cm >> lane) & 1u)) { tp = true; tp_idx = best_idx; pending = false; }
            }
          }
        }
        if (!__syncthreads_or(pending ? 1 : 0)) break;     // a claimed candidate somewhere: the next one, for the waves that need it
        const DmSweep r = dm_sweep<false>(__ballot(pending) != 0ull, c, ax1, ay1, ax2, ay2, area_a, best_iou, best_idx, s_gbox, s_gcode,
                                          gbox, gcls, gign, g0, ng, nchunks, C);
        best_iou = r.best_iou; best_idx = r.best_idx;
      }
      if (has && lane < T) {
        const long long o = (row0 + k) * T + lane;
        s_mt[pos * T + lane] = tp ? (unsigned short)tp_idx : (unsigned short)0xffff;
        if (tp) { flags[o] = 1; matched[o] = g0 + tp_idx; }
        else if (ig_idx != INT_MAX && ig_iou >= mythr) { flags[o] = 2; matched[o] = g0 + ig_idx; }
        else { flags[o] = 0; matched[o] = -1; }
      }
    }
  }
}

// count [B] int32, class_ids [B][K] int64, scores [B][K], boxes [B][K][4]: the packed detect output.  gt_boxes [total][4] fp32 xyxy,
// gt_class_ids [total] int32, gt_offsets [B+1] int32, gt_ignore [total] uint8 or NULL; thresholds [T] float64 (device).
// flags uint8 [B][K][T], matched_gt int32 [B][K][T]; npos int32 [num_classes] is ADDED to.
extern "C" int sqd_det_match_fwd(const int* count, const long long* class_ids, const float* scores, const float* boxes,
                                 const float* gt_boxes, const int* gt_class_ids, const int* gt_offsets, const unsigned char* gt_ignore,
                                 const double* thresholds, unsigned char* flags, int* matched_gt, int* npos, int B, int K, int total,
                                 int T, int num_classes, void* stream) {
  SQD_CHECK_ARG(count && class_ids && scores && boxes && gt_offsets && thresholds && flags && matched_gt && npos);
  SQD_CHECK_ARG(B >= 1 && total >= 0 && K >= 1 && K <= DM_MAX_K && T >= 1 && T <= DM_MAX_T && num_classes >= 1 && num_classes <= DM_MAX_C);
  SQD_CHECK_ARG(total == 0 || (gt_boxes && gt_class_ids));
  SQD_CHECK_ARG(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)gt_boxes & 15) == 0 && ((uintptr_t)thresholds & 7) == 0);
  static SqdDevOnce once;
  if (sqd_max_lds_once(once, (const void*)det_match_kernel, DM_MAX_K * (16 + 2 * DM_MAX_T)) != SQD_OK) return SQD_ERR_LAUNCH;
  hipLaunchKernelGGL(det_match_kernel, dim3((unsigned)B), dim3(DM_THREADS), (size_t)K * (16 + 2 * T), (hipStream_t)stream, count, class_ids, scores, boxes,
                     gt_boxes, gt_class_ids, gt_offsets, gt_ignore, thresholds, flags, matched_gt, npos, K, total, T, num_classes);
  return sqd_launch_status();
}

// ---------------------------------------------------------------------------------------------------------------------
constexpr int AP_THREADS = 1024;
constexpr int AP_WAVES = AP_THREADS / 64;
constexpr int AP_SAMPLES = 101;

__global__ __launch_bounds__(AP_THREADS) void det_ap_kernel(const int* __restrict__ cls, const unsigned char* __restrict__ flags,
                                                            const int* __restrict__ seg, const int* __restrict__ npos,
                                                            double* __restrict__ ap, int* tp_cum, int* fp_cum,
                                                            double* __restrict__ prec, int N, int T, int mode) {
  __shared__ int s_wt[AP_WAVES], s_wf[AP_WAVES];
  __shared__ double s_wm[AP_WAVES], s_red[AP_WAVES], s_samp[AP_SAMPLES];
  const int c = blockIdx.x / T, t = blockIdx.x - c * T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long s0 = min(max(seg[c], 0), N), s1 = min(max((long long)seg[c + 1], s0), (long long)N);
  const int np = npos[c];
  const unsigned long long le = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);

  // forward: running TP / FP counts
  int ctp = 0, cfp = 0;
  for (long long base = s0; base < s1; base += AP_THREADS) {
    const long long i = base + tid;
    const bool in = i < s1 && cls[i] == c;
    const int f = in ? (int)flags[i * T + t] : 3;
    const unsigned long long bt = __ballot(f == 1), bf = __ballot(f == 0);
    int itp = __popcll(bt & le), ifp = __popcll(bf & le);
    if (lane == 0) { s_wt[wave] = __popcll(bt); s_wf[wave] = __popcll(bf); }
    __syncthreads();
    int tt = 0, tf = 0;
    for (int w = 0; w < AP_WAVES; ++w) {
      if (w < wave) { itp += s_wt[w]; ifp += s_wf[w]; }
      tt += s_wt[w]; tf += s_wf[w];
    }
    if (i < s1) { tp_cum[i * T + t] = ctp + itp; fp_cum[i * T + t] = cfp + ifp; }
    ctp += tt; cfp += tf;
    __syncthreads();
  }
  const long long o = (long long)c * T + t;
  if (np <= 0) {                                           // a class without GT has no AP
    if (tid == 0) ap[o] = __longlong_as_double(0x7ff8000000000000ll);
    if (prec && mode == 2 && tid < AP_SAMPLES) prec[o * AP_SAMPLES + tid] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  if (tid < AP_SAMPLES) s_samp[tid] = 0.0;
  __syncthreads();

  // backward: precision envelope (running max from the end), integration
  const int S = mode == 1 ? 10 : 100;
  const double dnp = (double)np;
  double carry = 0.0, acc = 0.0;
  const long long nch = (s1 - s0 + AP_THREADS - 1) / AP_THREADS;
  for (long long ch = nch - 1; ch >= 0; --ch) {
    const long long i = s0 + ch * AP_THREADS + tid;
    const bool in = i < s1;
    const int tpv = in ? tp_cum[i * T + t] : 0, fpv = in ? fp_cum[i * T + t] : 0;     // (this thread's own stores)
    const double p = tpv + fpv > 0 ? (double)tpv / (double)(tpv + fpv) : 0.0;
    double v = p;
    for (int off = 1; off < 64; off <<= 1) {
      const double ov = __shfl_down(v, off);
      if (lane + off < 64) v = fmax(v, ov);
    }
    if (lane == 0) s_wm[wave] = v;
    __syncthreads();
    double later = carry, all = carry;
    for (int w = 0; w < AP_WAVES; ++w) {
      if (w > wave) later = fmax(later, s_wm[w]);
      all = fmax(all, s_wm[w]);
    }
    const double env = fmax(v, later);
    if (in && cls[i] == c && flags[i * T + t] == 1) {
      if (mode == 0) {
        acc += env;
      } else {                                             // the sample points first reached by tp = tpv
        const double r1 = (double)tpv / dnp, r0 = (double)(tpv - 1) / dnp;
        long long k = ((long long)(tpv - 1) * S) / np - 1;
        for (k = k < 0 ? 0 : k; k <= S; ++k) {
          const double r = (double)k / (double)S;
          if (!(r1 >= r)) break;
          if (!(r0 >= r)) s_samp[k] = env;
        }
      }
    }
    if (mode != 0 && i == s0) s_samp[0] = env;             // recall 0 is reached at the first entry
    carry = all;
    __syncthreads();
  }
  if (mode == 0) {
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if (lane == 0) s_red[wave] = acc;
    __syncthreads();
    if (tid == 0) {
      double sum = 0.0;
      for (int w = 0; w < AP_WAVES; ++w) sum += s_red[w];
      ap[o] = sum / dnp;
    }
  } else {
    if (tid == 0) {
      double sum = 0.0;
      for (int k = 0; k <= S; ++k) sum += s_samp[k];
      ap[o] = sum / (double)(S + 1);
    }
    if (prec && mode == 2 && tid < AP_SAMPLES) prec[o * AP_SAMPLES + tid] = s_samp[tid];
  }
}

// class_ids int32 [N] (num_classes = empty slot), flags uint8 [N][T], seg_offsets int32 [num_classes+1], npos int32 [num_classes]:
// the pool ordered by (class, score descending, insertion order).  ap float64 [num_classes][T]; tp_cum / fp_cum int32 [N][T] (entries
// outside every segment are not written); prec101 float64 [num_classes][T][101] or NULL (written in mode 2).
extern "C" int sqd_det_ap_fwd(const int* class_ids, const unsigned char* flags, const int* seg_offsets, const int* npos, double* ap,
                              int* tp_cum, int* fp_cum, double* prec101, int N, int T, int num_classes, int mode, void* stream) {
  SQD_CHECK_ARG(seg_offsets && npos && ap && N >= 0 && T >= 1 && T <= DM_MAX_T && num_classes >= 1 && num_classes <= DM_MAX_C);
  SQD_CHECK_ARG(mode >= 0 && mode <= 2);
  SQD_CHECK_ARG(N == 0 || (class_ids && flags && tp_cum && fp_cum));
  SQD_CHECK_ARG(((uintptr_t)ap & 7) == 0 && ((uintptr_t)prec101 & 7) == 0);
  hipLaunchKernelGGL(det_ap_kernel, dim3((unsigned)(num_classes * T)), dim3(AP_THREADS), 0, (hipStream_t)stream, class_ids, flags,
                     seg_offsets, npos, ap, tp_cum, fp_cum, prec101, N, T, mode);
  return sqd_launch_status();
}
