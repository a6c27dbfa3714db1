// Post-processing: per-anchor decode (softmax / sigmoid / anchor box transform) and the fused
// detection kernel (decode -> top-k by score -> class-wise NMS -> score threshold -> compact).
//
// Reference: PredictionResolver.forward src/model/squeezedet.py:109-120, safe_softmax
// src/model/modules.py:66-68, deltas_to_boxes :27-45, xywh_to_xyxy :17-24, SqueezeDet.forward
// src/model/squeezedet.py:199-206, Detector.filter src/engine/detector.py:87-122 (+ torchvision nms),
// boxes_postprocess src/utils/boxes.py:145-147 (the eval-time scale division).
//
// pred is [B][A][C+5] fp32 (anchor-major: C class logits, 1 confidence logit, 4 deltas), anchors
// [A][4] (cx,cy,w,h) fp32.  The reference runs ~15 elementwise launches plus a Python loop with
// >=10 host syncs per image; here ONE launch (detect_kernel, one workgroup per image) does everything on the device:
//   1. 16 waves score the image's anchors into LDS: score = max_c softmax_c * sigmoid(conf) per anchor; key = fp32 score
//      bits (non-negative floats order like uint32) if score > score_thresh else 0 (or, where ConvDet's launch already stored the
//      keys -- sqd_detect_keys_fwd -- copy them into LDS); then:
//   2. stable compaction of the non-zero keys into LDS, 4-pass 8-bit radix select of the K-th largest; ties at that
//      key taken in ascending anchor order (the build's documented tie rule),
//   3. one wave ranks the <=64 candidates (score desc, anchor index asc), decodes their boxes,
//      builds the 64x64 suppression bit matrix (one 64-bit row per lane) and runs greedy NMS with
//      a wave-uniform alive mask; survivors are compacted in class order 0..C-1, each class in
//      descending score, then thresholded -- the exact output order of Detector.filter.
// Arithmetic mirrors the oracle op for op in fp32 (built with -ffp-contract=off, IEEE division), so
// that, given identical pred, the kept anchor indices are bit-exact.
#include "sqd_common.h"
#include "anchor_score.h"        // anchor_score: shared with ConvDet's key-writing epilogue (conv_wino_vs.hip)
#include "many_class.h"
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

// ---- full decode (module surface of SqueezeDet.forward: dense class_ids / scores / boxes) ----
__global__ __launch_bounds__(256) void decode_kernel(const float* __restrict__ pred, const float* __restrict__ anchors,
                                                     long long* __restrict__ class_ids, float* __restrict__ scores,
                                                     float* __restrict__ boxes, int B, int A, int C, float wmax, float hmax) {
  const long long total = (long long)B * A;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int a = (int)(i % A);
    const float* p = pred + i * (C + 5);
    float s; int c;
    anchor_score(p, C, s, c);
    const BoxF b = anchor_box(p + C + 1, anchors + 4 * a, wmax, hmax);
    class_ids[i] = c; scores[i] = s;
    *(f32x4*)(boxes + 4 * i) = (f32x4){b.x1, b.y1, b.x2, b.y2};
  }
}

extern "C" int sqd_decode_fwd(const float* pred, const float* anchors, long long* class_ids, float* scores,
                              float* boxes, int B, int A, int num_classes, int input_h, int input_w, void* stream) {
  SQD_CHECK_ARG(pred && anchors && class_ids && scores && boxes && B > 0 && A > 0);
  SQD_CHECK_ARG(num_classes >= 1 && num_classes <= SQD_MAX_CLASSES);
  SQD_CHECK_ARG(((uintptr_t)pred & 15) == 0 && ((uintptr_t)boxes & 15) == 0);
  const long long total = (long long)B * A;
  const int blocks = (int)((total + 255) / 256);
  hipLaunchKernelGGL(decode_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pred, anchors, class_ids,
                     scores, boxes, B, A, num_classes, (float)(input_w - 1), (float)(input_h - 1));
  return sqd_launch_status();
}

// ---- PredictionResolver.forward proper: the reference's five dense outputs (src/model/squeezedet.py:109-120) ----
__global__ __launch_bounds__(256) void resolve_kernel(const float* __restrict__ pred, const float* __restrict__ anchors,
                                                      float* __restrict__ probs, float* __restrict__ logp, float* __restrict__ scores,
                                                      float* __restrict__ deltas, float* __restrict__ boxes, int B, int A, int C,
                                                      float wmax, float hmax) {
  const long long total = (long long)B * A;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int a = (int)(i % A);
    const float* p = pred + i * (C + 5);
    float l[SQD_MAX_CLASSES];
    float m = p[0];
    for (int c = 0; c < C; ++c) { l[c] = p[c]; m = fmaxf(m, l[c]); }
    float sum = 0.f;
    for (int c = 0; c < C; ++c) sum += expf(l[c] - m);
    const float lse = logf(sum);
    for (int c = 0; c < C; ++c) {
      probs[i * C + c] = expf(l[c] - m) / sum;                 // safe_softmax (modules.py:66-68)
      if (logp) logp[i * C + c] = (l[c] - m) - lse;            // torch.log_softmax
    }
    scores[i] = 1.f / (1.f + expf(-p[C]));
    const float* d = p + C + 1;
    *(f32x4*)(deltas + 4 * i) = (f32x4){d[0], d[1], d[2], d[3]};
    const BoxF b = anchor_box(d, anchors + 4 * a, wmax, hmax);
    *(f32x4*)(boxes + 4 * i) = (f32x4){b.x1, b.y1, b.x2, b.y2};
  }
}

// probs [B][A][C], logp [B][A][C] or NULL, scores [B][A] (the reference's [B,A,1]), deltas [B][A][4], boxes [B][A][4]
extern "C" int sqd_resolve_fwd(const float* pred, const float* anchors, float* probs, float* logp, float* scores,
                               float* deltas, float* boxes, int B, int A, int num_classes, int input_h, int input_w,
                               void* stream) {
  SQD_CHECK_ARG(pred && anchors && probs && scores && deltas && boxes && B > 0 && A > 0);
  SQD_CHECK_ARG(num_classes >= 1 && num_classes <= SQD_MAX_CLASSES);
  SQD_CHECK_ARG(((uintptr_t)deltas & 15) == 0 && ((uintptr_t)boxes & 15) == 0);
  const long long total = (long long)B * A;
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(resolve_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pred, anchors, probs, logp, scores,
                     deltas, boxes, B, A, num_classes, (float)(input_w - 1), (float)(input_h - 1));
  return sqd_launch_status();
}

// ---- fused detection ----
// One launch, one workgroup per image of 1024 threads.  Phase 1 scores the anchors into LDS keys -- the fp32 score bits if
// score > score_thresh, else 0; phase 2 compacts the non-zero keys (stable, ascending anchor index) and selects the top K
// (radix select; the 256 histogram bins belong to the first 256 threads, the candidate sweeps run on all 1024), ranks them,
// runs class-wise NMS on one wave and writes the compact result.  Three forms of phase 1, one kernel:
//   * keys given (sqd_detect_keys_fwd): ConvDet's epilogue already stored every key of the batch (sqd_conv_wino_vs_keys_fwd: the
//     lane that stores an anchor's logits scores it) -- phase 1 is a 16-byte copy of the image's keys into LDS, B workgroups, `pred`
//     is read for the <= 64 candidates only.  The kernel boundary orders the key stores before the loads: no fence, no sc1.  The
//     form of the benchmarked step (three classes, ConvDet on conv_wino_vs_kernel);
//   * pred, split (sqd_detect_shift_fwd with a workspace): eight workgroups score an image from `pred` and hand their keys to the
//     image's last arriver through the workspace (below);
//   * pred or dense, one workgroup per image: every other caller.
// (Tried and dropped in
// round 2: spreading phase 1 over the whole chip and handing the keys to the last-arriving workgroup of each image
// through global memory -- the device-scope release / acquire pair across the XCDs' L2s cost 12-100 us, more than the
// 20 idle-chip microseconds it saved; profiles/r02_detect_variants.log.  The split form above is its cheaper successor.)
// Why pre-filtering by the threshold is exact: Detector.filter thresholds AFTER NMS, but a box at or below the
// threshold can only suppress boxes with lower scores, which are dropped by the same threshold -- so the kept set
// is that of NMS over the top-K of the above-threshold anchors.
#define DET_THREADS 256
#define DET_K 64

struct DetArgs {
  const float* pred; const float* anchors; const float* scales;   // scales [B][2] = (sy, sx) or null
  const float* shifts;                                            // [B][2] = (dy, dx) added after the scale division, or null
  const long long* in_class; const float* in_score; const float* in_box;   // dense inputs (filter mode) or null
  unsigned* keys;                                                 // workspace [B][ceil4(A)] keys + [B] arrival counters, or null (one workgroup per image)
  int keys_ready = 0;                                             // the workspace already holds every key of the batch (words A .. ceil4(A)-1 of an image: any)
  int S, per;
  int* det_count; long long* det_class; float* det_score; float* det_box; int* det_anchor;
  int B, A, C, K;
  float wmax, hmax, nms_thresh, score_thresh;
};

#define DET_SCORE_THREADS 1024      // threads per workgroup (16 waves)
#define DET_SPLIT 8                 // workgroups scoring one image when a key workspace is given

__global__ __launch_bounds__(DET_SCORE_THREADS) void detect_kernel(DetArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  unsigned* keysL = (unsigned*)smem_raw;                      // [A4] all keys of this image (A rounded up to 4)
  unsigned short* cidx = (unsigned short*)(smem_raw + (size_t)((a.A + 3) & ~3) * 4);   // [A] candidate anchor indices
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_need, s_cnt, s_nlive;
  __shared__ unsigned wave_tot[DET_SCORE_THREADS / 64];
  __shared__ unsigned cand_key[DET_K];
  __shared__ int cand_idx[DET_K];
  __shared__ int sorted_pos[DET_K];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = a.S;                                          // workgroups scoring one image (1: everything in this workgroup)
  const int b = (int)blockIdx.x / S, seg = (int)blockIdx.x - b * S;
  const int A = a.A, C = a.C, K = a.K;
  const float* pred = a.pred ? a.pred + (long long)b * A * (C + 5) : nullptr;
  const bool dense = a.in_score != nullptr;
  const bool given = a.keys_ready != 0;                       // the keys come from ConvDet's epilogue (S == 1): nothing to score
  const int lo_a = given ? 0 : seg * a.per, hi_a = given ? 0 : min(A, lo_a + a.per);   // this workgroup's anchors (a.per is a multiple of 4)

  // 1. score the anchors straight into LDS.  Two passes keep the exp / divide work dense:
  //    1a. confidence only: score = max_c softmax_c * conf <= conf (softmax_c <= 1 and the products round monotonically), so
  //        conf <= threshold already decides key = 0 -- exactly; the others are listed in LDS (any order);
  //    1b. the listed anchors (typically ~15 %) get the full score.
  //    With S > 1 the image's anchors are split over S workgroups (one CU reads a 539 KB `pred` slice in ~20 us; eight read it in
  //    ~3): each writes its keys to the global workspace (write-through), drains and draws a ticket; the last arriver of the image
  //    loads all keys back into its LDS and carries on alone -- selection and NMS never leave that workgroup (in-launch hand-off of
  //    cdna_hip_programming.md Guideline 16: sc1 payload + drained stores + agent-scope counter, no release fence, so the hundreds
  //    of megabytes ConvDet's launch left dirty in the L2s are not written back for it; that is what made round 2's version of this
  //    cost 61-156 us).
  if (tid == 0) s_nlive = 0u;
  __syncthreads();
  for (int i0 = lo_a; i0 < hi_a; i0 += DET_SCORE_THREADS) {
    const int i = i0 + tid;
    bool live = false;
    if (i < hi_a) {
      if (dense) {
        const float s = a.in_score[(long long)b * A + i];
        keysL[i] = (s > a.score_thresh) ? __float_as_uint(s) : 0u;
      } else {
        const float conf = 1.f / (1.f + expf(-pred[(long long)i * (C + 5) + C]));
        live = conf > a.score_thresh;
        if (!live) keysL[i] = 0u;
      }
    }
    const unsigned long long m = __ballot(live);
    if (m) {
      unsigned base = 0u;
      if (lane == 0) base = atomicAdd(&s_nlive, (unsigned)__popcll(m));
      base = __shfl(base, 0);
      if (live) cidx[base + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)i;
    }
  }
  __syncthreads();
  {
    const int nlive = (int)s_nlive;
    for (int j = tid; j < nlive; j += DET_SCORE_THREADS) {
      const int i = cidx[j];
      float s; int c;
      anchor_score(pred + (long long)i * (C + 5), C, s, c);
      keysL[i] = (s > a.score_thresh) ? __float_as_uint(s) : 0u;   // scores are >= 0: bit patterns order like the floats
    }
  }
  __syncthreads();
  if (S > 1) {
    typedef unsigned int u32x4_d __attribute__((ext_vector_type(4)));
    const int A4 = (A + 3) & ~3;
    const __amdgpu_buffer_rsrc_t kres = __builtin_amdgcn_make_buffer_rsrc((void*)(a.keys + (long long)b * A4), 0, 0x7ffffff0, 0x00020000);
    for (int q = lo_a / 4 + tid; q < (hi_a + 3) / 4; q += DET_SCORE_THREADS) {       // (keys past A inside the last quad: never read back)
      u32x4_d v = *(const u32x4_d*)(keysL + 4 * q);
      __builtin_amdgcn_raw_buffer_store_b128(v, kres, q * 16, 0, 16);               // sc1: write-through
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // every storing wave drains its stores ...
    __syncthreads();                                         // ... before ONE lane counts the workgroup in
    unsigned* const tick = a.keys + (long long)a.B * A4 + b;
    if (tid == 0) s_cnt = __hip_atomic_fetch_add(tick, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if ((int)s_cnt != S - 1) return;                         // not the last arriver of this image: done
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      __hip_atomic_store(tick, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // the counter returns to zero for the next launch
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    for (int q = tid; q < A4 / 4; q += DET_SCORE_THREADS)
      *(u32x4_d*)(keysL + 4 * q) = __builtin_amdgcn_raw_buffer_load_b128(kres, q * 16, 0, 16);   // sc1 loads: every key of the image
    __syncthreads();
  }
  if (given) {
    // keys given: ConvDet's launch stored them, the kernel boundary made them visible -- plain 16-byte loads.  The words A .. A4-1 of
    // the last quad are whatever the workspace held: nothing below reads keysL past A
    typedef unsigned int u32x4_g __attribute__((ext_vector_type(4)));
    const int A4 = (A + 3) & ~3;
    const u32x4_g* __restrict__ src = (const u32x4_g*)(a.keys + (long long)b * A4);
    for (int q = tid; q < A4 / 4; q += DET_SCORE_THREADS) *(u32x4_g*)(keysL + 4 * q) = src[q];
    __syncthreads();
  }

  if (tid < DET_K) { cand_key[tid] = 0u; cand_idx[tid] = 0x7fffffff - DET_K + tid; }   // distinct sentinels: ranks stay a permutation
  if (tid == 0) { s_prefix = 0u; s_need = (unsigned)K; s_cnt = 0u; }

  // block-wide exclusive scan helper over one value per thread (fixed order -> deterministic)
  auto block_excl_scan = [&](unsigned c, unsigned& total) {
    unsigned incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned t = __shfl_up(incl, off);
      if (lane >= off) incl += t;
    }
    __syncthreads();
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    unsigned woff = 0u, tot = 0u;
    for (int w = 0; w < DET_SCORE_THREADS / 64; ++w) { if (w < wave) woff += wave_tot[w]; tot += wave_tot[w]; }
    total = tot;
    return incl - c + woff;
  };

  // 1. stable compaction of the above-threshold anchors: contiguous index range per thread
  const int chunk = (A + DET_SCORE_THREADS - 1) / DET_SCORE_THREADS;
  const int lo = tid * chunk, hi = min(A, lo + chunk);
  __syncthreads();
  unsigned c = 0u;
  for (int i = lo; i < hi; ++i) c += keysL[i] != 0u ? 1u : 0u;
  unsigned M;
  unsigned off = block_excl_scan(c, M);
  for (int i = lo; i < hi; ++i)
    if (keysL[i] != 0u) { cidx[off] = (unsigned short)i; ++off; }
  __syncthreads();

  int ncand;
  if ((int)M <= K) {
    for (int i = tid; i < (int)M; i += DET_SCORE_THREADS) { cand_key[i] = keysL[cidx[i]]; cand_idx[i] = cidx[i]; }
    ncand = (int)M;
    __syncthreads();
  } else {
    // 2. radix select of the K-th largest key among the M candidates
    unsigned mask = 0u;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      if (tid < DET_THREADS) hist[tid] = 0u;                   // DET_THREADS == 256 bins
      __syncthreads();
      const unsigned prefix = s_prefix;
      // scores cluster in 2-3 exponent bins: in the leading pass aggregate equal bins inside a wave (one
      // atomic per distinct bin) instead of serialising up to 64 same-address LDS atomics
      for (int i0 = 0; i0 < (int)M; i0 += DET_SCORE_THREADS) {
        const int i = i0 + tid;
        const unsigned k = (i < (int)M) ? keysL[cidx[i]] : 0u;
        const bool act = (i < (int)M) && ((k & mask) == prefix);
        const unsigned bin = (k >> shift) & 255u;
        if (pass == 0) {
          unsigned long long todo = __ballot(act);
          while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned lb = __shfl(bin, leader);
            const unsigned long long same = __ballot(act && bin == lb);
            if (lane == leader) atomicAdd(&hist[lb], (unsigned)__popcll(same));
            todo &= ~same;
          }
        } else if (act) {
          atomicAdd(&hist[bin], 1u);
        }
      }
      __syncthreads();
      {
        // bucket holding the need-th largest key: thread t owns bin 255-t; an exclusive block scan gives the
        // number of keys in higher bins (256 threads in parallel instead of a serial 256-step walk)
        const unsigned need = s_need;
        const unsigned h = (tid < DET_THREADS) ? hist[255 - tid] : 0u;
        unsigned tot;
        const unsigned above = block_excl_scan(h, tot);
        if (tid < DET_THREADS && above < need && above + h >= need) {          // exactly one thread
          s_need = need - above;                          // how many keys to take from this bucket (and below-level ties)
          s_prefix = prefix | ((unsigned)(255 - tid) << shift);
        }
      }
      mask |= 255u << shift;
      __syncthreads();
    }
    const unsigned tkey = s_prefix;       // K-th largest key
    const unsigned need = s_need;         // number of keys == tkey to take (>= 1)
    const unsigned n_gt = (unsigned)K - need;
    // 3a. keys strictly above the threshold key (unordered; ranked later)
    for (int i = tid; i < (int)M; i += DET_SCORE_THREADS) {
      const unsigned k = keysL[cidx[i]];
      if (k > tkey) { const unsigned pos = atomicAdd(&s_cnt, 1u); cand_key[pos] = k; cand_idx[pos] = cidx[i]; }
    }
    // 3b. ties at the threshold key in ascending anchor order (the compacted list is index-ordered)
    const int chunk2 = ((int)M + DET_SCORE_THREADS - 1) / DET_SCORE_THREADS;
    const int lo2 = tid * chunk2, hi2 = min((int)M, lo2 + chunk2);
    unsigned c2 = 0u;
    for (int i = lo2; i < hi2; ++i) c2 += (keysL[cidx[i]] == tkey) ? 1u : 0u;
    unsigned tot2;
    unsigned r = block_excl_scan(c2, tot2);
    for (int i = lo2; i < hi2 && r < need; ++i)
      if (keysL[cidx[i]] == tkey) { cand_key[n_gt + r] = tkey; cand_idx[n_gt + r] = cidx[i]; ++r; }
    ncand = K;
    __syncthreads();
  }

  // 4. rank the candidates: score desc, anchor index asc (sentinels: key 0, idx ~INT_MAX -> last)
  if (tid < DET_K) {
    const unsigned mykey = cand_key[tid];
    const int myidx = cand_idx[tid];
    int rank = 0;
    for (int j = 0; j < DET_K; ++j) {
      const unsigned kj = cand_key[j]; const int ij = cand_idx[j];
      rank += (kj > mykey || (kj == mykey && ij < myidx)) ? 1 : 0;
    }
    sorted_pos[rank] = tid;             // ranks are a permutation (indices are distinct)
  }
  __syncthreads();
  if (wave != 0) return;                // 5..7: one wave
  const int src = sorted_pos[lane];
  const int idx = cand_idx[src];
  const bool ok = src < ncand && lane < K;
  float score = 0.f; int cls = -1;
  BoxF bx = {0.f, 0.f, 0.f, 0.f};
  if (ok && dense) {
    const long long o = (long long)b * A + idx;
    score = a.in_score[o]; cls = (int)a.in_class[o];
    const f32x4 v = *(const f32x4*)(a.in_box + 4 * o);
    bx.x1 = v.x; bx.y1 = v.y; bx.x2 = v.z; bx.y2 = v.w;
  } else if (ok) {
    const float* p = pred + (long long)idx * (C + 5);
    anchor_score(p, C, score, cls);
    bx = anchor_box(p + C + 1, a.anchors + 4 * idx, a.wmax, a.hmax);
  }
  // suppression row: bit j set if j ranks after me, same class, IoU > thresh
  const float area = (bx.x2 - bx.x1) * (bx.y2 - bx.y1);
  unsigned long long row = 0ull;
  for (int j = 0; j < DET_K; ++j) {
    const float jx1 = __shfl(bx.x1, j), jy1 = __shfl(bx.y1, j), jx2 = __shfl(bx.x2, j), jy2 = __shfl(bx.y2, j);
    const float jarea = __shfl(area, j);
    const int jcls = __shfl(cls, j);
    const float w = fmaxf(0.f, fminf(bx.x2, jx2) - fmaxf(bx.x1, jx1));
    const float h = fmaxf(0.f, fminf(bx.y2, jy2) - fmaxf(bx.y1, jy1));
    const float inter = w * h;
    const float ovr = inter / ((area + jarea) - inter);
    if (j > lane && jcls == cls && cls >= 0 && ovr > a.nms_thresh) row |= 1ull << j;
  }
  unsigned long long alive = __ballot(ok);
  for (int i = 0; i < DET_K; ++i) {
    const unsigned lo32 = __shfl((unsigned)(row & 0xffffffffull), i);
    const unsigned hi32 = __shfl((unsigned)(row >> 32), i);
    if ((alive >> i) & 1ull) alive &= ~(((unsigned long long)hi32 << 32) | lo32);
  }
  const bool keep = ((alive >> lane) & 1ull) && score > a.score_thresh;
  int pos = 0, total = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int c = 0; c < C; ++c) {
    const unsigned long long m = __ballot(keep && cls == c);
    if (c < cls) pos += __popcll(m);
    else if (c == cls) pos += __popcll(m & below);
    total += __popcll(m);
  }
  if (lane == 0) a.det_count[b] = total;
  if (keep) {
    float sx = 1.f, sy = 1.f;
    if (a.scales) { sy = a.scales[2 * b]; sx = a.scales[2 * b + 1]; }
    const long long o = (long long)b * K + pos;
    a.det_class[o] = cls;
    a.det_score[o] = score;
    a.det_anchor[o] = idx;
    f32x4 ob = (f32x4){bx.x1 / sx, bx.y1 / sy, bx.x2 / sx, bx.y2 / sy};
    // boxes_postprocess' padding / crops terms (src/utils/boxes.py:149-155): per axis only one of the two is non-zero, so
    // (b - padding) + crops == b + (crops - padding) bit for bit
    if (a.shifts) { const float dy = a.shifts[2 * b], dx = a.shifts[2 * b + 1]; ob.x += dx; ob.y += dy; ob.z += dx; ob.w += dy; }
    *(f32x4*)(a.det_box + 4 * o) = ob;
  }
}

static int launch_detect(DetArgs a, hipStream_t stream) {
  if (a.K < 1 || a.K > DET_K) return SQD_ERR_UNSUPPORTED;                 // one wave holds the NMS bit matrix
  const size_t lds = (size_t)((a.A + 3) & ~3) * 4 + (size_t)a.A * 2 + 16;  // keys + uint16 candidate indices
  if (a.A > 65535 || lds > 150 * 1024) return SQD_ERR_UNSUPPORTED;        // A <= 25596 anchors per image
  static SqdDevOnce lds_once;                                              // raise the dynamic-LDS cap once per device
  if (lds > 48 * 1024 && sqd_max_lds_once(lds_once, (const void*)detect_kernel, 150 * 1024) != SQD_OK) return SQD_ERR_LAUNCH;
  // pred mode with a workspace: eight workgroups score an image, its last arriver selects and suppresses (the workspace holds B x
  // ceil4(A) keys + B counters that are zero between launches)
  // keys given (keys_ready): one workgroup per image copies them, nothing is split and no counter is touched
  a.S = (a.pred && a.keys && !a.keys_ready) ? DET_SPLIT : 1;
  a.per = (((a.A + 3) / 4 + a.S - 1) / a.S) * 4;
  hipLaunchKernelGGL(detect_kernel, dim3((unsigned)(a.B * a.S)), dim3(DET_SCORE_THREADS), lds, stream, a);
  return sqd_launch_status();
}

// Fused decode + Detector.filter for a batch, straight from pred.  sqd_detect_fwd's keys_ws: unused (may be NULL; earlier versions kept
// the per-anchor keys in global memory).  Outputs are fixed-capacity
// [B][K]; rows >= det_count[b] are left untouched.  scales ([B][2] = (sy,sx), may be null) folds
// boxes_postprocess' division into the store.
// sqd_detect_shift_fwd: the same with shifts ([B][2] = (dy, dx), may be null) added to the boxes after the scale division --
// boxes_postprocess' padding / crops terms of the reference's forbid_resize branch (src/utils/boxes.py:149-155) -- and, when keys_ws
// is given (B * ceil4(A) + B uint32, the last B zero before the first launch; every launch leaves them zero), the scoring of an
// image spread over eight workgroups whose last arriver selects and suppresses.  keys_ws NULL: one workgroup per image.
// sqd_detect_keys_fwd: the same arguments, but keys_ws (required, 16-byte aligned) already HOLDS the keys of this pred -- [B][ceil4(A)],
// written by sqd_conv_wino_vs_keys_fwd with the same score_thresh earlier on the same stream: one workgroup per image loads them,
// selects and suppresses; nothing is scored, the arrival counters behind the keys are neither read nor written.
static int detect_pred(const float* pred, const float* anchors, const float* scales, const float* shifts, unsigned* keys_ws, int keys_ready,
                       int* det_count, long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                       int num_classes, int input_h, int input_w, int keep_top_k, float nms_thresh, float score_thresh, void* stream) {
  SQD_CHECK_ARG(pred && anchors && det_count && det_class && det_score && det_box && det_anchor);
  SQD_CHECK_ARG(B > 0 && A > 0 && num_classes >= 1 && num_classes <= SQD_MAX_CLASSES);
  SQD_CHECK_ARG(((uintptr_t)pred & 15) == 0 && ((uintptr_t)det_box & 15) == 0);
  SQD_CHECK_ARG(!keys_ready || (keys_ws && ((uintptr_t)keys_ws & 15) == 0));
  DetArgs a;
  a.shifts = shifts;
  a.pred = pred; a.anchors = anchors; a.scales = scales; a.in_class = nullptr; a.in_score = nullptr; a.in_box = nullptr; a.keys = keys_ws;
  a.keys_ready = keys_ready;
  a.det_count = det_count; a.det_class = det_class; a.det_score = det_score; a.det_box = det_box; a.det_anchor = det_anchor;
  a.B = B; a.A = A; a.C = num_classes; a.K = keep_top_k;
  a.wmax = (float)(input_w - 1); a.hmax = (float)(input_h - 1);
  a.nms_thresh = nms_thresh; a.score_thresh = score_thresh;
  return launch_detect(a, (hipStream_t)stream);
}

extern "C" int sqd_detect_shift_fwd(const float* pred, const float* anchors, const float* scales, const float* shifts, unsigned* keys_ws,
                                    int* det_count, long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                    int num_classes, int input_h, int input_w, int keep_top_k, float nms_thresh,
                                    float score_thresh, void* stream) {
  return detect_pred(pred, anchors, scales, shifts, keys_ws, 0, det_count, det_class, det_score, det_box, det_anchor, B, A, num_classes,
                     input_h, input_w, keep_top_k, nms_thresh, score_thresh, stream);
}

extern "C" int sqd_detect_keys_fwd(const float* pred, const float* anchors, const float* scales, const float* shifts, unsigned* keys_ws,
                                   int* det_count, long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                   int num_classes, int input_h, int input_w, int keep_top_k, float nms_thresh,
                                   float score_thresh, void* stream) {
  return detect_pred(pred, anchors, scales, shifts, keys_ws, 1, det_count, det_class, det_score, det_box, det_anchor, B, A, num_classes,
                     input_h, input_w, keep_top_k, nms_thresh, score_thresh, stream);
}

extern "C" int sqd_detect_fwd(const float* pred, const float* anchors, const float* scales, unsigned* keys_ws, int* det_count,
                              long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                              int num_classes, int input_h, int input_w, int keep_top_k, float nms_thresh,
                              float score_thresh, void* stream) {
  (void)keys_ws;                      // (this entry point never required a sized workspace: one workgroup per image)
  return sqd_detect_shift_fwd(pred, anchors, scales, nullptr, nullptr, det_count, det_class, det_score, det_box, det_anchor, B, A,
                              num_classes, input_h, input_w, keep_top_k, nms_thresh, score_thresh, stream);
}

// Detector.filter(det) proper: the same kernel fed with already decoded dense tensors
// (class_ids int64 [B][A], scores [B][A], boxes [B][A][4]).
extern "C" int sqd_filter_fwd(const long long* class_ids, const float* scores, const float* boxes, unsigned* keys_ws, int* det_count,
                              long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                              int num_classes, int keep_top_k, float nms_thresh, float score_thresh, void* stream) {
  SQD_CHECK_ARG(class_ids && scores && boxes && det_count && det_class && det_score && det_box && det_anchor);
  SQD_CHECK_ARG(B > 0 && A > 0 && num_classes >= 1 && num_classes <= SQD_MAX_CLASSES);
  SQD_CHECK_ARG(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)det_box & 15) == 0);
  DetArgs a;
  a.shifts = nullptr;
  a.pred = nullptr; a.anchors = nullptr; a.scales = nullptr; a.in_class = class_ids; a.in_score = scores; a.in_box = boxes; a.keys = keys_ws;
  a.det_count = det_count; a.det_class = det_class; a.det_score = det_score; a.det_box = det_box; a.det_anchor = det_anchor;
  a.B = B; a.A = A; a.C = num_classes; a.K = keep_top_k;
  a.wmax = 0.f; a.hmax = 0.f; a.nms_thresh = nms_thresh; a.score_thresh = score_thresh;
  return launch_detect(a, (hipStream_t)stream);
}

// ---- wide fused detection: 1 <= K <= 1024, 1 <= A <= 2^20 -------------------------------------------------------------------------------
// The kernel above keeps an image's keys and its 64 x 64 suppression matrix in one workgroup's LDS and one wave's registers: K <= 64,
// A <= 25596.  This second path has the same inputs, outputs and semantics (oracle.filter_detections bit for bit: same key, same
// tie rule, same rank, same IoU expression, same output order, anchor_score / anchor_box shared with decode_kernel) without the two
// caps.  Two launches, stream-ordered, nothing carried from call to call:
//   1. detect_wide_score_kernel, grid over (image, 256-anchor slab): one key per anchor into the workspace [B][ceil4(A)] (the pad
//      keys of the last quad are written as 0, so the workspace needs no zeroing and every launch leaves it reusable);
//   2. detect_wide_select_kernel, one 1024-thread workgroup per image.  The keys stay in the workspace (L2-resident: 4 MB at A = 2^20)
//      and are streamed: 4 x 8-bit radix select of the K-th largest key (the first pass also counts the candidates M; M <= K skips the
//      rest), then one ordered sweep -- a contiguous run of quads per thread -- appends the keys above the K-th key (any order) and
//      the first `need` ties in ascending anchor order.  The <= K (key, ~anchor) pairs are ranked as 64-bit words by counting, one
//      per thread; thread r decodes the box of rank r.  The K x ceil(K/64) suppression bit matrix lives in LDS (128 KB at K = 1024):
//      its upper triangle is built in 64 x 64 blocks dealt round-robin to the 16 waves, wave 0 runs the greedy scan with the alive mask
//      held one 64-bit word per lane and eight row loads in flight ahead of the alive tests, and every thread places its own survivor
//      from per-wave per-class counts.
// Limits: K <= 1024 = one candidate per thread, and the matrix + candidates fit the 160 KB LDS; A <= 2^20 = gt_encode's limit.
#define DETW_THREADS 1024
#define DETW_MAX_K 1024
#define DETW_MAX_A (1 << 20)
#define DETW_SCORE_THREADS 256
#define DETW_LDS_FIXED (256 * 4 + 16 * 4 + 256 * 4 + 16 * 8 + 16)      // histogram, wave totals, class counts, alive words, scalars

typedef unsigned int u32x4_w __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(DETW_SCORE_THREADS) void detect_wide_score_kernel(DetArgs a) {
  const int A = a.A, C = a.C, A4 = (A + 3) & ~3;
  const int slabs = (A4 + DETW_SCORE_THREADS - 1) / DETW_SCORE_THREADS;
  const int b = (int)blockIdx.x / slabs;
  const int i = ((int)blockIdx.x - b * slabs) * DETW_SCORE_THREADS + (int)threadIdx.x;
  if (i >= A4) return;
  unsigned key = 0u;
  if (i < A) {
    if (a.in_score) {
      const float s = a.in_score[(long long)b * A + i];
      key = (s > a.score_thresh) ? __float_as_uint(s) : 0u;
    } else {
      // confidence first, as in detect_kernel: score <= conf, so conf <= threshold already decides key = 0, exactly
      const float* p = a.pred + ((long long)b * A + i) * (C + 5);
      const float conf = 1.f / (1.f + expf(-p[C]));
      if (conf > a.score_thresh) {
        float s; int c;
        anchor_score(p, C, s, c);
        key = (s > a.score_thresh) ? __float_as_uint(s) : 0u;
      }
    }
  }
  a.keys[(long long)b * A4 + i] = key;
}

// block-wide exclusive scan over one value per thread (fixed order -> deterministic); every thread of the workgroup calls it
__device__ __forceinline__ unsigned detw_excl_scan(unsigned c, unsigned& total, unsigned* wave_tot, int lane, int wave) {
  unsigned incl = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned t = __shfl_up(incl, off);
    if (lane >= off) incl += t;
  }
  __syncthreads();
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  unsigned woff = 0u, tot = 0u;
  for (int w = 0; w < DETW_THREADS / 64; ++w) { const unsigned t = wave_tot[w]; if (w < wave) woff += t; tot += t; }
  total = tot;
  return incl - c + woff;
}

// one histogram count per active lane.  Scores cluster (a few exponent bins in the leading pass, one bin in every pass when thousands
// of keys tie): the two most common bins of the wave are counted with one atomic each, only the rest lane by lane.  Whole waves call it.
__device__ __forceinline__ void detw_hist_add(unsigned* hist, bool act, unsigned bin, int lane) {
  unsigned long long todo = __ballot(act);
  for (int round = 0; round < 2 && todo; ++round) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned lb = __shfl(bin, leader);
    const unsigned long long same = __ballot(act && bin == lb);
    if (lane == leader) atomicAdd(&hist[lb], (unsigned)__popcll(same));
    todo &= ~same;
    act = act && bin != lb;
  }
  if (act) atomicAdd(&hist[bin], 1u);
}

// One detection row -- row `pos` of image b, boxes_postprocess' scale division and padding / crops shift folded in (see detect_kernel)
// -- for every placement of the wide kernels.  A macro, not a function, for the reason given in detw_select_body.h: the text is what
// detect_wide_select_kernel always held, so its device code stays what it was.
#define DETW_STORE_ROW(a, b, K, pos, cls, score, idx, bx) do { \
    float sx = 1.f, sy = 1.f; \
    if ((a).scales) { sy = (a).scales[2 * (b)]; sx = (a).scales[2 * (b) + 1]; } \
    const long long o = (long long)(b) * (K) + (pos); \
    (a).det_class[o] = (cls); \
    (a).det_score[o] = (score); \
    (a).det_anchor[o] = (idx); \
    f32x4 ob = (f32x4){(bx).x1 / sx, (bx).y1 / sy, (bx).x2 / sx, (bx).y2 / sy}; \
    if ((a).shifts) { const float dy = (a).shifts[2 * (b)], dx = (a).shifts[2 * (b) + 1]; ob.x += dx; ob.y += dy; ob.z += dx; ob.w += dy; } \
    *(f32x4*)((a).det_box + 4 * o) = ob; \
  } while (0)

// MANY = false: the <= 16-class form (thread r re-decodes rank r with anchor_score, placement from per-wave per-class counts).
// MANY = true: the many-class form (see "many-class head" below); everything that does not depend on C is shared.
template <bool MANY>
__global__ __launch_bounds__(DETW_THREADS) void detect_wide_select_kernel(DetArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int K = a.K, Kp = (K + 63) & ~63;                     // Kp <= 1024: one candidate slot per thread
  unsigned long long* cand = (unsigned long long*)smem_raw;   // [Kp] (key << 32) | ~anchor: larger word = earlier rank
  f32x4* boxL = (f32x4*)(cand + Kp);                          // [Kp] boxes in rank order
  int* clsL = (int*)(boxL + Kp);                              // [Kp] classes in rank order, -1 past the candidates
  unsigned* hist = (unsigned*)(clsL + Kp);                    // [256]
  unsigned* wave_tot = hist + 256;                            // [16]
  unsigned* cls_cnt = wave_tot + 16;                          // [16 waves][16 classes] survivors
  unsigned long long* aliveL = (unsigned long long*)(cls_cnt + 256);   // [16]
  unsigned* sv = (unsigned*)(aliveL + 16);                    // prefix, need, appended
  unsigned long long* mat = (unsigned long long*)(sv + 4);    // [64 Wn][Wn] suppression bits, Wn = ceil(candidates / 64) <= Kp / 64

#define DETW_PAD_ANY false
#include "detw_select_body.h"     // 1.-4. select, sweep, rank, decode: tid, lane, wave, b, A, C, ncand, ok, score, cls, idx, bx
#undef DETW_PAD_ANY

  // 5. suppression matrix: bit j of row i set if j ranks after i, same class, IoU > thresh.  Only blocks on or above the diagonal
  //    can hold bits: those Wn (Wn + 1) / 2 blocks of 64 rows x 64 columns go round-robin to the waves, lane = row; the rest is zeroed
  const int Wn = (ncand + 63) >> 6;
  for (int t = tid; t < 64 * Wn * Wn; t += DETW_THREADS) {
    const int i = t / Wn, w = t - i * Wn;
    if (w < (i >> 6)) mat[t] = 0ull;
  }
  for (int t = wave; t < Wn * (Wn + 1) / 2; t += DETW_THREADS / 64) {
    int rb = 0, rem = t;
    while (rem >= Wn - rb) { rem -= Wn - rb; ++rb; }
    const int w = rb + rem, i = rb * 64 + lane;
    const f32x4 me = boxL[i];
    const int mcls = clsL[i];
    const float area = (me.z - me.x) * (me.w - me.y);
    unsigned long long row = 0ull;
    for (int jj = 0; jj < 64; ++jj) {
      const int j = w * 64 + jj;
      const f32x4 o = boxL[j];
      const int jcls = clsL[j];
      const float jarea = (o.z - o.x) * (o.w - o.y);
      const float iw = fmaxf(0.f, fminf(me.z, o.z) - fmaxf(me.x, o.x));
      const float ih = fmaxf(0.f, fminf(me.w, o.w) - fmaxf(me.y, o.y));
      const float inter = iw * ih;
      const float ovr = inter / ((area + jarea) - inter);
      if (j > i && jcls == mcls && mcls >= 0 && ovr > a.nms_thresh) row |= 1ull << jj;
    }
    mat[(long long)i * Wn + w] = row;
  }
  __syncthreads();

  // 6. greedy scan on wave 0: lane w holds the alive bits of ranks 64 w .. 64 w + 63; the rows of eight ranks are loaded before
  //    their alive bits are tested (a row is applied only if its rank is still alive)
  if (wave == 0) {
    unsigned long long alive = 0ull;
    if (lane < Wn) { const int n = min(64, ncand - lane * 64); alive = (n >= 64) ? ~0ull : ((1ull << n) - 1ull); }
    for (int i0 = 0; i0 < ncand; i0 += 8) {
      unsigned long long rws[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) rws[u] = (lane < Wn) ? mat[(long long)(i0 + u) * Wn + lane] : 0ull;   // i0 + 7 < 64 Wn
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = i0 + u;
        const unsigned half = (i & 32) ? (unsigned)(alive >> 32) : (unsigned)alive;
        if ((__shfl(half, i >> 6) >> (i & 31)) & 1u) alive &= ~rws[u];
      }
    }
    if (lane < DETW_THREADS / 64) aliveL[lane] = alive;
  }
  __syncthreads();

  // 7. compaction: class 0..C-1, each class by rank, then the score threshold
  const bool keep = ok && ((aliveL[wave] >> lane) & 1ull) && score > a.score_thresh && cls >= 0 && cls < C;
  if (MANY) {
    // placement by counting (class, rank) pairs: a [16 waves][256 classes] count table does not fit beside the matrix at K = 1024,
    // and clsL is dead after the matrix was built -- it now holds the class of every survivor (-1: dropped); a survivor's row is the
    // number of survivors with a smaller (class, rank).  <= 1024 LDS broadcast reads per thread, independent of C.
    __syncthreads();
    if (tid < Kp) clsL[tid] = keep ? cls : -1;
    const unsigned long long km = __ballot(keep);
    if (lane == 0) wave_tot[wave] = (unsigned)__popcll(km);
    __syncthreads();
    if (tid == 0) {
      unsigned total = 0u;
      for (int w = 0; w < DETW_THREADS / 64; ++w) total += wave_tot[w];
      a.det_count[b] = (int)total;
    }
    if (keep) {
      unsigned pos = 0u;
      for (int r = 0; r < ncand; ++r) {
        const int cr = clsL[r];
        pos += (cr >= 0 && (cr < cls || (cr == cls && r < tid))) ? 1u : 0u;
      }
      DETW_STORE_ROW(a, b, K, pos, cls, score, idx, bx);
    }
    return;
  }
  unsigned long long mine = 0ull;
  for (int c = 0; c < C; ++c) {
    const unsigned long long m = __ballot(keep && cls == c);
    if (lane == 0) cls_cnt[wave * 16 + c] = (unsigned)__popcll(m);
    if (cls == c) mine = m;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned total = 0u;
    for (int w = 0; w < DETW_THREADS / 64; ++w)
      for (int c = 0; c < C; ++c) total += cls_cnt[w * 16 + c];
    a.det_count[b] = (int)total;
  }
  if (keep) {
    unsigned pos = (unsigned)__popcll(mine & ((1ull << lane) - 1ull));
    for (int w = 0; w < DETW_THREADS / 64; ++w) {
      for (int c = 0; c < cls; ++c) pos += cls_cnt[w * 16 + c];
      if (w < wave) pos += cls_cnt[w * 16 + cls];
    }
    DETW_STORE_ROW(a, b, K, pos, cls, score, idx, bx);
  }
}

// int32 words of the wide workspace: B x ceil4(A) keys.  -1: (B, A, K) is outside what the wide path takes.
extern "C" int sqd_detect_wide_workspace_words(int B, int A, int keep_top_k) {
  if (B < 1 || A < 1 || A > DETW_MAX_A || keep_top_k < 1 || keep_top_k > DETW_MAX_K) return -1;
  const long long words = (long long)B * ((A + 3) & ~3);
  return words > 0x7fffffffll ? -1 : (int)words;
}

static int launch_detect_wide(DetArgs a, int ws_words, hipStream_t stream) {
  SQD_CHECK_ARG(a.B > 0 && a.A > 0 && a.C >= 1 && a.K >= 1);
  if (a.K > DETW_MAX_K || a.A > DETW_MAX_A || a.C > SQD_MAX_CLASSES) return SQD_ERR_UNSUPPORTED;
  const int words = sqd_detect_wide_workspace_words(a.B, a.A, a.K);
  if (words < 0) return SQD_ERR_UNSUPPORTED;                  // (B x ceil4(A) past 2^31 - 1 words)
  SQD_CHECK_ARG(a.keys && ws_words >= words && ((uintptr_t)a.keys & 15) == 0);
  const int Kp = (a.K + 63) & ~63, A4 = (a.A + 3) & ~3;
  const size_t lds = (size_t)Kp * (8 + 16 + 4) + DETW_LDS_FIXED + (size_t)Kp * (Kp / 64) * 8;   // <= 162000 bytes at K = 1024
  static SqdDevOnce lds_once;
  if (lds > 48 * 1024 && sqd_max_lds_once(lds_once, (const void*)detect_wide_select_kernel<false>, 160 * 1024) != SQD_OK) return SQD_ERR_LAUNCH;
  const int slabs = (A4 + DETW_SCORE_THREADS - 1) / DETW_SCORE_THREADS;          // B x slabs <= 2^23 + B
  hipLaunchKernelGGL(detect_wide_score_kernel, dim3((unsigned)(a.B * slabs)), dim3(DETW_SCORE_THREADS), 0, stream, a);
  hipLaunchKernelGGL(detect_wide_select_kernel<false>, dim3((unsigned)a.B), dim3(DETW_THREADS), lds, stream, a);
  return sqd_launch_status();
}

// sqd_detect_shift_fwd for any 1 <= keep_top_k <= 1024 and 1 <= A <= 2^20: same outputs bit for bit where both run.  keys_ws: a
// 16-byte aligned workspace of ws_words >= sqd_detect_wide_workspace_words(B, A, keep_top_k) uint32, any contents; nothing in it
// carries over from launch to launch.  Status 2 for keep_top_k, A or num_classes past the limits, 1 for anything malformed
// (a null pointer, keep_top_k < 1, a short or misaligned workspace); nothing is launched then.
extern "C" int sqd_detect_wide_fwd(const float* pred, const float* anchors, const float* scales, const float* shifts, unsigned* keys_ws,
                                   int* det_count, long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                   int num_classes, int input_h, int input_w, int keep_top_k, float nms_thresh, float score_thresh,
                                   int ws_words, void* stream) {
  SQD_CHECK_ARG(pred && anchors && keys_ws && det_count && det_class && det_score && det_box && det_anchor);
  SQD_CHECK_ARG(((uintptr_t)pred & 15) == 0 && ((uintptr_t)det_box & 15) == 0);
  DetArgs a;
  a.shifts = shifts;
  a.pred = pred; a.anchors = anchors; a.scales = scales; a.in_class = nullptr; a.in_score = nullptr; a.in_box = nullptr; a.keys = keys_ws;
  a.S = 1; a.per = 0;
  a.det_count = det_count; a.det_class = det_class; a.det_score = det_score; a.det_box = det_box; a.det_anchor = det_anchor;
  a.B = B; a.A = A; a.C = num_classes; a.K = keep_top_k;
  a.wmax = (float)(input_w - 1); a.hmax = (float)(input_h - 1);
  a.nms_thresh = nms_thresh; a.score_thresh = score_thresh;
  return launch_detect_wide(a, ws_words, (hipStream_t)stream);
}

// sqd_filter_fwd for the same ranges (dense class_ids int64 [B][A], scores [B][A], boxes [B][A][4])
extern "C" int sqd_filter_wide_fwd(const long long* class_ids, const float* scores, const float* boxes, unsigned* keys_ws, int* det_count,
                                   long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                   int num_classes, int keep_top_k, float nms_thresh, float score_thresh, int ws_words, void* stream) {
  SQD_CHECK_ARG(class_ids && scores && boxes && keys_ws && det_count && det_class && det_score && det_box && det_anchor);
  SQD_CHECK_ARG(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)det_box & 15) == 0);
  DetArgs a;
  a.shifts = nullptr;
  a.pred = nullptr; a.anchors = nullptr; a.scales = nullptr; a.in_class = class_ids; a.in_score = scores; a.in_box = boxes; a.keys = keys_ws;
  a.S = 1; a.per = 0;
  a.det_count = det_count; a.det_class = det_class; a.det_score = det_score; a.det_box = det_box; a.det_anchor = det_anchor;
  a.B = B; a.A = A; a.C = num_classes; a.K = keep_top_k;
  a.wmax = 0.f; a.hmax = 0.f; a.nms_thresh = nms_thresh; a.score_thresh = score_thresh;
  return launch_detect_wide(a, ws_words, (hipStream_t)stream);
}

// ---- many-class head: 1 <= num_classes <= 256 = 16 lanes x 16 registers (many_class.h) ------------------------------------------------
// The same five roles as above -- decode, resolve, fused detect from pred, dense filter -- with a 16-lane group per anchor row instead
// of one lane.  mc_anchor_score is the only scoring routine (decode, the detect scoring kernel and the re-decode of the <= K
// candidates), so the fused detect equals the dense decode + filter bit for bit.  The detect is the wide two-launch structure:
// detect_many_score_kernel -> keys, then detect_wide_select_kernel<true>, which differs from the <= 16-class form in the re-decode
// and in the final placement only.  There is no one-launch narrow form past 16 classes.  The <= 16-class entry points keep their
// limit and their answers; these are separate functions that take any class count up to 256.
template <int R>
__global__ __launch_bounds__(MC_THREADS) void decode_many_kernel(const float* __restrict__ pred, const float* __restrict__ anchors,
                                                                 long long* __restrict__ class_ids, float* __restrict__ scores,
                                                                 float* __restrict__ boxes, int B, int A, int C, float wmax, float hmax) {
  const long long total = (long long)B * A;
  const int j = threadIdx.x & (MC_LANES - 1);
  for (long long i = (long long)blockIdx.x * MC_GROUPS + threadIdx.x / MC_LANES; i < total; i += (long long)gridDim.x * MC_GROUPS) {
    const float* p = pred + i * (C + 5);
    float s; int c;
    mc_anchor_score<R>(p, C, j, s, c);
    if (j == 0) {
      const BoxF b = anchor_box(p + C + 1, anchors + 4 * (int)(i % A), wmax, hmax);
      class_ids[i] = c; scores[i] = s;
      *(f32x4*)(boxes + 4 * i) = (f32x4){b.x1, b.y1, b.x2, b.y2};
    }
  }
}

template <int R>
__global__ __launch_bounds__(MC_THREADS) void resolve_many_kernel(const float* __restrict__ pred, const float* __restrict__ anchors,
                                                                  float* __restrict__ probs, float* __restrict__ logp, float* __restrict__ scores,
                                                                  float* __restrict__ deltas, float* __restrict__ boxes, int B, int A, int C,
                                                                  float wmax, float hmax) {
  const long long total = (long long)B * A;
  const int j = threadIdx.x & (MC_LANES - 1);
  for (long long i = (long long)blockIdx.x * MC_GROUPS + threadIdx.x / MC_LANES; i < total; i += (long long)gridDim.x * MC_GROUPS) {
    const float* p = pred + i * (C + 5);
    float l[R], e[R];
    const float m = mc_load_logits<R>(p, C, j, l);
    const float sum = mc_exp_sum<R>(C, j, m, l, e);
    const float lse = logf(sum);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int c = j + MC_LANES * r;
      if (c < C) {
        probs[i * C + c] = e[r] / sum;                           // safe_softmax (modules.py:66-68)
        if (logp) logp[i * C + c] = (l[r] - m) - lse;            // torch.log_softmax
      }
    }
    if (j == 0) {
      scores[i] = 1.f / (1.f + expf(-p[C]));
      const float* d = p + C + 1;
      *(f32x4*)(deltas + 4 * i) = (f32x4){d[0], d[1], d[2], d[3]};
      const BoxF b = anchor_box(d, anchors + 4 * (int)(i % A), wmax, hmax);
      *(f32x4*)(boxes + 4 * i) = (f32x4){b.x1, b.y1, b.x2, b.y2};
    }
  }
}

// keys of one 256-anchor slab of one image: a group takes the slab's anchors g, g + 16, ... (16 rounds); dense mode (in_score) and
// the pad keys of the last quad go one per thread as in detect_wide_score_kernel
template <int R>
__global__ __launch_bounds__(MC_THREADS) void detect_many_score_kernel(DetArgs a) {
  const int A = a.A, C = a.C, A4 = (A + 3) & ~3;
  const int slabs = (A4 + MC_THREADS - 1) / MC_THREADS;
  const int b = (int)blockIdx.x / slabs;
  const int base = ((int)blockIdx.x - b * slabs) * MC_THREADS;
  unsigned* __restrict__ keys = a.keys + (long long)b * A4;
  if (a.in_score) {
    const int i = base + (int)threadIdx.x;
    if (i >= A4) return;
    unsigned key = 0u;
    if (i < A) {
      const float s = a.in_score[(long long)b * A + i];
      key = (s > a.score_thresh) ? __float_as_uint(s) : 0u;
    }
    keys[i] = key;
    return;
  }
  const int j = threadIdx.x & (MC_LANES - 1), g = threadIdx.x / MC_LANES;
  for (int it = 0; it < MC_THREADS / MC_GROUPS; ++it) {
    const int i = base + it * MC_GROUPS + g;                   // (group-uniform)
    if (i >= A4) break;
    unsigned key = 0u;
    if (i < A) {
      // confidence first, as in detect_kernel: score <= conf, so conf <= threshold already decides key = 0, exactly
      const float* p = a.pred + ((long long)b * A + i) * (C + 5);
      const float conf = 1.f / (1.f + expf(-p[C]));
      if (conf > a.score_thresh) {
        float s; int c;
        mc_anchor_score<R>(p, C, j, s, c);
        key = (s > a.score_thresh) ? __float_as_uint(s) : 0u;
      }
    }
    if (j == 0) keys[i] = key;
  }
}

#define MC_CHECK_CLASSES(C) do { SQD_CHECK_ARG((C) >= 1); if ((C) > SQD_MANY_MAX_CLASSES) return SQD_ERR_UNSUPPORTED; } while (0)

static inline unsigned mc_row_blocks(long long rows) {
  const long long blocks = (rows + MC_GROUPS - 1) / MC_GROUPS;
  return (unsigned)(blocks < (1 << 20) ? blocks : (1 << 20));   // grid-stride past 2^24 rows
}

// sqd_decode_fwd for 1 <= num_classes <= 256.  Status 1 for anything malformed, 2 for num_classes > 256.
extern "C" int sqd_decode_many_fwd(const float* pred, const float* anchors, long long* class_ids, float* scores, float* boxes, int B, int A,
                                   int num_classes, int input_h, int input_w, void* stream) {
  SQD_CHECK_ARG(pred && anchors && class_ids && scores && boxes && B > 0 && A > 0);
  MC_CHECK_CLASSES(num_classes);
  SQD_CHECK_ARG(((uintptr_t)boxes & 15) == 0);
  const unsigned blocks = mc_row_blocks((long long)B * A);
#define CALL(R) hipLaunchKernelGGL(decode_many_kernel<R>, dim3(blocks), dim3(MC_THREADS), 0, (hipStream_t)stream, pred, anchors, class_ids, \
                                   scores, boxes, B, A, num_classes, (float)(input_w - 1), (float)(input_h - 1))
  MC_DISPATCH(num_classes, CALL);
#undef CALL
  return sqd_launch_status();
}

// sqd_resolve_fwd for 1 <= num_classes <= 256 (logp may be NULL)
extern "C" int sqd_resolve_many_fwd(const float* pred, const float* anchors, float* probs, float* logp, float* scores, float* deltas,
                                    float* boxes, int B, int A, int num_classes, int input_h, int input_w, void* stream) {
  SQD_CHECK_ARG(pred && anchors && probs && scores && deltas && boxes && B > 0 && A > 0);
  MC_CHECK_CLASSES(num_classes);
  SQD_CHECK_ARG(((uintptr_t)deltas & 15) == 0 && ((uintptr_t)boxes & 15) == 0);
  const unsigned blocks = mc_row_blocks((long long)B * A);
#define CALL(R) hipLaunchKernelGGL(resolve_many_kernel<R>, dim3(blocks), dim3(MC_THREADS), 0, (hipStream_t)stream, pred, anchors, probs, logp, \
                                   scores, deltas, boxes, B, A, num_classes, (float)(input_w - 1), (float)(input_h - 1))
  MC_DISPATCH(num_classes, CALL);
#undef CALL
  return sqd_launch_status();
}

static int launch_detect_many(DetArgs a, int ws_words, hipStream_t stream) {
  SQD_CHECK_ARG(a.B > 0 && a.A > 0 && a.C >= 1 && a.K >= 1);
  if (a.K > DETW_MAX_K || a.A > DETW_MAX_A || a.C > SQD_MANY_MAX_CLASSES) return SQD_ERR_UNSUPPORTED;
  const int words = sqd_detect_wide_workspace_words(a.B, a.A, a.K);
  if (words < 0) return SQD_ERR_UNSUPPORTED;                  // (B x ceil4(A) past 2^31 - 1 words)
  SQD_CHECK_ARG(a.keys && ws_words >= words && ((uintptr_t)a.keys & 15) == 0);
  const int Kp = (a.K + 63) & ~63, A4 = (a.A + 3) & ~3;
  const size_t lds = (size_t)Kp * (8 + 16 + 4) + DETW_LDS_FIXED + (size_t)Kp * (Kp / 64) * 8;   // the <= 16-class form's, unchanged
  static SqdDevOnce lds_once;
  if (lds > 48 * 1024 && sqd_max_lds_once(lds_once, (const void*)detect_wide_select_kernel<true>, 160 * 1024) != SQD_OK) return SQD_ERR_LAUNCH;
  const int slabs = (A4 + MC_THREADS - 1) / MC_THREADS;
#define CALL(R) hipLaunchKernelGGL(detect_many_score_kernel<R>, dim3((unsigned)(a.B * slabs)), dim3(MC_THREADS), 0, stream, a)
  MC_DISPATCH(a.C, CALL);
#undef CALL
  hipLaunchKernelGGL(detect_wide_select_kernel<true>, dim3((unsigned)a.B), dim3(DETW_THREADS), lds, stream, a);
  return sqd_launch_status();
}

// sqd_detect_wide_fwd for 1 <= num_classes <= 256: same arguments, same workspace (sqd_detect_wide_workspace_words), every
// 1 <= keep_top_k <= 1024 and 1 <= A <= 2^20.  Status 2 for num_classes > 256, keep_top_k > 1024 or A > 2^20; 1 for anything malformed.
extern "C" int sqd_detect_many_fwd(const float* pred, const float* anchors, const float* scales, const float* shifts, unsigned* keys_ws,
                                   int* det_count, long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                   int num_classes, int input_h, int input_w, int keep_top_k, float nms_thresh, float score_thresh,
                                   int ws_words, void* stream) {
  SQD_CHECK_ARG(pred && anchors && keys_ws && det_count && det_class && det_score && det_box && det_anchor);
  SQD_CHECK_ARG(((uintptr_t)det_box & 15) == 0);
  DetArgs a;
  a.shifts = shifts;
  a.pred = pred; a.anchors = anchors; a.scales = scales; a.in_class = nullptr; a.in_score = nullptr; a.in_box = nullptr; a.keys = keys_ws;
  a.S = 1; a.per = 0;
  a.det_count = det_count; a.det_class = det_class; a.det_score = det_score; a.det_box = det_box; a.det_anchor = det_anchor;
  a.B = B; a.A = A; a.C = num_classes; a.K = keep_top_k;
  a.wmax = (float)(input_w - 1); a.hmax = (float)(input_h - 1);
  a.nms_thresh = nms_thresh; a.score_thresh = score_thresh;
  return launch_detect_many(a, ws_words, (hipStream_t)stream);
}

// sqd_filter_wide_fwd for class ids up to 255
extern "C" int sqd_filter_many_fwd(const long long* class_ids, const float* scores, const float* boxes, unsigned* keys_ws, int* det_count,
                                   long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                   int num_classes, int keep_top_k, float nms_thresh, float score_thresh, int ws_words, void* stream) {
  SQD_CHECK_ARG(class_ids && scores && boxes && keys_ws && det_count && det_class && det_score && det_box && det_anchor);
  SQD_CHECK_ARG(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)det_box & 15) == 0);
  DetArgs a;
  a.shifts = nullptr;
  a.pred = nullptr; a.anchors = nullptr; a.scales = nullptr; a.in_class = class_ids; a.in_score = scores; a.in_box = boxes; a.keys = keys_ws;
  a.S = 1; a.per = 0;
  a.det_count = det_count; a.det_class = det_class; a.det_score = det_score; a.det_box = det_box; a.det_anchor = det_anchor;
  a.B = B; a.A = A; a.C = num_classes; a.K = keep_top_k;
  a.wmax = 0.f; a.hmax = 0.f; a.nms_thresh = nms_thresh; a.score_thresh = score_thresh;
  return launch_detect_many(a, ws_words, (hipStream_t)stream);
}

// ---- NMS modes: Soft-NMS (linear / Gaussian, Bodla et al. 2017) and class-agnostic NMS ------------------------------------------------
// The wide two-launch structure with another suppression step: the scoring launch (or ConvDet's epilogue: keys_ready) fills the key
// workspace, detect_nms_select_kernel -- one 1024-thread workgroup per image -- runs detw_select_body.h (the selection, ranking and
// decode of detect_wide_select_kernel, the same text) and then, instead of the bit matrix, the rule of DESIGN.md section 3 "NMS modes":
//   groups = the classes 0 .. C-1 (agnostic: one group of all candidates).  Within a group, repeatedly pick the candidate with the
//   largest current score (tie: the lower rank); stop when that score is not above score_thresh; emit it with its current score; then
//   for every remaining candidate j of the group, with u = IoU(pick, j) -- detect_kernel's fp32 expression
//   inter / ((area_i + area_j) - inter) --   hard: drop j if u > nms_thresh;   linear: if u > nms_thresh, s_j = s_j * (1 - u);
//   gaussian: s_j = s_j * expf(-(u * u) / sigma) for every j.  Output: groups in class order, each in pick order.
// Why stopping at the first pick at or below the threshold equals thresholding after a full scan: scores only fall (every factor is in
// [0, 1]), so once the largest current score of a group is at or below the threshold every remaining one is and stays there, and a
// pick at or below the threshold could only decay candidates that the same threshold drops anyway -- the emitted rows and their scores
// are those of the full scan followed by the threshold (the argument of the pre-filter above, applied to the tail of the scan).
// A soft pick changes the scores that decide the next pick, so the scan is sequential; its state is ONE float per candidate (the
// current score; -1 = emitted or dropped, never picked again) and the IoUs are computed at pick time, one per remaining candidate
// per step -- no K x K matrix.  The candidates are first ordered by (group, rank), every group a contiguous segment, then:
//   * class-wise: the groups are dealt to the 16 waves.  A group of <= 64 candidates is one wave with box and score in registers:
//     a step = a 6-step cross-lane max, a ballot (lowest lane = lowest rank wins a tie), one broadcast LDS read of the pick's box,
//     one IoU per lane; no barrier.  A longer group strides over the lanes of its wave with the scores in LDS, each step one fused
//     pass (apply the pick, find the lane's next maximum);
//   * agnostic with more than 64 candidates -- the one case where a single group is worth more than a wave: candidate p sits in
//     thread p's registers, a step = wave-local argmax, one slot per wave in LDS, ONE barrier (the slots alternate between two
//     banks, so the next step's writes never meet this step's reads), then every wave reduces the 16 slots redundantly.
// Steps = emitted rows + 1 per group, not K.  The placement is that of the hard kernels: a row = (rows of earlier groups) + pick order.
// NaN: a current score that becomes NaN (Gaussian mode on two zero-area boxes: u = 0 / 0) is never picked and never emitted.
#define NMS_HARD 0
#define NMS_LINEAR 1
#define NMS_GAUSSIAN 2
#define NMS_LDS_FIXED (256 * 4 + 16 * 4 + 16 + 4 * 256 * 4 + 2 * 16 * 8)     // histogram, wave totals, scalars, 4 group tables, argmax slots

struct NmsArgs { int mode; float sigma; int agnostic; };

__device__ __forceinline__ float nms_wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

__device__ __forceinline__ int nms_wave_min(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}

// current score s of a remaining candidate after the pick `pk` (area pa) was emitted; o = the candidate's box
__device__ __forceinline__ float nms_decay(const NmsArgs n, float nms_thresh, const f32x4 pk, float pa, const f32x4 o, float s) {
  const float oa = (o.z - o.x) * (o.w - o.y);
  const float iw = fmaxf(0.f, fminf(pk.z, o.z) - fmaxf(pk.x, o.x));
  const float ih = fmaxf(0.f, fminf(pk.w, o.w) - fmaxf(pk.y, o.y));
  const float inter = iw * ih;
  const float u = inter / ((pa + oa) - inter);
  if (n.mode == NMS_GAUSSIAN) return s * expf(-(u * u) / n.sigma);
  if (u > nms_thresh) return n.mode == NMS_LINEAR ? s * (1.f - u) : -1.f;
  return s;
}

template <bool MANY>
__global__ __launch_bounds__(DETW_THREADS) void detect_nms_select_kernel(DetArgs a, NmsArgs n) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int K = a.K, Kp = (K + 63) & ~63;                     // Kp <= 1024: one candidate slot per thread
  unsigned long long* cand = (unsigned long long*)smem_raw;   // [Kp] as detect_wide_select_kernel
  f32x4* boxL = (f32x4*)(cand + Kp);                          // [Kp] boxes in rank order
  f32x4* boxP = boxL + Kp;                                    // [Kp] boxes in (group, rank) order
  int* clsL = (int*)(boxP + Kp);                              // [Kp] classes in rank order
  int* grpL = clsL + Kp;                                      // [Kp] group of rank r, -1: none (no candidate, class outside 0 .. C-1)
  float* curL = (float*)(grpL + Kp);                          // [Kp] current scores in (group, rank) order
  float* outS = curL + Kp;                                    // [Kp] score at pick time
  int* emitL = (int*)(outS + Kp);                             // [Kp] pick order within the group, -1: not emitted
  unsigned* hist = (unsigned*)(emitL + Kp);                   // [256]
  unsigned* wave_tot = hist + 256;                            // [16]
  unsigned* sv = wave_tot + 16;                               // prefix, need, appended
  int* gstart = (int*)(sv + 4);                               // [256] first slot of a group
  int* glen = gstart + 256;                                   // [256] its candidates
  unsigned* gcnt = (unsigned*)(glen + 256);                   // [256] its emitted rows
  unsigned* goff = gcnt + 256;                                // [256] rows of the groups before it
  float* slot_s = (float*)(goff + 256);                       // [2][16] a wave's best current score ...
  int* slot_p = (int*)(slot_s + 32);                          // [2][16] ... and its slot

#define DETW_PAD_ANY true
#include "detw_select_body.h"     // 1.-4. select, sweep, rank, decode: tid, lane, wave, b, A, C, ncand, ok, score, cls, idx, bx
#undef DETW_PAD_ANY
#define DETN_STORE(pos, sc) DETW_STORE_ROW(a, b, K, pos, cls, sc, idx, bx)
#include "detn_scan_body.h"     // 5.-7. (group, rank) order, the scan, the placement
#undef DETN_STORE
}

static int launch_detect_nms(DetArgs a, NmsArgs n, int ws_words, hipStream_t stream) {
  SQD_CHECK_ARG(a.B > 0 && a.A > 0 && a.C >= 1 && a.K >= 1);
  SQD_CHECK_ARG(n.mode == NMS_HARD || n.mode == NMS_LINEAR || n.mode == NMS_GAUSSIAN);
  SQD_CHECK_ARG(n.mode != NMS_GAUSSIAN || (isfinite(n.sigma) && n.sigma > 0.f));
  SQD_CHECK_ARG(a.score_thresh >= 0.f);                       // (the keys: see ops._check_score_thresh; the scan's -1 marks rely on it too)
  if (a.K > DETW_MAX_K || a.A > DETW_MAX_A || a.C > SQD_MANY_MAX_CLASSES) return SQD_ERR_UNSUPPORTED;
  const int words = sqd_detect_wide_workspace_words(a.B, a.A, a.K);
  if (words < 0) return SQD_ERR_UNSUPPORTED;                  // (B x ceil4(A) past 2^31 - 1 words)
  SQD_CHECK_ARG(a.keys && ws_words >= words && ((uintptr_t)a.keys & 15) == 0);
  const bool many = a.C > SQD_MAX_CLASSES;
  SQD_CHECK_ARG(!a.keys_ready || (a.pred && !many));          // ConvDet's epilogue writes the <= 16-class keys of a pred
  const int Kp = (a.K + 63) & ~63, A4 = (a.A + 3) & ~3;
  const size_t lds = (size_t)Kp * (8 + 16 + 16 + 4 * 5) + NMS_LDS_FIXED;           // <= 67 KB at K = 1024
  static SqdDevOnce once_few, once_many;
  if (lds > 48 * 1024 && (many ? sqd_max_lds_once(once_many, (const void*)detect_nms_select_kernel<true>, 96 * 1024)
                               : sqd_max_lds_once(once_few, (const void*)detect_nms_select_kernel<false>, 96 * 1024)) != SQD_OK)
    return SQD_ERR_LAUNCH;
  if (!a.keys_ready) {
    if (many) {
      const int slabs = (A4 + MC_THREADS - 1) / MC_THREADS;
#define CALL(R) hipLaunchKernelGGL(detect_many_score_kernel<R>, dim3((unsigned)(a.B * slabs)), dim3(MC_THREADS), 0, stream, a)
      MC_DISPATCH(a.C, CALL);
#undef CALL
    } else {
      const int slabs = (A4 + DETW_SCORE_THREADS - 1) / DETW_SCORE_THREADS;
      hipLaunchKernelGGL(detect_wide_score_kernel, dim3((unsigned)(a.B * slabs)), dim3(DETW_SCORE_THREADS), 0, stream, a);
    }
  }
  if (many) hipLaunchKernelGGL(detect_nms_select_kernel<true>, dim3((unsigned)a.B), dim3(DETW_THREADS), lds, stream, a, n);
  else hipLaunchKernelGGL(detect_nms_select_kernel<false>, dim3((unsigned)a.B), dim3(DETW_THREADS), lds, stream, a, n);
  return sqd_launch_status();
}

// sqd_detect_wide_fwd / sqd_detect_many_fwd (either head form: 1 <= num_classes <= 256) with the suppression rule as an argument:
// nms_mode 0 hard, 1 linear, 2 gaussian (nms_sigma finite and > 0, read in that mode only); nms_agnostic != 0: one group for all
// classes.  keys_ready != 0 (num_classes <= 16): keys_ws already holds the keys of this pred ([B][ceil4(A)], written by
// sqd_conv_wino_vs_keys_fwd with the same score_thresh earlier on the same stream; the pad words may hold anything) -- no scoring
// launch.  (hard, class-wise) gives sqd_detect_wide_fwd's rows bit for bit.  Status 1 for anything malformed, an unknown mode, a bad
// sigma or a negative score_thresh included; 2 past the limits; nothing is launched then.
extern "C" int sqd_detect_nms_fwd(const float* pred, const float* anchors, const float* scales, const float* shifts, unsigned* keys_ws,
                                  int* det_count, long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                  int num_classes, int input_h, int input_w, int keep_top_k, float nms_thresh, float score_thresh,
                                  int ws_words, int nms_mode, float nms_sigma, int nms_agnostic, int keys_ready, void* stream) {
  SQD_CHECK_ARG(pred && anchors && keys_ws && det_count && det_class && det_score && det_box && det_anchor);
  SQD_CHECK_ARG(((uintptr_t)det_box & 15) == 0 && (num_classes > SQD_MAX_CLASSES || ((uintptr_t)pred & 15) == 0));
  DetArgs a;
  a.shifts = shifts;
  a.pred = pred; a.anchors = anchors; a.scales = scales; a.in_class = nullptr; a.in_score = nullptr; a.in_box = nullptr; a.keys = keys_ws;
  a.keys_ready = keys_ready ? 1 : 0;
  a.S = 1; a.per = 0;
  a.det_count = det_count; a.det_class = det_class; a.det_score = det_score; a.det_box = det_box; a.det_anchor = det_anchor;
  a.B = B; a.A = A; a.C = num_classes; a.K = keep_top_k;
  a.wmax = (float)(input_w - 1); a.hmax = (float)(input_h - 1);
  a.nms_thresh = nms_thresh; a.score_thresh = score_thresh;
  const NmsArgs n = {nms_mode, nms_sigma, nms_agnostic ? 1 : 0};
  return launch_detect_nms(a, n, ws_words, (hipStream_t)stream);
}

// sqd_filter_wide_fwd / sqd_filter_many_fwd with the same four arguments (keys_ready must be 0: dense scores have no ConvDet keys)
extern "C" int sqd_filter_nms_fwd(const long long* class_ids, const float* scores, const float* boxes, unsigned* keys_ws, int* det_count,
                                  long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                  int num_classes, int keep_top_k, float nms_thresh, float score_thresh, int ws_words,
                                  int nms_mode, float nms_sigma, int nms_agnostic, int keys_ready, void* stream) {
  SQD_CHECK_ARG(class_ids && scores && boxes && keys_ws && det_count && det_class && det_score && det_box && det_anchor);
  SQD_CHECK_ARG(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)det_box & 15) == 0 && !keys_ready);
  DetArgs a;
  a.shifts = nullptr;
  a.pred = nullptr; a.anchors = nullptr; a.scales = nullptr; a.in_class = class_ids; a.in_score = scores; a.in_box = boxes; a.keys = keys_ws;
  a.S = 1; a.per = 0;
  a.det_count = det_count; a.det_class = det_class; a.det_score = det_score; a.det_box = det_box; a.det_anchor = det_anchor;
  a.B = B; a.A = A; a.C = num_classes; a.K = keep_top_k;
  a.wmax = 0.f; a.hmax = 0.f; a.nms_thresh = nms_thresh; a.score_thresh = score_thresh;
  const NmsArgs n = {nms_mode, nms_sigma, nms_agnostic ? 1 : 0};
  return launch_detect_nms(a, n, ws_words, (hipStream_t)stream);
}

// ---- pooled views: V network views of one image, one top-k and one suppression in image coordinates (DESIGN.md section 3 "Pooled views") ----
// Test-time augmentation (the image, its mirror image, other scales) and sliced inference (overlapping tiles of a large frame) are the
// same operation: pred holds V rows per image -- view v of image b is row b * V + v -- and view_xf [B * V][6] = (sy, sx, dy, dx, flip,
// mirror) says how a row's canvas maps into the image.  The rule:
//   candidates of image b = all pairs (v, a), pooled index p = v * A + a; key = the score key of every other detect launch (score >
//   score_thresh), so the scoring launches run unchanged on the B * V rows; top K of the pool by (score descending, p ascending) --
//   equal scores in two views go to the lower view; the box of a candidate is anchor_box's (clamped to the canvas), then in fp32, op
//   for op (no contraction: -ffp-contract=off)   x' = x / sx + dx,   y' = y / sy + dy   -- DETW_STORE_ROW's expression: one division,
//   one addition --   and, if flip != 0,   (x1'', x2'') = (mirror - x2', mirror - x1');   then the rule of "NMS modes" (hard, linear,
//   Gaussian; class-wise or agnostic) on those IMAGE-coordinate boxes.  Rows come out in class order and pick order, det_box is the
//   image box (nothing more is applied at the store), det_anchor = p (view = p / A, anchor = p % A), det_score the current score at
//   pick time.
// The division comes before the IoU because the views have different scales: two canvas boxes of different views are not comparable.
// V = 1 with view_xf = (1, 1, 0, 0, 0, 0) gives sqd_detect_nms_fwd's rows bit for bit; with another scale it need not (that launch
// suppresses on canvas boxes and divides afterwards).
// Two launches, as the other wide forms: the scoring kernel of the head form on B * V rows -> the workspace [B * V][ceil4(A)], pad words
// 0, so that the V key rows of an image ARE one pooled row of V * ceil4(A) words; then detect_views_select_kernel, one 1024-thread
// workgroup per image: steps 1-3 of detw_select_body.h over the pooled row, its view-aware step 4 (DETW_VIEWS), and the scan of
// detect_nms_select_kernel (detn_scan_body.h), the same text.  LDS: that kernel's.  The view data is a kernel argument of its own, so
// DetArgs and every other kernel stay what they were.  Limits: V >= 1, V * ceil4(A) <= 2^20, K <= 1024, C <= 256.
struct ViewArgs { const float* xf; int V; };

// a canvas box of a view in image coordinates; xf = (sy, sx, dy, dx, flip, mirror) of that view
__device__ __forceinline__ BoxF detv_map(BoxF c, const float* __restrict__ xf) {
  const float sy = xf[0], sx = xf[1], dy = xf[2], dx = xf[3];
  BoxF m;
  m.x1 = c.x1 / sx + dx;
  m.y1 = c.y1 / sy + dy;
  m.x2 = c.x2 / sx + dx;
  m.y2 = c.y2 / sy + dy;
  if (xf[4] != 0.f) {
    const float mirror = xf[5], t = mirror - m.x2;
    m.x2 = mirror - m.x1;
    m.x1 = t;
  }
  return m;
}

// one detection row of the pooled launch: the box is already the image box
#define DETV_STORE_ROW(a, b, K, pos, cls, score, idx, bx) do { \
    const long long o = (long long)(b) * (K) + (pos); \
    (a).det_class[o] = (cls); \
    (a).det_score[o] = (score); \
    (a).det_anchor[o] = (idx); \
    *(f32x4*)((a).det_box + 4 * o) = (f32x4){(bx).x1, (bx).y1, (bx).x2, (bx).y2}; \
  } while (0)

template <bool MANY>
__global__ __launch_bounds__(DETW_THREADS) void detect_views_select_kernel(DetArgs a, NmsArgs n, ViewArgs vw) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int K = a.K, Kp = (K + 63) & ~63;                     // the layout of detect_nms_select_kernel
  unsigned long long* cand = (unsigned long long*)smem_raw;
  f32x4* boxL = (f32x4*)(cand + Kp);
  f32x4* boxP = boxL + Kp;
  int* clsL = (int*)(boxP + Kp);
  int* grpL = clsL + Kp;
  float* curL = (float*)(grpL + Kp);
  float* outS = curL + Kp;
  int* emitL = (int*)(outS + Kp);
  unsigned* hist = (unsigned*)(emitL + Kp);
  unsigned* wave_tot = hist + 256;
  unsigned* sv = wave_tot + 16;
  int* gstart = (int*)(sv + 4);
  int* glen = gstart + 256;
  unsigned* gcnt = (unsigned*)(glen + 256);
  unsigned* goff = gcnt + 256;
  float* slot_s = (float*)(goff + 256);
  int* slot_p = (int*)(slot_s + 32);

#define DETW_PAD_ANY false
#define DETW_VIEWS vw.V
#define DETW_VIEW_XF vw.xf
#include "detw_select_body.h"     // 1.-3. over the pooled row, 4. the view-aware decode: idx = p, bx = the image box
#undef DETW_VIEW_XF
#undef DETW_VIEWS
#undef DETW_PAD_ANY
#define DETN_STORE(pos, sc) DETV_STORE_ROW(a, b, K, pos, cls, sc, idx, bx)
#include "detn_scan_body.h"       // 5.-7. (group, rank) order, the scan, the placement
#undef DETN_STORE
}

// Pooled-view fused detect: pred [B * V][A][C + 5] (view v of image b = row b * V + v), anchors [A][4], view_xf fp32 [B * V][6] =
// (sy, sx, dy, dx, flip, mirror); the five result buffers are [B] / [B][K].  keys_ws: 16-byte aligned, ws_words >=
// sqd_detect_wide_workspace_words(B * V, A, keep_top_k) = B * V * ceil4(A) uint32, any contents.  Either head form (1 <= num_classes
// <= 256); nms_mode / nms_sigma / nms_agnostic as sqd_detect_nms_fwd.  Status 2 past the limits (V * ceil4(A) > 2^20, keep_top_k >
// 1024, num_classes > 256, a workspace past 2^31 - 1 words); 1 for anything malformed (a null pointer, V < 1, a short or misaligned
// workspace, an unknown mode, a bad sigma, a negative score_thresh); nothing is launched in either case.
extern "C" int sqd_detect_views_fwd(const float* pred, const float* anchors, const float* view_xf, unsigned* keys_ws, int* det_count,
                                    long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int V, int A,
                                    int num_classes, int input_h, int input_w, int keep_top_k, float nms_thresh, float score_thresh,
                                    int ws_words, int nms_mode, float nms_sigma, int nms_agnostic, void* stream) {
  SQD_CHECK_ARG(pred && anchors && view_xf && keys_ws && det_count && det_class && det_score && det_box && det_anchor);
  SQD_CHECK_ARG(((uintptr_t)det_box & 15) == 0 && (num_classes > SQD_MAX_CLASSES || ((uintptr_t)pred & 15) == 0));
  SQD_CHECK_ARG(B > 0 && V >= 1 && A > 0 && num_classes >= 1 && keep_top_k >= 1);
  SQD_CHECK_ARG(nms_mode == NMS_HARD || nms_mode == NMS_LINEAR || nms_mode == NMS_GAUSSIAN);
  SQD_CHECK_ARG(nms_mode != NMS_GAUSSIAN || (isfinite(nms_sigma) && nms_sigma > 0.f));
  SQD_CHECK_ARG(score_thresh >= 0.f);
  if (keep_top_k > DETW_MAX_K || A > DETW_MAX_A || num_classes > SQD_MANY_MAX_CLASSES) return SQD_ERR_UNSUPPORTED;
  const int A4 = (A + 3) & ~3;
  if ((long long)V * A4 > DETW_MAX_A || (long long)B * V > 0x7fffffffll) return SQD_ERR_UNSUPPORTED;
  const int rows = B * V;
  const int words = sqd_detect_wide_workspace_words(rows, A, keep_top_k);
  if (words < 0) return SQD_ERR_UNSUPPORTED;                  // (B x V x ceil4(A) past 2^31 - 1 words)
  SQD_CHECK_ARG(ws_words >= words && ((uintptr_t)keys_ws & 15) == 0);
  DetArgs a;
  a.shifts = nullptr;
  a.pred = pred; a.anchors = anchors; a.scales = nullptr; a.in_class = nullptr; a.in_score = nullptr; a.in_box = nullptr; a.keys = keys_ws;
  a.S = 1; a.per = 0;
  a.det_count = det_count; a.det_class = det_class; a.det_score = det_score; a.det_box = det_box; a.det_anchor = det_anchor;
  a.B = rows; a.A = A; a.C = num_classes; a.K = keep_top_k;
  a.wmax = (float)(input_w - 1); a.hmax = (float)(input_h - 1);
  a.nms_thresh = nms_thresh; a.score_thresh = score_thresh;
  const NmsArgs n = {nms_mode, nms_sigma, nms_agnostic ? 1 : 0};
  const ViewArgs vw = {view_xf, V};
  const bool many = num_classes > SQD_MAX_CLASSES;
  const int Kp = (keep_top_k + 63) & ~63;
  const size_t lds = (size_t)Kp * (8 + 16 + 16 + 4 * 5) + NMS_LDS_FIXED;           // detect_nms_select_kernel's: <= 67 KB at K = 1024
  static SqdDevOnce once_few, once_many;
  if (lds > 48 * 1024 && (many ? sqd_max_lds_once(once_many, (const void*)detect_views_select_kernel<true>, 96 * 1024)
                               : sqd_max_lds_once(once_few, (const void*)detect_views_select_kernel<false>, 96 * 1024)) != SQD_OK)
    return SQD_ERR_LAUNCH;
  hipStream_t st = (hipStream_t)stream;
  if (many) {                                                 // the scoring launch of the head form, on the B * V rows
    const int slabs = (A4 + MC_THREADS - 1) / MC_THREADS;
#define CALL(R) hipLaunchKernelGGL(detect_many_score_kernel<R>, dim3((unsigned)((long long)rows * slabs)), dim3(MC_THREADS), 0, st, a)
    MC_DISPATCH(a.C, CALL);
#undef CALL
  } else {
    const int slabs = (A4 + DETW_SCORE_THREADS - 1) / DETW_SCORE_THREADS;
    hipLaunchKernelGGL(detect_wide_score_kernel, dim3((unsigned)((long long)rows * slabs)), dim3(DETW_SCORE_THREADS), 0, st, a);
  }
  a.B = B;
  if (many) hipLaunchKernelGGL(detect_views_select_kernel<true>, dim3((unsigned)B), dim3(DETW_THREADS), lds, st, a, n, vw);
  else hipLaunchKernelGGL(detect_views_select_kernel<false>, dim3((unsigned)B), dim3(DETW_THREADS), lds, st, a, n, vw);
  return sqd_launch_status();
}
