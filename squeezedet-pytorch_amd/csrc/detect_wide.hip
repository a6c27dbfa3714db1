// Wide fused detection: 1 <= K <= 1024, 1 <= A <= 2^20, 1 <= num_classes <= 256, with the suppression rule and pooled views as arguments.
// detect_kernel (postproc.hip) keeps an image's keys and its 64 x 64 suppression matrix in one workgroup's LDS and one wave's registers:
// K <= 64, A <= 25596, <= 16 classes.  This family has the same inputs, outputs and semantics (oracle.filter_detections bit for bit:
// same key, same tie rule, same rank, same IoU expression, same output order, anchor_score / anchor_box shared with decode_kernel)
// without the caps.  Two launches, stream-ordered, nothing carried from call to call:
//   1. a scoring kernel, grid over (image, 256-anchor slab): one key per anchor into the workspace [B][ceil4(A)] (the pad keys of the
//      last quad are written as 0, so the workspace needs no zeroing and every launch leaves it reusable).  detect_wide_score_kernel
//      up to 16 classes (one lane per anchor), detect_many_score_kernel<R> up to 256 (a 16-lane group per anchor, many_class.h);
//   2. a select kernel, one 1024-thread workgroup per image.  The keys stay in the workspace (L2-resident: 4 MB at A = 2^20) and are
//      streamed: 4 x 8-bit radix select of the K-th largest key (the first pass also counts the candidates M; M <= K skips the rest),
//      then one ordered sweep -- a contiguous run of quads per thread -- appends the keys above the K-th key (any order) and the
//      first `need` ties in ascending anchor order.  The <= K (key, ~anchor) pairs are ranked as 64-bit words by counting, one per
//      thread; thread r decodes the box of rank r (steps 1-4: detw_select_body.h).  Then the suppression:
//      * detect_wide_select_kernel<MANY>, hard class-wise NMS: the K x ceil(K/64) suppression bit matrix lives in LDS (128 KB at K =
//        1024): its upper triangle is built in 64 x 64 blocks dealt round-robin to the 16 waves, wave 0 runs the greedy scan with the
//        alive mask held one 64-bit word per lane and eight row loads in flight ahead of the alive tests, and every thread places its
//        own survivor;
//      * detect_nms_select_kernel<MANY>, any rule ("NMS modes" below), and detect_views_select_kernel<MANY>, the same on the pooled
//        candidates of V views ("pooled views" below): the sequential scan of detn_scan_body.h;
//      * detect_vote_select_kernel<MANY> and detect_views_vote_select_kernel<MANY>: those two with the voting step between the scan
//        and the store ("box voting" below).
// The select kernels keep the device code they always had: steps 1-4 and the scan are shared as included text, steered by
// DETW_PAD_ANY / DETW_VIEWS / DETN_STORE.  As __forceinline__ functions they computed the same rows bit for bit, but every one of
// them had a figure slower than the parent build's slowest repeat (profiles/detect_family_refactor_ab.json), so that form was kept back.
// MANY is the head form: false = thread r re-decodes rank r with anchor_score, true = a 16-lane group per candidate with
// mc_anchor_score (the only scoring routine past 16 classes, so the fused detect equals the dense decode + filter bit for bit) and a
// placement that does not need a per-class table.
// Limits: K <= 1024 = one candidate per thread, and the matrix + candidates fit the 160 KB LDS; A <= 2^20 = gt_encode's limit.
#include "detect_common.h"
#include "anchor_score.h"
#include "many_class.h"

#define DETW_THREADS 1024
#define DETW_MAX_K 1024
#define DETW_MAX_A (1 << 20)
#define DETW_SCORE_THREADS 256

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
// MANY = true: the many-class form (a 16-lane group per candidate); everything that does not depend on C is shared.
// Dynamic LDS of the launch -- the arrays the kernel carves below, in its order: <= 162000 bytes at K = 1024
static size_t detw_matrix_lds_bytes(int Kp) {
  return (size_t)Kp * (8 + 16 + 4) + (256 + 16 + 256) * 4 + 16 * 8 + 4 * 4 + (size_t)Kp * (Kp / 64) * 8;
}

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

struct NmsArgs { int mode; float sigma; int agnostic; };

// Dynamic LDS of a scan select launch (detect_nms_select_kernel and detect_views_select_kernel carve the same arrays): eight [Kp]
// arrays, then histogram, wave totals, scalars, 4 group tables, argmax slots -- <= 67 KB at K = 1024
static size_t detn_scan_lds_bytes(int Kp) {
  return (size_t)Kp * (8 + 16 + 16 + 4 * 5) + 256 * 4 + 16 * 4 + 4 * 4 + 4 * 256 * 4 + 2 * 32 * 4;
}

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

// the LDS arrays of a scan select kernel, carved from the launch's dynamic LDS in the order detn_scan_lds_bytes counts them
#define DETN_SCAN_CARVE \
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[]; \
  const int K = a.K, Kp = (K + 63) & ~63;                     /* Kp <= 1024: one candidate slot per thread */ \
  unsigned long long* cand = (unsigned long long*)smem_raw;   /* [Kp] as detect_wide_select_kernel */ \
  f32x4* boxL = (f32x4*)(cand + Kp);                          /* [Kp] boxes in rank order */ \
  f32x4* boxP = boxL + Kp;                                    /* [Kp] boxes in (group, rank) order */ \
  int* clsL = (int*)(boxP + Kp);                              /* [Kp] classes in rank order */ \
  int* grpL = clsL + Kp;                                      /* [Kp] group of rank r, -1: none (no candidate, class outside 0 .. C-1) */ \
  float* curL = (float*)(grpL + Kp);                          /* [Kp] current scores in (group, rank) order */ \
  float* outS = curL + Kp;                                    /* [Kp] score at pick time */ \
  int* emitL = (int*)(outS + Kp);                             /* [Kp] pick order within the group, -1: not emitted */ \
  unsigned* hist = (unsigned*)(emitL + Kp);                   /* [256] */ \
  unsigned* wave_tot = hist + 256;                            /* [16] */ \
  unsigned* sv = wave_tot + 16;                               /* prefix, need, appended */ \
  int* gstart = (int*)(sv + 4);                               /* [256] first slot of a group */ \
  int* glen = gstart + 256;                                   /* [256] its candidates */ \
  unsigned* gcnt = (unsigned*)(glen + 256);                   /* [256] its emitted rows */ \
  unsigned* goff = gcnt + 256;                                /* [256] rows of the groups before it */ \
  float* slot_s = (float*)(goff + 256);                       /* [2][16] a wave's best current score ... */ \
  int* slot_p = (int*)(slot_s + 32);                          /* [2][16] ... and its slot */

template <bool MANY>
__global__ __launch_bounds__(DETW_THREADS) void detect_nms_select_kernel(DetArgs a, NmsArgs n) {
  DETN_SCAN_CARVE

#define DETW_PAD_ANY true
#include "detw_select_body.h"     // 1.-4. select, sweep, rank, decode: tid, lane, wave, b, A, C, ncand, ok, score, cls, idx, bx
#undef DETW_PAD_ANY
#define DETN_STORE(pos, sc) DETW_STORE_ROW(a, b, K, pos, cls, sc, idx, bx)
#include "detn_scan_body.h"     // 5.-7. (group, rank) order, the scan, the placement
#undef DETN_STORE
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
  DETN_SCAN_CARVE                                             // the layout of detect_nms_select_kernel

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

// ---- box voting: an emitted box becomes the score-weighted mean of its cluster (DESIGN.md section 3 "Box voting") ----------------------
// Gidaris & Komodakis 2015 / Detectron's bbox_vote, as a step between the scan and the store of the two scan select kernels.  The scan
// is untouched: the emitted set, its order, det_count / det_class / det_score / det_anchor are those of the launch without voting.
// For an emitted candidate i (rank order, c = class, s = ORIGINAL fp32 score, b = the box the scan took its IoUs on):
//   voters V_i = { r : c_r == c_i and (r == i or u(i, r) >= vote_iou) },  u = nms_decay's fp32 expression, a NaN u compares false;
//   (c_r == c_i with c_i in 0 .. C-1 makes r eligible -- grpL[r] >= 0 -- in either grouping, so grpL is not read; under nms_agnostic the
//   classes still vote apart);  W = sum (double)s_r,  X_k = sum (double)s_r * (double)b_r[k]  over V_i in ascending r, in float64;
//   voted coordinate = (float)(X_k / W).  Voters include suppressed, decayed and emitted candidates; weights are never the decayed scores.
// A row nobody agreed with (|V_i| = 1) keeps its box bit for bit: (s * b) / s is exact in fp64 and b is an fp32 value.
// All inputs are resident in LDS in rank order when the scan ends (boxL, clsL, the score bits in cand's upper half) and the scan wrote
// none of them: the thread of every emitted candidate walks the ranks 0 .. ncand-1 -- the threads of a wave read the same rank at the same
// time, LDS broadcasts -- and hands the voted box to the store the launch always did (DETW_STORE_ROW's x / sx + dx; the plain store of
// the pooled launch).  No new global traffic but the optional det_votes [B][K] (|V_i| per row), no new launch, the LDS of the scan kernels.
struct VoteArgs { float iou; int* votes; };

// the voted box of the emitted candidate of rank i (class cls, box bx) -> bx; returns |V_i|
__device__ __forceinline__ int detn_vote(const unsigned long long* cand, const f32x4* boxL, const int* clsL, int ncand, int i, int cls,
                                         float vote_iou, BoxF& bx) {
  const f32x4 pk = (f32x4){bx.x1, bx.y1, bx.x2, bx.y2};
  const float pa = (pk.z - pk.x) * (pk.w - pk.y);
  double W = 0.0, X0 = 0.0, X1 = 0.0, X2 = 0.0, X3 = 0.0;
  int nv = 0;
  // four ranks per trip: their IoUs are independent (the walk is bound by the latency of one LDS read and one division chain, not by
  // their number), the sums then take the voters in ascending rank.  The ranks ncand .. Kp-1 a last trip may touch exist in LDS with
  // class -1 (detw_select_body.h), so they never vote; Kp is a multiple of 64.
  for (int r0 = 0; r0 < ncand; r0 += 4) {
    f32x4 o[4];
    bool in[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = r0 + e;
      o[e] = boxL[r];
      const float oa = (o[e].z - o[e].x) * (o[e].w - o[e].y);
      const float iw = fmaxf(0.f, fminf(pk.z, o[e].z) - fmaxf(pk.x, o[e].x));
      const float ih = fmaxf(0.f, fminf(pk.w, o[e].w) - fmaxf(pk.y, o[e].y));
      const float inter = iw * ih;
      const float u = inter / ((pa + oa) - inter);
      in[e] = clsL[r] == cls && (r == i || u >= vote_iou);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (in[e]) {
        const double s = (double)__uint_as_float((unsigned)(cand[r0 + e] >> 32));
        W += s;
        X0 += s * (double)o[e].x; X1 += s * (double)o[e].y; X2 += s * (double)o[e].z; X3 += s * (double)o[e].w;
        ++nv;
      }
    }
  }
  bx.x1 = (float)(X0 / W); bx.y1 = (float)(X1 / W); bx.x2 = (float)(X2 / W); bx.y2 = (float)(X3 / W);   // (W >= s_i > score_thresh >= 0)
  return nv;
}

// detect_nms_select_kernel with the voting step
template <bool MANY>
__global__ __launch_bounds__(DETW_THREADS) void detect_vote_select_kernel(DetArgs a, NmsArgs n, VoteArgs vt) {
  DETN_SCAN_CARVE
#define DETW_PAD_ANY true
#include "detw_select_body.h"
#undef DETW_PAD_ANY
#define DETN_STORE(pos, sc) DETW_STORE_ROW(a, b, K, pos, cls, sc, idx, bx)
#define DETN_VOTE vt
#include "detn_scan_body.h"
#undef DETN_VOTE
#undef DETN_STORE
}

// detect_views_select_kernel with the voting step: the vote runs on the image-coordinate boxes, across the views
template <bool MANY>
__global__ __launch_bounds__(DETW_THREADS) void detect_views_vote_select_kernel(DetArgs a, NmsArgs n, ViewArgs vw, VoteArgs vt) {
  DETN_SCAN_CARVE
#define DETW_PAD_ANY false
#define DETW_VIEWS vw.V
#define DETW_VIEW_XF vw.xf
#include "detw_select_body.h"
#undef DETW_VIEW_XF
#undef DETW_VIEWS
#undef DETW_PAD_ANY
#define DETN_STORE(pos, sc) DETV_STORE_ROW(a, b, K, pos, cls, sc, idx, bx)
#define DETN_VOTE vt
#include "detn_scan_body.h"
#undef DETN_VOTE
#undef DETN_STORE
}

// ---- host side ----
// int32 words of the wide workspace: B x ceil4(A) keys.  -1: (B, A, K) is outside what the wide path takes.
extern "C" int sqd_detect_wide_workspace_words(int B, int A, int keep_top_k) {
  if (B < 1 || A < 1 || A > DETW_MAX_A || keep_top_k < 1 || keep_top_k > DETW_MAX_K) return -1;
  const long long words = (long long)B * ((A + 3) & ~3);
  return words > 0x7fffffffll ? -1 : (int)words;
}

// the scoring launch of the head form on `rows` key rows (B, or B * V with views): B x slabs <= 2^23 + B workgroups
static void launch_wide_score(DetArgs a, bool many, int rows, hipStream_t stream) {
  const int A4 = (a.A + 3) & ~3;
  a.B = rows;
  if (many) {
    const int slabs = (A4 + MC_THREADS - 1) / MC_THREADS;
#define CALL(R) hipLaunchKernelGGL(detect_many_score_kernel<R>, dim3((unsigned)((long long)rows * slabs)), dim3(MC_THREADS), 0, stream, a)
    MC_DISPATCH(a.C, CALL);
#undef CALL
  } else {
    const int slabs = (A4 + DETW_SCORE_THREADS - 1) / DETW_SCORE_THREADS;
    hipLaunchKernelGGL(detect_wide_score_kernel, dim3((unsigned)((long long)rows * slabs)), dim3(DETW_SCORE_THREADS), 0, stream, a);
  }
}

// Every wide launch: (bit matrix | scan rule `n`) x (few | many classes) x (views | not) x (box voting `vt` | not; with a rule only).
// a.B images of vw.V views each; `many` is the head form and sets the class limit (16 or 256).  Refuses in this order, launching
// nothing: a size below 1, then (with a rule) an unknown mode, a bad sigma, a negative score_thresh or a vote_iou outside (0, 1]:
// status 1; past a limit: 2; a short or misaligned workspace, then keys_ready without a <= 16-class pred: 1.
static int launch_wide(DetArgs a, int ws_words, bool many, const NmsArgs* n, ViewArgs vw, const VoteArgs* vt, hipStream_t stream) {
  SQD_CHECK_ARG(a.B > 0 && vw.V >= 1 && a.A > 0 && a.C >= 1 && a.K >= 1);
  if (n) {
    SQD_CHECK_ARG(n->mode == NMS_HARD || n->mode == NMS_LINEAR || n->mode == NMS_GAUSSIAN);
    SQD_CHECK_ARG(n->mode != NMS_GAUSSIAN || (isfinite(n->sigma) && n->sigma > 0.f));
    SQD_CHECK_ARG(a.score_thresh >= 0.f);                     // (the keys: see ops._check_score_thresh; the scan's -1 marks rely on it too)
  }
  SQD_CHECK_ARG(!vt || (n && vt->iou > 0.f && vt->iou <= 1.f));   // (a NaN compares false)
  if (a.K > DETW_MAX_K || a.A > DETW_MAX_A || a.C > (many ? SQD_MANY_MAX_CLASSES : SQD_MAX_CLASSES)) return SQD_ERR_UNSUPPORTED;
  if ((long long)vw.V * ((a.A + 3) & ~3) > DETW_MAX_A || (long long)a.B * vw.V > 0x7fffffffll) return SQD_ERR_UNSUPPORTED;
  const int rows = a.B * vw.V;
  const int words = sqd_detect_wide_workspace_words(rows, a.A, a.K);
  if (words < 0) return SQD_ERR_UNSUPPORTED;                  // (rows x ceil4(A) past 2^31 - 1 words)
  SQD_CHECK_ARG(a.keys && ws_words >= words && det_aligned16(a.keys));
  SQD_CHECK_ARG(!a.keys_ready || (a.pred && !many));          // ConvDet's epilogue writes the <= 16-class keys of a pred
  // the select kernel of the form; the dynamic-LDS cap is raised once per device and instantiation
  static const void* const kernels[5][2] = {
      {(const void*)detect_wide_select_kernel<false>, (const void*)detect_wide_select_kernel<true>},
      {(const void*)detect_nms_select_kernel<false>, (const void*)detect_nms_select_kernel<true>},
      {(const void*)detect_views_select_kernel<false>, (const void*)detect_views_select_kernel<true>},
      {(const void*)detect_vote_select_kernel<false>, (const void*)detect_vote_select_kernel<true>},
      {(const void*)detect_views_vote_select_kernel<false>, (const void*)detect_views_vote_select_kernel<true>}};
  static SqdDevOnce once[5][2];
  const int form = !n ? 0 : (!vw.xf ? 1 : 2) + (vt ? 2 : 0), Kp = (a.K + 63) & ~63;
  const size_t lds = n ? detn_scan_lds_bytes(Kp) : detw_matrix_lds_bytes(Kp);
  if (lds > 48 * 1024 && sqd_max_lds_once(once[form][many], kernels[form][many], n ? 96 * 1024 : 160 * 1024) != SQD_OK) return SQD_ERR_LAUNCH;
  if (!a.keys_ready) launch_wide_score(a, many, rows, stream);
  void* args[4];                                              // DetArgs, then what the form has: NmsArgs, ViewArgs, VoteArgs
  int na = 0;
  args[na++] = &a;
  if (n) args[na++] = (void*)n;
  if (n && vw.xf) args[na++] = &vw;
  if (vt) args[na++] = (void*)vt;
  (void)hipLaunchKernel(kernels[form][many], dim3((unsigned)a.B), dim3(DETW_THREADS), args, lds, stream);
  return sqd_launch_status();
}

static const ViewArgs NO_VIEWS = {nullptr, 1};

// sqd_detect_shift_fwd for any 1 <= keep_top_k <= 1024 and 1 <= A <= 2^20: same outputs bit for bit where both run.  keys_ws: a
// 16-byte aligned workspace of ws_words >= sqd_detect_wide_workspace_words(B, A, keep_top_k) uint32, any contents; nothing in it
// carries over from launch to launch.  Status 2 for keep_top_k, A or num_classes past the limits, 1 for anything malformed
// (a null pointer, keep_top_k < 1, a short or misaligned workspace); nothing is launched then.
extern "C" int sqd_detect_wide_fwd(const float* pred, const float* anchors, const float* scales, const float* shifts, unsigned* keys_ws,
                                   int* det_count, long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                   int num_classes, int input_h, int input_w, int keep_top_k, float nms_thresh, float score_thresh,
                                   int ws_words, void* stream) {
  const DetArgs a = det_args_pred(pred, anchors, scales, shifts, keys_ws, det_count, det_class, det_score, det_box, det_anchor, B, A,
                                  num_classes, input_h, input_w, keep_top_k, nms_thresh, score_thresh);
  SQD_CHECK_ARG(det_ptrs_ok(a) && keys_ws && det_aligned16(pred));
  return launch_wide(a, ws_words, false, nullptr, NO_VIEWS, nullptr, (hipStream_t)stream);
}

// sqd_filter_fwd for the same ranges (dense class_ids int64 [B][A], scores [B][A], boxes [B][A][4])
extern "C" int sqd_filter_wide_fwd(const long long* class_ids, const float* scores, const float* boxes, unsigned* keys_ws, int* det_count,
                                   long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                   int num_classes, int keep_top_k, float nms_thresh, float score_thresh, int ws_words, void* stream) {
  const DetArgs a = det_args_dense(class_ids, scores, boxes, keys_ws, det_count, det_class, det_score, det_box, det_anchor, B, A,
                                   num_classes, keep_top_k, nms_thresh, score_thresh);
  SQD_CHECK_ARG(det_ptrs_ok(a) && keys_ws);
  return launch_wide(a, ws_words, false, nullptr, NO_VIEWS, nullptr, (hipStream_t)stream);
}

// sqd_detect_wide_fwd for 1 <= num_classes <= 256 (the many-class head form at every class count; pred needs no alignment): same
// arguments, same workspace.  Status 2 for num_classes > 256, keep_top_k > 1024 or A > 2^20; 1 for anything malformed.
extern "C" int sqd_detect_many_fwd(const float* pred, const float* anchors, const float* scales, const float* shifts, unsigned* keys_ws,
                                   int* det_count, long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                   int num_classes, int input_h, int input_w, int keep_top_k, float nms_thresh, float score_thresh,
                                   int ws_words, void* stream) {
  const DetArgs a = det_args_pred(pred, anchors, scales, shifts, keys_ws, det_count, det_class, det_score, det_box, det_anchor, B, A,
                                  num_classes, input_h, input_w, keep_top_k, nms_thresh, score_thresh);
  SQD_CHECK_ARG(det_ptrs_ok(a) && keys_ws);
  return launch_wide(a, ws_words, true, nullptr, NO_VIEWS, nullptr, (hipStream_t)stream);
}

// sqd_filter_wide_fwd for class ids up to 255
extern "C" int sqd_filter_many_fwd(const long long* class_ids, const float* scores, const float* boxes, unsigned* keys_ws, int* det_count,
                                   long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                   int num_classes, int keep_top_k, float nms_thresh, float score_thresh, int ws_words, void* stream) {
  const DetArgs a = det_args_dense(class_ids, scores, boxes, keys_ws, det_count, det_class, det_score, det_box, det_anchor, B, A,
                                   num_classes, keep_top_k, nms_thresh, score_thresh);
  SQD_CHECK_ARG(det_ptrs_ok(a) && keys_ws);
  return launch_wide(a, ws_words, true, nullptr, NO_VIEWS, nullptr, (hipStream_t)stream);
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
  DetArgs a = det_args_pred(pred, anchors, scales, shifts, keys_ws, det_count, det_class, det_score, det_box, det_anchor, B, A,
                            num_classes, input_h, input_w, keep_top_k, nms_thresh, score_thresh);
  a.keys_ready = keys_ready ? 1 : 0;
  const bool many = num_classes > SQD_MAX_CLASSES;
  SQD_CHECK_ARG(det_ptrs_ok(a) && keys_ws && (many || det_aligned16(pred)));
  const NmsArgs n = {nms_mode, nms_sigma, nms_agnostic ? 1 : 0};
  return launch_wide(a, ws_words, many, &n, NO_VIEWS, nullptr, (hipStream_t)stream);
}

// sqd_filter_wide_fwd / sqd_filter_many_fwd with the same four arguments (keys_ready must be 0: dense scores have no ConvDet keys)
extern "C" int sqd_filter_nms_fwd(const long long* class_ids, const float* scores, const float* boxes, unsigned* keys_ws, int* det_count,
                                  long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                  int num_classes, int keep_top_k, float nms_thresh, float score_thresh, int ws_words,
                                  int nms_mode, float nms_sigma, int nms_agnostic, int keys_ready, void* stream) {
  const DetArgs a = det_args_dense(class_ids, scores, boxes, keys_ws, det_count, det_class, det_score, det_box, det_anchor, B, A,
                                   num_classes, keep_top_k, nms_thresh, score_thresh);
  SQD_CHECK_ARG(det_ptrs_ok(a) && keys_ws && !keys_ready);
  const NmsArgs n = {nms_mode, nms_sigma, nms_agnostic ? 1 : 0};
  return launch_wide(a, ws_words, num_classes > SQD_MAX_CLASSES, &n, NO_VIEWS, nullptr, (hipStream_t)stream);
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
  const DetArgs a = det_args_pred(pred, anchors, nullptr, nullptr, keys_ws, det_count, det_class, det_score, det_box, det_anchor, B, A,
                                  num_classes, input_h, input_w, keep_top_k, nms_thresh, score_thresh);
  const bool many = num_classes > SQD_MAX_CLASSES;
  SQD_CHECK_ARG(det_ptrs_ok(a) && view_xf && keys_ws && (many || det_aligned16(pred)));
  const NmsArgs n = {nms_mode, nms_sigma, nms_agnostic ? 1 : 0};
  return launch_wide(a, ws_words, many, &n, ViewArgs{view_xf, V}, nullptr, (hipStream_t)stream);
}

// Box voting (DESIGN.md section 3 "Box voting"): sqd_detect_nms_fwd / sqd_filter_nms_fwd / sqd_detect_views_fwd with `float vote_iou,
// int* det_votes` before the stream.  The scan, det_count, det_class, det_score and det_anchor are those of the sibling; det_box of every
// row is the score-weighted mean (float64 sums in rank order, original scores) of the same-class candidates that overlap the row's own
// box by u >= vote_iou, the row's candidate included -- the canvas box in the first two (then the sibling's store: x / sx + dx), the
// image box in the pooled form.  det_votes: int32 [B][keep_top_k], the number of voters per row, or null: not written.  vote_iou: in
// (0, 1]; NaN, <= 0 or > 1 is status 1, checked with the rule (before the limits); everything else as the sibling.
extern "C" int sqd_detect_vote_fwd(const float* pred, const float* anchors, const float* scales, const float* shifts, unsigned* keys_ws,
                                   int* det_count, long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                   int num_classes, int input_h, int input_w, int keep_top_k, float nms_thresh, float score_thresh,
                                   int ws_words, int nms_mode, float nms_sigma, int nms_agnostic, int keys_ready, float vote_iou,
                                   int* det_votes, void* stream) {
  DetArgs a = det_args_pred(pred, anchors, scales, shifts, keys_ws, det_count, det_class, det_score, det_box, det_anchor, B, A,
                            num_classes, input_h, input_w, keep_top_k, nms_thresh, score_thresh);
  a.keys_ready = keys_ready ? 1 : 0;
  const bool many = num_classes > SQD_MAX_CLASSES;
  SQD_CHECK_ARG(det_ptrs_ok(a) && keys_ws && (many || det_aligned16(pred)));
  const NmsArgs n = {nms_mode, nms_sigma, nms_agnostic ? 1 : 0};
  const VoteArgs vt = {vote_iou, det_votes};
  return launch_wide(a, ws_words, many, &n, NO_VIEWS, &vt, (hipStream_t)stream);
}

extern "C" int sqd_filter_vote_fwd(const long long* class_ids, const float* scores, const float* boxes, unsigned* keys_ws, int* det_count,
                                   long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int A,
                                   int num_classes, int keep_top_k, float nms_thresh, float score_thresh, int ws_words,
                                   int nms_mode, float nms_sigma, int nms_agnostic, int keys_ready, float vote_iou, int* det_votes,
                                   void* stream) {
  const DetArgs a = det_args_dense(class_ids, scores, boxes, keys_ws, det_count, det_class, det_score, det_box, det_anchor, B, A,
                                   num_classes, keep_top_k, nms_thresh, score_thresh);
  SQD_CHECK_ARG(det_ptrs_ok(a) && keys_ws && !keys_ready);
  const NmsArgs n = {nms_mode, nms_sigma, nms_agnostic ? 1 : 0};
  const VoteArgs vt = {vote_iou, det_votes};
  return launch_wide(a, ws_words, num_classes > SQD_MAX_CLASSES, &n, NO_VIEWS, &vt, (hipStream_t)stream);
}

extern "C" int sqd_detect_views_vote_fwd(const float* pred, const float* anchors, const float* view_xf, unsigned* keys_ws, int* det_count,
                                         long long* det_class, float* det_score, float* det_box, int* det_anchor, int B, int V, int A,
                                         int num_classes, int input_h, int input_w, int keep_top_k, float nms_thresh, float score_thresh,
                                         int ws_words, int nms_mode, float nms_sigma, int nms_agnostic, float vote_iou, int* det_votes,
                                         void* stream) {
  const DetArgs a = det_args_pred(pred, anchors, nullptr, nullptr, keys_ws, det_count, det_class, det_score, det_box, det_anchor, B, A,
                                  num_classes, input_h, input_w, keep_top_k, nms_thresh, score_thresh);
  const bool many = num_classes > SQD_MAX_CLASSES;
  SQD_CHECK_ARG(det_ptrs_ok(a) && view_xf && keys_ws && (many || det_aligned16(pred)));
  const NmsArgs n = {nms_mode, nms_sigma, nms_agnostic ? 1 : 0};
  const VoteArgs vt = {vote_iou, det_votes};
  return launch_wide(a, ws_words, many, &n, ViewArgs{view_xf, V}, &vt, (hipStream_t)stream);
}
