// Stem weight gradient, dense forms, and the C entries of all three forms (the gather form is stem_wgrad_gather.hip: its own
// translation unit for its compiler flags).  Reference: the backward of src/model/squeezedet.py:34-36 / :52-54 as autograd derives it.
//
//   dW0[n][ci][ky][kx] = sum_p dY[p][n] * img[ci][2*py+ky-pad][2*px+kx-pad],   db[n] = sum_p dY[p][n]
//
// (no data gradient: the image needs none).  The split-K slab scheme of wgrad.hip: a workgroup walks conv tiles of 8 x 16 pixels,
// accumulates in MFMA registers and writes ONE slab [n][K] + [N]; sqd_wgrad_reduce_launch sums the slabs in a fixed order.
#include "stem.h"

extern "C" int sqd_wgrad_reduce_launch(const float* slab, float* dw, float* db, int S, long long slab_stride, int N, int C, int taps,
                                       void* stream);      // wgrad.hip

// The constants the two dense kernels and their launchers share.
template <int KS, int TN> struct StemWgradDense {
  static constexpr int TH = 8;                                          // conv tile: TH x 16 pixels
  static constexpr int K = 3 * KS * KS, KT = (K + 15) / 16;             // k-tiles of 16 im2col columns
  static constexpr int PN = TN * 16 + ((TN & 1) ? 0 : 16);              // pitch of the conv-gradient tile dyT [128][PN]
  static constexpr int IH = 2 * (TH - 1) + KS, IW = 2 * 15 + KS;        // image patch of a tile
  static constexpr int TILES = TN * KT, NACC = (TILES + 3) / 4, BACC = (TN + 3) / 4;
  // stem_wgrad_kernel: planar patch [3][IH][IWP], odd pitch, then one zero slot
  static constexpr int IWP = IW | 1;
  static constexpr size_t lds_plain = (size_t)(128 * PN + 3 * IH * IWP + 1) * sizeof(float);
  // stem_wgrad_pooled_kernel: two flat DMA patches [ci][r][c] of INSLOTS floats, then the two 9 x 9 tables
  static constexpr int NIN = 3 * IH * IW, IN_IT = (NIN + 255) / 256, INSLOTS = IN_IT * 256;
  static constexpr size_t lds_pooled = (size_t)(128 * PN + 2 * INSLOTS + 81 + 81) * sizeof(float);
  static_assert(lds_pooled <= 160 * 1024, "stem wgrad LDS budget");
};

// The MFMA side of both dense kernels: D[n][k] += dyT^T x im2col(patch) over one tile, wave w owning output tiles w, w + 4, ..
// of the TN x KT grid (plus bias tiles with B = 1).  PITCH = row pitch of the image patch in LDS.
// (wave, lr, kq and the kernel's arguments come by reference and are read where they are used: by value the register allocator
// gives the 7x7 kernels four registers more than they had as two separate kernels; this way it gives them 12 fewer.)
template <int KS, int TN, int PITCH>
struct StemWgradMma {
  using D = StemWgradDense<KS, TN>;
  f32x4 acc[D::NACC], bacc[D::BACC];
  // per-lane LDS offsets computed once; the unrolled k-loop adds compile-time immediates only.  Padded im2col
  // columns (k >= K) read a valid address (offset 0 of the patch); their products land in columns of D that are
  // never stored, so no zero slot is needed on this side.
  int al[D::NACC], bl[D::NACC], abias[D::BACC];

  __device__ __forceinline__ StemWgradMma(const int& wave, const int& lr, const int& kq) {
#pragma unroll
    for (int i = 0; i < D::NACC; ++i) {
      acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      int t = wave + 4 * i;
      if (t >= D::TILES) t = D::TILES - 1;
      const int kt = t % D::KT, nt = t / D::KT;
      const int k = kt * 16 + lr;                                 // this lane's im2col column
      const int ci = k / (KS * KS), rem = k - ci * (KS * KS), ky = rem / KS, kx = rem - ky * KS;
      al[i] = kq * D::PN + nt * 16 + lr;
      bl[i] = 2 * kq + ((k < D::K) ? (ci * D::IH + ky) * PITCH + kx : 0);
    }
#pragma unroll
    for (int i = 0; i < D::BACC; ++i) {
      bacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const int bt = (wave + 4 * i < TN) ? wave + 4 * i : 0;
      abias[i] = kq * D::PN + bt * 16 + lr;
    }
  }
  // one tile: TH * 4 k-steps of 4 pixels
  __device__ __forceinline__ void walk(const float* dyT, const float* inT) {
#pragma unroll
    for (int s = 0; s < D::TH * 4; ++s) {
      const int r = s >> 2, cq = s & 3;
      const int immA = (r * 16 + cq * 4) * D::PN;                 // compile-time after unrolling
      const int immB = (2 * r) * PITCH + 8 * cq;
#pragma unroll
      for (int i = 0; i < D::NACC; ++i) acc[i] = mfma16(dyT[al[i] + immA], inT[bl[i] + immB], acc[i]);
#pragma unroll
      for (int i = 0; i < D::BACC; ++i) bacc[i] = mfma16(dyT[abias[i] + immA], 1.0f, bacc[i]);
    }
  }
  // the workgroup's slab: [n][K] (already OIHW-flat) + [N]
  __device__ __forceinline__ void store(const StemWgradArgs& a, const int& wave, const int& lr, const int& kq) const {
    float* slab = a.slab + (long long)blockIdx.x * a.slab_stride;
#pragma unroll
    for (int i = 0; i < D::NACC; ++i) {
      const int t = wave + 4 * i;
      if (t >= D::TILES) continue;
      const int kt = t % D::KT, nt = t / D::KT;
      const int k = kt * 16 + lr;
      if (k >= D::K) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = nt * 16 + 4 * kq + r;
        if (n < a.N) slab[(long long)n * D::K + k] = acc[i][r];
      }
    }
    if (lr == 0) {
#pragma unroll
      for (int i = 0; i < D::BACC; ++i) {
        const int bt = wave + 4 * i;
        if (bt >= TN) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = bt * 16 + 4 * kq + r;
          if (n < a.N) slab[(long long)a.N * D::K + n] = bacc[i][r];
        }
      }
    }
  }
};

// ---------------------------------------------------------------------------------------------
// Behind the unfused forward: dy is the (ReLU-masked) gradient of the conv output, NHWC [B][Ho][Wo][N].
// ---------------------------------------------------------------------------------------------
template <int KS, int PAD, int TN>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(StemWgradArgs a) {
  using D = StemWgradDense<KS, TN>;
  constexpr int TH = D::TH, PN = D::PN, IH = D::IH, IW = D::IW, IWP = D::IWP;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* dyT = smem;                   // [128][PN]
  float* inT = smem + 128 * PN;        // [3][IH][IWP] + zero slot

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, kq = lane >> 4;
  StemWgradMma<KS, TN, IWP> mma(wave, lr, kq);

  bool first = true;
  for (int pb = blockIdx.x; pb < a.nblocks; pb += gridDim.x) {
    int t = pb;
    const int tx = t % a.tiles_x; t /= a.tiles_x;
    const int ty = t % a.tiles_y; const int b = t / a.tiles_y;
    const int y0 = ty * TH, x0 = tx * 16;
    if (!first) __syncthreads();
    first = false;
    for (int idx = tid; idx < 128 * TN * 4; idx += 256) {
      const int pix = idx / (TN * 4), v = idx - pix * (TN * 4);
      const int oy = y0 + (pix >> 4), ox = x0 + (pix & 15), n = 4 * v;
      f32x4 val = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (oy < a.Ho && ox < a.Wo && n < a.N) val = *(const f32x4*)(a.dy + (((long long)b * a.Ho + oy) * a.Wo + ox) * a.N + n);
      *(f32x4*)(dyT + pix * PN + 4 * v) = val;
    }
    stem_stage_planar<PAD, IH, IW, IWP>(inT, a.img, b, y0, x0, a.Hin, a.Win, tid);
    __syncthreads();
    mma.walk(dyT, inT);
  }
  mma.store(a, wave, lr, kq);
}

// ---------------------------------------------------------------------------------------------
// Behind the FUSED forward (conv + ReLU + MaxPool(3,2,ceil)): dy is dPool [B][Hp][Wp][N].  The gradient of a conv output is the sum of
// dPool over the (at most 4) windows whose argmax it is, masked by pooled > 0 (the pooled value IS the conv output at the argmax,
// so this is the ReLU mask); the kernel rebuilds that tensor tile by tile in LDS and multiplies it like the kernel above.
// On gfx950 every VALU instruction delays the fp32 MFMA stream (DESIGN.md cost model), so:
//  * the routing is a scatter by pooled item with everything tile-invariant precomputed once per thread: for each
//    of the four (row parity, column parity) phases a thread owns at most SL (window, channel quad) items whose global
//    offset, LDS base and border class are fixed; same-parity windows never overlap, so the read-modify-write of the
//    conv-gradient tile needs no atomics and its summation order is fixed (bitwise reproducible);
//  * argmax code -> (LDS offset, 0/1 weight) comes from two 9x9 LDS tables indexed by (border class, code): windows
//    hanging over the tile edge have their outside taps clamped to an inside address with weight 0, so there are no
//    per-element bounds checks;
//  * the NCHW image patch goes global -> LDS by 4-byte LDS-DMA into a double buffer (next tile under this tile's
//    MFMAs), and the dPool / pooled / argmax words of the next tile are prefetched into registers;
//  * MFMA operand addresses are per-lane bases + compile-time immediates.
// This is the kernel of the 7x7 stem, of 3x3 images the gather kernel refuses, and that kernel's parity partner
// (SQD_STEM_WGRAD_GATHER=0, stem.h).
// ---------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* wg_lds_ptr_t;
__device__ __attribute__((aligned(16))) float sqd_wgrad_zero[4] = {0.f, 0.f, 0.f, 0.f};

template <int KS, int PAD, int TN>
__global__ __launch_bounds__(256) void stem_wgrad_pooled_kernel(StemWgradArgs a) {
  using D = StemWgradDense<KS, TN>;
  constexpr int TH = D::TH, PN = D::PN, IH = D::IH, IW = D::IW;
  constexpr int NIN = D::NIN, IN_IT = D::IN_IT, INSLOTS = D::INSLOTS;
  constexpr int SL = (15 * TN * 4 + 255) / 256;             // item slots per thread and phase
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* const dyT = smem;                                  // [128][PN]   conv-output gradient of the tile
  float* const inB = dyT + 128 * PN;                        // [2][INSLOTS] image patches, flat [ci][r][c]
  int* const relT = (int*)(inB + 2 * INSLOTS);              // [9 classes][9 codes] byte offset of the (clamped) tap
  float* const mskT = (float*)(relT + 81);                  // [9][9] 1 = tap inside the tile, 0 = outside

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, kq = lane >> 4;
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  const int NQ = a.N >> 2;

  if (tid < 81) {
    const int cls = tid / 9, t = tid - cls * 9, rc = cls / 3, cc = cls - rc * 3;
    const int dy = t / 3, dx = t - dy * 3;
    // row class 0: window row -1 (only dy = 2 is inside), 1: interior, 2: window row 3 (dy = 0, 1 inside); columns alike
    const bool oky = rc == 0 ? dy == 2 : (rc == 2 ? dy < 2 : true);
    const bool okx = cc == 0 ? dx == 2 : (cc == 2 ? dx < 2 : true);
    const int dyc = rc == 0 ? 2 : (rc == 2 ? (dy < 2 ? dy : 1) : dy);
    const int dxc = cc == 0 ? 2 : (cc == 2 ? (dx < 2 ? dx : 1) : dx);
    relT[tid] = (dyc * 16 + dxc) * PN * 4;
    mskT[tid] = (oky && okx) ? 1.f : 0.f;
  }

  StemWgradMma<KS, TN, IW> mma(wave, lr, kq);

  // tile-invariant item lists: phase ph = 2 * (window-row parity) + (window-column parity); tile origins are multiples of
  // (4, 8) in window units, so parity of the absolute window index = parity of the tile-relative one
  int it_goff[4][SL], it_lds[4][SL], it_key[4][SL];       // key = class * 36 | (wrow + 1) << 16 | (wcol + 1) << 24, -1 = no item
#pragma unroll
  for (int ph = 0; ph < 4; ++ph) {
    const int odd_r = ph >> 1, odd_c = ph & 1;
    const int ncols = odd_c ? 5 : 4, nrows = odd_r ? 3 : 2;
#pragma unroll
    for (int sl = 0; sl < SL; ++sl) {
      const int idx = tid + 256 * sl;
      const int q = idx % NQ, w = idx / NQ;
      const int wr = w / ncols, wc = w - wr * ncols;
      const bool real = w < nrows * ncols;
      const int pr = odd_r ? 2 * wr - 1 : 2 * wr, pc = odd_c ? 2 * wc - 1 : 2 * wc;      // window index relative to the tile
      const int rcls = pr < 0 ? 0 : (pr >= 3 ? 2 : 1), ccls = pc < 0 ? 0 : (pc >= 7 ? 2 : 1);
      it_goff[ph][sl] = real ? (pr * a.Wp + pc) * a.N + 4 * q : 0;
      it_lds[ph][sl] = real ? ((2 * pr) * 16 + 2 * pc) * PN * 4 + 16 * q : 0;
      it_key[ph][sl] = real ? ((rcls * 3 + ccls) * 36 | (pr + 1) << 16 | (pc + 1) << 24) : -1;
    }
  }
  // image-patch DMA slots
  int in_off[IN_IT], in_key[IN_IT];
#pragma unroll
  for (int it = 0; it < IN_IT; ++it) {
    const int idx = tid + it * 256;
    const int c = idx % IW; int r = idx / IW; const int ci = r / IH; r -= ci * IH;
    const bool real = idx < NIN;
    in_off[it] = real ? (ci * a.Hin + r) * a.Win + c : 0;
    in_key[it] = real ? (r << 8 | c) : -1;
  }

  struct Tile { int wy0, wx0, iy0, ix0, img_inner, win_inner; long long wbase; const float* xorg; };
  auto tile_at = [&](int t) {
    Tile q;
    const int tx = t % a.tiles_x; t /= a.tiles_x;
    const int ty = t % a.tiles_y; const int b = t / a.tiles_y;
    q.wy0 = ty * (TH / 2); q.wx0 = tx * 8;                                   // first window (row, col) owned by the tile
    q.iy0 = 2 * ty * TH - PAD; q.ix0 = 2 * tx * 16 - PAD;
    q.xorg = a.img + ((long long)b * 3 * a.Hin + q.iy0) * a.Win + q.ix0;
    q.img_inner = (int)(((unsigned)(-q.iy0 - 1) & (unsigned)(q.iy0 + IH - a.Hin - 1) & (unsigned)(-q.ix0 - 1) & (unsigned)(q.ix0 + IW - a.Win - 1)) >> 31);
    // all windows (rows wy0-1 .. wy0+3, cols wx0-1 .. wx0+7) exist
    q.win_inner = (int)(((unsigned)(-q.wy0) & (unsigned)(q.wy0 + 3 - a.Hp) & (unsigned)(-q.wx0) & (unsigned)(q.wx0 + 7 - a.Wp)) >> 31);
    q.wbase = (((long long)b * a.Hp + q.wy0) * a.Wp + q.wx0) * a.N;
    return q;
  };
  auto dma_in = [&](const Tile q, int buf) {
#pragma unroll
    for (int it = 0; it < IN_IT; ++it) {
      const float* src = q.xorg + in_off[it];
      if (!q.img_inner) {
        asm volatile("" ::: "memory");
        const int key = in_key[it];
        const bool ok = key >= 0 && (unsigned)(q.iy0 + (key >> 8)) < (unsigned)a.Hin && (unsigned)(q.ix0 + (key & 255)) < (unsigned)a.Win;
        src = ok ? src : sqd_wgrad_zero;
      }
      __builtin_amdgcn_global_load_lds(src, (wg_lds_ptr_t)(inB + buf * INSLOTS + it * 256 + wave_s * 64), 4, 0, 0);
    }
  };
  // dPool / pooled / argmax words of a tile's items -> registers
  unsigned r_am[4][SL]; f32x4 r_dp[4][SL], r_pl[4][SL];
  const bool has_pl = a.pooled != nullptr;
  auto fetch_items = [&](const Tile q) {
#pragma unroll
    for (int ph = 0; ph < 4; ++ph)
#pragma unroll
      for (int sl = 0; sl < SL; ++sl) {
        const int key = it_key[ph][sl];
        bool ok = key >= 0;
        if (!q.win_inner) {
          asm volatile("" ::: "memory");
          const int wy = q.wy0 + ((key >> 16) & 255) - 1, wx = q.wx0 + ((key >> 24) & 255) - 1;
          ok = ok && (unsigned)wy < (unsigned)a.Hp && (unsigned)wx < (unsigned)a.Wp;
        }
        r_am[ph][sl] = 0x09090909u;                                           // code 9 never matches a tap: weight 0 below
        r_dp[ph][sl] = (f32x4){0.f, 0.f, 0.f, 0.f}; r_pl[ph][sl] = (f32x4){1.f, 1.f, 1.f, 1.f};
        if (ok) {
          const long long o = q.wbase + it_goff[ph][sl];
          r_am[ph][sl] = *(const unsigned*)(a.amax + o);
          r_dp[ph][sl] = *(const f32x4*)(a.dy + o);
          // the fused forward's codes already carry the ReLU mask (15 = pooled value not > 0): `pooled` is optional and only
          // read when given (uniform branch)
          if (has_pl) r_pl[ph][sl] = *(const f32x4*)(a.pooled + o);
        }
      }
  };

  int tile = sqd_xcd_contiguous((int)blockIdx.x, (int)gridDim.x);     // neighbouring tiles (shared halo lines) through one XCD's L2
  if (tile < a.nblocks) {
    Tile cur = tile_at(tile);
    dma_in(cur, 0);
    fetch_items(cur);
    int buf = 0;
    for (;;) {
      const int ntile = tile + (int)gridDim.x;
      const bool has_next = ntile < a.nblocks;
      const Tile nxt = tile_at(has_next ? ntile : tile);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of the patch DMA has landed (explicit, see conv_igemm.hip)
      __syncthreads();                       // previous tile's MFMAs left dyT / inB; the patch is published
      for (int idx = tid; idx < 128 * PN / 4; idx += 256) ((f32x4*)dyT)[idx] = (f32x4){0.f, 0.f, 0.f, 0.f};
      __syncthreads();
#pragma unroll
      for (int ph = 0; ph < 4; ++ph) {
#pragma unroll
        for (int sl = 0; sl < SL; ++sl) {
          const int key = it_key[ph][sl];
          if (key < 0) continue;
          const unsigned am = r_am[ph][sl];
          const f32x4 dp = r_dp[ph][sl], pl = r_pl[ph][sl];
          const int cls_off = key & 0xffff;
          char* const base = (char*)dyT + it_lds[ph][sl];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const unsigned code = (am >> (8 * e)) & 255u;
            const unsigned tix = code < 9u ? code : 0u;                        // out-of-image item: any valid table slot ...
            const int rel = relT[cls_off / 4 + tix];
            float w = mskT[cls_off / 4 + tix];
            float v = (pl[e] > 0.f && code < 9u) ? dp[e] : 0.f;                // ... its dp is 0; code 15 = ReLU mask 0
            float* dst = (float*)(base + rel) + e;
            *dst += v * w;
          }
        }
        __syncthreads();
      }
      if (has_next) { dma_in(nxt, buf ^ 1); fetch_items(nxt); }
      mma.walk(dyT, inB + buf * INSLOTS);
      if (!has_next) break;
      tile = ntile; cur = nxt; buf ^= 1;
    }
  }
  mma.store(a, wave, lr, kq);
}

template <int KS, int PAD, int TN>
static int launch_stem_wgrad_dense(StemWgradArgs a, int S, bool pooled, hipStream_t s) {
  using D = StemWgradDense<KS, TN>;
  a.tiles_x = sqd_cdiv(a.Wo, 16); a.tiles_y = sqd_cdiv(a.Ho, D::TH);
  a.nblocks = a.B * a.tiles_x * a.tiles_y;
  const size_t lds = pooled ? D::lds_pooled : D::lds_plain;
  const void* kern = pooled ? (const void*)stem_wgrad_pooled_kernel<KS, PAD, TN> : (const void*)stem_wgrad_kernel<KS, PAD, TN>;
  static SqdDevOnce lds_once[2];
  if (lds > 64 * 1024 && sqd_max_lds_once(lds_once[pooled], kern, (int)lds) != SQD_OK) return SQD_ERR_LAUNCH;
  if (pooled) hipLaunchKernelGGL((stem_wgrad_pooled_kernel<KS, PAD, TN>), dim3((unsigned)S), dim3(256), lds, s, a);
  else hipLaunchKernelGGL((stem_wgrad_kernel<KS, PAD, TN>), dim3((unsigned)S), dim3(256), lds, s, a);
  return sqd_launch_status();
}

static int stem_wgrad_common(StemWgradArgs a, int ksize, int S, float* dw, float* db, bool pooled, hipStream_t s) {
  const int K = 3 * ksize * ksize;
  a.slab_stride = (long long)a.N * K + a.N;
  const StemGeom g = stem_geom(a.Hin, a.Win, ksize);
  a.Ho = g.Ho; a.Wo = g.Wo; a.Hp = g.Hp; a.Wp = g.Wp;
  int rc;
  if (pooled && !stem_hook_off("SQD_STEM_WGRAD_GATHER") && stem_wave_ok(g, a.B, a.N, a.img)) {
    const int ng = launch_stem_wgrad_gather(a, S, s);
    if (ng < 0) return SQD_ERR_LAUNCH;
    S = ng; rc = SQD_OK;
  } else {
    rc = stem_dispatch(ksize, a.N, [&](auto sh) {
      using T = decltype(sh);
      return launch_stem_wgrad_dense<T::KS, T::PAD, T::NT>(a, S, pooled, s);
    });
  }
  if (rc != SQD_OK) return rc;
  // slab layout [n][K] is already OIHW-flat: reduce with C := K, TAPS := 1
  return sqd_wgrad_reduce_launch(a.slab, dw, db, S, a.slab_stride, a.N, K, 1, s);
}

// dy: NHWC [B][Ho][Wo][N] (ReLU-masked); img: NCHW [B][3][Hin][Win]; slab: S*(N*3*k*k + N) floats;
// dw: OIHW [N][3][k][k]; db: [N].
extern "C" int sqd_stem_wgrad(const float* dy, const float* img, float* slab, float* dw, float* db, int B, int Hin,
                              int Win, int N, int ksize, int S, void* stream) {
  SQD_CHECK_ARG(dy && img && slab && dw && B > 0 && Hin > 0 && Win > 0 && S > 0 && S <= 65535);
  SQD_CHECK_ARG(((uintptr_t)dy & 15) == 0);
  StemWgradArgs a;
  a.dy = dy; a.img = img; a.slab = slab; a.pooled = nullptr; a.amax = nullptr; a.B = B; a.Hin = Hin; a.Win = Win; a.N = N;
  return stem_wgrad_common(a, ksize, S, dw, db, false, (hipStream_t)stream);
}

// The same gradient when the forward ran fused (sqd_stem_conv_relu_pool_fwd): dpool / pooled are NHWC
// [B][Hp][Wp][N] (gradient w.r.t. and value of the pooled output), argmax the uint8 tensor the forward wrote.
extern "C" int sqd_stem_wgrad_pooled(const float* dpool, const float* pooled, const unsigned char* argmax, const float* img,
                                     float* slab, float* dw, float* db, int B, int Hin, int Win, int N, int ksize, int S,
                                     void* stream) {
  SQD_CHECK_ARG(dpool && argmax && img && slab && dw && B > 0 && Hin > 0 && Win > 0 && S > 0 && S <= 65535);
  SQD_CHECK_ARG(((uintptr_t)dpool & 15) == 0 && ((uintptr_t)pooled & 15) == 0 && ((uintptr_t)argmax & 3) == 0);
  StemWgradArgs a;
  a.dy = dpool; a.img = img; a.slab = slab; a.pooled = pooled; a.amax = argmax; a.B = B; a.Hin = Hin; a.Win = Win; a.N = N;
  return stem_wgrad_common(a, ksize, S, dw, db, true, (hipStream_t)stream);
}
