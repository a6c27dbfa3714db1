// What the stem translation units share (stem_pool.hip: forward; stem_wgrad.hip: dense weight gradients and the C entries;
// stem_wgrad_gather.hip: the gather weight gradient).  Host part: ONE derivation of the output geometry, the supported stems, the
// wave-kernel eligibility rule, the tile split and the two test hooks.  Device part: the wave-private patch loader of
// stem_wave_kernel and stem_wgrad_gather_kernel, and the planar patch staging of the two first-generation kernels.
// Reference: src/model/squeezedet.py:34-36 (Conv2d(3,64,3,s2,p1)+ReLU+MaxPool(3,2,ceil)), :52-54 (Conv2d(3,96,7,s2,p3)).
#pragma once
#include "sqd_common.h"
#include <stdlib.h>

// ---------------------------------------------------------------------------------------------
// Host: geometry
// ---------------------------------------------------------------------------------------------
// Image Hin x Win -> conv (stride 2, pad = ksize / 2) Ho x Wo -> MaxPool(3, 2, ceil) Hp x Wp.
struct StemGeom { int Hin, Win, ksize, pad, Ho, Wo, Hp, Wp; };

static inline StemGeom stem_geom(int Hin, int Win, int ksize) {
  StemGeom g;
  g.Hin = Hin; g.Win = Win; g.ksize = ksize; g.pad = ksize == 3 ? 1 : 3;
  g.Ho = (Hin + 2 * g.pad - ksize) / 2 + 1; g.Wo = (Win + 2 * g.pad - ksize) / 2 + 1;
  g.Hp = (g.Ho - 3 + 1) / 2 + 1; g.Wp = (g.Wo - 3 + 1) / 2 + 1;
  return g;
}

// The supported stems and their template triple <KS, PAD, NT> (NT = N / 16: 16-channel blocks; the weight gradients call it TN).
// f is called with a StemShape value; anything else is SQD_ERR_UNSUPPORTED.
template <int KS_, int PAD_, int NT_> struct StemShape { static constexpr int KS = KS_, PAD = PAD_, NT = NT_; };
template <class F> static inline int stem_dispatch(int ksize, int N, F&& f) {
  if (ksize == 3 && N == 64) return f(StemShape<3, 1, 4>{});
  if (ksize == 7 && N == 96) return f(StemShape<7, 3, 6>{});
  return SQD_ERR_UNSUPPORTED;
}

// Where the wave-autonomous kernels (stem_wave_kernel, stem_wgrad_gather_kernel) run: the 3x3 / 64-channel stem, image rows made of
// whole 16-byte slots (Win % 4 == 0, 16-byte aligned image) and both tensors within the 2^31-byte range of a buffer resource.
static inline bool stem_wave_ok(const StemGeom& g, int B, int N, const void* x) {
  return g.ksize == 3 && N == 64 && (g.Win & 3) == 0 && ((uintptr_t)x & 15) == 0 &&
         (long long)B * 3 * g.Hin * g.Win * 4 < (1ll << 31) && (long long)B * g.Hp * g.Wp * N * 4 < (1ll << 31);
}

// Tile split of the pooled map into PH x PW tiles: fills tiles_x, tiles_y, ntiles and the magic divisors ceil(2^32 / tiles) the
// kernels split a tile index with (scalar multiply-highs; 0 = divisor 1).  The split is exact while ntiles * max(tiles) < 2^32:
// false (nothing launched) past that.
template <class Args> static inline bool stem_fill_tiles(Args& a, int PH, int PW) {
  a.tiles_x = sqd_cdiv(a.Wp, PW); a.tiles_y = sqd_cdiv(a.Hp, PH);
  a.ntiles = a.B * a.tiles_x * a.tiles_y;
  if ((long long)a.ntiles * (a.tiles_x > a.tiles_y ? a.tiles_x : a.tiles_y) >= (1ll << 32)) return false;
  a.tiles_x_m = a.tiles_x > 1 ? (unsigned)(((1ull << 32) + a.tiles_x - 1) / a.tiles_x) : 0u;
  a.tiles_y_m = a.tiles_y > 1 ? (unsigned)(((1ull << 32) + a.tiles_y - 1) / a.tiles_y) : 0u;
  return true;
}

struct StemWaveArgs {
  const float* x; const float* w; const float* bias; float* y; uint8_t* amax;
  const float* wsq; const float* bsq;       // SQ variant: the next Fire's squeeze (1x1, 64 -> SQ channels, OIHW + bias); y is ITS output
  float* ysq;                               // ARGMAX + SQ (training): y and amax as without SQ, the squeeze output goes HERE
  int B, Hin, Win, Ho, Wo, Hp, Wp;
  int tiles_x, tiles_y, ntiles;
  unsigned tiles_x_m, tiles_y_m;
};

static inline StemWaveArgs stem_wave_args(const StemGeom& g, int B, const float* x, const float* w, const float* bias, float* y,
                                          uint8_t* amax, const float* wsq, const float* bsq, float* ysq) {
  StemWaveArgs a;
  a.x = x; a.w = w; a.bias = bias; a.y = y; a.amax = amax; a.wsq = wsq; a.bsq = bsq; a.ysq = ysq;
  a.B = B; a.Hin = g.Hin; a.Win = g.Win; a.Ho = g.Ho; a.Wo = g.Wo; a.Hp = g.Hp; a.Wp = g.Wp;
  a.tiles_x = a.tiles_y = a.ntiles = 0; a.tiles_x_m = a.tiles_y_m = 0u;     // (the launcher: stem_fill_tiles)
  return a;
}

struct StemWgradArgs {
  const float* dy; const float* img; float* slab;
  const float* pooled; const unsigned char* amax;    // pooled forms: dy is dPool [B][Hp][Wp][N]
  int Hp, Wp;
  int B, Hin, Win, Ho, Wo, N;
  int tiles_x, tiles_y, nblocks;
  long long slab_stride;
};

// stem_wgrad_gather.hip: the gather form of the pooled stem weight gradient (3x3 / 64-channel stem).  Launches one workgroup per
// slab, at most S; returns the number of slabs written (the caller reduces exactly that many) or -1 on a launch failure.
int launch_stem_wgrad_gather(StemWgradArgs a, int S, hipStream_t s);

// Test hooks, read from the environment on every call (the parity tests and tools/fuzz_stem.py switch them at run time).  Each
// has one meaning, "a value that starts with 0 turns the shipped kernel off"; unset or anything else is the shipped kernel:
//   SQD_STEM_WAVE=0          the fused forward runs the workgroup kernel stem_pool_kernel where stem_wave_kernel would run;
//   SQD_STEM_WGRAD_GATHER=0  the pooled weight gradient runs the dense stem_wgrad_pooled_kernel where the gather kernel would run.
// Both pairs agree bit for bit (forward) / to rounding (weight gradient); nothing else reads the environment in the stem.
static inline bool stem_hook_off(const char* name) {
  const char* e = getenv(name);
  return e && e[0] == '0';
}

// ---------------------------------------------------------------------------------------------
// Device: planar patch staging of stem_conv_kernel and stem_wgrad_kernel.  The NCHW input patch [3][IH][IW] of the conv tile at
// (y0, x0) goes through registers into LDS with row pitch IWP, zeros outside the image (the convolution's padding).
// ---------------------------------------------------------------------------------------------
template <int PAD, int IH, int IW, int IWP>
__device__ __forceinline__ void stem_stage_planar(float* inT, const float* const& img, int b, int y0, int x0, const int& Hin, const int& Win, int tid) {
  for (int idx = tid; idx < 3 * IH * IW; idx += 256) {
    const int c = idx % IW; int r = idx / IW; const int ci = r / IH; r -= ci * IH;
    const int iy = 2 * y0 - PAD + r, ix = 2 * x0 - PAD + c;
    float v = 0.f;
    if (iy >= 0 && iy < Hin && ix >= 0 && ix < Win) v = img[(((long long)b * 3 + ci) * Hin + iy) * Win + ix];
    inT[(ci * IH + r) * IWP + c] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// Device: the wave-private patch loader.  A wave owns a pooled tile of PH x PW pixels; the NCHW patch that feeds it is
// [3 planes][IH = 4 PH + 3 rows][SL 16-byte slots] (RP = 4 SL floats per row, SL >= PW + 2), flat in a wave-private LDS buffer of
// BUFF floats.  Origin convention: buffer resource based at img - (Win + 4) floats, so that the patch origin -- input row
// 4 PH ty - 1, column 4 PW tx - 4: four floats left of the first tap, which keeps every row segment 16-byte aligned in a
// 4-float-aligned image row -- is never negative relative to it.  Lane l owns slots l, l + 64, ..: d_off[] is the slot's byte offset
// from the patch origin, computed once; a tile contributes one scalar offset.  Slots past the patch, and on border tiles (a uniform
// test) slots outside the image, carry an out-of-range offset and are zero-filled by the hardware: the convolution's padding.
// dma_in issues exactly N_IT buffer-resource LDS-DMA loads, in slot order: the kernels' counted s_waitcnt vmcnt rely on that.
// ---------------------------------------------------------------------------------------------
template <int PH_, int PW_, int SL_>
struct StemPatch {
  static constexpr int PH = PH_, PW = PW_, SL = SL_;
  static constexpr int IH = 4 * PH + 3, RP = 4 * SL;
  static constexpr int NSLOT = 3 * IH * SL, N_IT = (NSLOT + 63) / 64, BUFF = N_IT * 64 * 4;   // slots, loads per lane, floats per buffer
  static constexpr unsigned OOB = 0x80000000u;
  // What each kernel takes from here is what leaves its generated code as it was (profiles/stem_refactor_device_asm_diff.log):
  //  * both: the geometry constants and resource(); both keep the five-line d_off[] loop in the kernel (as a function it changes
  //    their code, the wave kernel's by half);
  //  * stem_wgrad_gather_kernel: origin() and dma_in() -- byte-identical code.  The kernel's arguments come by reference and are
  //    read where they are used (Hin, Win by value: two more vector-memory instructions);
  //  * stem_wave_kernel keeps its own copy of the bodies of origin() and dma_in() (its lambdas are inlined by cost, not by
  //    attribute, and every form of a call inside them changed the kernel: 62 -> 63 vector-memory instructions at best).
  //    A change to either body is made in both places.
#if defined(__HIP_DEVICE_COMPILE__)
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  static __device__ __forceinline__ __amdgpu_buffer_rsrc_t resource(const float* img, int Win) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(img - (Win + 4)), 0, 0x7ffffff0, 0x00020000);
  }
  // tile (b, ty, tx): the scalar byte offset of its patch origin, and whether the whole patch lies inside the image
  template <class Args>
  static __device__ __forceinline__ void origin(int b, int ty, int tx, const Args& a, unsigned& soff, int& inner) {
    const int iy0 = 4 * PH * ty - 1, ix0 = 4 * PW * tx - 4;
    soff = (unsigned)(((b * 3 * a.Hin + 4 * PH * ty) * a.Win + 4 * PW * tx) * 4);
    inner = iy0 >= 0 && iy0 + IH <= a.Hin && ix0 >= 0 && ix0 + RP <= a.Win;
  }
  template <class Args>
  static __device__ __forceinline__ void dma_in(__amdgpu_buffer_rsrc_t xres, float* buf, const int (&d_off)[N_IT], int ty, int tx,
                                                int inner, unsigned soff, const int& lane, const Args& a) {
    const int iy0 = 4 * PH * ty - 1, ix0 = 4 * PW * tx - 4;
#pragma unroll
    for (int it = 0; it < N_IT; ++it) {
      int off = d_off[it];
      if (!inner) {                                    // uniform: border tile (the slot's row / column are recomputed here only)
        const int slot = it * 64 + lane;
        const int ci = slot / (IH * SL), rem = slot - ci * (IH * SL), row = rem / SL, k4 = rem - row * SL;
        const bool ok = slot < NSLOT && (unsigned)(iy0 + row) < (unsigned)a.Hin && (unsigned)(ix0 + 4 * k4) < (unsigned)a.Win;
        off = ok ? off : (int)OOB;
      }
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xres, (lds_ptr_t)(buf + it * 256), 16, off, (int)soff, 0, 0);
    }
  }
#endif
};
