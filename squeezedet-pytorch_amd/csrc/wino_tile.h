// Shared pieces of the Winograd F(2x2, 3x3) kernel family (conv_wino.hip with wino_bridge.h / wino_poolbridge.h, conv_wino_sk.hip,
// conv_wino_vs.hip): group geometry, patch addressing, the two transforms, the hazard-safe 16-byte store, and the launch
// geometry / entry checks of the host side.  Everything is force-inlined and takes its arrays by reference: no accumulator
// escapes to memory, and register and LDS budgets of the kernels are those of the hand-written copies the helpers replaced.
// A kernel whose copy differs in substance keeps it and says so in one line.
#pragma once
#include "sqd_common.h"

// ---------------------------------------------------------------------------------------------------------------------
// Device side
// ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ f32x4 wino_relu4(f32x4 v, float lo) {
  asm volatile("v_max_f32 %0, %4, %0\n\tv_max_f32 %1, %4, %1\n\tv_max_f32 %2, %4, %2\n\tv_max_f32 %3, %4, %3"
               : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w) : "s"(lo));
  return v;
}

// A GROUP is 4 rows x 16 columns of output = 16 Winograd tiles; groups are numbered image-major, then row-group, then
// column-group.  Position of group q (all wave-uniform): first output pixel (y0, x0), its flat pixel index p0, the byte offset
// of its patch origin from the patch resource's base (soff), inner = the 6x18 patch lies wholly inside the image, valid =
// q < ngroups.  An invalid q is clamped to the last group: idle waves of the last super-group redo it and do not store.
// The index is split with two scalar multiply-highs by gxn_m = ceil(2^32 / gxn), gyn_m = ceil(2^32 / gyn) (exact:
// (ngroups + 8) * max(gxn, gyn) < 2^32, host-checked; magic 0 = divisor 1) -- a division of wave-uniform integers otherwise
// goes through ~10 vector instructions + readfirstlane, and every vector instruction delays the SIMD's MFMA stream.
// Args: any struct with ngroups, gxn, gyn, gxn_m, gyn_m, H, W, x_pitch.
struct WinoGPos { int y0, x0, inner, valid; long long p0; unsigned soff; };

template <class Args>
__device__ __forceinline__ WinoGPos wino_group_pos(const Args& a, int q) {
  WinoGPos gp;
  gp.valid = (int)((unsigned)(q - a.ngroups) >> 31);       // q < ngroups
  q = gp.valid ? q : a.ngroups - 1;
  const int q1 = a.gxn_m ? (int)__umulhi((unsigned)q, a.gxn_m) : q;        // q / gxn
  const int gxi = q - q1 * a.gxn;
  const int b = a.gyn_m ? (int)__umulhi((unsigned)q1, a.gyn_m) : q1;       // q1 / gyn
  const int gyi = q1 - b * a.gyn;
  gp.y0 = gyi * 4; gp.x0 = gxi * 16;
  gp.p0 = ((long long)b * a.H + gp.y0) * a.W + gp.x0;
  gp.soff = (unsigned)(gp.p0 * a.x_pitch * 4);
  gp.inner = (int)(((unsigned)(-gp.y0) & (unsigned)(gp.y0 + 4 - a.H) & (unsigned)(-gp.x0) & (unsigned)(gp.x0 + 16 - a.W)) >> 31);
  return gp;
}

// The raw patch of a group and K chunk in LDS: 8 channels as two k-quad planes of 6 x 18 pixels, one 16-byte slot per (plane,
// pixel).  WINO_RP slots per plane (108 used): 113 * 16 B = 16 mod 256, so the two planes interleave in the LDS bank row and
// the transform's reads do not collide.  A wave fetches it with RAW_IT LDS-DMA instructions of 64 slots.
constexpr int WINO_RP = 113;
// Per-lane DMA offset of a slot outside the image: beyond the resource's range, so the hardware range check returns zeros
// (the zero padding of the convolution) without touching memory.  Only the per-lane offset is range-checked, the SGPR
// offset is not (MI355X_MICROARCH.md buffer addressing), so the range only has to exceed any in-patch offset.
constexpr unsigned WINO_OOB = 0x80000000u;

// One slot of the patch: byte offset inside the patch (padding slots: 0) and row << 8 | col (-1 = padding).
__device__ __forceinline__ void wino_patch_slot(int slot, int W, int x_pitch, int& offB, int& key) {
  const int kq = slot / WINO_RP, pix = slot - kq * WINO_RP;
  const bool real = kq < 2 && pix < 108;
  const int r = pix / 18, c = pix - r * 18;
  key = real ? (r << 8 | c) : -1;
  offB = real ? ((r * W + c) * x_pitch + 4 * kq) * 4 : 0;
}

// (A wave's slots are it * 64 + lane, it < RAW_IT.  That loop stays at the call on purpose: a function holding it is simplified
// on its own, without the caller's lane = tid & 63, and folds the slot compares into a form that costs the callers four more
// SGPR spills.)

// Per-lane patch offsets of one group, evaluated once per group: the plain offsets for an interior group, WINO_OOB for the
// slots outside the image otherwise.
template <int RAW_IT>
__device__ __forceinline__ void wino_group_offsets(int y0, int x0, int inner, int H, int W, const int (&r_offB)[RAW_IT],
                                                   const int (&r_key)[RAW_IT], int (&r_offG)[RAW_IT]) {
  if (inner) {
#pragma unroll
    for (int it = 0; it < RAW_IT; ++it) r_offG[it] = r_offB[it];
    return;
  }
#pragma unroll
  for (int it = 0; it < RAW_IT; ++it) {
    const int key = r_key[it];
    const bool ok = key >= 0 && (unsigned)(y0 + (key >> 8) - 1) < (unsigned)H && (unsigned)(x0 + (key & 255) - 1) < (unsigned)W;
    r_offG[it] = ok ? r_offB[it] : (int)WINO_OOB;
  }
}

// A lane's transform unit inside a raw patch starts at float offset
//   ((g >> 1) * WINO_RP + (2 * (lr >> 3)) * 18 + 2 * (lr & 7)) * 4 + 2 * (g & 1)
// -- tile lr (lanes 0-31 of a ds_read_b64 = tile row 0, 32-63 = tile row 1; within a half 8 tiles x (k-quad, channel half):
// 32 distinct 8-byte units of one 256-byte bank row, conflict-free), channel pair g of the chunk: the lane's role as MFMA B
// operand (column = tile lr, k = channel pair g), so the transformed values are consumed by the lane that computed them and
// never leave its registers.  (The kernels write the expression out: as a function it is simplified without the ranges of lr
// and g, and that form cost the fused Fire kernels four more SGPR spills.)

// A 16-byte MUBUF store whose soffset is an SGPR, directly followed by a VALU write of its first data register, stored
// the NEW value in the last four lanes of every 16-lane row on this chip (found as rare wrong outputs, always component
// 0 of tile columns 12..15; the compiler only pads this write-after-read hazard when soffset is NOT a register): two
// wait states behind every such store, pinned in place.
__device__ __forceinline__ void wino_store16(f32x4 v, __amdgpu_buffer_rsrc_t res, int voff, int soff) {
  typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), res, voff, soff, 0);
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 1" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// Input transform V = B^T d B of (tile, channel pair): rawL = the lane's unit in the raw patch (above), vv[pos] the
// 16 transformed positions for its two channels.  16 ds_read_b64 (2-way bank conflicted in this order, cheap next to a V round
// trip through LDS) and 32 packed adds.
__device__ __forceinline__ void wino_input_transform(const float* rawL, f32x2 (&vv)[16]) {
  f32x2 t[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x2 d0 = *(const f32x2*)(rawL + (0 * 18 + j) * 4), d1 = *(const f32x2*)(rawL + (1 * 18 + j) * 4);
    const f32x2 d2 = *(const f32x2*)(rawL + (2 * 18 + j) * 4), d3 = *(const f32x2*)(rawL + (3 * 18 + j) * 4);
    t[0][j] = d0 - d2; t[1][j] = d1 + d2; t[2][j] = d2 - d1; t[3][j] = d1 - d3;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    vv[i * 4 + 0] = t[i][0] - t[i][2]; vv[i * 4 + 1] = t[i][1] + t[i][2];
    vv[i * 4 + 2] = t[i][2] - t[i][1]; vv[i * 4 + 3] = t[i][1] - t[i][3];
  }
}

// expand1x1 slices (a 1x1 convolution in the Winograd domain) only need the four inner positions (1,1), (1,2), (2,1), (2,2):
// rows 1, 2 x columns 1, 2 of the tile's 4x4 patch -> vv[5], vv[6], vv[9], vv[10]; the rest of vv is left alone.
__device__ __forceinline__ void wino_input_transform_inner(const float* rawL, f32x2 (&vv)[16]) {
  const f32x2 d11 = *(const f32x2*)(rawL + (1 * 18 + 1) * 4), d12 = *(const f32x2*)(rawL + (1 * 18 + 2) * 4);
  const f32x2 d21 = *(const f32x2*)(rawL + (2 * 18 + 1) * 4), d22 = *(const f32x2*)(rawL + (2 * 18 + 2) * 4);
  const f32x2 t11 = d11 + d21, t12 = d12 + d22, t21 = d21 - d11, t22 = d22 - d12;      // column transform rows 1, 2
  vv[5] = t11 + t12; vv[6] = t12 - t11; vv[9] = t21 + t22; vv[10] = t22 - t21;
}

// Inverse transform Y = A^T M A of channel block j: acc[pos][j] -> ov[px], the tile's four pixels (px = 2 row + column).  On
// register pairs (f32x2): adds AND subtracts then compile to one v_pk_add_f32 per pair (a 4-wide subtract would be four
// scalar v_sub_f32).
template <class Get>
__device__ __forceinline__ void wino_inverse_of(Get m, f32x4 (&ov)[4]) {      // m(pos): accumulator of a position
  auto inv = [&](auto half, auto put) {             // half(v): the register pair to work on; put(px, y): store it
    f32x2 s[4][2];
#pragma unroll
    for (int xi = 0; xi < 4; ++xi) {
      const f32x2 m0 = half(m(xi * 4 + 0)), m1 = half(m(xi * 4 + 1));
      const f32x2 m2 = half(m(xi * 4 + 2)), m3 = half(m(xi * 4 + 3));
      s[xi][0] = m0 + m1 + m2;
      s[xi][1] = m1 - (m2 + m3);
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      put(0 * 2 + b, s[0][b] + s[1][b] + s[2][b]);
      put(1 * 2 + b, s[1][b] - (s[2][b] + s[3][b]));
    }
  };
  inv([](const f32x4& v) { return (f32x2)v.lo; }, [&](int px, f32x2 y) { ov[px].lo = y; });
  inv([](const f32x4& v) { return (f32x2)v.hi; }, [&](int px, f32x2 y) { ov[px].hi = y; });
}
template <int NT>
__device__ __forceinline__ void wino_inverse(const f32x4 (&acc)[16][NT], int j, f32x4 (&ov)[4]) {
  wino_inverse_of([&](int p) -> const f32x4& { return acc[p][j]; }, ov);
}
// ... of a wave that holds one channel block: acc[pos]
__device__ __forceinline__ void wino_inverse(const f32x4 (&acc)[16], f32x4 (&ov)[4]) {
  wino_inverse_of([&](int p) -> const f32x4& { return acc[p]; }, ov);
}

// expand1x1 pass of 16-wide passes: M is non-zero only at the inner 2x2, y00 = m11+m12+m21+m22, y01 = m11-m12+m21-m22,
// y10 = m11+m12-m21-m22, y11 = m11-m12-m21+m22; channel block r lives in accumulators [4 q + r], q = 0..3.
__device__ __forceinline__ void wino_inverse_inner(const f32x4 (&acc)[16], int r, f32x4 (&ov)[4]) {
  auto inv1 = [&](auto half, auto put) {            // (register pairs: packed adds)
    const f32x2 m0 = half(acc[0 + r]), m1 = half(acc[4 + r]), m2 = half(acc[8 + r]), m3 = half(acc[12 + r]);
    const f32x2 s01 = m0 + m1, d01 = m0 - m1, s23 = m2 + m3, d23 = m2 - m3;
    put(0, s01 + s23); put(1, d01 + d23); put(2, s01 - s23); put(3, d01 - d23);
  };
  inv1([](const f32x4& v) { return (f32x2)v.lo; }, [&](int px, f32x2 y) { ov[px].lo = y; });
  inv1([](const f32x4& v) { return (f32x2)v.hi; }, [&](int px, f32x2 y) { ov[px].hi = y; });
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------------------------

// What every 3x3 entry point of the family asks of its tensors: x window [x_coff, +C) of x_pitch, y window [y_coff, +N) of
// y_pitch (float4-aligned), per-lane byte offsets inside a group (pitch = the widest tensor a lane addresses) below 2^30, the
// 32-bit SGPR byte offset of a group origin, and the packed weights (C/8 chunks of 16 positions x Npad x 8 channels) below 4 GiB.
static inline int wino_check_common(int B, int H, int W, int C, int x_pitch, int x_coff, int N, int Npad, int y_pitch, int y_coff,
                                    int widest_pitch) {
  SQD_CHECK_ARG(x_pitch % 4 == 0 && x_coff % 4 == 0 && y_pitch % 4 == 0 && y_coff % 4 == 0);
  SQD_CHECK_ARG(x_coff >= 0 && x_coff + C <= x_pitch && y_coff >= 0 && y_coff + N <= y_pitch);
  SQD_CHECK_ARG((long long)W * 6 * widest_pitch * 4 < (1ll << 30));
  SQD_CHECK_ARG((long long)B * H * W * x_pitch * 4 < (1ll << 32) - (1ll << 30));
  SQD_CHECK_ARG((long long)(C >> 3) * 16 * Npad * 8 * 4 < (1ll << 32));
  return SQD_OK;
}

// (The three functions below are templates only because WinoArgs is declared in conv_wino.hip, behind this header; WinoArgs is
// their one instantiation -- conv_wino_sk and conv_wino_vs keep their own geometry.)
// The WinoArgs fields every entry point of conv_wino.hip sets the same way (N = the expand3x3 / only output width).
template <class Args>
static inline void wino_fill_args(Args& a, const float* x, const float* u, float* y, int B, int H, int W, int C, int x_pitch, int x_coff,
                                  int N, int Npad, int y_pitch, int y_coff, int relu) {
  a.x = x; a.u = u; a.y = y;
  a.B = B; a.H = H; a.W = W; a.C = C; a.x_pitch = x_pitch; a.x_coff = x_coff;
  a.N = N; a.Npad = Npad; a.y_pitch = y_pitch; a.y_coff = y_coff; a.relu = relu;
}

// Groups, magic multipliers (see wino_group_pos) and super-groups of WV groups.
template <class Args>
static inline int wino_launch_geometry(Args& a, int WV) {
  a.gxn = sqd_cdiv(a.W, 16); a.gyn = sqd_cdiv(a.H, 4);
  a.ngroups = a.B * a.gxn * a.gyn;
  if ((long long)(a.ngroups + 8) * (a.gxn > a.gyn ? a.gxn : a.gyn) >= (1ll << 32)) return SQD_ERR_UNSUPPORTED;
  a.gxn_m = a.gxn > 1 ? (unsigned)(((1ull << 32) + a.gxn - 1) / a.gxn) : 0u;
  a.gyn_m = a.gyn > 1 ? (unsigned)(((1ull << 32) + a.gyn - 1) / a.gyn) : 0u;
  a.ntiles = sqd_cdiv(a.ngroups, WV);
  return SQD_OK;
}
