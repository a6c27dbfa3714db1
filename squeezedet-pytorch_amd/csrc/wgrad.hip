// Weight / bias gradients of the convolutions (the reference gets them from autograd through
// nn.Conv2d, src/engine/trainer.py:47), the deterministic slab reduction, and the weight packer.
//
// dW[n][c][tap] = sum over pixels p of dY[p][n] * X[p + offset(tap)][c]      (dY already ReLU-masked)
// db[n]         = sum over pixels p of dY[p][n]
//
// This is a GEMM whose reduction axis is the pixel axis (B*H*W up to 599,040), so it is split over
// workgroups: each workgroup owns an output tile (TN*16 out-channels x TC*16 in-channels x all taps),
// walks a strided subset of the pixel blocks accumulating in MFMA registers, and writes ONE partial
// slab; a second kernel sums the slabs in fixed order (bitwise reproducible -- no float atomics)
// and emits the gradient in the checkpoint's OIHW layout.  MFMA operand A = dY^T (row = out-channel,
// k = pixel), operand B = X (k = pixel, column = in-channel); both are read from pixel-major LDS
// tiles whose pitch is = 16 (mod 32) floats so the two k-groups of a 32-lane half hit disjoint banks.
// The bias gradient rides along as extra tiles with B = 1.
#include "sqd_common.h"
#include <stdlib.h>
#include <type_traits>

#ifndef SQD_WG9_TH
#define SQD_WG9_TH 4
#endif
struct WgradArgs {
  const float* dy; const float* x; float* slab;
  int B, H, W;
  int N, dy_pitch, dy_coff;
  int C, x_pitch, x_coff;
  int tiles_x, tiles_y, nblocks, n_groups;
  long long total_px;
  long long slab_stride;
  // DG instantiation (sqd_squeeze_bwd: a Fire squeeze's weight AND data gradient in one launch): the layer's own weight
  // [N][C] (OIHW, 1x1), the data-gradient output window and whether x's ReLU mask applies to it
  const float* w; float* dx;
  int dx_pitch, dx_coff, dx_mask;
};

// LDS tiles are pixel-major rows of exactly TN*16 (dY) / TC*16 (X) floats, filled by LDS-DMA
// (global_load_lds_dwordx4: 64 consecutive 16-byte slots per wave instruction, arbitrary per-lane source,
// out-of-range sources read a zero page) into a double buffer: the next pixel block streams in during the
// MFMAs of the current one, one barrier per block.  When a row is a multiple of 32 floats the 16-byte
// slot index is XOR-ed with 4*(pixel&1) so the two k-groups of a 32-lane half (adjacent pixels, same
// channel) land in different banks for the ds_read_b32 operand fetches; other row lengths are = 16 (mod 32)
// floats and need no swizzle.  With TN a multiple of 4 every wave owns whole out-channel tiles and its
// dY operand is fetched once per k-step for all taps / in-channel tiles.
__device__ __attribute__((aligned(16))) float sqd_wg_zero_page[4] = {0.f, 0.f, 0.f, 0.f};
typedef __attribute__((address_space(3))) void* wg_lds_ptr_t;

// DG = true (1x1 only, all N output channels in one group): the workgroup that streams pixel block pb for in-channels
// [c0, c0 + TC*16) also emits that block's DATA gradient dx[p][c] = sum_n dy[p][n] w[n][c] (x's ReLU mask applied from the staged
// x tile) -- both operands are already in LDS for the weight gradient, every pixel block is visited exactly once per channel
// group, so the separate data-gradient launch and its second (mask) and third (weight-gradient) read of x go away.  MFMA form:
// rows = in-channel, columns = pixel, k = out-channel with the k-slice permuted as in the Fire bridges (MFMA r of a 16-channel
// block takes n = 16 j + 4 g + r from lane group g): one ds_read_b128 of a dy row piece / of a transposed-weight row piece feeds
// four MFMAs, and a lane ends with four consecutive in-channels of one pixel = one 16-byte store.
// The body serves the one-layer launch (conv_wgrad_kernel: grid = (splits, channel-tile groups)) and the grouped one below.
// ``split`` / ``nsplit``: which pixel blocks (split, split + nsplit, ...) and which slab; ``by``: the (out, in)-channel tile group.
template <int TAPS, int TN, int TC, int TH, bool DG = false>
__device__ __forceinline__ void wg_body(const WgradArgs& a, const int split, const int nsplit, const int by) {
  static_assert(!DG || TAPS == 1, "the fused data gradient exists for 1x1 layers");
  constexpr int PB = TH * 16;                                 // pixels per block
  constexpr int RN = TN * 4, RC = TC * 4;                     // 16-byte slots per row
  constexpr bool SWN = (RN % 8) == 0, SWC = (RC % 8) == 0;    // row = multiple of 32 floats -> swizzle
  constexpr int XPIX = (TAPS == 9) ? (TH + 2) * 18 : PB;
  constexpr int DSLOTS = (PB * RN + 255) & ~255, XSLOTS = (XPIX * RC + 255) & ~255;
  constexpr int D_IT = DSLOTS / 256, X_IT = XSLOTS / 256;
  constexpr bool SHARED = (TN % 4) == 0;                      // wave w owns n-tiles w, w+4, ...
  constexpr int NU = SHARED ? TN / 4 : 1;
  constexpr int TILES = TN * TC * TAPS;
  constexpr int NACC = SHARED ? NU * TC * TAPS : (TILES + 3) / 4;
  constexpr int BACC = (TN + 3) / 4;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  // layout: dy[0], dy[1], x[0], x[1] (, transposed weights [TC*16][WP] for DG)
  float* const dyB = smem;
  float* const xB = smem + 2 * DSLOTS * 4;
  constexpr int WP = ((TN * 16 + 63) / 64) * 64 + 8;          // row pitch = 8 (mod 64) floats: conflict-free ds_read_b128 over (row lr, piece g)
  float* const wtT = xB + 2 * XSLOTS * 4;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, kq = lane >> 4;
  const int ng = by % a.n_groups, cg = by / a.n_groups;
  const int n0 = ng * TN * 16, c0 = cg * TC * 16;
  const bool do_bias = (cg == 0);

  const int wave_s = __builtin_amdgcn_readfirstlane(wave);

  // Block-independent part of this lane's DMA slots: a 32-bit element offset from the block's origin pointer (dY: its
  // first pixel; X, 3x3: the halo pixel (y0-1, x0-1)).  Interior blocks issue their DMA as uniform base + offset with
  // no per-lane arithmetic; only border blocks look at the packed (row, col) key to send out-of-image slots to the
  // zero page.  Slots of channels beyond N / C and padding slots fetch the origin element: whatever they hold only
  // reaches accumulator rows / columns that are never stored.
  int d_off[D_IT], d_key[D_IT], x_off[X_IT], x_key[X_IT];
#pragma unroll
  for (int it = 0; it < D_IT; ++it) {
    const int slot = it * 256 + tid;
    const int pix = slot / RN, qp = slot - pix * RN;
    const int q = SWN ? (qp ^ ((pix & 1) << 2)) : qp;
    const bool real = pix < PB && n0 + 4 * q < a.N;
    const int r = (TAPS == 9) ? (pix >> 4) : 0, c = (TAPS == 9) ? (pix & 15) : pix;
    d_off[it] = real ? (r * a.W + c) * a.dy_pitch + n0 + 4 * q : 0;
    d_key[it] = real ? (r << 16 | c) : -1;
  }
#pragma unroll
  for (int it = 0; it < X_IT; ++it) {
    const int slot = it * 256 + tid;
    const int pix = slot / RC, qp = slot - pix * RC;
    const int q = SWC ? (qp ^ ((pix & 1) << 2)) : qp;
    const bool real = pix < XPIX && c0 + 4 * q < a.C;
    const int r = (TAPS == 9) ? pix / 18 : 0, c = (TAPS == 9) ? pix - r * 18 : pix;
    x_off[it] = real ? (r * a.W + c) * a.x_pitch + c0 + 4 * q : 0;
    x_key[it] = real ? (r << 16 | c) : -1;
  }

  auto dma_block = [&](int pb, int buf) {
    int y0 = 0, x0 = 0, inner;
    long long p0;                                          // flat index of the block's first pixel
    if (TAPS == 9) {
      int t = pb;
      const int tx = t % a.tiles_x; t /= a.tiles_x;
      const int ty = t % a.tiles_y; const int b = t / a.tiles_y;
      y0 = ty * TH; x0 = tx * 16;
      p0 = ((long long)b * a.H + y0) * a.W + x0;
      // y0 >= 1, y0 + TH + 1 <= H, x0 >= 1, x0 + 17 <= W (then the dY tile is whole too)
      inner = (int)(((unsigned)(-y0) & (unsigned)(y0 + TH - a.H) & (unsigned)(-x0) & (unsigned)(x0 + 16 - a.W)) >> 31);
    } else {
      p0 = (long long)pb * PB;
      inner = (int)((unsigned long long)(p0 + PB - a.total_px - 1) >> 63);
    }
    const float* dorg = a.dy + p0 * a.dy_pitch + a.dy_coff;
    const float* xorg = a.x + ((TAPS == 9) ? p0 - a.W - 1 : p0) * a.x_pitch + a.x_coff;   // dereferenced only where valid
#pragma unroll
    for (int it = 0; it < D_IT; ++it) {
      const float* src = dorg + d_off[it];
      if (!inner) {
        asm volatile("" ::: "memory");                     // keep the border path a real scalar branch
        const int key = d_key[it];
        bool ok = key >= 0;
        if (TAPS == 9) ok = ok && y0 + (key >> 16) < a.H && x0 + (key & 0xffff) < a.W;
        else ok = ok && p0 + (key & 0xffff) < a.total_px;
        src = ok ? src : sqd_wg_zero_page;
      }
      __builtin_amdgcn_global_load_lds(src, (wg_lds_ptr_t)(dyB + (buf * DSLOTS + it * 256 + wave_s * 64) * 4), 16, 0, 0);
    }
#pragma unroll
    for (int it = 0; it < X_IT; ++it) {
      const float* src = xorg + x_off[it];
      if (!inner) {
        asm volatile("" ::: "memory");
        const int key = x_key[it];
        bool ok = key >= 0;
        if (TAPS == 9) ok = ok && (unsigned)(y0 + (key >> 16) - 1) < (unsigned)a.H && (unsigned)(x0 + (key & 0xffff) - 1) < (unsigned)a.W;
        else ok = ok && p0 + (key & 0xffff) < a.total_px;
        src = ok ? src : sqd_wg_zero_page;
      }
      __builtin_amdgcn_global_load_lds(src, (wg_lds_ptr_t)(xB + (buf * XSLOTS + it * 256 + wave_s * 64) * 4), 16, 0, 0);
    }
  };

  if (DG) {
    // w[n][c0 + c] -> wtT[c][n] (zero beyond N / C: padded dy slots hold finite garbage, times 0); published by the first
    // block barrier below
    for (int idx = threadIdx.x; idx < TC * 16 * TN * 16; idx += 256) {
      const int n = idx / (TC * 16), c = idx - n * (TC * 16);
      wtT[c * WP + n] = (n < a.N && c0 + c < a.C) ? a.w[(long long)n * a.C + c0 + c] : 0.f;
    }
  }
  f32x4 acc[NACC], bacc[BACC];
  // Per-lane LDS float offsets, computed ONCE: in every k-step the pixel index is (compile-time part) + kq
  // (+ the tap shift), and because row strides / tap shifts (18*dy + dx) / 4*cq are even except dx, the
  // swizzle parity is (kq + dx) & 1 -- constant per lane and tile.  The unrolled loop then addresses LDS as
  // lane_offset + immediate with no VALU arithmetic per MFMA.
  const int swA = SWN ? ((kq & 1) << 4) : 0;
  int al[NACC], bl[NACC], abias[BACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int nt, ct, tap;
    if (SHARED) {
      const int u = i / (TC * TAPS), rem = i - u * (TC * TAPS);
      nt = wave + 4 * u; tap = rem / TC; ct = rem - tap * TC;
    } else {
      int t = wave + 4 * i;
      if (t >= TILES) t = TILES - 1;                           // harmless duplicate, never stored
      ct = t % TC; tap = (t / TC) % TAPS; nt = t / (TC * TAPS);
    }
    const int dy = (TAPS == 9) ? tap / 3 : 0, dx = (TAPS == 9) ? tap % 3 : 0;
    const int swB = SWC ? (((kq + dx) & 1) << 4) : 0;
    al[i] = kq * (RN * 4) + ((nt * 16 + lr) ^ swA);
    bl[i] = (kq + dy * 18 + dx) * (RC * 4) + ((ct * 16 + lr) ^ swB);
  }
#pragma unroll
  for (int i = 0; i < BACC; ++i) {
    bacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int bt = (wave + 4 * i < TN) ? wave + 4 * i : 0;
    abias[i] = kq * (RN * 4) + ((bt * 16 + lr) ^ swA);
  }
  // SHARED path: the distinct lane-dependent parts only -- out-channel tile u of this wave, and per in-channel tile the two
  // swizzle parities a tap's column shift can produce; everything else of an operand address is a compile-time immediate
  int aS[NU], bS[2][TC];
#pragma unroll
  for (int u = 0; u < NU; ++u) aS[u] = kq * (RN * 4) + (((wave + 4 * u) * 16 + lr) ^ swA);
#pragma unroll
  for (int par = 0; par < 2; ++par)
#pragma unroll
    for (int ct = 0; ct < TC; ++ct) bS[par][ct] = kq * (RC * 4) + ((ct * 16 + lr) ^ (SWC ? (((kq + par) & 1) << 4) : 0));

  // DG: the data-gradient stores go through a buffer resource and are ALWAYS issued (a lane without a pixel / channel carries an
  // out-of-range offset: the hardware drops it), DG_ST per wave and block, so the block barrier can wait with a COUNTED vmcnt that
  // covers the older LDS-DMA of this block but leaves the previous block's stores in flight; a vmcnt(0) there exposed the write
  // latency of every block.  This relies on (i) vmcnt counting loads, stores and LDS-DMA TOGETHER and retiring them in issue order on
  // gfx9-family parts (MI355X_MICROARCH.md, "s_waitcnt vmcnt(N)": "Loads, stores, atomics and LDS-DMA count together, in issue
  // order (flat_* excepted)" -- no flat instruction is used here; the same model LLVM's SIInsertWaitcnts uses for gfx9), and (ii) the
  // compiler placing no vector-memory instruction of its own -- a scratch reload -- between the stores and the wait:
  // tests/test_build_spills.py asserts zero spills / zero scratch for every DG instantiation.  SQD_SQBWD_VMCNT0=1 switches the
  // wait to vmcnt(0) for A/B parity runs (tests/test_training_gpu.py).
  constexpr int DG_ST = DG ? ((TH * TC + 3) / 4) : 0;
  typedef unsigned int wg_u32x4_t __attribute__((ext_vector_type(4)));
  __amdgpu_buffer_rsrc_t dxres;
  if (DG) dxres = __builtin_amdgcn_make_buffer_rsrc((void*)(a.dx + a.dx_coff + c0), 0, 0x7ffffff0, 0x00020000);
  // block-invariant per-lane byte offsets of the data-gradient phase: dy row pieces (per 16-channel block j), transposed-weight row
  // piece, x mask piece, store offset (out of range when the channel does not exist), pixel inside the block, tile exists
  constexpr int DGN = DG ? DG_ST : 1;
  int dg_d[DGN][DG ? TN : 1], dg_w[DGN], dg_m[DGN], dg_v[DGN], dg_px[DGN];
  bool dg_live[DGN];
  if constexpr (DG) {
#pragma unroll
    for (int it = 0; it < DG_ST; ++it) {
      const int t = wave_s + 4 * it;
      dg_live[it] = t < (PB / 16) * TC;
      const int tt = dg_live[it] ? t : 0;
      const int pt = tt / TC, ct = tt - pt * TC;
      const int px = pt * 16 + lr;
      const int swd = SWN ? ((px & 1) << 2) : 0, swx = SWC ? ((px & 1) << 2) : 0;
#pragma unroll
      for (int j = 0; j < TN; ++j) dg_d[it][j] = (px * RN + ((4 * j + kq) ^ swd)) * 16;
      dg_w[it] = ((ct * 16 + lr) * WP + 4 * kq) * 4;
      dg_m[it] = (px * RC + ((4 * ct + kq) ^ swx)) * 16;
      const int c = ct * 16 + 4 * kq;
      dg_px[it] = dg_live[it] ? px : PB;                        // (a tile that does not exist never stores)
      dg_v[it] = (c0 + c < a.C) ? (px * a.dx_pitch + c) * 4 : (int)0x80000000;
    }
  }
  int pb = split, buf = 0;
  bool first_block = true;
  if (pb < a.nblocks) dma_block(pb, 0);
  for (; pb < a.nblocks; pb += nsplit) {
    if (DG) {
      if (first_block) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" :: "n"(DG_ST) : "memory");
      first_block = false;
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // explicit: every wave's share of the block's LDS-DMA has landed ...
      __syncthreads();                   // ... before the barrier publishes it; previous compute finished
    }
    const int nxt = pb + nsplit;
    if (nxt < a.nblocks) dma_block(nxt, buf ^ 1);
    const float* dyT = dyB + buf * DSLOTS * 4;
    const float* xT = xB + buf * XSLOTS * 4;
    if (SHARED) {
      // k-step loop, branch-free and software-pipelined over two operand sets: the reads of step s+1 are issued in the
      // middle of step s's MFMAs (the compiler's wait in front of step s+1 is then free), LDS addresses are per-lane
      // bases + compile-time immediates (tap shifts folded into the immediate), the bias tile always rides along
      // (one extra MFMA per step; stored only by the workgroups that own it) so no branch splits the schedule.
      constexpr int NB = TC * TAPS, STEPS = TH * 4, HALF = (NB + 1) / 2;
      auto load_step = [&](int st, float (&av)[NU], float (&bv)[NB], float (&ab)[BACC]) {
        const int r = st >> 2, cq = st & 3;
        const int immA = (r * 16 + cq * 4) * (RN * 4);
        const int immB = ((TAPS == 9) ? (r * 18 + cq * 4) : (r * 16 + cq * 4)) * (RC * 4);
#pragma unroll
        for (int u = 0; u < NU; ++u) av[u] = dyT[aS[u] + immA];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const int tap = j / TC, ct = j - tap * TC;
          const int dy = (TAPS == 9) ? tap / 3 : 0, dx = (TAPS == 9) ? tap % 3 : 0;
          bv[j] = xT[bS[dx & 1][ct] + immB + (dy * 18 + dx) * (RC * 4)];
        }
#pragma unroll
        for (int i = 0; i < BACC; ++i) ab[i] = dyT[abias[i] + immA];
      };
      auto mfma_part = [&](const float (&av)[NU], const float (&bv)[NB], const float (&ab)[BACC], int part) {
#pragma unroll
        for (int j = part * HALF; j < (part ? NB : HALF); ++j)
#pragma unroll
          for (int u = 0; u < NU; ++u) acc[u * NB + j] = mfma16(av[u], bv[j], acc[u * NB + j]);
        if (part) {
#pragma unroll
          for (int i = 0; i < BACC; ++i) bacc[i] = mfma16(ab[i], 1.0f, bacc[i]);
        }
      };
      float av0[NU], bv0[NB], ab0[BACC], av1[NU], bv1[NB], ab1[BACC];
      load_step(0, av0, bv0, ab0);
#pragma unroll
      for (int st = 0; st < STEPS; ++st) {
        if (st & 1) {
          mfma_part(av1, bv1, ab1, 0);
          __builtin_amdgcn_sched_barrier(0);
          if (st + 1 < STEPS) load_step(st + 1, av0, bv0, ab0);
          __builtin_amdgcn_sched_barrier(0);
          mfma_part(av1, bv1, ab1, 1);
        } else {
          mfma_part(av0, bv0, ab0, 0);
          __builtin_amdgcn_sched_barrier(0);
          if (st + 1 < STEPS) load_step(st + 1, av1, bv1, ab1);
          __builtin_amdgcn_sched_barrier(0);
          mfma_part(av0, bv0, ab0, 1);
        }
      }
    } else {
#pragma unroll
      for (int s = 0; s < TH * 4; ++s) {
        const int r = s >> 2, cq = s & 3;
        const int immA = (r * 16 + cq * 4) * (RN * 4);           // compile-time after unrolling
        const int immB = ((TAPS == 9) ? (r * 18 + cq * 4) : (r * 16 + cq * 4)) * (RC * 4);
#pragma unroll
        for (int i = 0; i < NACC; ++i) acc[i] = mfma16(dyT[al[i] + immA], xT[bl[i] + immB], acc[i]);
#pragma unroll
        for (int i = 0; i < BACC; ++i) bacc[i] = mfma16(dyT[abias[i] + immA], 1.0f, bacc[i]);   // always (stored by cg == 0 only)
      }
    }
    if constexpr (DG) {
      // ---- data gradient of this pixel block for this workgroup's in-channels ----
      // every per-lane LDS / store offset is block-invariant (dg_*, computed once before the loop); the input buffer is a
      // compile-time offset inside each of the two copies of the phase, so the phase is reads at base + immediate, MFMAs, the
      // mask selects and one store per tile
      const long long p0 = (long long)pb * PB;
      const unsigned soff = (unsigned)(p0 * a.dx_pitch * 4);    // (tensor < 4 GiB: checked by the launcher)
      const int px_left = (int)((a.total_px - p0 < (long long)PB) ? (a.total_px - p0) : (long long)PB);   // valid pixels of this block
      auto dgrad_phase = [&](auto bufc) {
        constexpr int BUF = decltype(bufc)::value;
#pragma unroll
        for (int it = 0; it < DG_ST; ++it) {
          f32x4 o = (f32x4){0.f, 0.f, 0.f, 0.f};
          if (dg_live[it]) {                                    // (wave-uniform)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
              const f32x4 bq = *(const f32x4*)((const char*)dyB + dg_d[it][j] + BUF * DSLOTS * 16);    // dy[px][16 j + 4 kq .. + 3]
              const f32x4 aq = *(const f32x4*)((const char*)wtT + dg_w[it] + j * 64);                  // w[16 j + 4 kq .. + 3][c]
              o = mfma16(aq.x, bq.x, o); o = mfma16(aq.y, bq.y, o); o = mfma16(aq.z, bq.z, o); o = mfma16(aq.w, bq.w, o);
            }
            if (a.dx_mask) {
              const f32x4 m = *(const f32x4*)((const char*)xB + dg_m[it] + BUF * XSLOTS * 16);
              o.x = m.x > 0.f ? o.x : 0.f; o.y = m.y > 0.f ? o.y : 0.f; o.z = m.z > 0.f ? o.z : 0.f; o.w = m.w > 0.f ? o.w : 0.f;
            }
          }
          const int voff = (dg_px[it] < px_left) ? dg_v[it] : (int)0x80000000;      // out of range: the store is dropped
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(wg_u32x4_t, o), dxres, voff, (int)soff, 0);
          __builtin_amdgcn_sched_barrier(0);
          asm volatile("s_nop 1" ::: "memory");                 // (MUBUF store with an SGPR soffset: write-after-read hazard, see conv_wino.hip)
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      if (buf) dgrad_phase(std::integral_constant<int, 1>{}); else dgrad_phase(std::integral_constant<int, 0>{});
    }
    buf ^= 1;
  }

  // one slab per split; layout [n][tap][c] then [N] bias sums
  float* slab = a.slab + (long long)split * a.slab_stride;
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    int nt, ct, tap;
    if (SHARED) {
      const int u = i / (TC * TAPS), rem = i - u * (TC * TAPS);
      nt = wave + 4 * u; tap = rem / TC; ct = rem - tap * TC;
    } else {
      const int t = wave + 4 * i;
      if (t >= TILES) continue;
      ct = t % TC; tap = (t / TC) % TAPS; nt = t / (TC * TAPS);
    }
    const int c = c0 + ct * 16 + lr;
    if (c >= a.C) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + nt * 16 + 4 * kq + r;
      if (n < a.N) slab[((long long)n * TAPS + tap) * a.C + c] = acc[i][r];
    }
  }
  if (do_bias && lr == 0) {
#pragma unroll
    for (int i = 0; i < BACC; ++i) {
      const int bt = wave + 4 * i;
      if (bt >= TN) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + bt * 16 + 4 * kq + r;
        if (n < a.N) slab[(long long)a.N * TAPS * a.C + n] = bacc[i][r];
      }
    }
  }
}

template <int TAPS, int TN, int TC, int TH, bool DG = false>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradArgs a) {
  wg_body<TAPS, TN, TC, TH, DG>(a, (int)blockIdx.x, (int)gridDim.x, (int)blockIdx.y);
}

// Several 1x1 layers of one pixel grid (the expand1x1 layers of a backward stage that are too wide for the fused squeeze backward) in
// ONE launch, every layer cut into the same S splits: as wino_wgrad_group_kernel (wino_wgrad.hip) -- a layer alone needs 42-170 splits to
// fill the chip and then walks only 7-28 pixel blocks per workgroup.  Records by value in the kernel arguments; a layer's workgroups
// are a contiguous run, split-major inside it.
#define WG_MAX_GROUP 6
struct WgGroupArgs { WgradArgs l[WG_MAX_GROUP]; int wg0[WG_MAX_GROUP + 1]; int S, n; };

template <int TN, int TC, int TH>
__global__ __launch_bounds__(256) void conv_wgrad_group_kernel(WgGroupArgs ga) {
  const int pos = (int)blockIdx.x;
  int i = 0;
#pragma unroll
  for (int k = 1; k < WG_MAX_GROUP; ++k) i = (k < ga.n && pos >= ga.wg0[k]) ? k : i;
  i = __builtin_amdgcn_readfirstlane(i);
  const WgradArgs a = ga.l[i];
  const int local = pos - ga.wg0[i];
  wg_body<1, TN, TC, TH, false>(a, local % ga.S, ga.S, local / ga.S);
}

// dw (OIHW: [N][C][TAPS]) and db ([N]) = fixed-order sum of S slabs.  A block reduces 32 consecutive
// outputs; its 8 thread groups each sum the slabs k = g, g+8, ... in ascending order, then the 8 partials
// are combined in a fixed order through LDS -- parallel over slabs yet bitwise reproducible.
#define WGR_OUT 64          /* outputs per workgroup: 256 contiguous bytes of every slab row */
#define WGR_PARTS 4        /* slab partitions summed in parallel, combined in a fixed order */
__global__ __launch_bounds__(WGR_OUT * WGR_PARTS) void wgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dw,
                                                                           float* __restrict__ db, int S, long long slab_stride,
                                                                           int N, int C, int TAPS) {
  __shared__ float red[WGR_PARTS][WGR_OUT];
  const long long nw = (long long)N * TAPS * C;
  const int o = threadIdx.x & (WGR_OUT - 1), part = threadIdx.x / WGR_OUT;
  const long long idx = (long long)blockIdx.x * WGR_OUT + o;
  const bool live = idx < nw + N;
  float s = 0.f;
  if (live) {
#pragma unroll 8
    for (int k = part; k < S; k += WGR_PARTS) s += slab[(long long)k * slab_stride + idx];
  }
  red[part][o] = s;
  __syncthreads();
  if (part != 0 || !live) return;
  float t = red[0][o];
#pragma unroll
  for (int p = 1; p < WGR_PARTS; ++p) t += red[p][o];
  if (idx < nw) {
    const int c = (int)(idx % C); const long long q = idx / C;
    const int tap = (int)(q % TAPS); const int n = (int)(q / TAPS);
    dw[((long long)n * C + c) * TAPS + tap] = t;
  } else if (db) {
    db[idx - nw] = t;
  }
}

template <int TAPS, int TN, int TC, int TH, bool DG = false>
static int launch_wgrad(WgradArgs a, int S, hipStream_t stream) {
  constexpr int PB = TH * 16;
  constexpr int XPIX = (TAPS == 9) ? (TH + 2) * 18 : PB;
  constexpr int DSLOTS = (PB * TN * 4 + 255) & ~255, XSLOTS = (XPIX * TC * 4 + 255) & ~255;
  constexpr int WP = ((TN * 16 + 63) / 64) * 64 + 8;
  constexpr size_t lds = (size_t)(2 * DSLOTS + 2 * XSLOTS) * 16 + (DG ? (size_t)TC * 16 * WP * 4 : 0);
  static_assert(lds <= 160 * 1024, "wgrad LDS budget");
  auto kern = conv_wgrad_kernel<TAPS, TN, TC, TH, DG>;
  static SqdDevOnce lds_once;
  if (lds > 64 * 1024 && sqd_max_lds_once(lds_once, (const void*)kern, (int)lds) != SQD_OK) return SQD_ERR_LAUNCH;
  if (TAPS == 9) {
    a.tiles_x = sqd_cdiv(a.W, 16); a.tiles_y = sqd_cdiv(a.H, TH);
    a.nblocks = a.B * a.tiles_x * a.tiles_y;
  } else {
    a.tiles_x = a.tiles_y = 0;
    a.nblocks = (int)((a.total_px + PB - 1) / PB);
  }
  a.n_groups = sqd_cdiv(a.N, TN * 16);
  const int c_groups = sqd_cdiv(a.C, TC * 16);
  hipLaunchKernelGGL(kern, dim3((unsigned)S, (unsigned)(a.n_groups * c_groups)), dim3(256), lds, stream, a);
  return sqd_launch_status();
}

// Single-layer slab reduction for the other translation units of the library (wino_wgrad.hip, stem_wgrad.hip)
extern "C" int sqd_wgrad_reduce_launch(const float* slab, float* dw, float* db, int S, long long slab_stride, int N, int C, int taps,
                                       void* stream) {
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((slab_stride + WGR_OUT - 1) / WGR_OUT)), dim3(WGR_OUT * WGR_PARTS), 0,
                     (hipStream_t)stream, slab, dw, db, S, slab_stride, N, C, taps);
  return sqd_launch_status();
}

// ---------------------------------------------------------------------------------------------
// The tile form of a launch -- out-channel tiles tn, in-channel tiles tc (of 16), th * 16 pixels per block -- decided HERE and nowhere
// else: the three entry points dispatch on it and the host sizes its slab workspaces and split counts from it (sqd_wgrad_tile_form).
// kind: 0 = sqd_conv_wgrad, 1 = sqd_conv_wgrad_group (1x1, 64-out-channel forms only), 2 = sqd_squeeze_bwd (1x1, all N <= 128 in one
// group).
// ---------------------------------------------------------------------------------------------
enum { WG_PLAIN = 0, WG_GROUP = 1, WG_FUSED = 2 };
struct WgForm { int tn, tc, th; };
// 1x1: pixels per block sized so the double-buffered LDS image stays <= 40 KB: 4-5 workgroups per CU instead of one
// (the late 24x78 layers have only ~300 blocks of 128 pixels: with one resident workgroup per CU nothing overlapped)
static constexpr int wg1_th(int tn, int tc) { return tn + tc >= 6 ? 2 : (tn + tc >= 3 ? 4 : 8); }
static constexpr int wg9_th(int tn, int tc) { return (tn == 4 && tc == 2) ? SQD_WG9_TH : 4; }

static int wgrad_form(int kind, int taps, int N, int C, WgForm& f) {
  SQD_CHECK_ARG(kind >= WG_PLAIN && kind <= WG_FUSED && (taps == 1 || taps == 9) && N > 0 && C > 0);
  if (kind != WG_PLAIN && taps != 1) return SQD_ERR_UNSUPPORTED;
  if (kind == WG_FUSED) {
    if (N > 128) return SQD_ERR_UNSUPPORTED;
    f = {N > 96 ? 8 : (N > 64 ? 6 : sqd_cdiv(N, 16)), C >= 64 ? 4 : sqd_cdiv(C, 16), 2};
    return SQD_OK;
  }
  if (kind == WG_GROUP && (N < 64 || (N > 64 && N <= 96))) return SQD_ERR_UNSUPPORTED;     // (those layers run other forms: their own launch)
  f.tn = N >= 64 ? 4 : sqd_cdiv(N, 16);
  if (taps == 9) {
    if (N > 64 && N <= 80) { f.tn = 5; f.tc = 1; }          // ConvDet (N = 72)
    else if (f.tn == 4) f.tc = (C % 32 == 0) ? 2 : 1;
    else f.tc = (f.tn == 3) ? 1 : 2;
    f.th = wg9_th(f.tn, f.tc);
  } else {
    // Round 3: wider output tiles where the layer is wide enough.  A workgroup that owns TC = 8 in-channel tiles (128 channels)
    // re-reads dY half as often as with 4, and N = 96 (the squeeze of fire13 / fire14) runs as ONE 6-tile group instead of 64 + a
    // half-empty 64 (X streamed once instead of twice, no padded MFMAs): the 24x78 1x1 weight gradients were bound by L2 -> LDS
    // bytes per MFMA, not by HBM or the matrix pipe.
    if (N > 64 && N <= 96) f.tn = 6;
    f.tc = C >= 256 ? 8 : (C >= 64 ? 4 : sqd_cdiv(C, 16));            // (C = 128 at 96x312 measured slower with the wide tile: 60.7 -> 74.2 us)
    f.th = wg1_th(f.tn, f.tc);
  }
  return SQD_OK;
}

// The host's view of the rule: launches nothing, touches no device.  px_per_block = th * 16 (3x3: a th x 16 window).
extern "C" int sqd_wgrad_tile_form(int kind, int taps, int N, int C, int* tn, int* tc, int* px_per_block) {
  WgForm f;
  if (int rc = wgrad_form(kind, taps, N, C, f)) return rc;
  if (tn) *tn = f.tn;
  if (tc) *tc = f.tc;
  if (px_per_block) *px_per_block = f.th * 16;
  return SQD_OK;
}

// What the three entries check and fill for one layer (the fused entry adds w / dx).
static int wgrad_args(WgradArgs& a, const float* dy, const float* x, float* slab, int B, int H, int W, int N, int dy_pitch, int dy_coff,
                      int C, int x_pitch, int x_coff, int taps) {
  SQD_CHECK_ARG(dy && x && slab && B > 0 && H > 0 && W > 0 && N > 0 && C > 0);
  SQD_CHECK_ARG((N & 3) == 0 && (C & 3) == 0 && (dy_pitch & 3) == 0 && (dy_coff & 3) == 0 && (x_pitch & 3) == 0 && (x_coff & 3) == 0);
  SQD_CHECK_ARG(dy_coff + N <= dy_pitch && x_coff + C <= x_pitch);
  SQD_CHECK_ARG(((uintptr_t)dy & 15) == 0 && ((uintptr_t)x & 15) == 0);
  SQD_CHECK_ARG(taps == 1 || taps == 9);
  a.dy = dy; a.x = x; a.slab = slab; a.B = B; a.H = H; a.W = W;
  a.N = N; a.dy_pitch = dy_pitch; a.dy_coff = dy_coff; a.C = C; a.x_pitch = x_pitch; a.x_coff = x_coff;
  a.total_px = (long long)B * H * W;
  a.slab_stride = (long long)N * taps * C + N;
  a.w = nullptr; a.dx = nullptr; a.dx_pitch = a.dx_coff = a.dx_mask = 0;
  return SQD_OK;
}

// dy: [B][H][W][dy_pitch] window [dy_coff, dy_coff+N) (ReLU mask already applied); x: input window
// [x_coff, x_coff+C); slab: workspace of S * (N*taps*C + N) floats; dw: [N][C][k][k]; db: [N] or NULL.
extern "C" int sqd_conv_wgrad(const float* dy, const float* x, float* slab, float* dw, float* db, int B, int H, int W,
                              int N, int dy_pitch, int dy_coff, int C, int x_pitch, int x_coff, int taps, int S,
                              void* stream) {
  SQD_CHECK_ARG(S > 0 && S <= 65535);
  WgradArgs a; WgForm f;
  if (int rc = wgrad_args(a, dy, x, slab, B, H, W, N, dy_pitch, dy_coff, C, x_pitch, x_coff, taps)) return rc;
  if (int rc = wgrad_form(WG_PLAIN, taps, N, C, f)) return rc;
  hipStream_t s = (hipStream_t)stream;
  int rc = SQD_ERR_UNSUPPORTED;
#define SQD_WG_CASE(TAPSv, TNv, TCv) \
  if (taps == TAPSv && f.tn == TNv && f.tc == TCv) rc = launch_wgrad<TAPSv, TNv, TCv, (TAPSv == 9 ? wg9_th(TNv, TCv) : wg1_th(TNv, TCv))>(a, S, s);
  SQD_WG_CASE(9, 5, 1) SQD_WG_CASE(9, 4, 2) SQD_WG_CASE(9, 4, 1) SQD_WG_CASE(9, 1, 2) SQD_WG_CASE(9, 2, 2) SQD_WG_CASE(9, 3, 1)
  SQD_WG_CASE(1, 1, 1) SQD_WG_CASE(1, 1, 2) SQD_WG_CASE(1, 1, 3) SQD_WG_CASE(1, 1, 4) SQD_WG_CASE(1, 1, 8)
  SQD_WG_CASE(1, 2, 1) SQD_WG_CASE(1, 2, 2) SQD_WG_CASE(1, 2, 3) SQD_WG_CASE(1, 2, 4) SQD_WG_CASE(1, 2, 8)
  SQD_WG_CASE(1, 3, 1) SQD_WG_CASE(1, 3, 2) SQD_WG_CASE(1, 3, 3) SQD_WG_CASE(1, 3, 4) SQD_WG_CASE(1, 3, 8)
  SQD_WG_CASE(1, 4, 1) SQD_WG_CASE(1, 4, 2) SQD_WG_CASE(1, 4, 3) SQD_WG_CASE(1, 4, 4) SQD_WG_CASE(1, 4, 8)
  SQD_WG_CASE(1, 6, 1) SQD_WG_CASE(1, 6, 2) SQD_WG_CASE(1, 6, 3) SQD_WG_CASE(1, 6, 4) SQD_WG_CASE(1, 6, 8)
#undef SQD_WG_CASE
  if (rc != SQD_OK) return rc;
  if (!dw) return sqd_launch_status();       // partial slabs only: the caller reduces many layers at once (sqd_wgrad_reduce_batched)
  return sqd_wgrad_reduce_launch(slab, dw, db, S, a.slab_stride, N, C, taps, stream);
}

template <int TN, int TC, int TH>
static int launch_wgrad_group(WgGroupArgs& ga, hipStream_t stream) {
  constexpr int PB = TH * 16;
  constexpr int DSLOTS = (PB * TN * 4 + 255) & ~255, XSLOTS = (PB * TC * 4 + 255) & ~255;
  constexpr size_t lds = (size_t)(2 * DSLOTS + 2 * XSLOTS) * 16;
  static_assert(lds <= 160 * 1024, "wgrad LDS budget");
  auto kern = conv_wgrad_group_kernel<TN, TC, TH>;
  static SqdDevOnce once;
  if (lds > 64 * 1024 && sqd_max_lds_once(once, (const void*)kern, (int)lds) != SQD_OK) return SQD_ERR_LAUNCH;
  int wg = 0;
  for (int i = 0; i < ga.n; ++i) {
    WgradArgs& a = ga.l[i];
    a.tiles_x = a.tiles_y = 0;
    a.nblocks = (int)((a.total_px + PB - 1) / PB);
    if (ga.S > a.nblocks) return SQD_ERR_UNSUPPORTED;
    a.n_groups = sqd_cdiv(a.N, TN * 16);
    ga.wg0[i] = wg;
    wg += ga.S * a.n_groups * sqd_cdiv(a.C, TC * 16);
  }
  for (int i = ga.n; i <= WG_MAX_GROUP; ++i) ga.wg0[i] = wg;
  hipLaunchKernelGGL(kern, dim3((unsigned)wg), dim3(256), lds, stream, ga);
  return sqd_launch_status();
}

// The weight-gradient slabs of up to WG_MAX_GROUP 1x1 layers that share B, H, W in ONE launch, every layer cut into the same S splits
// (see conv_wgrad_group_kernel).  ``layers``: n records of 9 64-bit words {dy, x, slab, N, dy_pitch, dy_coff, C, x_pitch, x_coff} (host
// memory).  All layers must select the same tile form as sqd_conv_wgrad would (N >= 64 and not in (64, 96]: 64 out-channels; in-channel
// tile 16 * ceil(C / 16) up to 64, 128 from C = 256); SQD_ERR_UNSUPPORTED otherwise.  Slabs only.
extern "C" int sqd_conv_wgrad_group(const long long* layers, int n, int B, int H, int W, int S, void* stream) {
  SQD_CHECK_ARG(layers && n >= 1 && n <= WG_MAX_GROUP && B > 0 && H > 0 && W > 0 && S > 0 && S <= 65535);
  WgGroupArgs ga;
  ga.n = n; ga.S = S;
  WgForm f0 = {0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const long long* r = layers + 9 * i;
    WgForm f;
    if (int rc = wgrad_args(ga.l[i], (const float*)(uintptr_t)r[0], (const float*)(uintptr_t)r[1], (float*)(uintptr_t)r[2], B, H, W, (int)r[3],
                            (int)r[4], (int)r[5], (int)r[6], (int)r[7], (int)r[8], 1)) return rc;
    if (int rc = wgrad_form(WG_GROUP, 1, ga.l[i].N, ga.l[i].C, f)) return rc;
    if (i == 0) f0 = f;
    if (f.tc != f0.tc) return SQD_ERR_UNSUPPORTED;
  }
  for (int i = n; i < WG_MAX_GROUP; ++i) ga.l[i] = ga.l[0];
  hipStream_t s = (hipStream_t)stream;
#define SQD_WGG_CASE(TCv) case TCv: return launch_wgrad_group<4, TCv, wg1_th(4, TCv)>(ga, s);
  switch (f0.tc) { SQD_WGG_CASE(1) SQD_WGG_CASE(2) SQD_WGG_CASE(3) SQD_WGG_CASE(4) SQD_WGG_CASE(8) }
#undef SQD_WGG_CASE
  return SQD_ERR_UNSUPPORTED;
}

// A Fire squeeze's backward in ONE launch (reference: autograd of Fire.squeeze + squeeze_activation, src/model/squeezedet.py:12,19,
// as triggered by loss.backward(), src/engine/trainer.py:47): the weight / bias gradient slabs exactly as sqd_conv_wgrad writes
// them (taps = 1, dw == NULL convention: the caller reduces the slabs) AND the data gradient
//   dx[p][dx_coff + c] = (x[p][x_coff + c] > 0 or !relu_mask) ? sum_n dy[p][dy_coff + n] * w[n][c] : 0
// for every pixel.  w: the layer's weight itself, OIHW [N][C][1][1] (no packed copy).  N <= 128 (one out-channel group).  The same
// launch serves a Fire's expand1x1 where its width allows (dy = the e1 window of the Fire's output gradient, x = the squeeze
// output, relu_mask = 0: the expand3x3 data gradient that accumulates onto dx applies the mask).
// S as in sqd_conv_wgrad; the slab split uses 64-channel in-tiles (host: tiles.wgrad_split(..., fused_dgrad=True)).
extern "C" int sqd_squeeze_bwd(const float* dy, const float* x, const float* w_oihw, float* slab, float* dx, int B, int H, int W,
                               int N, int dy_pitch, int dy_coff, int C, int x_pitch, int x_coff, int dx_pitch, int dx_coff,
                               int relu_mask, int S, void* stream) {
  SQD_CHECK_ARG(w_oihw && dx && S > 0 && S <= 65535);
  WgradArgs a; WgForm f;
  if (int rc = wgrad_args(a, dy, x, slab, B, H, W, N, dy_pitch, dy_coff, C, x_pitch, x_coff, 1)) return rc;
  SQD_CHECK_ARG((dx_pitch & 3) == 0 && (dx_coff & 3) == 0 && dx_coff >= 0 && dx_coff + C <= dx_pitch);
  SQD_CHECK_ARG(((uintptr_t)dx & 15) == 0);
  SQD_CHECK_ARG((long long)B * H * W * dx_pitch * 4 < (1ll << 32) - (1ll << 24));       // 32-bit SGPR byte offset of a pixel block
  SQD_CHECK_ARG((long long)32 * dx_pitch * 4 < (1ll << 30));                             // per-lane byte offsets inside a block
  if (int rc = wgrad_form(WG_FUSED, 1, N, C, f)) return rc;
  a.w = w_oihw; a.dx = dx; a.dx_pitch = dx_pitch; a.dx_coff = dx_coff; a.dx_mask = relu_mask;
  hipStream_t s = (hipStream_t)stream;
  int rc = SQD_ERR_UNSUPPORTED;
#define SQD_SB_CASE(TNv, TCv) if (f.tn == TNv && f.tc == TCv) rc = launch_wgrad<1, TNv, TCv, 2, true>(a, S, s);
  SQD_SB_CASE(1, 1) SQD_SB_CASE(1, 2) SQD_SB_CASE(1, 3) SQD_SB_CASE(1, 4)
  SQD_SB_CASE(2, 1) SQD_SB_CASE(2, 2) SQD_SB_CASE(2, 3) SQD_SB_CASE(2, 4)
  SQD_SB_CASE(3, 1) SQD_SB_CASE(3, 2) SQD_SB_CASE(3, 3) SQD_SB_CASE(3, 4)
  SQD_SB_CASE(4, 1) SQD_SB_CASE(4, 2) SQD_SB_CASE(4, 3) SQD_SB_CASE(4, 4)
  SQD_SB_CASE(6, 1) SQD_SB_CASE(6, 2) SQD_SB_CASE(6, 3) SQD_SB_CASE(6, 4)
  SQD_SB_CASE(8, 1) SQD_SB_CASE(8, 2) SQD_SB_CASE(8, 3) SQD_SB_CASE(8, 4)
#undef SQD_SB_CASE
  return rc;
}

// The slab reduction of MANY layers in one launch (a training step has 32 of them, 8 us each when launched one by one).
// descs: device array of n records of 9 int64 {slab offset, dw offset, db offset (floats; db < 0: none), S, slab stride,
// N, C, TAPS, first workgroup}; slabs live in one workspace (slab_base), gradients in one flat buffer (grad_base), so the
// table is the same every step.  Same arithmetic and order as wgrad_reduce_kernel (bitwise identical results).
struct WgrDesc { long long slab_off, dw_off, db_off, S, slab_stride, N, C, TAPS, block_begin; };

// One wave per workgroup: 16 lanes x float4 cover the workgroup's 64 outputs, the four lane groups are the four slab partitions, so one
// load instruction fetches 256 contiguous bytes of FOUR slab rows (1 KB per wave instruction; the scalar form moved 256 B).  Partition p
// still sums rows p, p + 4, ... in order and the partitions are combined 0..3: bitwise the sums of wgrad_reduce_kernel.
// (Slab offsets, strides and record sizes are multiples of 4 floats -- N % 4 == 0, C % 4 == 0 -- so a float4 is live or dead as a whole.)
__global__ __launch_bounds__(64) void wgrad_reduce_batched_kernel(const WgrDesc* __restrict__ descs, int n,
                                                                  const float* __restrict__ slab_base,
                                                                  float* __restrict__ grad_base, int block_first, float scale) {
  static_assert(WGR_OUT == 64 && WGR_PARTS == 4, "16 lanes x float4 x 4 partitions = one wave");
  __shared__ f32x4 red[WGR_PARTS][WGR_OUT / 4];
  const long long wg = (long long)blockIdx.x + block_first;      // workgroup id in the numbering of the whole table
  int row = 0;
  while (row + 1 < n && descs[row + 1].block_begin <= wg) ++row;      // uniform (scalar loads)
  const WgrDesc d = descs[row];
  const float* slab = slab_base + d.slab_off;
  const int S = (int)d.S, C = (int)d.C, TAPS = (int)d.TAPS;
  const long long nw = d.N * d.TAPS * d.C;
  const int o4 = threadIdx.x & 15, part = threadIdx.x >> 4;
  const long long idx = (wg - d.block_begin) * WGR_OUT + 4 * o4;
  const bool live = idx < nw + d.N;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (live) {
#pragma unroll 8
    for (int k = part; k < S; k += WGR_PARTS) s += *(const f32x4*)(slab + (long long)k * d.slab_stride + idx);
  }
  red[part][o4] = s;
  __syncthreads();
  if (part != 0 || !live) return;
  f32x4 t = red[0][o4];
#pragma unroll
  for (int p = 1; p < WGR_PARTS; ++p) t += red[p][o4];
  t *= scale;                                  // (1 = bitwise the plain sum; the data-parallel exchange passes this rank's image count)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long e = idx + i;
    if (e < nw) {
      const int c = (int)(e % C); const long long q = e / C;
      const int tap = (int)(q % TAPS); const int nn = (int)(q / TAPS);
      grad_base[d.dw_off + ((long long)nn * C + c) * TAPS + tap] = t[i];
    } else if (d.db_off >= 0) {
      grad_base[d.db_off + (e - nw)] = t[i];
    }
  }
}

extern "C" int sqd_wgrad_reduce_batched(const void* descs_dev, int n, int total_blocks, const float* slab_base, float* grad_base,
                                        float scale, void* stream) {
  SQD_CHECK_ARG(descs_dev && n > 0 && n <= 4096 && total_blocks > 0 && slab_base && grad_base);
  hipLaunchKernelGGL(wgrad_reduce_batched_kernel, dim3((unsigned)total_blocks), dim3(64), 0, (hipStream_t)stream,
                     (const WgrDesc*)descs_dev, n, slab_base, grad_base, 0, scale);
  return sqd_launch_status();
}

// A contiguous range of the table's records only (the training backward reduces each finished stage as soon as its
// slabs are written, so that stage's gradient bucket can enter the all-reduce while earlier layers are still being
// differentiated): descs_dev points at the first record of the range, block_first = that record's first workgroup.
extern "C" int sqd_wgrad_reduce_batched_range(const void* descs_dev, int n, int block_first, int nblocks, const float* slab_base,
                                              float* grad_base, float scale, void* stream) {
  SQD_CHECK_ARG(descs_dev && n > 0 && n <= 4096 && block_first >= 0 && nblocks > 0 && slab_base && grad_base);
  hipLaunchKernelGGL(wgrad_reduce_batched_kernel, dim3((unsigned)nblocks), dim3(64), 0, (hipStream_t)stream,
                     (const WgrDesc*)descs_dev, n, slab_base, grad_base, block_first, scale);
  return sqd_launch_status();
}

// ---------------------------------------------------------------------------------------------
// Weight packer: canonical OIHW parameter -> [ceil(C/kc)][kc/4][taps][Npad][4] (zero padded), forward
// orientation or the data-gradient orientation (in/out channels swapped, taps flipped).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_weight_kernel(const float* __restrict__ w, float* __restrict__ out, int No, int Ci,
                                                          int taps, int kc, int Npad, int nchunks, int dgrad) {
  // forward: N = No (out ch), C = Ci;  dgrad: N = Ci, C = No, tap flipped
  // out[chunk][plane v][tap][n][e]  with channel c = chunk*kc + 4*v + e
  const int N = dgrad ? Ci : No, C = dgrad ? No : Ci;
  const int kv = kc >> 2;
  const long long total = (long long)nchunks * kv * taps * Npad * 4;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int e = (int)(idx & 3); long long t = idx >> 2;
    const int n = (int)(t % Npad); t /= Npad;
    const int tap = (int)(t % taps); t /= taps;
    const int v = (int)(t % kv); const int cc = (int)(t / kv);
    const int c = cc * kc + 4 * v + e;
    float val = 0.f;
    if (n < N && c < C) {
      if (!dgrad) val = w[((long long)n * Ci + c) * taps + tap];
      else val = w[((long long)c * Ci + n) * taps + (taps - 1 - tap)];
    }
    out[idx] = val;
  }
}

// w: OIHW [No][Ci][k][k]; out: packed for a conv with (N,C) = (No,Ci) (dgrad=0) or (Ci,No) (dgrad=1).
extern "C" int sqd_pack_conv_weight(const float* w, float* out, int No, int Ci, int taps, int kc, int Npad, int dgrad,
                                    void* stream) {
  SQD_CHECK_ARG(w && out && No > 0 && Ci > 0 && (taps == 1 || taps == 9) && kc > 0 && Npad > 0);
  const int N = dgrad ? Ci : No, C = dgrad ? No : Ci;
  SQD_CHECK_ARG(Npad >= N);
  const int nchunks = sqd_cdiv(C, kc);
  const long long total = (long long)nchunks * taps * Npad * kc;
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(pack_weight_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, out, No, Ci, taps, kc, Npad,
                     nchunks, dgrad);
  return sqd_launch_status();
}

// Batched re-pack: one launch refreshes every packed copy after an optimizer step.  descs: device array of
// n records of 10 int64 {w ptr, out ptr, No, Ci, taps, kc, Npad, nchunks, dgrad, total elements}.
struct PackDesc { const float* w; float* out; long long No, Ci, taps, kc, Npad, nchunks, dgrad, total; };

__global__ __launch_bounds__(256) void pack_weight_batched_kernel(const PackDesc* __restrict__ descs) {
  const PackDesc d = descs[blockIdx.y];
  const int Ci = (int)d.Ci, taps = (int)d.taps, kc = (int)d.kc, Npad = (int)d.Npad;
  const int N = d.dgrad ? (int)d.Ci : (int)d.No, C = d.dgrad ? (int)d.No : (int)d.Ci;
  const int kv = kc >> 2;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < d.total; idx += (long long)gridDim.x * blockDim.x) {
    const int e = (int)(idx & 3); long long t = idx >> 2;
    const int n = (int)(t % Npad); t /= Npad;
    const int tap = (int)(t % taps); t /= taps;
    const int v = (int)(t % kv); const int cc = (int)(t / kv);
    const int c = cc * kc + 4 * v + e;
    float val = 0.f;
    if (n < N && c < C) {
      if (!d.dgrad) val = d.w[((long long)n * Ci + c) * taps + tap];
      else val = d.w[((long long)c * Ci + n) * taps + (taps - 1 - tap)];
    }
    d.out[idx] = val;
  }
}

extern "C" int sqd_pack_conv_weights_batched(const void* descs_dev, int n, int blocks_per_desc, void* stream) {
  SQD_CHECK_ARG(descs_dev && n > 0 && n <= 65535 && blocks_per_desc > 0 && blocks_per_desc <= 4096);
  hipLaunchKernelGGL(pack_weight_batched_kernel, dim3((unsigned)blocks_per_desc, (unsigned)n), dim3(256), 0, (hipStream_t)stream,
                     (const PackDesc*)descs_dev);
  return sqd_launch_status();
}
