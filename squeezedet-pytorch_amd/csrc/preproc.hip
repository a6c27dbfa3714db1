// GPU-side input pipeline: uint8 HWC RGB images of arbitrary sizes ->
// whiten -> bilinear resize to the network input -> fp32 NCHW, one launch for the whole batch.
//
// Reference (CPU, per image inside DataLoader workers): DataWrapper.__getitem__ src/engine/detector.py:132-142,
// BaseDataset.preprocess src/datasets/base.py:43-59 (eval: drift/flip inactive), whiten src/utils/image.py:9-19
// ((image - mean) / std on float32 HWC), resize :77-88 (cv2.resize(image, (W, H)), default INTER_LINEAR;
// scales = [H/H0, W/W0] float32), transpose(2,0,1) detector.py:140.  KITTI mean/std: src/datasets/kitti.py:17-18.
//
// cv2.resize INTER_LINEAR on float32 data (OpenCV, third party, not under /root/reference -- published algorithm
// restated): for destination x, fx = (x + 0.5) * (W0 / W) - 0.5; sx = floor(fx); fx -= sx; if sx < 0 -> (sx, fx) =
// (0, 0); if sx >= W0 - 1 -> (sx, fx) = (W0 - 1, 0); likewise y; value = (1-fy) * ((1-fx) * s00 + fx * s01) +
// fy * ((1-fx) * s10 + fx * s11), horizontal pass first, all in float32.  Uploading uint8 instead of the
// reference's fp32 cuts host->device bytes 4x (5.75 MB -> ~1.4 MB per KITTI image).
//
// Three geometries (resize, crop_or_pad, letterbox) x three forms (eval, AUG, AUG + COLOR) = nine kernels and nine entry points, from
// two device bodies (preprocess_bilinear_body: resize and letterbox; preprocess_padcrop_body) that share the per-image prologue
// (pre_image), the whitening table (pre_build_table) and the staging (pre_stage), and one host-side check / fill / launch path.
// Mosaic (training only: AUG, AUG + COLOR) adds two kernels and two entry points from a third body, preprocess_mosaic_body, which
// composes up to four source images per output image with the same prologue, table, staging and tap arithmetic.
#include "sqd_common.h"

struct PreArgs {
  const unsigned char* src;      // packed images, image b at src + offsets[b], HWC uint8, 3 channels
  const long long* offsets;      // [B]
  const int* sizes;              // [B][2] = (H0, W0)
  float* out;                    // [B][3][H][W]
  float* scales;                 // [B][2] = (H / H0, W / W0)  (may be null)
  float mean[3], stdv[3];
  int B, H, W;
};

// All kernels: a workgroup produces 256 consecutive pixels of one output row.  The source bytes it needs are one or two CONTIGUOUS
// row segments, so they are fetched once as aligned dwords (coalesced) into LDS and the per-pixel 3-byte gathers read LDS -- a byte
// gather from global memory is one texture-addresser instruction per byte and wave (12 per pixel for the bilinear taps: ~50 us of
// address processing for a 20-image batch, against 25 us of HBM time for its 143 MB).  Whitening is a 256-entry table per channel,
// ((float)v - mean) / std evaluated once per workgroup with the same float32 subtract and IEEE divide the per-pixel form used: bit for bit
// the same values.  A segment that does not fit the LDS buffer (down-scaling by more than ~10x) takes the direct path.
constexpr int PRE_ROWB = 8192;                       // bytes of LDS per staged row segment
constexpr int PRE_ROWS = 4;                          // output rows per workgroup (the whitening table is built once for all of them)

// bytes [begin, begin + len) of the image at ``img`` (``img_end`` = one past its last byte) -> dst[shift ...]; returns shift (0..3).
// Aligned dword loads; a dword that would reach past the image's last byte is assembled from byte loads (the packed buffer may end there).
__device__ __forceinline__ int pre_stage(unsigned* dst, const unsigned char* img, const unsigned char* img_end, long long begin, int len) {
  const unsigned char* a0 = img + begin;
  const int shift = (int)((uintptr_t)a0 & 3);
  const unsigned* base = (const unsigned*)(a0 - shift);
  const int ndw = (shift + len + 3) >> 2;
  for (int i = threadIdx.x; i < ndw; i += 256) {
    const unsigned char* q = (const unsigned char*)(base + i);
    unsigned v;
    if (q + 4 <= img_end) v = base[i];
    else {
      v = 0;
      for (int k = 0; k < 4; ++k) if (q + k < img_end) v |= (unsigned)q[k] << (8 * k);
    }
    dst[i] = v;
  }
  return shift;
}

// Photometric jitter ("Colour jitter"): per image color[b] = (fb, fc, fs) -- brightness, contrast, saturation -- applied
// to the SOURCE pixels in float32, before whitening and interpolation.  g = (0.299 Sr + 0.587 Sg + 0.114 Sb) / (H0 W0) is the mean luma
// of the untouched image, formed in float64 from the exact channel sums sqd_image_stats_u8 wrote and rounded to float32 once;
// p = min(fb g, 255) the contrast pivot;  t(v) = clamp(fc min(fb v, 255) + (1 - fc) p, 0, 255) per byte;  y = 0.299 t(r) + 0.587 t(g) +
// 0.114 t(b) per tap;  c' = clamp(fs t(c) + (1 - fs) y, 0, 255) per channel, then whiten(c') = (c' - mean) / std as above.
// Uniform per workgroup (one image each): with fs == 1 the whole chain is per channel (c' = t(c) exactly: t is already inside
// [0, 255], 1 * t + 0 * y = t), so the 768-entry table holds whiten(t(v)) and the per-pixel loop is the plain one; otherwise the
// first 256 entries hold t(v) and the saturation blend and the whitening run per tap.  (1, 1, 1) reproduces the plain table bit
// for bit: min(1 * v, 255) = v and 1 * v + 0 * p = v.
struct PreColor {
  float fb, fc, fs;
  float cp;                      // (1 - fc) * p
  bool per_tap;                  // fs != 1: the table holds t(v), not whiten(t(v))
};

// the factors at ``c`` = (fb, fc, fs) with the channel sums at ``s`` = [3][2] of an H0 x W0 image (mosaic: an output image's factors, a source's sums)
__device__ __forceinline__ PreColor pre_color_rows(const float* c, const unsigned long long* s, int H0, int W0) {
  PreColor k;
  k.fb = c[0]; k.fc = c[1]; k.fs = c[2];
  const double g64 = (0.299 * (double)s[0] + 0.587 * (double)s[2] + 0.114 * (double)s[4]) / ((double)H0 * (double)W0);
  const float p = fminf(k.fb * (float)g64, 255.f);
  k.cp = (1.f - k.fc) * p;
  k.per_tap = k.fs != 1.f;
  return k;
}

__device__ __forceinline__ PreColor pre_color_of(const float* color, const unsigned long long* sums, int b, int H0, int W0) {
  return pre_color_rows(color + 3 * b, sums + 6ll * b, H0, W0);      // sums: [3][2] = (sum x, sum x*x) per channel
}

__device__ __forceinline__ float pre_color_t(const PreColor& k, float v) {
  return fminf(fmaxf(k.fc * fminf(k.fb * v, 255.f) + k.cp, 0.f), 255.f);
}

// The workgroup's table (256 threads): whiten(v), or COLOR whiten(t(v)), per channel; COLOR with per_tap only t(v).
template <bool COLOR>
__device__ __forceinline__ void pre_fill_table(float* lut, const PreColor& k, const float (&mean)[3], const float (&stdv)[3]) {
  if (COLOR && k.per_tap) {
    lut[threadIdx.x] = pre_color_t(k, (float)threadIdx.x);
    return;
  }
  const float m0 = mean[0], m1 = mean[1], m2 = mean[2], s0 = stdv[0], s1 = stdv[1], s2 = stdv[2];
  for (int i = threadIdx.x; i < 768; i += 256) {
    const int c = i >> 8, v = i & 255;
    const float m = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
    lut[i] = ((COLOR ? pre_color_t(k, (float)v) : (float)v) - m) / sd;
  }
}

template <bool COLOR>
__device__ __forceinline__ PreColor pre_build_table(float* lut, const float* color, const unsigned long long* sums, int b, int H0, int W0,
                                                    const float (&mean)[3], const float (&stdv)[3]) {
  PreColor k = {};
  if (COLOR) k = pre_color_of(color, sums, b, H0, W0);
  pre_fill_table<COLOR>(lut, k, mean, stdv);
  return k;
}

// one tap of the per-tap form: the three bytes at p through the t table, the saturation blend, then whiten
__device__ __forceinline__ void pre_color_tap(const float* lut, const PreColor& k, const unsigned char* p, const float* mean, const float* stdv,
                                              float (&o)[3]) {
  const float t0 = lut[p[0]], t1 = lut[p[1]], t2 = lut[p[2]];
  const float q = (1.f - k.fs) * (0.299f * t0 + 0.587f * t1 + 0.114f * t2);
  o[0] = (fminf(fmaxf(k.fs * t0 + q, 0.f), 255.f) - mean[0]) / stdv[0];
  o[1] = (fminf(fmaxf(k.fs * t1 + q, 0.f), 255.f) - mean[1]) / stdv[1];
  o[2] = (fminf(fmaxf(k.fs * t2 + q, 0.f), 255.f) - mean[2]) / stdv[2];
}

// Training augmentation (reference train phase, src/datasets/base.py:43-59 with drift / flip active; src/utils/image.py:22-74): per image
// aug[b] = (dy, dx, flipped).  The drifted image V is Hd x Wd = (H0 - dy) x (W0 - dx); before the flip V[y][x] = whiten(I[y+dy][x+dx])
// where y + dy >= 0 and x + dx >= 0, else exactly 0.0f (the reference zero-fills AFTER whitening); the flip reads V[y][Wd-1-x].  Every
// kernel below is a template on AUG: the resize / crop_or_pad / letterbox coordinate rule runs in V coordinates (Hd, Wd), and only then
// is a V column mapped to a column of I, col(v) = (flipped ? Wd-1-v : v) + dx (a row: v + dy).  A tap in the fill region reads 0 and is
// never loaded; a workgroup's source segment is bounded by the mapped columns of its two end pixels (min / max: under a flip the
// column falls as x rises), clamped to the image, and a row wholly in the fill region is not staged.  dy / dx are clamped to
// [-2^20, H0-1] / [-2^20, W0-1] so that Hd, Wd >= 1 whatever the buffer holds.  AUG = false is the untouched eval-time kernel.
// COLOR (with AUG only): the photometric jitter above; COLOR = false instantiates exactly the body without it.
template <bool AUG>
__device__ __forceinline__ int pre_drift(const int* aug, int k, int n0) {
  return AUG ? max(min(aug[k], n0 - 1), -(1 << 20)) : 0;
}

// image b of size (H0, W0): (AUG) its clamped drift and flip, and the size (Hd, Wd) of the drifted image V the coordinate rule sees
// (the bodies load H0 and W0 themselves: inside this struct the pair costs the letterbox kernels an SGPR and reorders pad / crop)
struct PreView {
  int dy, dx; bool flip;
  int Hd, Wd;
  template <bool AUG> __device__ __forceinline__ int col(int v) const { return AUG ? (flip ? Wd - 1 - v : v) + dx : v; }     // V column -> image column
};

template <bool AUG>
__device__ __forceinline__ PreView pre_view(const int* aug, int b, int H0, int W0) {
  PreView v;
  v.dy = pre_drift<AUG>(aug, 3 * b, H0); v.dx = pre_drift<AUG>(aug, 3 * b + 1, W0);
  v.flip = AUG && aug[3 * b + 2] != 0;
  v.Hd = AUG ? H0 - v.dy : H0; v.Wd = AUG ? W0 - v.dx : W0;
  return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// The third geometry, cfg.letterbox (no reference counterpart; DESIGN.md 6b, "Letterbox and zoom-out"): the drifted, flipped image
// V (Hd x Wd; eval: the image itself) is resized with its aspect ratio kept into a window (top, left, h1, w1) of the H x W canvas,
// and everything outside the window is exactly +0.0f -- the whitened mean, as the reference's zero fill after whitening.  Inside
// the window the value at (y, x) is the resize rule with destination size (h1, w1) evaluated at (y - top, x - left): the same
// expressions of the same body (LB), so a window that is the whole canvas gives the resize kernel's bits.
// The window comes from win[B][4] int32 (zoom-out: the host shrinks and places it) or, win == null, from the integer rule
//   H * Wd <= W * Hd (height-limited):  h1 = H, w1 = max(1, (Wd * H + Hd / 2) / Hd);  else  w1 = W, h1 = max(1, (Hd * W + Wd / 2) / Wd);
//   top = (H - h1) / 2, left = (W - w1) / 2     (64-bit, integer divisions: boxes.letterbox_window evaluates the same)
// A given window is clamped into the canvas (h1 to 1..H, w1 to 1..W, then top to 0..H-h1, left to 0..W-w1), in the spirit of pre_drift: no
// buffer content makes the kernel read or write out of range.  scales = (h1 / Hd, w1 / Wd) (float64 division, cast to float32) and
// shifts = (-(float)top / sy, -(float)left / sx): box / scales + shifts in the detect kernels is boxes_postprocess with
// padding = (top / sy, ., left / sx, .), i.e. the padding in original-image pixels.
// The staged segment is bounded by the workgroup's columns INSIDE the window; a workgroup with no column or no row in the window
// stores zeros and returns before the table is built; one cut by a window edge takes both cases per thread (the barriers run for
// every row, window or not).
// ---------------------------------------------------------------------------------------------------------------------
struct LetterboxArgs {
  const unsigned char* src; const long long* offsets; const int* sizes;
  const int* win;                // [B][4] = (top, left, h1, w1), or null: the centred window of the integer rule
  float* out; float* scales; float* shifts;
  float mean[3], stdv[3];
  int B, H, W;
};

// The bilinear body of the resize (LB = false, Args = PreArgs) and letterbox (LB = true, Args = LetterboxArgs) geometries.  Everything
// the window adds sits behind LB: with LB = false the destination is the canvas itself and the expressions are the resize rule's own.
template <bool LB, bool AUG, bool COLOR, class Args>
__device__ __forceinline__ void preprocess_bilinear_body(const Args& a, const int* aug, const float* color, const unsigned long long* sums) {
  __shared__ float lut[768];
  __shared__ unsigned rows[2][PRE_ROWB / 4];
  const int b = blockIdx.z;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int H0 = a.sizes[2 * b], W0 = a.sizes[2 * b + 1];
  const PreView im = pre_view<AUG>(aug, b, H0, W0);
  const int dy = im.dy, Hd = im.Hd, Wd = im.Wd;
  int top = 0, left = 0, h1 = a.H, w1 = a.W;         // the destination window (!LB: the canvas)
  if constexpr (LB) {
    if (a.win) {
      const int* w = a.win + 4 * b;
      h1 = max(min(w[2], a.H), 1); w1 = max(min(w[3], a.W), 1);
      top = max(min(w[0], a.H - h1), 0); left = max(min(w[1], a.W - w1), 0);
    } else {
      const long long H = a.H, W = a.W, hd = Hd, wd = Wd;
      if (H * wd <= W * hd) { h1 = a.H; w1 = (int)min(max((wd * H + hd / 2) / hd, 1ll), W); }
      else { w1 = a.W; h1 = (int)min(max((hd * W + wd / 2) / wd, 1ll), H); }
      top = (a.H - h1) / 2; left = (a.W - w1) / 2;
    }
    if (x == 0 && blockIdx.y == 0 && (a.scales || a.shifts)) {
      const float sy = (float)((double)h1 / (double)Hd), sx = (float)((double)w1 / (double)Wd);
      if (a.scales) { a.scales[2 * b] = sy; a.scales[2 * b + 1] = sx; }
      if (a.shifts) { a.shifts[2 * b] = -(float)top / sy; a.shifts[2 * b + 1] = -(float)left / sx; }
    }
  } else {
    if (x == 0 && blockIdx.y == 0 && a.scales) {
      a.scales[2 * b] = (float)a.H / (float)Hd;       // np.array([H/H0, W/W0], dtype=float32): float64 division then cast;
      a.scales[2 * b + 1] = (float)a.W / (float)Wd;   // identical for these integer ratios up to float32 rounding
    }
  }
  const long long plane = (long long)a.H * a.W;
  // the workgroup's columns and rows, (LB) those inside the window (all uniform)
  const int xa = blockIdx.x * 256, xb = min(a.W, xa + 256) - 1;
  const int ia = LB ? max(xa, left) : xa, ib = LB ? min(xb, left + w1 - 1) : xb;
  const int ya = blockIdx.y * PRE_ROWS, yb = min(a.H, ya + PRE_ROWS) - 1;
  if constexpr (LB) {
    if (ia > ib || yb < top || ya >= top + h1) {     // wholly in the fill region: zeros, nothing staged
      if (x < a.W)
        for (int y = ya; y <= yb; ++y) {
          float* o = a.out + (long long)b * 3 * plane + (long long)y * a.W + x;
          o[0] = 0.f; o[plane] = 0.f; o[2 * plane] = 0.f;
        }
      return;
    }
  }
  const unsigned char* img = a.src + a.offsets[b];
  const unsigned char* img_end = img + (long long)H0 * W0 * 3;
  // source coordinates of a destination pixel (double scale like OpenCV, then float weights)
  const double sclx = (double)Wd / (double)w1, scly = (double)Hd / (double)h1;
  auto src_x = [&](int xx, float& f) {
    f = (float)((xx + 0.5) * sclx - 0.5);
    int sx = (int)floorf(f); f -= (float)sx;
    if (sx < 0) { sx = 0; f = 0.f; }
    if (sx >= Wd - 1) { sx = Wd - 1; f = 0.f; }
    return sx;
  };
  // the source column range [lo, hi] of the workgroup's (window) columns (sx is monotone in x): one segment per source row
  float fdummy;
  int lo = src_x(ia - left, fdummy), hi = min(src_x(ib - left, fdummy) + 1, Wd - 1);
  if (AUG) {
    const int ca = im.col<AUG>(lo), cb = im.col<AUG>(hi);
    lo = max(min(ca, cb), 0); hi = min(max(ca, cb), W0 - 1);
  }
  const bool seg = !AUG || hi >= lo;                 // (AUG) false: every (window) column of the workgroup lies in the drift fill
  const int len = (hi - lo + 1) * 3;
  const bool staged = len + 8 <= PRE_ROWB;
  const int xc = min(x, a.W - 1);
  const bool xin = !LB || (xc >= left && xc < left + w1);
  float fx;
  const int sx = src_x(LB ? min(max(xc - left, 0), w1 - 1) : xc, fx);     // (a thread outside the window: the nearest window column, never read)
  const int sx1 = min(sx + 1, Wd - 1);
  const int cx0 = im.col<AUG>(sx), cx1 = im.col<AUG>(sx1);
  const bool vx0 = !AUG || cx0 >= 0, vx1 = !AUG || cx1 >= 0;
  const int ux0 = AUG ? max(cx0, 0) : cx0, ux1 = AUG ? max(cx1, 0) : cx1;     // (a fill tap's address: any in-range one)
  const float ax0 = 1.f - fx, ax1 = fx;
  const PreColor kc = pre_build_table<COLOR>(lut, color, sums, b, H0, W0, a.mean, a.stdv);
  for (int r = 0; r < PRE_ROWS; ++r) {
    const int y = ya + r;
    if (y >= a.H) break;                             // (uniform)
    const bool yin = !LB || (y >= top && y < top + h1);       // (uniform)
    float fy = (float)(((LB ? min(max(y - top, 0), h1 - 1) : y) + 0.5) * scly - 0.5);
    int sy = (int)floorf(fy); fy -= (float)sy;
    if (sy < 0) { sy = 0; fy = 0.f; }
    if (sy >= Hd - 1) { sy = Hd - 1; fy = 0.f; }
    const int sy1 = min(sy + 1, Hd - 1);
    const int ry0 = sy + dy, ry1 = sy1 + dy;         // image rows (AUG: negative = fill)
    const bool vy0 = !AUG || ry0 >= 0, vy1 = !AUG || ry1 >= 0;
    const int uy0 = AUG ? max(ry0, 0) : ry0, uy1 = AUG ? max(ry1, 0) : ry1;
    int sh0 = 0, sh1 = 0;
    if (r) __syncthreads();                          // the previous row's readers are done with the segments
    if (staged && seg && yin) {
      if (vy0) sh0 = pre_stage(rows[0], img, img_end, ((long long)uy0 * W0 + lo) * 3, len);
      if (vy1) sh1 = pre_stage(rows[1], img, img_end, ((long long)uy1 * W0 + lo) * 3, len);
    }
    __syncthreads();
    if (x >= a.W) continue;
    float* o = a.out + (long long)b * 3 * plane + (long long)y * a.W + x;
    if (LB && !(yin && xin)) {                       // outside the window: the whitened mean
      o[0] = 0.f; o[plane] = 0.f; o[2 * plane] = 0.f;
      continue;
    }
    const float ay0 = 1.f - fy, ay1 = fy;
    const unsigned char *p00, *p01, *p10, *p11;
    if (staged) {
      const unsigned char* r0 = (const unsigned char*)rows[0] + sh0;
      const unsigned char* r1 = (const unsigned char*)rows[1] + sh1;
      const int ox0 = AUG ? (vx0 ? ux0 - lo : 0) : sx - lo, ox1 = AUG ? (vx1 ? ux1 - lo : 0) : sx1 - lo;
      p00 = r0 + ox0 * 3; p01 = r0 + ox1 * 3; p10 = r1 + ox0 * 3; p11 = r1 + ox1 * 3;
    } else {
      p00 = img + ((long long)uy0 * W0 + ux0) * 3; p01 = img + ((long long)uy0 * W0 + ux1) * 3;
      p10 = img + ((long long)uy1 * W0 + ux0) * 3; p11 = img + ((long long)uy1 * W0 + ux1) * 3;
    }
    const bool t00 = vy0 && vx0, t01 = vy0 && vx1, t10 = vy1 && vx0, t11 = vy1 && vx1;
    if (COLOR && kc.per_tap) {                       // (uniform) saturation mixes the channels of a tap: blend and whiten per tap
      float v00[3] = {0.f, 0.f, 0.f}, v01[3] = {0.f, 0.f, 0.f}, v10[3] = {0.f, 0.f, 0.f}, v11[3] = {0.f, 0.f, 0.f};     // (fill: 0)
      if (t00) pre_color_tap(lut, kc, p00, a.mean, a.stdv, v00);
      if (t01) pre_color_tap(lut, kc, p01, a.mean, a.stdv, v01);
      if (t10) pre_color_tap(lut, kc, p10, a.mean, a.stdv, v10);
      if (t11) pre_color_tap(lut, kc, p11, a.mean, a.stdv, v11);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float r0 = v00[c] * ax0 + v01[c] * ax1;
        const float r1 = v10[c] * ax0 + v11[c] * ax1;
        o[c * plane] = r0 * ay0 + r1 * ay1;
      }
      continue;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* l = lut + 256 * c;                                    // whiten (image.py:17) in float32: the table holds (v - mean) / std
      const float v00 = t00 ? l[p00[c]] : 0.f, v01 = t01 ? l[p01[c]] : 0.f;
      const float v10 = t10 ? l[p10[c]] : 0.f, v11 = t11 ? l[p11[c]] : 0.f;
      const float r0 = v00 * ax0 + v01 * ax1;
      const float r1 = v10 * ax0 + v11 * ax1;
      o[c * plane] = r0 * ay0 + r1 * ay1;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The reference's OTHER pre-processing branch, cfg.forbid_resize (src/datasets/base.py:53-54): whiten (src/utils/image.py:9-19),
// then crop_or_pad (:91-124) -- per axis, a smaller image is zero-padded to the target (floor half in front, np.pad constant 0
// AFTER whitening: padded pixels are 0.0), a larger one is centre-cropped (floor half cut off in front) -- then HWC -> CHW.
// Pure index arithmetic plus the one float32 subtract and divide of whiten: bit-exact against the reference.
// Also writes what boxes_postprocess (src/utils/boxes.py:149-155) needs to map detections back: padding / crops (top, bottom,
// left, right) and the box shift (dy, dx) = (crops[0] - padding[0], crops[2] - padding[2]) the fused detect kernel adds.
// AUG: crop_or_pad of the drifted, flipped image V: padding / crops / shifts from (Hd, Wd).
// ---------------------------------------------------------------------------------------------------------------------
struct PadCropArgs {
  const unsigned char* src; const long long* offsets; const int* sizes;
  float* out; float* shifts; int* padcrop;
  float mean[3], stdv[3];
  int B, H, W;
};

template <bool AUG, bool COLOR>
__device__ __forceinline__ void preprocess_padcrop_body(const PadCropArgs& a, const int* aug, const float* color, const unsigned long long* sums) {
  __shared__ float lut[768];
  __shared__ unsigned row[PRE_ROWB / 4];
  const int b = blockIdx.z;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int H0 = a.sizes[2 * b], W0 = a.sizes[2 * b + 1];
  const PreView im = pre_view<AUG>(aug, b, H0, W0);
  const int dy = im.dy, Hd = im.Hd, Wd = im.Wd;
  // (target - size) // 2 in front when padding, (size - target) // 2 cut in front when cropping
  const int pt = Hd < a.H ? (a.H - Hd) / 2 : 0, ct = Hd > a.H ? (Hd - a.H) / 2 : 0;
  const int pl = Wd < a.W ? (a.W - Wd) / 2 : 0, cl = Wd > a.W ? (Wd - a.W) / 2 : 0;
  if (x == 0 && blockIdx.y == 0) {
    if (a.padcrop) {
      int* pc = a.padcrop + 8 * b;
      pc[0] = pt; pc[1] = Hd < a.H ? (a.H - Hd) - pt : 0; pc[2] = pl; pc[3] = Wd < a.W ? (a.W - Wd) - pl : 0;
      pc[4] = ct; pc[5] = Hd > a.H ? (Hd - a.H) - ct : 0; pc[6] = cl; pc[7] = Wd > a.W ? (Wd - a.W) - cl : 0;
    }
    if (a.shifts) { a.shifts[2 * b] = (float)(ct - pt); a.shifts[2 * b + 1] = (float)(cl - pl); }
  }
  const int sx = x - pl + cl;
  const unsigned char* img = a.src + a.offsets[b];
  // the workgroup's source columns: [lo, hi] of the source row, clipped to the image (256 pixels = 768 bytes: always fits)
  const int xa = blockIdx.x * 256;
  int lo = max(xa - pl + cl, 0), hi = min(min(a.W, xa + 256) - 1 - pl + cl, Wd - 1);
  if (AUG && hi >= lo) {
    const int ca = im.col<AUG>(lo), cb = im.col<AUG>(hi);
    lo = max(min(ca, cb), 0); hi = min(max(ca, cb), W0 - 1);
  }
  const long long plane = (long long)a.H * a.W;
  const PreColor kc = pre_build_table<COLOR>(lut, color, sums, b, H0, W0, a.mean, a.stdv);
  for (int r = 0; r < PRE_ROWS; ++r) {
    const int y = blockIdx.y * PRE_ROWS + r;
    if (y >= a.H) break;                             // (uniform)
    const int sy = y - pt + ct;
    const bool row_in = sy >= 0 && sy < Hd && hi >= lo && (!AUG || sy + dy >= 0);
    int sh = 0;
    if (r) __syncthreads();
    if (row_in) sh = pre_stage(row, img, img + (long long)H0 * W0 * 3, ((long long)(AUG ? sy + dy : sy) * W0 + lo) * 3, (hi - lo + 1) * 3);
    __syncthreads();
    if (x >= a.W) continue;
    const int cx = im.col<AUG>(sx);
    const bool inside = row_in && sx >= 0 && sx < Wd && (!AUG || cx >= 0);
    float* o = a.out + (long long)b * 3 * plane + (long long)y * a.W + x;
    const unsigned char* p = (const unsigned char*)row + sh + (inside ? (cx - lo) * 3 : 0);
    if (COLOR && kc.per_tap) {                       // (uniform)
      float v[3] = {0.f, 0.f, 0.f};
      if (inside) pre_color_tap(lut, kc, p, a.mean, a.stdv, v);
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c * plane] = v[c];
      continue;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = inside ? lut[256 * c + p[c]] : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Mosaic (no reference counterpart; DESIGN.md 6b, "Mosaic"; training only): an output image is a list of at most four TILES,
// tiles[b][t] = (src, top, left, h1, w1, y0, x0, y1, x1).  src indexes the S SOURCE images of the upload (offsets, sizes, aug and
// sums have one row per source), (top, left, h1, w1) is a letterbox window that may hang over the canvas on any side, and
// [y0, y1) x [x0, x1) is the tile's rectangle inside canvas and window.  A pixel of the rectangle holds the letterbox rule's
// value for that window -- the expressions of preprocess_bilinear_body, restated below op for op, so that a one-tile image
// whose rectangle is its window has the letterbox_aug kernel's bits --, a pixel in no rectangle is +0.0f, and where
// rectangles overlap the first tile of the list owns the pixel.  src < 0 ends the list.
// Whatever the buffer holds: src is clamped to S - 1, h1 / w1 to 1..65535, top / left to -65535..65535 and the rectangle into
// canvas and window; an empty rectangle contributes nothing.  No side outputs: the tile list is the record.
// A workgroup walks the tiles in order (uniform control flow).  For each tile that meets its 256 x PRE_ROWS block it builds
// the table (COLOR: of the output image's factors and THAT source's mean luma; rebuilt only when src changes, without COLOR
// built once), stages the one or two source row segments bounded by its columns inside the rectangle, and stores the pixels
// of the rectangle no earlier tile owned; a per-thread bit per row records ownership, and what is left at the end is
// stored as zero.  Every pixel is stored exactly once.  One table and two row buffers, as the bilinear body: a table per tile
// would cost 3 KB of LDS each for a rebuild that only seam-crossing workgroups of the colour form ever run.
// ---------------------------------------------------------------------------------------------------------------------
struct MosaicArgs {
  const unsigned char* src; const long long* offsets; const int* sizes;
  const int* tiles;              // [B][4][9]
  float* out;
  float mean[3], stdv[3];
  int B, S, H, W;
};
constexpr int PRE_TILES = 4, PRE_TILE_INTS = 9, PRE_WIN_MAX = 65535;

template <bool COLOR>
__device__ __forceinline__ void preprocess_mosaic_body(const MosaicArgs& a, const int* aug, const float* color, const unsigned long long* sums) {
  __shared__ float lut[768];
  __shared__ unsigned rows[2][PRE_ROWB / 4];
  const int b = blockIdx.z;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const long long plane = (long long)a.H * a.W;
  const int xa = blockIdx.x * 256, xb = min(a.W, xa + 256) - 1;
  const int ya = blockIdx.y * PRE_ROWS, yb = min(a.H, ya + PRE_ROWS) - 1;
  const int xc = min(x, a.W - 1);
  float* const obase = a.out + (long long)b * 3 * plane + x;
  unsigned owned = 0;                                // bit r: row ya + r of this thread's column is stored
  int lut_src = -1;                                  // the source the table was built for (!COLOR: any)
  bool used = false;                                 // LDS has readers since the last barrier
  PreColor kc = {};
  for (int t = 0; t < PRE_TILES; ++t) {              // (everything but the per-thread column is uniform)
    const int* tl = a.tiles + ((long long)b * PRE_TILES + t) * PRE_TILE_INTS;
    if (tl[0] < 0) break;
    const int s = min(tl[0], a.S - 1);
    const int h1 = max(min(tl[3], PRE_WIN_MAX), 1), w1 = max(min(tl[4], PRE_WIN_MAX), 1);
    const int top = max(min(tl[1], PRE_WIN_MAX), -PRE_WIN_MAX), left = max(min(tl[2], PRE_WIN_MAX), -PRE_WIN_MAX);
    const int y0 = max(max(tl[5], 0), top), x0 = max(max(tl[6], 0), left);
    const int y1 = min(min(tl[7], a.H), top + h1), x1 = min(min(tl[8], a.W), left + w1);
    // the workgroup's columns and rows inside the rectangle
    const int ia = max(xa, x0), ib = min(xb, x1 - 1);
    const int ja = max(ya, y0), jb = min(yb, y1 - 1);
    if (ia > ib || ja > jb) continue;                // (also: an empty rectangle)
    const int H0 = a.sizes[2 * s], W0 = a.sizes[2 * s + 1];
    const PreView im = pre_view<true>(aug, s, H0, W0);
    const int dy = im.dy, Hd = im.Hd, Wd = im.Wd;
    const unsigned char* img = a.src + a.offsets[s];
    const unsigned char* img_end = img + (long long)H0 * W0 * 3;
    const double sclx = (double)Wd / (double)w1, scly = (double)Hd / (double)h1;
    auto src_x = [&](int xx, float& f) {
      f = (float)((xx + 0.5) * sclx - 0.5);
      int sx = (int)floorf(f); f -= (float)sx;
      if (sx < 0) { sx = 0; f = 0.f; }
      if (sx >= Wd - 1) { sx = Wd - 1; f = 0.f; }
      return sx;
    };
    float fdummy;
    int lo = src_x(ia - left, fdummy), hi = min(src_x(ib - left, fdummy) + 1, Wd - 1);
    {
      const int ca = im.col<true>(lo), cb = im.col<true>(hi);
      lo = max(min(ca, cb), 0); hi = min(max(ca, cb), W0 - 1);
    }
    const bool seg = hi >= lo;                       // false: every column of the workgroup in the rectangle lies in the drift fill
    const int len = (hi - lo + 1) * 3;
    const bool staged = len + 8 <= PRE_ROWB;
    const bool xin = xc >= x0 && xc < x1;
    float fx;
    const int sx = src_x(min(max(xc - left, 0), w1 - 1), fx);     // (a thread outside the rectangle: some window column, never read)
    const int sx1 = min(sx + 1, Wd - 1);
    const int cx0 = im.col<true>(sx), cx1 = im.col<true>(sx1);
    const bool vx0 = cx0 >= 0, vx1 = cx1 >= 0;
    const int ux0 = max(cx0, 0), ux1 = max(cx1, 0);
    const float ax0 = 1.f - fx, ax1 = fx;
    if (used) __syncthreads();                       // the previous tile's readers are done with the table and the segments
    used = true;
    if (COLOR ? s != lut_src : lut_src < 0) {
      if (COLOR) kc = pre_color_rows(color + 3 * b, sums + 6ll * s, H0, W0);
      pre_fill_table<COLOR>(lut, kc, a.mean, a.stdv);
      lut_src = s;
    }
    for (int y = ja; y <= jb; ++y) {
      float fy = (float)((min(max(y - top, 0), h1 - 1) + 0.5) * scly - 0.5);
      int sy = (int)floorf(fy); fy -= (float)sy;
      if (sy < 0) { sy = 0; fy = 0.f; }
      if (sy >= Hd - 1) { sy = Hd - 1; fy = 0.f; }
      const int sy1 = min(sy + 1, Hd - 1);
      const int ry0 = sy + dy, ry1 = sy1 + dy;       // image rows (negative = fill)
      const bool vy0 = ry0 >= 0, vy1 = ry1 >= 0;
      const int uy0 = max(ry0, 0), uy1 = max(ry1, 0);
      int sh0 = 0, sh1 = 0;
      if (y > ja) __syncthreads();                   // the previous row's readers are done with the segments
      if (staged && seg) {
        if (vy0) sh0 = pre_stage(rows[0], img, img_end, ((long long)uy0 * W0 + lo) * 3, len);
        if (vy1) sh1 = pre_stage(rows[1], img, img_end, ((long long)uy1 * W0 + lo) * 3, len);
      }
      __syncthreads();
      const unsigned bit = 1u << (y - ya);
      if (x >= a.W || !xin || (owned & bit)) continue;            // off the canvas, outside the rectangle, or an earlier tile's pixel
      owned |= bit;
      float* o = obase + (long long)y * a.W;
      const float ay0 = 1.f - fy, ay1 = fy;
      const unsigned char *p00, *p01, *p10, *p11;
      if (staged) {
        const unsigned char* r0 = (const unsigned char*)rows[0] + sh0;
        const unsigned char* r1 = (const unsigned char*)rows[1] + sh1;
        const int ox0 = vx0 ? ux0 - lo : 0, ox1 = vx1 ? ux1 - lo : 0;
        p00 = r0 + ox0 * 3; p01 = r0 + ox1 * 3; p10 = r1 + ox0 * 3; p11 = r1 + ox1 * 3;
      } else {
        p00 = img + ((long long)uy0 * W0 + ux0) * 3; p01 = img + ((long long)uy0 * W0 + ux1) * 3;
        p10 = img + ((long long)uy1 * W0 + ux0) * 3; p11 = img + ((long long)uy1 * W0 + ux1) * 3;
      }
      const bool t00 = vy0 && vx0, t01 = vy0 && vx1, t10 = vy1 && vx0, t11 = vy1 && vx1;
      if (COLOR && kc.per_tap) {                     // (uniform)
        float v00[3] = {0.f, 0.f, 0.f}, v01[3] = {0.f, 0.f, 0.f}, v10[3] = {0.f, 0.f, 0.f}, v11[3] = {0.f, 0.f, 0.f};     // (fill: 0)
        if (t00) pre_color_tap(lut, kc, p00, a.mean, a.stdv, v00);
        if (t01) pre_color_tap(lut, kc, p01, a.mean, a.stdv, v01);
        if (t10) pre_color_tap(lut, kc, p10, a.mean, a.stdv, v10);
        if (t11) pre_color_tap(lut, kc, p11, a.mean, a.stdv, v11);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float r0 = v00[c] * ax0 + v01[c] * ax1;
          const float r1 = v10[c] * ax0 + v11[c] * ax1;
          o[c * plane] = r0 * ay0 + r1 * ay1;
        }
        continue;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* l = lut + 256 * c;
        const float v00 = t00 ? l[p00[c]] : 0.f, v01 = t01 ? l[p01[c]] : 0.f;
        const float v10 = t10 ? l[p10[c]] : 0.f, v11 = t11 ? l[p11[c]] : 0.f;
        const float r0 = v00 * ax0 + v01 * ax1;
        const float r1 = v10 * ax0 + v11 * ax1;
        o[c * plane] = r0 * ay0 + r1 * ay1;
      }
    }
  }
  if (x >= a.W) return;
  for (int y = ya; y <= yb; ++y) {                   // in no rectangle: the whitened mean
    if (owned & (1u << (y - ya))) continue;
    float* o = obase + (long long)y * a.W;
    o[0] = 0.f; o[plane] = 0.f; o[2 * plane] = 0.f;
  }
}

// The nine kernels: geometry x (eval, AUG, AUG + COLOR), and the two mosaic ones (training only: AUG, AUG + COLOR).
__global__ __launch_bounds__(256) void preprocess_mosaic_aug_kernel(MosaicArgs a, const int* aug) { preprocess_mosaic_body<false>(a, aug, nullptr, nullptr); }
__global__ __launch_bounds__(256) void preprocess_mosaic_aug_color_kernel(MosaicArgs a, const int* aug, const float* color,
                                                                          const unsigned long long* sums) {
  preprocess_mosaic_body<true>(a, aug, color, sums);
}
__global__ __launch_bounds__(256) void preprocess_kernel(PreArgs a) { preprocess_bilinear_body<false, false, false>(a, nullptr, nullptr, nullptr); }
__global__ __launch_bounds__(256) void preprocess_aug_kernel(PreArgs a, const int* aug) { preprocess_bilinear_body<false, true, false>(a, aug, nullptr, nullptr); }
__global__ __launch_bounds__(256) void preprocess_aug_color_kernel(PreArgs a, const int* aug, const float* color, const unsigned long long* sums) {
  preprocess_bilinear_body<false, true, true>(a, aug, color, sums);
}
__global__ __launch_bounds__(256) void preprocess_padcrop_kernel(PadCropArgs a) { preprocess_padcrop_body<false, false>(a, nullptr, nullptr, nullptr); }
__global__ __launch_bounds__(256) void preprocess_padcrop_aug_kernel(PadCropArgs a, const int* aug) { preprocess_padcrop_body<true, false>(a, aug, nullptr, nullptr); }
__global__ __launch_bounds__(256) void preprocess_padcrop_aug_color_kernel(PadCropArgs a, const int* aug, const float* color,
                                                                           const unsigned long long* sums) {
  preprocess_padcrop_body<true, true>(a, aug, color, sums);
}
__global__ __launch_bounds__(256) void preprocess_letterbox_kernel(LetterboxArgs a) { preprocess_bilinear_body<true, false, false>(a, nullptr, nullptr, nullptr); }
__global__ __launch_bounds__(256) void preprocess_letterbox_aug_kernel(LetterboxArgs a, const int* aug) {
  preprocess_bilinear_body<true, true, false>(a, aug, nullptr, nullptr);
}
__global__ __launch_bounds__(256) void preprocess_letterbox_aug_color_kernel(LetterboxArgs a, const int* aug, const float* color,
                                                                             const unsigned long long* sums) {
  preprocess_bilinear_body<true, true, true>(a, aug, color, sums);
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side.  Every entry: SQD_ERR_BAD_ARG before any launch unless pre_args and pre_blocks accept its arguments.
// ---------------------------------------------------------------------------------------------------------------------
// the part common to all nine entries: checks it and copies it into the kernel's argument struct
template <class Args>
static inline bool pre_args(Args& a, const unsigned char* src, const long long* offsets, const int* sizes, float* out, const float* mean3,
                            const float* std3, int B, int H, int W) {
  if (!(src && offsets && sizes && out && mean3 && std3 && B > 0 && H > 0 && W > 0 && B <= 65535 && H <= 65535)) return false;
  a.src = src; a.offsets = offsets; a.sizes = sizes; a.out = out; a.B = B; a.H = H; a.W = W;
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.stdv[c] = std3[c]; if (std3[c] == 0.f) return false; }
  return true;
}

// the optional blocks: aug required by the AUG forms, color and sums (aligned) by the COLOR forms; win (letterbox) may be null
enum { PRE_AUG = 1, PRE_COLOR = 2 };
static inline bool pre_blocks(int need, const int* aug, const float* color, const unsigned long long* sums, const int* win) {
  if ((need & PRE_AUG) && !aug) return false;
  if ((need & PRE_COLOR) && !(color && sums && ((uintptr_t)sums & 7) == 0 && ((uintptr_t)color & 3) == 0)) return false;
  return ((uintptr_t)win & 3) == 0;
}

template <class... T>
static inline int pre_launch(void (*kernel)(T...), int B, int H, int W, void* stream, T... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)sqd_cdiv(W, 256), (unsigned)sqd_cdiv(H, PRE_ROWS), (unsigned)B), dim3(256), 0, (hipStream_t)stream, args...);
  return sqd_launch_status();
}

// src: device buffer holding the B images back to back (HWC uint8 RGB); offsets [B] byte offsets; sizes [B][2] =
// (H0, W0) int32; out: NCHW fp32 [B][3][H][W]; scales: [B][2] fp32 or NULL; mean/std: 3 floats each (host).
extern "C" int sqd_preprocess_u8_fwd(const unsigned char* src, const long long* offsets, const int* sizes, float* out, float* scales,
                                     const float* mean3, const float* std3, int B, int H, int W, void* stream) {
  PreArgs a; a.scales = scales;
  SQD_CHECK_ARG(pre_args(a, src, offsets, sizes, out, mean3, std3, B, H, W));
  return pre_launch(preprocess_kernel, B, H, W, stream, a);
}

// Arguments as sqd_preprocess_u8_fwd; shifts: [B][2] fp32 (dy, dx) or NULL; padcrop: [B][8] int32 = padding (top, bottom, left,
// right) then crops (top, bottom, left, right), or NULL.
extern "C" int sqd_preprocess_u8_padcrop_fwd(const unsigned char* src, const long long* offsets, const int* sizes, float* out, float* shifts,
                                             int* padcrop, const float* mean3, const float* std3, int B, int H, int W, void* stream) {
  PadCropArgs a; a.shifts = shifts; a.padcrop = padcrop;
  SQD_CHECK_ARG(pre_args(a, src, offsets, sizes, out, mean3, std3, B, H, W));
  return pre_launch(preprocess_padcrop_kernel, B, H, W, stream, a);
}

// Training forms (reference train phase: drift + flip before the resize / crop_or_pad).  aug: device int32 [B][3] = (dy, dx, flipped)
// per image; scales = (H / Hd, W / Wd) and padding / crops / shifts are those of the drifted size (Hd, Wd) = (H0 - dy, W0 - dx).
// Other arguments as sqd_preprocess_u8_fwd / sqd_preprocess_u8_padcrop_fwd.
extern "C" int sqd_preprocess_u8_aug_fwd(const unsigned char* src, const long long* offsets, const int* sizes, const int* aug, float* out,
                                         float* scales, const float* mean3, const float* std3, int B, int H, int W, void* stream) {
  PreArgs a; a.scales = scales;
  SQD_CHECK_ARG(pre_blocks(PRE_AUG, aug, nullptr, nullptr, nullptr) && pre_args(a, src, offsets, sizes, out, mean3, std3, B, H, W));
  return pre_launch(preprocess_aug_kernel, B, H, W, stream, a, aug);
}

extern "C" int sqd_preprocess_u8_padcrop_aug_fwd(const unsigned char* src, const long long* offsets, const int* sizes, const int* aug, float* out,
                                                 float* shifts, int* padcrop, const float* mean3, const float* std3, int B, int H, int W,
                                                 void* stream) {
  PadCropArgs a; a.shifts = shifts; a.padcrop = padcrop;
  SQD_CHECK_ARG(pre_blocks(PRE_AUG, aug, nullptr, nullptr, nullptr) && pre_args(a, src, offsets, sizes, out, mean3, std3, B, H, W));
  return pre_launch(preprocess_padcrop_aug_kernel, B, H, W, stream, a, aug);
}

// Colour forms of the two above (the photometric jitter of pre_color_of): color: device fp32 [B][3] = (brightness, contrast, saturation)
// factors per image; sums: device uint64 [B][3][2] as sqd_image_stats_u8 writes it for the same src / offsets / sizes (launched before this
// call on the same stream).  Both are required.  color = (1, 1, 1) everywhere gives the results of the _aug_ entry points bit for bit.
extern "C" int sqd_preprocess_u8_aug_color_fwd(const unsigned char* src, const long long* offsets, const int* sizes, const int* aug,
                                               const float* color, const unsigned long long* sums, float* out, float* scales, const float* mean3,
                                               const float* std3, int B, int H, int W, void* stream) {
  PreArgs a; a.scales = scales;
  SQD_CHECK_ARG(pre_blocks(PRE_AUG | PRE_COLOR, aug, color, sums, nullptr) && pre_args(a, src, offsets, sizes, out, mean3, std3, B, H, W));
  return pre_launch(preprocess_aug_color_kernel, B, H, W, stream, a, aug, color, sums);
}

extern "C" int sqd_preprocess_u8_padcrop_aug_color_fwd(const unsigned char* src, const long long* offsets, const int* sizes, const int* aug,
                                                       const float* color, const unsigned long long* sums, float* out, float* shifts, int* padcrop,
                                                       const float* mean3, const float* std3, int B, int H, int W, void* stream) {
  PadCropArgs a; a.shifts = shifts; a.padcrop = padcrop;
  SQD_CHECK_ARG(pre_blocks(PRE_AUG | PRE_COLOR, aug, color, sums, nullptr) && pre_args(a, src, offsets, sizes, out, mean3, std3, B, H, W));
  return pre_launch(preprocess_padcrop_aug_color_kernel, B, H, W, stream, a, aug, color, sums);
}

// Letterbox forms.  Arguments as sqd_preprocess_u8_fwd / _aug_fwd / _aug_color_fwd; win: device int32 [B][4] = (top, left, h1, w1) per
// image or NULL (the centred window of the integer rule above); scales [B][2] = (h1 / Hd, w1 / Wd) and shifts [B][2] = (-top / sy,
// -left / sx), either may be NULL.
extern "C" int sqd_preprocess_u8_letterbox_fwd(const unsigned char* src, const long long* offsets, const int* sizes, const int* win, float* out,
                                               float* scales, float* shifts, const float* mean3, const float* std3, int B, int H, int W,
                                               void* stream) {
  LetterboxArgs a; a.win = win; a.scales = scales; a.shifts = shifts;
  SQD_CHECK_ARG(pre_blocks(0, nullptr, nullptr, nullptr, win) && pre_args(a, src, offsets, sizes, out, mean3, std3, B, H, W));
  return pre_launch(preprocess_letterbox_kernel, B, H, W, stream, a);
}

extern "C" int sqd_preprocess_u8_letterbox_aug_fwd(const unsigned char* src, const long long* offsets, const int* sizes, const int* aug,
                                                   const int* win, float* out, float* scales, float* shifts, const float* mean3, const float* std3,
                                                   int B, int H, int W, void* stream) {
  LetterboxArgs a; a.win = win; a.scales = scales; a.shifts = shifts;
  SQD_CHECK_ARG(pre_blocks(PRE_AUG, aug, nullptr, nullptr, win) && pre_args(a, src, offsets, sizes, out, mean3, std3, B, H, W));
  return pre_launch(preprocess_letterbox_aug_kernel, B, H, W, stream, a, aug);
}

extern "C" int sqd_preprocess_u8_letterbox_aug_color_fwd(const unsigned char* src, const long long* offsets, const int* sizes, const int* aug,
                                                         const int* win, const float* color, const unsigned long long* sums, float* out,
                                                         float* scales, float* shifts, const float* mean3, const float* std3, int B, int H, int W,
                                                         void* stream) {
  LetterboxArgs a; a.win = win; a.scales = scales; a.shifts = shifts;
  SQD_CHECK_ARG(pre_blocks(PRE_AUG | PRE_COLOR, aug, color, sums, win) && pre_args(a, src, offsets, sizes, out, mean3, std3, B, H, W));
  return pre_launch(preprocess_letterbox_aug_color_kernel, B, H, W, stream, a, aug, color, sums);
}

// Mosaic forms (training only).  Arguments as the letterbox _aug_ / _aug_color_ entries with these changes: offsets, sizes, aug and sums
// have one row per SOURCE image, S rows (1 <= S <= 4 B); tiles: device int32 [B][4][9] = (src, top, left, h1, w1, y0, x0, y1, x1) per
// output image and tile, src < 0 ends an image's list; color stays [B][3], one row per output image (the contrast pivot is the mean
// luma of each tile's own source, sums[src]); no scales / shifts outputs.  B, H and W each in 1..65535.
static inline bool mosaic_args(MosaicArgs& a, const int* tiles, int B, int S, int W) {
  if (!(tiles && ((uintptr_t)tiles & 3) == 0 && W <= 65535 && S >= 1 && (long long)S <= 4ll * B)) return false;
  a.tiles = tiles; a.S = S;
  return true;
}

extern "C" int sqd_preprocess_u8_mosaic_aug_fwd(const unsigned char* src, const long long* offsets, const int* sizes, const int* aug,
                                                const int* tiles, float* out, const float* mean3, const float* std3, int B, int S, int H, int W,
                                                void* stream) {
  MosaicArgs a;
  SQD_CHECK_ARG(pre_blocks(PRE_AUG, aug, nullptr, nullptr, nullptr) && pre_args(a, src, offsets, sizes, out, mean3, std3, B, H, W) &&
                mosaic_args(a, tiles, B, S, W));
  return pre_launch(preprocess_mosaic_aug_kernel, B, H, W, stream, a, aug);
}

extern "C" int sqd_preprocess_u8_mosaic_aug_color_fwd(const unsigned char* src, const long long* offsets, const int* sizes, const int* aug,
                                                      const int* tiles, const float* color, const unsigned long long* sums, float* out,
                                                      const float* mean3, const float* std3, int B, int S, int H, int W, void* stream) {
  MosaicArgs a;
  SQD_CHECK_ARG(pre_blocks(PRE_AUG | PRE_COLOR, aug, color, sums, nullptr) && pre_args(a, src, offsets, sizes, out, mean3, std3, B, H, W) &&
                mosaic_args(a, tiles, B, S, W));
  return pre_launch(preprocess_mosaic_aug_color_kernel, B, H, W, stream, a, aug, color, sums);
}
