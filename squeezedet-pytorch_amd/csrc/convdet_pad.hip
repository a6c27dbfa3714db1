// ConvDet of any width.  The 3x3 convolution forms (direct, Winograd, their data and weight gradients) take channel counts that are
// multiples of 4 / 8 / 64; ConvDet's anchors_per_grid * (num_classes + 5) is whatever the dataset makes it (225 for 20 classes).  A
// misaligned ConvDet therefore runs at a padded width Npad (ops.convdet_width: the next multiple of 64, zero weight and bias rows past
// N) into a scratch tensor, and the three small kernels here move between the padded and the reference's layout:
//   sqd_channel_pack_fwd     [rows][Npad] -> [rows][N]      the contiguous pred [B, A, C+5] every head kernel reads
//   sqd_channel_unpack_fwd   [rows][N] -> [rows][Npad]      dpred, zero past N: the data- and weight-gradient launches see Npad
//   sqd_wgrad_reduce_rows    the split-K slabs of the padded weight gradient, reduced over the first N rows only, straight into the
//                            parameter-shaped gradient (OIHW [N][C][k][k], [N])
// rows = B * H * W pixels.  One thread per float of the NARROW side, consecutive threads on consecutive floats.
#include "sqd_common.h"

__global__ __launch_bounds__(256) void channel_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, long long total,
                                                           int N, int Npad) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / N;
    const int c = (int)(i - r * N);
    dst[i] = src[r * Npad + c];
  }
}

__global__ __launch_bounds__(256) void channel_unpack_kernel(const float* __restrict__ src, float* __restrict__ dst, long long total,
                                                             int N, int Npad) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / Npad;
    const int c = (int)(i - r * Npad);
    dst[i] = (c < N) ? src[r * N + c] : 0.f;
  }
}

static inline unsigned pad_blocks(long long total) {
  const long long b = (total + 255) / 256;
  return (unsigned)(b < (1 << 20) ? b : (1 << 20));
}

// dst [rows][N] = src [rows][Npad][:N].  Status 1 for anything malformed (N < 1, Npad < N, rows < 1, null pointers).
extern "C" int sqd_channel_pack_fwd(const float* src, float* dst, long long rows, int N, int Npad, void* stream) {
  SQD_CHECK_ARG(src && dst && rows > 0 && N > 0 && Npad >= N && rows <= (1ll << 40) / Npad);
  const long long total = rows * N;
  hipLaunchKernelGGL(channel_pack_kernel, dim3(pad_blocks(total)), dim3(256), 0, (hipStream_t)stream, src, dst, total, N, Npad);
  return sqd_launch_status();
}

// dst [rows][Npad] = src [rows][N], zero in channels N .. Npad - 1
extern "C" int sqd_channel_unpack_fwd(const float* src, float* dst, long long rows, int N, int Npad, void* stream) {
  SQD_CHECK_ARG(src && dst && rows > 0 && N > 0 && Npad >= N && rows <= (1ll << 40) / Npad);
  const long long total = rows * Npad;
  hipLaunchKernelGGL(channel_unpack_kernel, dim3(pad_blocks(total)), dim3(256), 0, (hipStream_t)stream, src, dst, total, N, Npad);
  return sqd_launch_status();
}

// slab: S partial slabs of Npad * taps * C + Npad floats each ([Npad][taps][C] weight sums, then [Npad] bias sums: what
// sqd_conv_wgrad / sqd_conv_wgrad_wino write for an Npad-wide layer).  Output element e < N * taps * C is one weight, the N after them
// the bias; each is the sum of its S partials in slab order (a fixed order: results do not change from run to run), times scale.
__global__ __launch_bounds__(256) void wgrad_reduce_rows_kernel(const float* __restrict__ slab, int S, long long stride, int N, int Npad,
                                                                int C, int taps, float* __restrict__ dw, float* __restrict__ db, float scale) {
  const long long nw = (long long)N * taps * C, total = nw + N;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long src = e < nw ? e : (long long)Npad * taps * C + (e - nw);
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += slab[(long long)k * stride + src];
    s *= scale;
    if (e < nw) {
      const int c = (int)(e % C); const long long q = e / C;
      const int tap = (int)(q % taps); const long long n = q / taps;
      dw[(n * C + c) * taps + tap] = s;
    } else {
      db[e - nw] = s;
    }
  }
}

extern "C" int sqd_wgrad_reduce_rows(const float* slab, float* dw, float* db, int S, int N, int Npad, int C, int taps, float scale,
                                     void* stream) {
  SQD_CHECK_ARG(slab && dw && db && S > 0 && N > 0 && Npad >= N && C > 0 && (taps == 1 || taps == 9));
  const long long stride = (long long)Npad * taps * C + Npad;
  const long long total = (long long)N * taps * C + N;
  hipLaunchKernelGGL(wgrad_reduce_rows_kernel, dim3(pad_blocks(total)), dim3(256), 0, (hipStream_t)stream, slab, S, stride, N, Npad, C,
                     taps, dw, db, scale);
  return sqd_launch_status();
}
