// Gradient clipping + the optimizer step for ALL parameter tensors in one launch (reference: src/engine/trainer.py:47-50,
// `clip_grad_norm_(params, cfg.grad_norm)` + `optimizer.step()` with torch.optim.SGD(lr, momentum, weight_decay)).
// torch runs these as ~10 foreach / elementwise launches over the 64 parameter tensors (about 0.15 ms per step, nothing else
// on the GPU meanwhile); here a descriptor table {param, grad, momentum buffer, elements} per tensor feeds one grid.
// SGD arithmetic in torch's order, element for element:
//   coef = min(1, max_norm / (total_norm + 1e-6));  g = grad * coef;  g = g + wd * p;  buf = mom * buf + g;  p = p - lr * buf
// (a zero-initialised buffer reproduces torch's first step, where buf = g).  total_norm is read from device memory (the L2
// norm of the flat gradient buffer, computed by the caller), so the step stays capturable in a hipGraph.
//
// How the file is put together (every piece exists once):
//   sgd_one / adamw_one / ema_one   one element of a rule, torch's order (-ffp-contract=off: equal values, equal bits)
//   Lanes<W>, ld<W>, st<W>          W = 4: one 16-byte quad, W = 1: one float; a rule writes its element body once, as at<W>(i)
//   SgdRule<EMA>, AdamwRule<EMA>,   the streams of one tensor and the scalars of the step; at<W>(i) loads the streams, calls the
//   SwapRule                        element expression per lane and stores m, then v, then p, then e
//   chunk_walk                      one workgroup, one chunk of SQD_SGD_CHUNK elements: chunk end, alignment test, quads, scalar tail
//   clip_coef                       the clip coefficient from the partials of sqd_grad_sumsq, from a device scalar, or 1
//   the kernels                     read their descriptor and scalars, build a rule, call chunk_walk (sgd_clip_batched_kernel:
//                                   its own grid-stride ranges over the same SgdRule)
#include "sqd_common.h"

#define SQD_NORM_PARTS 256      // partial sums of squares of the flat gradient (sqd_grad_sumsq), summed in index order by every workgroup of the step
#define SQD_SGD_CHUNK 4096      // elements of one tensor that a workgroup of a chunked launch handles

struct SgdDesc { float* p; long long g; float* m; long long n; };      // g: element offset into g_base, or an address when g_base is null
struct OptDesc { float* p; long long g; float* m; long long n; float* v; float* e; };      // SgdDesc widened by the second moment and the EMA

// One element of the SGD step, torch's order.  The ONE source expression of every SGD kernel below.
__device__ __forceinline__ void sgd_one(float p, float gr, float m, float coef, float wd, float momentum, float lr, float& pn, float& mn) {
  float g = gr * coef;
  g = g + wd * p;
  mn = momentum * m + g;
  pn = p - lr * mn;
}

// One element of the AdamW step, torch's order.  The ONE source expression of every instantiation.
__device__ __forceinline__ void adamw_one(float p, float gr, float m, float v, float coef, float lrwd, float b1, float omb1, float b2,
                                          float omb2, float eps, float step, float rbc2, float& pn, float& mn, float& vn) {
  const float g = gr * coef;
  const float pd = p - lrwd * p;
  mn = b1 * m + omb1 * g;
  vn = b2 * v + omb2 * (g * g);
  const float den = sqrtf(vn) * rbc2 + eps;
  pn = pd - step * (mn / den);
}

// One element of the EMA (the first averaged step copies, later ones lerp).  The ONE source expression, as above.
__device__ __forceinline__ float ema_one(float e, float pn, float omd, bool copy) { return copy ? pn : e + omd * (pn - e); }

// W consecutive floats of a stream: unit i of a W-wide walk (W = 4: 16-byte accesses, the base must be 16-byte aligned).
template <int W> struct Lanes {
  float v[W];
  __device__ __forceinline__ float& operator[](int k) { return v[k]; }
  __device__ __forceinline__ float operator[](int k) const { return v[k]; }
};
template <int W> __device__ __forceinline__ Lanes<W> ld(const float* base, long long i) {
  if constexpr (W == 4) { const f32x4 q = ((const f32x4*)base)[i]; return {{q[0], q[1], q[2], q[3]}}; }
  else return {{base[i]}};
}
template <int W> __device__ __forceinline__ void st(float* base, long long i, const Lanes<W>& x) {
  if constexpr (W == 4) ((f32x4*)base)[i] = (f32x4){x[0], x[1], x[2], x[3]};
  else base[i] = x[0];
}

// The walk of a chunked launch: this workgroup's chunk is [e0, min(e0 + SQD_SGD_CHUNK, n)) of one tensor (chunk origins are
// multiples of 4 elements).  16-byte accesses where every stream allows it (align_bits: the OR of their addresses; they do for
// every tensor of the model), else -- and for the last n & 3 elements -- scalar.
template <class Rule>
__device__ __forceinline__ void chunk_walk(long long e0, long long n, uintptr_t align_bits, const Rule& rule) {
  const long long e1 = (e0 + SQD_SGD_CHUNK < n) ? e0 + SQD_SGD_CHUNK : n;
  const long long q0 = e0 >> 2, q1 = (align_bits & 15) == 0 ? (e1 >> 2) : q0;
  for (long long i = q0 + threadIdx.x; i < q1; i += 256) rule.template at<4>(i);
  for (long long i = 4 * q1 + threadIdx.x; i < e1; i += 256) rule.template at<1>(i);
}

// The clip coefficient min(1, max_norm / (norm + 1e-6)) from the partials of sqd_grad_sumsq (every wave evaluates it for itself:
// lane l adds parts l, l + 64, ..., then a shuffle tree, then the root; norm_out, or NULL, receives the norm from the first
// thread of the launch's first workgroup row) or from a device scalar holding the norm (separate gradients).  Whether the norm
// is evaluated at all is structural: with neither given the step does not clip, whatever max_norm says.
__device__ __forceinline__ float clip_coef(const float* __restrict__ parts, const float* __restrict__ total_norm, float max_norm,
                                           float* __restrict__ norm_out) {
  if (!(max_norm > 0.f) || (!parts && !total_norm)) return 1.f;
  float tn;
  if (parts) {
    const int lane = threadIdx.x & 63;
    float ssum = 0.f;
    for (int i = lane; i < SQD_NORM_PARTS; i += 64) ssum += parts[i];
    for (int off = 32; off >= 1; off >>= 1) ssum += __shfl_xor(ssum, off);
    tn = sqrtf(ssum);
    if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) *norm_out = tn;
  } else {
    tn = *total_norm;
  }
  const float coef = max_norm / (tn + 1e-6f);
  return coef < 1.f ? coef : 1.f;
}

// ---- the rules ----
template <bool EMA> struct SgdRule {
  float* p; const float* g; float* m; float* e;
  float coef, wd, momentum, lr, omd; bool copy;
  __device__ __forceinline__ uintptr_t align_bits() const { return (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (EMA ? (uintptr_t)e : 0); }
  template <int W> __device__ __forceinline__ void at(long long i) const {
    const Lanes<W> pv = ld<W>(p, i), gv = ld<W>(g, i), mv = ld<W>(m, i);
    Lanes<W> ev, pn, mn;
    if (EMA) ev = ld<W>(e, i);
#pragma unroll
    for (int k = 0; k < W; ++k) sgd_one(pv[k], gv[k], mv[k], coef, wd, momentum, lr, pn[k], mn[k]);
    st<W>(m, i, mn); st<W>(p, i, pn);
    if (EMA) {
#pragma unroll
      for (int k = 0; k < W; ++k) ev[k] = ema_one(ev[k], pn[k], omd, copy);
      st<W>(e, i, ev);
    }
  }
};

template <bool EMA> struct AdamwRule {
  float* p; const float* g; float* m; float* v; float* e;
  float coef, lrwd, b1, omb1, b2, omb2, eps, step, rbc2, omd; bool copy;
  __device__ __forceinline__ uintptr_t align_bits() const { return (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (EMA ? (uintptr_t)e : 0); }
  template <int W> __device__ __forceinline__ void at(long long i) const {
    const Lanes<W> pv = ld<W>(p, i), gv = ld<W>(g, i), mv = ld<W>(m, i), vv = ld<W>(v, i);
    Lanes<W> pn, mn, vn;
#pragma unroll
    for (int k = 0; k < W; ++k) adamw_one(pv[k], gv[k], mv[k], vv[k], coef, lrwd, b1, omb1, b2, omb2, eps, step, rbc2, pn[k], mn[k], vn[k]);
    st<W>(m, i, mn); st<W>(v, i, vn); st<W>(p, i, pn);
    if (EMA) {                                   // (read behind the stores: the fresh parameter is still in a register)
      Lanes<W> ev = ld<W>(e, i);
#pragma unroll
      for (int k = 0; k < W; ++k) ev[k] = ema_one(ev[k], pn[k], omd, copy);
      st<W>(e, i, ev);
    }
  }
};

// p <-> e, exactly.
struct SwapRule {
  float* p; float* e;
  __device__ __forceinline__ uintptr_t align_bits() const { return (uintptr_t)p | (uintptr_t)e; }
  template <int W> __device__ __forceinline__ void at(long long i) const {
    const Lanes<W> pv = ld<W>(p, i), ev = ld<W>(e, i);
    st<W>(p, i, ev); st<W>(e, i, pv);
  }
};

// A descriptor's gradient stream: an offset into the flat buffer, or an address of its own.
template <class Desc> __device__ __forceinline__ const float* grad_of(const Desc& d, const float* g_base) {
  return g_base ? g_base + d.g : (const float*)d.g;
}

// ---- SGD, a fixed number of workgroups per tensor: grid (blocks_per_desc, tensors), grid-stride ranges over the SGD rule ----
// total_norm: norm_parts > 0: the partials of sqd_grad_sumsq; 0: a device scalar holding the norm (or NULL: no clipping).
__global__ __launch_bounds__(256) void sgd_clip_batched_kernel(const SgdDesc* __restrict__ descs, const float* __restrict__ g_base,
                                                               const float* __restrict__ total_norm, float max_norm, float lr, float momentum,
                                                               float wd, int norm_parts, float* __restrict__ norm_out) {
  const SgdDesc d = descs[blockIdx.y];
  const float coef = clip_coef(norm_parts > 0 ? total_norm : nullptr, norm_parts > 0 ? nullptr : total_norm, max_norm,
                               blockIdx.y == 0 ? norm_out : nullptr);
  const SgdRule<false> rule = {d.p, grad_of(d, g_base), d.m, nullptr, coef, wd, momentum, lr, 0.f, false};
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n4 = (rule.align_bits() & 15) == 0 ? d.n >> 2 : 0;
  for (long long i = tid; i < n4; i += stride) rule.at<4>(i);
  for (long long i = 4 * n4 + tid; i < d.n; i += stride) rule.at<1>(i);
}

// ---- SGD with the work dealt in equal CHUNKS instead of a fixed number of workgroups per tensor (the 64 tensors of the model span
// 16 to 500 k elements: 64 workgroups each left the large ones 8 serial rounds and the small ones 63 idle workgroups -- 47 us for 42 MB).
// chunks: device array of [nchunks][2] int64 = {tensor, first element}; a workgroup handles SQD_SGD_CHUNK elements of one tensor.
// The three kernels below are this one body: hyper-parameters as launch arguments, read from a device table, and that with the EMA.
template <bool EMA, class Desc>
__device__ __forceinline__ void sgd_clip_chunk(const Desc* __restrict__ descs, const long long* __restrict__ chunks,
                                               const float* __restrict__ g_base, const float* __restrict__ parts, float max_norm,
                                               float lr, float momentum, float wd, const float* __restrict__ derived,
                                               float* __restrict__ norm_out) {
  const long long tensor = chunks[2 * blockIdx.x], e0 = chunks[2 * blockIdx.x + 1];
  const Desc d = descs[tensor];
  float* e = nullptr;
  if constexpr (EMA) e = d.e;
  const float omd = EMA ? derived[2] : 0.f;                                              // (every scalar load in front of the norm's)
  const bool copy = EMA && derived[3] != 0.f;
  const SgdRule<EMA> rule = {d.p, grad_of(d, g_base), d.m, e, clip_coef(parts, nullptr, max_norm, norm_out), wd, momentum, lr, omd, copy};
  chunk_walk(e0, d.n, rule.align_bits(), rule);
}

__global__ __launch_bounds__(256) void sgd_clip_chunked_kernel(const SgdDesc* __restrict__ descs, const long long* __restrict__ chunks,
                                                               const float* __restrict__ g_base, const float* __restrict__ parts, float max_norm,
                                                               float lr, float momentum, float wd, float* __restrict__ norm_out) {
  sgd_clip_chunk<false>(descs, chunks, g_base, parts, max_norm, lr, momentum, wd, nullptr, norm_out);
}

// The hyper-parameters read from DEVICE memory: hyper = {lr, momentum, weight_decay, max_norm}, read by every workgroup.  A captured
// step (hipGraph) then follows a learning-rate schedule without a re-capture: the table is rewritten in front of a replay
// (sqd_fill_f32x4).  Without parts the step does not clip, whatever hyper[3] says (clip_coef).
__global__ __launch_bounds__(256) void sgd_clip_chunked_dev_kernel(const SgdDesc* __restrict__ descs, const long long* __restrict__ chunks,
                                                                   const float* __restrict__ g_base, const float* __restrict__ parts,
                                                                   const float* __restrict__ hyper, float* __restrict__ norm_out) {
  sgd_clip_chunk<false>(descs, chunks, g_base, parts, hyper[3], hyper[0], hyper[1], hyper[2], nullptr, norm_out);
}

// The same with the EMA behind it: 6-word descriptors, hyper[0..3] as above, derived[2..3] = {1 - d_t, copy flag} (see below).
__global__ __launch_bounds__(256) void sgd_clip_chunked_ema_kernel(const OptDesc* __restrict__ descs, const long long* __restrict__ chunks,
                                                                   const float* __restrict__ g_base, const float* __restrict__ parts,
                                                                   const float* __restrict__ hyper, const float* __restrict__ derived,
                                                                   float* __restrict__ norm_out) {
  sgd_clip_chunk<true>(descs, chunks, g_base, parts, hyper[3], hyper[0], hyper[1], hyper[2], derived, norm_out);
}

// hyper[0..4) = {a, b, c, d}: one thread.  The values travel as launch arguments (no staging buffer that a later call could overwrite
// while a copy is still in flight).
__global__ void fill_f32x4_kernel(float* __restrict__ dst, float a, float b, float c, float d) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { dst[0] = a; dst[1] = b; dst[2] = c; dst[3] = d; }
}

extern "C" int sqd_fill_f32x4(float* dst, float a, float b, float c, float d, void* stream) {
  SQD_CHECK_ARG(dst);
  hipLaunchKernelGGL(fill_f32x4_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, dst, a, b, c, d);
  return sqd_launch_status();
}

extern "C" int sqd_sgd_chunk_elems(void) { return SQD_SGD_CHUNK; }

// sqd_sgd_clip_step_chunked with hyper_dev = DEVICE float[4] {lr, momentum, weight_decay, max_norm}; sumsq_parts NULL = no clipping.
extern "C" int sqd_sgd_clip_step_chunked_dev(const void* descs_dev, const void* chunks_dev, int nchunks, const float* grad_base,
                                             const float* sumsq_parts, float* norm_out, const float* hyper_dev, void* stream) {
  SQD_CHECK_ARG(descs_dev && chunks_dev && nchunks > 0 && hyper_dev);
  hipLaunchKernelGGL(sgd_clip_chunked_dev_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, (const SgdDesc*)descs_dev,
                     (const long long*)chunks_dev, grad_base, sumsq_parts, hyper_dev, norm_out);
  return sqd_launch_status();
}

// descs_dev as for sqd_sgd_clip_step; chunks_dev: [nchunks][2] int64 {tensor index, first element (a multiple of sqd_sgd_chunk_elems())}
// covering every tensor; sumsq_parts / norm_out as for sqd_sgd_clip_step_parts (sumsq_parts may be NULL when max_norm <= 0).
extern "C" int sqd_sgd_clip_step_chunked(const void* descs_dev, const void* chunks_dev, int nchunks, const float* grad_base,
                                         const float* sumsq_parts, float* norm_out, float max_norm, float lr, float momentum,
                                         float weight_decay, void* stream) {
  SQD_CHECK_ARG(descs_dev && chunks_dev && nchunks > 0 && (sumsq_parts || max_norm <= 0.f));
  hipLaunchKernelGGL(sgd_clip_chunked_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, (const SgdDesc*)descs_dev,
                     (const long long*)chunks_dev, grad_base, sumsq_parts, max_norm, lr, momentum, weight_decay, norm_out);
  return sqd_launch_status();
}

// descs_dev: device array of n records of 4 int64 {param ptr, grad, momentum ptr, elements}; grad = element offset into grad_base (the
// flat gradient buffer the backward writes: the table then never changes, only this one pointer does) or, with grad_base NULL, the
// gradient's address; total_norm: device float (may be NULL when max_norm <= 0 = no clipping).
extern "C" int sqd_sgd_clip_step(const void* descs_dev, int n, const float* grad_base, const float* total_norm, float max_norm, float lr,
                                 float momentum, float weight_decay, int blocks_per_desc, void* stream) {
  SQD_CHECK_ARG(descs_dev && n > 0 && n <= 65535 && blocks_per_desc > 0 && blocks_per_desc <= 4096 && (total_norm || max_norm <= 0.f));
  hipLaunchKernelGGL(sgd_clip_batched_kernel, dim3((unsigned)blocks_per_desc, (unsigned)n), dim3(256), 0, (hipStream_t)stream,
                     (const SgdDesc*)descs_dev, grad_base, total_norm, max_norm, lr, momentum, weight_decay, 0, (float*)nullptr);
  return sqd_launch_status();
}

// ---- the gradient norm of clip_grad_norm_ (src/engine/trainer.py:49) without a torch reduction kernel ----
// sqd_grad_sumsq: parts[i] = sum of squares of block i of the flat gradient (SQD_NORM_PARTS equal blocks; within a block a fixed
// tree: bitwise reproducible).  sqd_sgd_clip_step_parts: the step above with total_norm = sqrt(sum of those partials in index order),
// evaluated redundantly by every workgroup; norm_out (or NULL) receives the norm for logging.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long long n, float* __restrict__ parts) {
  // blocks of whole 16-byte quads (the flat buffer is 16-byte aligned: checked by the launcher); the tail rides in the last block
  const long long nq = n >> 2;
  const long long per = (nq + SQD_NORM_PARTS - 1) / SQD_NORM_PARTS;
  const long long lo = (long long)blockIdx.x * per, hi = (lo + per < nq) ? lo + per : nq;
  float acc = 0.f;
  for (long long i = lo + threadIdx.x; i < hi; i += 256) {
    const f32x4 v = ((const f32x4*)g)[i];
    acc += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
  }
  if (blockIdx.x == SQD_NORM_PARTS - 1 && threadIdx.x < (n & 3)) { const float v = g[4 * nq + threadIdx.x]; acc += v * v; }
  __shared__ float red[256];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) parts[blockIdx.x] = red[0];
}

extern "C" int sqd_grad_sumsq(const float* grad_flat, long long n, float* parts, void* stream) {
  SQD_CHECK_ARG(grad_flat && parts && n > 0 && ((uintptr_t)grad_flat & 15) == 0);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(SQD_NORM_PARTS), dim3(256), 0, (hipStream_t)stream, grad_flat, n, parts);
  return sqd_launch_status();
}

extern "C" int sqd_grad_sumsq_parts(void) { return SQD_NORM_PARTS; }

extern "C" int sqd_sgd_clip_step_parts(const void* descs_dev, int n, const float* grad_base, const float* sumsq_parts, float* norm_out,
                                       float max_norm, float lr, float momentum, float weight_decay, int blocks_per_desc, void* stream) {
  SQD_CHECK_ARG(descs_dev && n > 0 && n <= 65535 && blocks_per_desc > 0 && blocks_per_desc <= 4096 && sumsq_parts && max_norm > 0.f);
  hipLaunchKernelGGL(sgd_clip_batched_kernel, dim3((unsigned)blocks_per_desc, (unsigned)n), dim3(256), 0, (hipStream_t)stream,
                     (const SgdDesc*)descs_dev, grad_base, sumsq_parts, max_norm, lr, momentum, weight_decay, SQD_NORM_PARTS, norm_out);
  return sqd_launch_status();
}

// ---- the element-wise steps of the data-parallel gradient exchange (exchange.GradientExchange) without a torch kernel ----
// The reference's DataParallel (src/utils/data_parallel.py:93-113) gathers the per-sample losses and differentiates their mean
// (src/engine/trainer.py:43,47); one process per GPU gets the same gradient as sum_r(B_r * g_r) / sum_r(B_r).  g[0..n) = g * mul /
// (*div_by if given); fill_ptr (or NULL) receives fill_value: the rank's image count that rides through the same all-reduce.
__global__ __launch_bounds__(256) void grad_scale_kernel(float* __restrict__ g, long long n, float mul, const float* __restrict__ div_by,
                                                         float* __restrict__ fill_ptr, float fill_value) {
  if (fill_ptr && blockIdx.x == 0 && threadIdx.x == 0) *fill_ptr = fill_value;
  const float d = div_by ? *div_by : 1.f;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float v = g[i] * mul;
    g[i] = div_by ? v / d : v;                 // a true division: the same rounding as torch's div_ by the summed count
  }
}

extern "C" int sqd_grad_scale(float* g, long long n, float mul, const float* div_by, float* fill_ptr, float fill_value, void* stream) {
  SQD_CHECK_ARG(n >= 0 && (g || n == 0) && (n > 0 || fill_ptr));
  SQD_CHECK_ARG(!fill_ptr || !g || fill_ptr < g || fill_ptr >= g + n);          // the slot is not part of the scaled range
  long long blocks = (n + 1023) / 1024;
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, n, mul, div_by, fill_ptr, fill_value);
  return sqd_launch_status();
}

// ---- the training log on the device (graph_step.GraphedStep): per-epoch sums and a ring of batch means, no host sync per iteration ----
// losses: float[4][B], the loss launches' per-image values.  For each component k: s = the B values added in index order in float64;
// sums[k] += s; ring[(cursor % cap)][k] = (float)(s / B).  sums[4] += B; cursor += 1.  ONE workgroup, so the read-modify-writes need no
// atomics; thread k adds component k, thread 0 stores.
__global__ __launch_bounds__(64) void train_log_push_kernel(const float* __restrict__ losses, int B, double* __restrict__ sums,
                                                            float* __restrict__ ring, unsigned* __restrict__ cursor, int cap) {
  __shared__ double s[4];
  if (threadIdx.x < 4) {
    double acc = 0.0;
    for (int b = 0; b < B; ++b) acc += (double)losses[(long long)threadIdx.x * B + b];
    s[threadIdx.x] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned c = *cursor;
    float* slot = ring + 4ll * (c % (unsigned)cap);
    for (int k = 0; k < 4; ++k) {
      sums[k] += s[k];
      slot[k] = (float)(s[k] / (double)B);
    }
    sums[4] += (double)B;
    *cursor = c + 1u;
  }
}

extern "C" int sqd_train_log_push(const float* losses, int B, double* sums, float* ring, unsigned* cursor, int cap, void* stream) {
  SQD_CHECK_ARG(losses && sums && ring && cursor && B > 0 && cap > 0);
  hipLaunchKernelGGL(train_log_push_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, losses, B, sums, ring, cursor, cap);
  return sqd_launch_status();
}

// ---- AdamW and a weight EMA in the same one-launch form (optim.FusedClipAdamW, FusedClipSGD(ema_decay > 0)) ----
// torch.optim.AdamW (non-amsgrad, decoupled decay) behind clip_grad_norm_, and the exponential moving average of
// torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d)), as more rules on the chunked walk: the step
// streams p, grad, m (and v), and the EMA adds one read and one write while the fresh parameter is still in a register.
//   g = grad * coef;  p = p - (lr * wd) * p;  m = b1 * m + (1 - b1) * g;  v = b2 * v + (1 - b2) * (g * g)
//   den = sqrt(v) * (1 / sqrt(bc2)) + eps;  p = p - (lr / bc1) * (m / den);  e = first averaged step ? p : e + (1 - d_t) * (p - e)
// The step count t (bias corrections bc1 = 1 - b1^t, bc2 = 1 - b2^t) and the number of averaged steps n (warm-up:
// d_t = min(d, (1 + n) / (10 + n))) live in DEVICE memory: a replayed hipGraph advances them without a host write.  A one-thread
// launch in front of every step (optim_begin_kernel) increments them and leaves lr / bc1, 1 / sqrt(bc2), 1 - d_t (evaluated in
// double from the float hyper table) and the copy flag in a derived table; the big launch only reads that table, so no workgroup
// reads a counter that another workgroup of its launch writes.
//   hyper (float[8], always on the device: one form, one set of bits):
//     AdamW {lr, beta1, beta2, eps | weight_decay, max_norm, ema_decay, ema_warmup};  SGD {lr, momentum, weight_decay, max_norm |
//     ema_decay, ema_warmup, -, -} (the first four as sgd_clip_chunked_dev_kernel reads them)
//   counters (int[2]) {t, n};  derived (float[4]) {lr / bc1, 1 / sqrt(bc2), 1 - d_t, first averaged step ? 1 : 0}
__global__ void optim_begin_kernel(const float* __restrict__ hyper, int* __restrict__ counters, float* __restrict__ derived, int adam, int ema) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (adam) {
    const int t = counters[0] + 1;
    counters[0] = t;
    const double bc1 = 1.0 - pow((double)hyper[1], (double)t), bc2 = 1.0 - pow((double)hyper[2], (double)t);
    derived[0] = (float)((double)hyper[0] / bc1);
    derived[1] = (float)(1.0 / sqrt(bc2));
  }
  if (ema) {
    const int n = counters[1];
    const float* eh = adam ? hyper + 6 : hyper + 4;
    double d = (double)eh[0];
    if (eh[1] != 0.f) { const double w = (1.0 + (double)n) / (10.0 + (double)n); d = d < w ? d : w; }
    derived[2] = (float)(1.0 - d);
    derived[3] = n == 0 ? 1.f : 0.f;
    counters[1] = n + 1;
  }
}

extern "C" int sqd_optim_begin(const float* hyper_dev, int* counters_dev, float* derived_dev, int adam, int ema, void* stream) {
  SQD_CHECK_ARG(hyper_dev && counters_dev && derived_dev && (adam == 0 || adam == 1) && (ema == 0 || ema == 1) && (adam || ema));
  hipLaunchKernelGGL(optim_begin_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, hyper_dev, counters_dev, derived_dev, adam, ema);
  return sqd_launch_status();
}

template <bool EMA>
__global__ __launch_bounds__(256) void adamw_clip_chunked_kernel(const OptDesc* __restrict__ descs, const long long* __restrict__ chunks,
                                                                 const float* __restrict__ g_base, const float* __restrict__ parts,
                                                                 const float* __restrict__ total_norm, const float* __restrict__ hyper,
                                                                 const float* __restrict__ derived, float* __restrict__ norm_out) {
  const long long tensor = chunks[2 * blockIdx.x], e0 = chunks[2 * blockIdx.x + 1];
  const OptDesc d = descs[tensor];
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4];
  const float step = derived[0], rbc2 = derived[1], omd = EMA ? derived[2] : 0.f;       // (every scalar load in front of the norm's)
  const bool copy = EMA && derived[3] != 0.f;
  const AdamwRule<EMA> rule = {d.p, grad_of(d, g_base), d.m, d.v, d.e, clip_coef(parts, total_norm, hyper[5], norm_out),
                               lr * wd, b1, 1.f - b1, b2, 1.f - b2, eps, step, rbc2, omd, copy};
  chunk_walk(e0, d.n, rule.align_bits(), rule);
}

// descs_dev: n records of 6 int64 {param ptr, grad (offset into grad_base, or an address when grad_base is NULL), exp_avg ptr, elements,
// exp_avg_sq ptr, EMA ptr (read only when ema)}; chunks_dev as for sqd_sgd_clip_step_chunked.  The clip: sumsq_parts (the partials of
// sqd_grad_sumsq), else total_norm (a device float holding the norm), else none -- structural, as in sqd_sgd_clip_step_chunked_dev.
extern "C" int sqd_adamw_clip_step_chunked(const void* descs_dev, const void* chunks_dev, int nchunks, const float* grad_base,
                                           const float* sumsq_parts, const float* total_norm, float* norm_out, const float* hyper_dev,
                                           const float* derived_dev, int ema, void* stream) {
  SQD_CHECK_ARG(descs_dev && chunks_dev && nchunks > 0 && hyper_dev && derived_dev && (ema == 0 || ema == 1));
  hipLaunchKernelGGL(ema ? adamw_clip_chunked_kernel<true> : adamw_clip_chunked_kernel<false>, dim3((unsigned)nchunks), dim3(256), 0,
                     (hipStream_t)stream, (const OptDesc*)descs_dev, (const long long*)chunks_dev, grad_base, sumsq_parts, total_norm,
                     hyper_dev, derived_dev, norm_out);
  return sqd_launch_status();
}

// sqd_sgd_clip_step_chunked_dev with the EMA: descs_dev in the 6-word form (exp_avg_sq unused), hyper_dev float[8], derived_dev as
// written by sqd_optim_begin(adam = 0, ema = 1).
extern "C" int sqd_sgd_clip_step_chunked_ema(const void* descs_dev, const void* chunks_dev, int nchunks, const float* grad_base,
                                             const float* sumsq_parts, float* norm_out, const float* hyper_dev, const float* derived_dev,
                                             void* stream) {
  SQD_CHECK_ARG(descs_dev && chunks_dev && nchunks > 0 && hyper_dev && derived_dev);
  hipLaunchKernelGGL(sgd_clip_chunked_ema_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, (const OptDesc*)descs_dev,
                     (const long long*)chunks_dev, grad_base, sumsq_parts, hyper_dev, derived_dev, norm_out);
  return sqd_launch_status();
}

// p <-> e over the same tables, exactly (optimizer.averaged_weights()).
__global__ __launch_bounds__(256) void param_swap_kernel(const OptDesc* __restrict__ descs, const long long* __restrict__ chunks) {
  const long long tensor = chunks[2 * blockIdx.x], e0 = chunks[2 * blockIdx.x + 1];
  const OptDesc d = descs[tensor];
  const SwapRule rule = {d.p, d.e};
  chunk_walk(e0, d.n, rule.align_bits(), rule);
}

extern "C" int sqd_param_swap(const void* descs_dev, const void* chunks_dev, int nchunks, void* stream) {
  SQD_CHECK_ARG(descs_dev && chunks_dev && nchunks > 0);
  hipLaunchKernelGGL(param_swap_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, (const OptDesc*)descs_dev,
                     (const long long*)chunks_dev);
  return sqd_launch_status();
}
