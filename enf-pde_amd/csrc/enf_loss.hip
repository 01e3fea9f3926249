// enf_loss.hip -- the inner loop's reconstruction loss and its gradient in one pass.
//   loss = mean((out - target)^2)          (pde_trainer.py:185)
//   dout = 2 (out - target) / n * grad_scale
// optionally with one weight per signal and point on the squared error (enf_mse_value_grad_w),
// so that a fit step is forward -> this kernel -> backward, without a framework autograd graph of tiny
// elementwise kernels in between.  `loss` is accumulated with one atomic per block: the caller zeroes it.  Deterministic mode
// (enf_mse_value_grad_ex with ENF_MSE_DETERMINISTIC; the fused tail of enf_fit_step_ex): the blocks / waves STORE their partials in
// scratch and enf_loss_sum_kernel, one workgroup, adds them in index order -- same inputs, same bits.
//
// enf_meta_sgd_update: the meta-SGD update of every latent component in ONE launch (pde_trainer.py:206-219):
//   out_k = x_k - lr_k (scale g_k),   scale = the batch size (the gradient of a batch-mean loss, :206)
#include <hip/hip_runtime.h>
#include "enf_launch.h"

// The block's sum of the threads' `s`, times inv_n: stored in part[block] (deterministic mode) or added to *loss with one atomic.
__device__ __forceinline__ void mse_block_sum(float s, float inv_n, float* loss, float* __restrict__ part) {
  __shared__ float red[4];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float v = (red[0] + red[1] + red[2] + red[3]) * inv_n;
    if (part) part[blockIdx.x] = v;
    else atomicAdd(loss, v);
  }
}

// The one MSE kernel.  WF, the weight form (include/enf_hip.h, "Weighted loss"): none; one weight per group of `m` = O consecutive
// elements (per signal and query point); one weight per element (per-channel weights).  Weighted: s += w d^2, dout = 2 w d inv_n gscale;
// an element of weight 0 does not exist -- its target is never used in arithmetic and its dout is 0.0f.
// SHARED, the shared-latent backward's loss (enf_layout.h: enf_shared_backward_rule): every signal's output is the ONE row `out` of
// `m` = N values (one channel), so element i = b N + n compares out[n] with target[i]; dout (B, N) is the only per-signal quantity
// the shared backward pair kernel reads.
enum { MSE_W_NONE = 0, MSE_W_GROUP = 1, MSE_W_ELEMENT = 2 };
template <int WF, bool SHARED>
__global__ __launch_bounds__(256) void enf_mse_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                      const float* __restrict__ weight, size_t n, int m, float inv_n, float gscale,
                                                      float* __restrict__ dout, float* loss, float* __restrict__ part) {
  float s = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float o = out[SHARED ? i % (size_t)m : i];
    float d;
    if constexpr (WF != MSE_W_NONE) {
      const float w = weight[WF == MSE_W_GROUP ? i / (size_t)m : i];
      const float dd = w > 0.f ? o - target[i] : 0.f;
      d = w * dd;
      s = fmaf(d, dd, s);
    } else {
      d = o - target[i];
      s = fmaf(d, d, s);
    }
    if (dout) dout[i] = 2.0f * d * inv_n * gscale;
  }
  mse_block_sum(s, inv_n, loss, part);
}
using MseKernel = decltype(&enf_mse_kernel<MSE_W_NONE, false>);

// red[0] of thread 0 = row[0] + ... + row[n - 1]: thread t adds row[t], row[t + 256], ... in order, then a fixed tree over the 256
// threads.  The order depends on n alone -- same inputs, same bits; n < 256 leaves zeros in the tree.
__device__ __forceinline__ float sum256(const float* __restrict__ row, int n) {
  __shared__ float red[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += row[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// *loss += part[0] + ... + part[n - 1] in the order of sum256: never in the order in which the producing kernel's workgroups finished.
__global__ __launch_bounds__(256) void enf_loss_sum_kernel(const float* __restrict__ part, int n, float* loss) {
  const float t = sum256(part, n);
  if (threadIdx.x == 0) *loss += t;
}
int enf_launch_loss_sum(const float* part, int n, float* loss, hipStream_t st) {
  hipLaunchKernelGGL(enf_loss_sum_kernel, dim3(1), dim3(256), 0, st, part, n, loss);
  return hipGetLastError() == hipSuccess ? ENF_OK : ENF_ELAUNCH;
}

// loss_b[b] = scale * sum_n err[b, n] (include/enf_hip.h, "Per-signal and per-point errors"; scale = 1 / (N O)): one workgroup per signal,
// the order of sum256 in every mode.  No atomics, no scratch.  64-bit offsets.
__global__ __launch_bounds__(256) void enf_signal_sum_kernel(const float* __restrict__ err, int N, float scale, float* __restrict__ loss_b) {
  const float t = sum256(err + (size_t)blockIdx.x * (size_t)N, N);
  if (threadIdx.x == 0) loss_b[blockIdx.x] = t * scale;
}
int enf_launch_signal_sum(const float* err, int B, int N, float scale, float* loss_b, hipStream_t st) {
  hipLaunchKernelGGL(enf_signal_sum_kernel, dim3((unsigned)B), dim3(256), 0, st, err, N, scale, loss_b);
  return hipGetLastError() == hipSuccess ? ENF_OK : ENF_ELAUNCH;
}

extern "C" int enf_signal_sum(const float* err, int32_t B, int32_t N, float scale, float* loss_b, void* stream) {
  if (!err || !loss_b || B < 1 || N < 1) return ENF_EINVAL;
  return enf_launch_signal_sum(err, B, N, scale, loss_b, (hipStream_t)stream);
}

static size_t mse_blocks(size_t n) { return n > 1024 * 256 ? 1024 : (n + 255) / 256; }
extern "C" size_t enf_mse_scratch_bytes(size_t n, unsigned flags) {
  if (n == 0 || (flags & ~ENF_MSE_DETERMINISTIC)) return 0;
  return (flags & ENF_MSE_DETERMINISTIC) ? enf_align(sizeof(float) * mse_blocks(n)) : 0;
}

// Every MSE launch: validation (`args_ok`: the entry point's own condition), scratch check, grid, kernel, deterministic sum of the partials.
static int mse_launch(MseKernel kern, bool args_ok, const float* out, const float* target, const float* weight, size_t n, int m,
                      float grad_scale, float* dout, float* loss, void* scratch, size_t scratch_bytes, unsigned flags, hipStream_t st) {
  if (!args_ok || !out || !target || !loss || n == 0 || (flags & ~ENF_MSE_DETERMINISTIC)) return ENF_EINVAL;
  const bool det = (flags & ENF_MSE_DETERMINISTIC) != 0;
  if (det && !scratch) return ENF_EINVAL;
  if (det && scratch_bytes < enf_mse_scratch_bytes(n, flags)) return ENF_EWORKSPACE;
  const size_t blocks = mse_blocks(n);
  float* part = det ? (float*)scratch : nullptr;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, st, out, target, weight, n, m, 1.0f / (float)n, grad_scale, dout, loss, part);
  if (hipGetLastError() != hipSuccess) return ENF_ELAUNCH;
  return det ? enf_launch_loss_sum(part, (int)blocks, loss, st) : ENF_OK;
}

int enf_launch_mse_shared(const float* out1, const float* target, const float* weight, int B, int N, float gscale, float* dout,
                          float* loss, hipStream_t st) {
  return mse_launch(weight ? enf_mse_kernel<MSE_W_ELEMENT, true> : enf_mse_kernel<MSE_W_NONE, true>, true, out1, target, weight,
                    (size_t)B * (size_t)N, N, gscale, dout, loss, nullptr, 0, 0u, st);
}

extern "C" int enf_mse_value_grad_w(const float* out, const float* target, const float* weight, size_t n, int32_t O, float grad_scale,
                                    float* dout, float* loss, void* scratch, size_t scratch_bytes, unsigned flags, void* stream) {
  return mse_launch(weight ? enf_mse_kernel<MSE_W_GROUP, false> : enf_mse_kernel<MSE_W_NONE, false>, O >= 1 && n % (size_t)O == 0, out,
                    target, weight, n, (int)O, grad_scale, dout, loss, scratch, scratch_bytes, flags, (hipStream_t)stream);
}

extern "C" int enf_mse_value_grad_cw(const float* out, const float* target, const float* cweight, size_t n, float grad_scale, float* dout,
                                     float* loss, void* scratch, size_t scratch_bytes, unsigned flags, void* stream) {
  return mse_launch(enf_mse_kernel<MSE_W_ELEMENT, false>, cweight != nullptr, out, target, cweight, n, 1, grad_scale, dout, loss, scratch,
                    scratch_bytes, flags, (hipStream_t)stream);
}

extern "C" int enf_mse_value_grad_ex(const float* out, const float* target, size_t n, float grad_scale, float* dout, float* loss,
                                     void* scratch, size_t scratch_bytes, unsigned flags, void* stream) {
  return enf_mse_value_grad_w(out, target, nullptr, n, 1, grad_scale, dout, loss, scratch, scratch_bytes, flags, stream);
}
extern "C" int enf_mse_value_grad(const float* out, const float* target, size_t n, float grad_scale, float* dout, float* loss,
                                  void* stream) {
  return enf_mse_value_grad_ex(out, target, n, grad_scale, dout, loss, nullptr, 0, 0u, stream);
}

// The grouped form of enf_mse_kernel (include/enf_hip.h, "Grouped observations": enf_mse_value_grad_g): the loss of a decode `out`
// (B, N, O) that exists in memory against observations (B, M, O), M = N / G.  One thread owns one (group, channel) i = (b M + m) O + o:
// it forms obs = sum_k q out over the group's G consecutive rows, dd = obs - target under the select on w, its share w dd^2 of the loss,
// and stores the G values d out = (q (w dd)) gs, gs = 2 inv_n gscale -- the operations of the fused tail's tail_sq_err_g in its order.
// The group sum is the tail's xor tree written over registers: products first, then pairs at distance 1, 2, 4, 8 (rows beyond G are
// zeros, and x + 0 is x).  Contraction is off, so the sum's bits do not depend on what the compiler fuses.
// err_g (B, M): the thread of channel 0 adds its group's O shares in channel order with the products the other channels' threads form
// (it recomputes their sums): one plain store per observation, no atomics.
// SHARED (the shared-latent backward, enf_layout.h: enf_shared_backward_rule; O == 1): `out` is the ONE row of N values every signal
// decodes to and q (N, or NULL) are signal 0's factors; target, w and d out stay per signal.
// cweight (enf_mse_value_grad_gc; never with SHARED): one weight per observed value (B, M, O) in place of oweight -- the thread reads
// cweight[i], its own (group, channel), and the err_g thread every channel's own weight; the arithmetic is the same.
__device__ __forceinline__ float mse_group_sum(const float* __restrict__ out, const float* __restrict__ q, size_t orow, size_t qrow, int O,
                                               int o, int G) {
#pragma clang fp contract(off)
  float v[16];
  const float qd = 1.0f / (float)G;
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = k < G ? (q ? q[qrow + k] : qd) * out[(orow + k) * (size_t)O + o] : 0.f;
#pragma unroll
  for (int d = 1; d < 16; d <<= 1)
#pragma unroll
    for (int k = 0; k < 16; k += 2 * d) v[k] += v[k + d];
  return v[0];
}

template <bool SHARED>
__global__ __launch_bounds__(256) void enf_mse_group_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                            const float* __restrict__ qweight, const float* __restrict__ oweight,
                                                            const float* __restrict__ cweight, size_t n, int M, int O, int G, float inv_n, float gscale, float* __restrict__ dout,
                                                            float* __restrict__ err_g, float* loss, float* __restrict__ part) {
#pragma clang fp contract(off)
  const float gs = 2.0f * inv_n * gscale;
  float s = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t bm = i / (size_t)O;                     // the observation, b M + m
    const int o = (int)(i - bm * (size_t)O);
    const size_t row = bm * (size_t)G;                   // its first query row, b N + m G
    const size_t orow = SHARED ? row % ((size_t)M * G) : row;     // the row of `out` (and of q) it reads
    const float w = cweight ? cweight[i] : (oweight ? oweight[bm] : 1.f);
    const bool live = w > 0.f;
    const float dd = live ? mse_group_sum(out, qweight, orow, orow, O, o, G) - target[i] : 0.f;
    const float wd = w * dd;
    s = fmaf(wd, dd, s);
    if (dout) {
      const float qd = 1.0f / (float)G;
      for (int k = 0; k < G; ++k) dout[(row + k) * (size_t)O + o] = ((qweight ? qweight[orow + k] : qd) * wd) * gs;
    }
    if (err_g && o == 0) {
      float e = fmaf(wd, dd, 0.f);
      for (int c = 1; c < O; ++c) {
        const float wc = cweight ? cweight[i + c] : w;
        const float dc = wc > 0.f ? mse_group_sum(out, qweight, orow, orow, O, c, G) - target[i + c] : 0.f;
        e = fmaf(wc * dc, dc, e);
      }
      err_g[bm] = e;
    }
  }
  mse_block_sum(s, inv_n, loss, part);
}

// Every grouped MSE launch: n = B M O threads' worth of (group, channel) pairs on the grid of mse_launch, the deterministic sum behind it.
static int mse_group_launch(bool shared, const float* out, const float* target, const float* qweight, const float* oweight, int B, int N,
                            int O, int G, float grad_scale, float* dout, float* err_g, float* loss, void* scratch, size_t scratch_bytes,
                            unsigned flags, hipStream_t st, const float* cweight = nullptr, bool args_ok = true) {
  if (!args_ok || !out || !target || !loss || B < 1 || N < 1 || O < 1 || !enf_group_size_ok(G) || N % G || (flags & ~ENF_MSE_DETERMINISTIC)) return ENF_EINVAL;
  const int M = N / G;
  const size_t n = (size_t)B * (size_t)M * (size_t)O;
  const bool det = (flags & ENF_MSE_DETERMINISTIC) != 0;
  if (det && !scratch) return ENF_EINVAL;
  if (det && scratch_bytes < enf_mse_scratch_bytes(n, flags)) return ENF_EWORKSPACE;
  const size_t blocks = mse_blocks(n);
  float* part = det ? (float*)scratch : nullptr;
  const float inv_n = 1.0f / ((float)B * (float)M * (float)O);      // the fused tail's (enf_tail.hip: tail_loss_kernel)
  hipLaunchKernelGGL(shared ? enf_mse_group_kernel<true> : enf_mse_group_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, out, target,
                     qweight, oweight, cweight, n, M, O, G, inv_n, grad_scale, dout, err_g, loss, part);
  if (hipGetLastError() != hipSuccess) return ENF_ELAUNCH;
  return det ? enf_launch_loss_sum(part, (int)blocks, loss, st) : ENF_OK;
}

int enf_launch_mse_group_shared(const float* out1, const float* target, const float* q0, const float* oweight, int B, int N, int G,
                                float gscale, float* dout, float* loss, hipStream_t st) {
  return mse_group_launch(true, out1, target, q0, oweight, B, N, 1, G, gscale, dout, nullptr, loss, nullptr, 0, 0u, st);
}

extern "C" int enf_mse_value_grad_g(const float* out, const float* target, int32_t B, int32_t N, int32_t O, int32_t G, const float* qweight,
                                    const float* oweight, float grad_scale, float* dout, float* loss, float* err_g, void* scratch,
                                    size_t scratch_bytes, unsigned flags, void* stream) {
  return mse_group_launch(false, out, target, qweight, oweight, B, N, O, G, grad_scale, dout, err_g, loss, scratch, scratch_bytes, flags,
                          (hipStream_t)stream);
}

extern "C" int enf_mse_value_grad_gc(const float* out, const float* target, int32_t B, int32_t N, int32_t O, int32_t G, const float* qweight,
                                     const float* cweight_g, float grad_scale, float* dout, float* loss, float* err_g, void* scratch,
                                     size_t scratch_bytes, unsigned flags, void* stream) {
  return mse_group_launch(false, out, target, qweight, nullptr, B, N, O, G, grad_scale, dout, err_g, loss, scratch, scratch_bytes, flags,
                          (hipStream_t)stream, cweight_g, cweight_g != nullptr);
}

struct SgdArgs { EnfSgdSegment seg[ENF_SGD_MAX_SEGMENTS]; int nseg; float scale; };

__global__ __launch_bounds__(256) void enf_meta_sgd_kernel(SgdArgs A) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
  for (int k = 0; k < ENF_SGD_MAX_SEGMENTS; ++k) {
    if (k >= A.nseg) return;
    const EnfSgdSegment& S = A.seg[k];
    if (i < S.n) {
      const int64_t row = i / S.width;
      const int c = (int)(i - row * S.width);
      const float g = S.g[row * S.g_stride + c] * A.scale;          // :206
      S.out[i] = S.x[i] - S.lr[S.lr_len == 1 ? 0 : c] * g;         // :215-219
      return;
    }
    i -= S.n;
  }
}

extern "C" int enf_meta_sgd_update(int nseg, const EnfSgdSegment* segs, float scale, void* stream) {
  if (nseg < 1 || nseg > ENF_SGD_MAX_SEGMENTS || !segs) return ENF_EINVAL;
  SgdArgs A{};
  int64_t total = 0;
  for (int k = 0; k < nseg; ++k) {
    const EnfSgdSegment& S = segs[k];
    if (!S.x || !S.g || !S.lr || !S.out || S.n <= 0 || S.width <= 0 || S.g_stride < S.width || S.n % S.width != 0) return ENF_EINVAL;
    if (S.lr_len != 1 && S.lr_len != S.width) return ENF_EDIM;
    A.seg[k] = S;
    total += S.n;
  }
  A.nseg = nseg;
  A.scale = scale;
  hipLaunchKernelGGL(enf_meta_sgd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? ENF_OK : ENF_ELAUNCH;
}

// enf_fit_inputs*: the inner loop's setup in one launch (include/enf_hip.h) -- broadcast of the latent initialisation over the signals,
// gather of the S + 1 sampled coordinate / target (/ weight) sets, zeroed loss accumulators.
struct FitInArgs {
  EnfFitComponent comp[ENF_SGD_MAX_SEGMENTS];
  int ncomp, B, Z, N, Ns, S1, dx, O;
  const float* coords; const float* img; const int64_t* masks;
  float* xs; float* ys; float* losses;
  const float* weight; float* ws;      // the loss weights (B, N) and their gather (S1, B, Ns); per value: (B, N, O) and (S1, B, Ns, O)
};

// The latent broadcast, one thread per value of every component in component order; a thread behind them runs rest(i), i rebased.
template <class Rest> __device__ __forceinline__ void fit_broadcast_then(const FitInArgs& A, int64_t i, Rest rest) {
#pragma unroll
  for (int k = 0; k < ENF_SGD_MAX_SEGMENTS; ++k) {
    if (k < A.ncomp) {
      const int64_t per = (int64_t)A.Z * A.comp[k].width, n = per * A.B;
      if (i < n) { A.comp[k].dst[i] = A.comp[k].src[i % per]; return; }
      i -= n;
    }
  }
  rest(i);
}

// Shared masks (Ns, S1), at most one weight per point: one flat index space over the five outputs, one thread per ELEMENT.
__global__ __launch_bounds__(256) void enf_fit_inputs_kernel(FitInArgs A) {
  fit_broadcast_then(A, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, [&](int64_t i) {
    const int64_t nx = (int64_t)A.S1 * A.Ns * A.dx;
    if (i < nx) {                                   // xs[s][q][c] = coords[masks[q][s]][c]
      const int c = (int)(i % A.dx);
      const int64_t sq = i / A.dx, q = sq % A.Ns, s = sq / A.Ns;
      A.xs[i] = A.coords[A.masks[q * A.S1 + s] * A.dx + c];
      return;
    }
    i -= nx;
    const int64_t ny = (int64_t)A.S1 * A.B * A.Ns * A.O;
    if (i < ny) {                                   // ys[s][b][q][o] = img[b][masks[q][s]][o]
      const int o = (int)(i % A.O);
      int64_t r = i / A.O;
      const int64_t q = r % A.Ns; r /= A.Ns;
      const int64_t b = r % A.B, s = r / A.B;
      A.ys[i] = A.img[(b * A.N + A.masks[q * A.S1 + s]) * A.O + o];
      return;
    }
    i -= ny;
    if (A.weight) {                                 // ws[s][b][q] = weight[b][masks[q][s]]
      const int64_t nw = (int64_t)A.S1 * A.B * A.Ns;
      if (i < nw) {
        const int64_t q = i % A.Ns, r = i / A.Ns, b = r % A.B, s = r / A.B;
        A.ws[i] = A.weight[b * A.N + A.masks[q * A.S1 + s]];
        return;
      }
      i -= nw;
    }
    if (i < A.S1) A.losses[i] = 0.f;
  });
}

// Per-signal masks (B, Ns, S1) (enf_fit_inputs_b) and / or per-value weights (enf_fit_inputs_cw, both mask layouts): one thread per
// (s, b, i) ROW of the outputs.  It reads its index once and copies the O target values and the weight(s) of that point -- per_value: O
// weights, (B, N, O) -> (S1, B, Ns, O); otherwise one, and 1.0f without `weight` --; with per-signal masks also its row of xs, with shared
// masks the threads of signal 0 write xs (S1, Ns, dx).  Consecutive threads write consecutive rows.  The threads after the rows
// broadcast the latent components and zero the loss accumulators.  An index outside [0, N) is never used as an offset: its row is
// coords[0], zero targets and zero weight(s) -- by the weighted-loss contract the point does not exist.  All offsets are 64-bit.
enum { FIT_ROWS = 1, FIT_PER_VALUE = 2, FIT_PER_SIGNAL = 4 };      // the forms of a gather; without FIT_ROWS: enf_fit_inputs_kernel
__global__ __launch_bounds__(256) void enf_fit_inputs_rows_kernel(FitInArgs A, unsigned form) {
  const bool per_value = form & FIT_PER_VALUE, per_signal = form & FIT_PER_SIGNAL;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nrow = (int64_t)A.S1 * A.B * A.Ns;
  if (i < nrow) {
    const int64_t q = i % A.Ns, r = i / A.Ns, b = r % A.B, s = r / A.B;
    const int64_t m = A.masks[per_signal ? (b * A.Ns + q) * A.S1 + s : q * A.S1 + s];
    const bool ok = m >= 0 && m < (int64_t)A.N;
    if (per_signal || b == 0) {
      const float* __restrict__ cx = A.coords + (ok ? m : (int64_t)0) * A.dx;
      float* __restrict__ x = A.xs + (per_signal ? i : s * A.Ns + q) * A.dx;
      for (int c = 0; c < A.dx; ++c) x[c] = cx[c];
    }
    const int W = per_value ? A.O : 1;
    float* __restrict__ y = A.ys + i * A.O;
    float* __restrict__ w = A.ws + i * W;
    if (ok) {
      const float* __restrict__ im = A.img + (b * A.N + m) * A.O;
      for (int o = 0; o < A.O; ++o) y[o] = im[o];
      for (int o = 0; o < W; ++o) w[o] = A.weight ? A.weight[(b * A.N + m) * W + o] : 1.0f;
    } else {
      for (int o = 0; o < A.O; ++o) y[o] = 0.f;
      for (int o = 0; o < W; ++o) w[o] = 0.f;
    }
    return;
  }
  fit_broadcast_then(A, i - nrow, [&](int64_t j) { if (j < A.S1) A.losses[j] = 0.f; });
}

// Sampled CELLS (enf_fit_inputs_g; include/enf_hip.h, "Grouped observations"): A.N = M cells, A.Ns = Ms sampled ones, A.coords = the
// cells' quadrature points (M G, dx), A.img = the observations (B, M, O), A.weight = the observation weights (B, M) or NULL.  One thread
// per (s, b, i) OBSERVATION of the outputs, as in enf_fit_inputs_rows_kernel: it reads its cell index once, copies the O targets and the
// weight, and -- with per-signal masks every thread, with shared masks the threads of signal 0 -- the cell's G rows of points and
// factors: row i G + k of the set is row m G + k of cell m.  An index outside [0, M) is never used as an offset: its rows are cell 0's
// (finite: q is a factor, not a select), its targets zeros and its weight 0.  A.ws NULL (shared masks without weights): not written.
// per_value (enf_fit_inputs_gc): A.weight holds one weight per observed value, (B, M, O) -> A.ws (S1, B, Ms, O), as
// enf_fit_inputs_rows_kernel gathers them for points; an index outside [0, M) gives O zeros.  All offsets are 64-bit.
__global__ __launch_bounds__(256) void enf_fit_inputs_cells_kernel(FitInArgs A, int G, const float* __restrict__ q, float* __restrict__ qs,
                                                                   bool per_signal, bool per_value) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nrow = (int64_t)A.S1 * A.B * A.Ns;
  if (i < nrow) {
    const int64_t c = i % A.Ns, r = i / A.Ns, b = r % A.B, s = r / A.B;
    const int64_t m = A.masks[per_signal ? (b * A.Ns + c) * A.S1 + s : c * A.S1 + s];
    const bool ok = m >= 0 && m < (int64_t)A.N;
    if (per_signal || b == 0) {
      const int64_t src = (ok ? m : (int64_t)0) * G, dst = (per_signal ? i : s * A.Ns + c) * G;
      const int nx = G * A.dx;
      for (int k = 0; k < nx; ++k) A.xs[dst * A.dx + k] = A.coords[src * A.dx + k];
      if (q)
        for (int k = 0; k < G; ++k) qs[dst + k] = q[src + k];
    }
    float* __restrict__ y = A.ys + i * A.O;
    if (ok) {
      const float* __restrict__ im = A.img + (b * A.N + m) * A.O;
      for (int o = 0; o < A.O; ++o) y[o] = im[o];
    } else {
      for (int o = 0; o < A.O; ++o) y[o] = 0.f;
    }
    if (per_value) {
      float* __restrict__ w = A.ws + i * A.O;
      for (int o = 0; o < A.O; ++o) w[o] = ok ? A.weight[(b * A.N + m) * A.O + o] : 0.f;
    } else if (A.ws) A.ws[i] = ok ? (A.weight ? A.weight[b * A.N + m] : 1.0f) : 0.f;
    return;
  }
  fit_broadcast_then(A, i - nrow, [&](int64_t j) { if (j < A.S1) A.losses[j] = 0.f; });
}

// Both gathers of cells: validation, FitInArgs, grid and launch.  per_value: `oweight` is cweight_g (B, M, O) and ws (S1, B, Ms, O).
static int fit_inputs_cells_launch(bool per_value, int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t M, int32_t Ms, int32_t S1,
                                   int32_t G, int32_t dx, int32_t O, const float* xq, const float* q, const float* obs, const int64_t* masks,
                                   float* xs, float* qs, float* ys, float* losses, const float* oweight, float* ws, int32_t per_signal_masks,
                                   void* stream) {
  const bool per_signal = per_signal_masks != 0;
  if (ncomp < 1 || ncomp > ENF_SGD_MAX_SEGMENTS || !comps || !xq || !obs || !masks || !xs || !ys || !losses) return ENF_EINVAL;
  if (B < 1 || Z < 1 || M < 1 || Ms < 1 || S1 < 1 || dx < 1 || O < 1 || !enf_group_size_ok(G)) return ENF_EINVAL;
  if ((q == nullptr) != (qs == nullptr)) return ENF_EINVAL;
  // ws is what says that an index outside [0, M) does not exist: required with per-signal masks (1 / 0 without oweight)
  if (per_value ? !(oweight && ws) : (per_signal ? ws == nullptr : (oweight == nullptr) != (ws == nullptr))) return ENF_EINVAL;
  FitInArgs A{};
  int64_t total = (int64_t)S1 * B * Ms + S1;
  for (int k = 0; k < ncomp; ++k) {
    if (!comps[k].src || !comps[k].dst || comps[k].width < 1) return ENF_EINVAL;
    A.comp[k] = comps[k];
    total += (int64_t)B * Z * comps[k].width;
  }
  if ((total + 255) / 256 > (int64_t)INT_MAX) return ENF_EDIM;
  A.ncomp = ncomp; A.B = B; A.Z = Z; A.N = M; A.Ns = Ms; A.S1 = S1; A.dx = dx; A.O = O;
  A.coords = xq; A.img = obs; A.masks = masks; A.xs = xs; A.ys = ys; A.losses = losses; A.weight = oweight; A.ws = ws;
  hipLaunchKernelGGL(enf_fit_inputs_cells_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A, (int)G, q, qs,
                     per_signal, per_value);
  return hipGetLastError() == hipSuccess ? ENF_OK : ENF_ELAUNCH;
}

extern "C" int enf_fit_inputs_g(int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t M, int32_t Ms, int32_t S1, int32_t G,
                                int32_t dx, int32_t O, const float* xq, const float* q, const float* obs, const int64_t* masks, float* xs,
                                float* qs, float* ys, float* losses, const float* oweight, float* ws, int32_t per_signal_masks, void* stream) {
  return fit_inputs_cells_launch(false, ncomp, comps, B, Z, M, Ms, S1, G, dx, O, xq, q, obs, masks, xs, qs, ys, losses, oweight, ws,
                                 per_signal_masks, stream);
}
extern "C" int enf_fit_inputs_gc(int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t M, int32_t Ms, int32_t S1, int32_t G,
                                 int32_t dx, int32_t O, const float* xq, const float* q, const float* obs, const int64_t* masks, float* xs,
                                 float* qs, float* ys, float* losses, const float* cweight_g, float* ws, int32_t per_signal_masks,
                                 void* stream) {
  return fit_inputs_cells_launch(true, ncomp, comps, B, Z, M, Ms, S1, G, dx, O, xq, q, obs, masks, xs, qs, ys, losses, cweight_g, ws,
                                 per_signal_masks, stream);
}

// Every enf_fit_inputs* call: validation (`args_ok` is the entry point's own condition on weight / ws), FitInArgs, grid and launch.
static int fit_inputs_launch(unsigned form, bool args_ok, int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t N,
                             int32_t Ns, int32_t S1, int32_t dx, int32_t O, const float* coords, const float* img, const int64_t* masks,
                             float* xs, float* ys, float* losses, const float* weight, float* ws, void* stream) {
  if (ncomp < 1 || ncomp > ENF_SGD_MAX_SEGMENTS || !comps || !coords || !img || !masks || !xs || !ys || !losses || !args_ok) return ENF_EINVAL;
  if (B < 1 || Z < 1 || N < 1 || Ns < 1 || S1 < 1 || dx < 1 || O < 1) return ENF_EDIM;
  FitInArgs A{};
  const int64_t rows = (int64_t)S1 * B * Ns;
  int64_t total = S1 + ((form & FIT_ROWS) ? rows : (int64_t)S1 * Ns * dx + rows * O + (weight ? rows : 0));
  for (int k = 0; k < ncomp; ++k) {
    if (!comps[k].src || !comps[k].dst || comps[k].width < 1) return ENF_EINVAL;
    A.comp[k] = comps[k];
    total += (int64_t)B * Z * comps[k].width;
  }
  if ((total + 255) / 256 > (int64_t)INT_MAX) return ENF_EDIM;
  A.ncomp = ncomp; A.B = B; A.Z = Z; A.N = N; A.Ns = Ns; A.S1 = S1; A.dx = dx; A.O = O;
  A.coords = coords; A.img = img; A.masks = masks; A.xs = xs; A.ys = ys; A.losses = losses; A.weight = weight; A.ws = ws;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (form & FIT_ROWS) hipLaunchKernelGGL(enf_fit_inputs_rows_kernel, grid, dim3(256), 0, (hipStream_t)stream, A, form);
  else hipLaunchKernelGGL(enf_fit_inputs_kernel, grid, dim3(256), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? ENF_OK : ENF_ELAUNCH;
}

extern "C" int enf_fit_inputs(int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t N, int32_t Ns, int32_t S1, int32_t dx,
                              int32_t O, const float* coords, const float* img, const int64_t* masks, float* xs, float* ys, float* losses,
                              void* stream) {
  return enf_fit_inputs_w(ncomp, comps, B, Z, N, Ns, S1, dx, O, coords, img, masks, xs, ys, losses, nullptr, nullptr, stream);
}
extern "C" int enf_fit_inputs_w(int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t N, int32_t Ns, int32_t S1, int32_t dx,
                                int32_t O, const float* coords, const float* img, const int64_t* masks, float* xs, float* ys,
                                float* losses, const float* weight, float* ws, void* stream) {
  return fit_inputs_launch(0u, (weight == nullptr) == (ws == nullptr), ncomp, comps, B, Z, N, Ns, S1, dx, O, coords, img, masks, xs, ys,
                           losses, weight, ws, stream);
}

// ws is what says that an index outside [0, N) does not exist; without weight it is 1 / 0
extern "C" int enf_fit_inputs_b(int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t N, int32_t Ns, int32_t S1, int32_t dx,
                                int32_t O, const float* coords, const float* img, const int64_t* masks, float* xs, float* ys,
                                float* losses, const float* weight, float* ws, void* stream) {
  return fit_inputs_launch(FIT_ROWS | FIT_PER_SIGNAL, ws != nullptr, ncomp, comps, B, Z, N, Ns, S1, dx, O, coords, img, masks, xs, ys,
                           losses, weight, ws, stream);
}

extern "C" int enf_fit_inputs_cw(int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t N, int32_t Ns, int32_t S1, int32_t dx,
                                 int32_t O, const float* coords, const float* img, const int64_t* masks, float* xs, float* ys,
                                 float* losses, const float* cweight, float* ws, int32_t per_signal_masks, void* stream) {
  return fit_inputs_launch(FIT_ROWS | FIT_PER_VALUE | (per_signal_masks != 0 ? FIT_PER_SIGNAL : 0u), cweight && ws, ncomp, comps, B, Z, N,
                           Ns, S1, dx, O, coords, img, masks, xs, ys, losses, cweight, ws, stream);
}
