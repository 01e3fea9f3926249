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

// weight != nullptr: one loss weight per group of O consecutive elements (per signal and query point; include/enf_hip.h, "Weighted
// loss"): s += w d^2, dout *= w; a point of weight 0 does not exist -- its target is never used in arithmetic and its dout is 0.0f.
__global__ __launch_bounds__(256) void enf_mse_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                      const float* __restrict__ weight, size_t n, int O, float inv_n, float gscale,
                                                      float* __restrict__ dout, float* loss, float* __restrict__ part) {
  __shared__ float red[4];
  float s = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float d;
    if (weight) {          // (uniform over the launch; the unweighted arithmetic stays as it was)
      const float w = weight[i / (size_t)O];
      const float dd = w > 0.f ? out[i] - target[i] : 0.f;
      d = w * dd;
      s = fmaf(d, dd, s);
    } else {
      d = out[i] - target[i];
      s = fmaf(d, d, s);
    }
    if (dout) dout[i] = 2.0f * d * inv_n * gscale;
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float v = (red[0] + red[1] + red[2] + red[3]) * inv_n;
    if (part) part[blockIdx.x] = v;
    else atomicAdd(loss, v);
  }
}

// One weight per ELEMENT (include/enf_hip.h, "Weighted loss": per-channel weights): s += w d^2, dout = 2 w d inv_n gscale; an element
// of weight 0 does not exist -- its target is never used in arithmetic and its dout is 0.0f.  A kernel of its own: the one above keeps
// its code.  Same grid, same partials, same reduction.
__global__ __launch_bounds__(256) void enf_mse_cw_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                         const float* __restrict__ cweight, size_t n, float inv_n, float gscale,
                                                         float* __restrict__ dout, float* loss, float* __restrict__ part) {
  __shared__ float red[4];
  float s = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float w = cweight[i];
    const float dd = w > 0.f ? out[i] - target[i] : 0.f;
    const float d = w * dd;
    s = fmaf(d, dd, s);
    if (dout) dout[i] = 2.0f * d * inv_n * gscale;
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float v = (red[0] + red[1] + red[2] + red[3]) * inv_n;
    if (part) part[blockIdx.x] = v;
    else atomicAdd(loss, v);
  }
}

// The shared-latent backward's loss (enf_layout.h: enf_shared_backward_rule): every signal's output is the ONE row out1 (N values, one
// channel), so element i = b N + n compares out1[n] with target[i].  The arithmetic per element, the partial sums and the one atomic
// per block are enf_mse_kernel's; dout (B, N) is the only per-signal quantity the shared backward pair kernel reads.
__global__ __launch_bounds__(256) void enf_mse_shared_kernel(const float* __restrict__ out1, const float* __restrict__ target,
                                                             const float* __restrict__ weight, size_t n, int N, float inv_n, float gscale,
                                                             float* __restrict__ dout, float* loss) {
  __shared__ float red[4];
  float s = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float o = out1[i % (size_t)N];
    float d;
    if (weight) {
      const float w = weight[i];
      const float dd = w > 0.f ? o - target[i] : 0.f;
      d = w * dd;
      s = fmaf(d, dd, s);
    } else {
      d = o - target[i];
      s = fmaf(d, d, s);
    }
    dout[i] = 2.0f * d * inv_n * gscale;
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(loss, (red[0] + red[1] + red[2] + red[3]) * inv_n);
}

int enf_launch_mse_shared(const float* out1, const float* target, const float* weight, int B, int N, float gscale, float* dout,
                          float* loss, hipStream_t st) {
  const size_t n = (size_t)B * (size_t)N;
  const size_t blocks = (n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256;
  hipLaunchKernelGGL(enf_mse_shared_kernel, dim3((unsigned)blocks), dim3(256), 0, st, out1, target, weight, n, N, 1.0f / (float)n, gscale,
                     dout, loss);
  return hipGetLastError() == hipSuccess ? ENF_OK : ENF_ELAUNCH;
}

// *loss += part[0] + ... + part[n - 1]: thread t adds part[t], part[t + 256], ... in order, then a fixed tree over the 256 threads.
// The order depends on n alone, never on which workgroup of the producing kernel finished first.
__global__ __launch_bounds__(256) void enf_loss_sum_kernel(const float* __restrict__ part, int n, float* loss) {
  __shared__ float red[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss += red[0];
}

int enf_launch_loss_sum(const float* part, int n, float* loss, hipStream_t st) {
  hipLaunchKernelGGL(enf_loss_sum_kernel, dim3(1), dim3(256), 0, st, part, n, loss);
  return hipGetLastError() == hipSuccess ? ENF_OK : ENF_ELAUNCH;
}

// loss_b[b] = scale * sum_n err[b, n] (include/enf_hip.h, "Per-signal and per-point errors"; scale = 1 / (N O)): one workgroup per signal.
// Thread t adds err[b, t], err[b, t + 256], ... in order, then the fixed tree of enf_loss_sum_kernel over the 256 threads: the order
// depends on N alone -- same inputs, same bits, in every mode.  No atomics, no scratch; N < 256 leaves zeros in the tree.  64-bit offsets.
__global__ __launch_bounds__(256) void enf_signal_sum_kernel(const float* __restrict__ err, int N, float scale, float* __restrict__ loss_b) {
  __shared__ float red[256];
  const float* __restrict__ row = err + (size_t)blockIdx.x * (size_t)N;
  float s = 0.f;
  for (int i = threadIdx.x; i < N; i += 256) s += row[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss_b[blockIdx.x] = red[0] * scale;
}

int enf_launch_signal_sum(const float* err, int B, int N, float scale, float* loss_b, hipStream_t st) {
  hipLaunchKernelGGL(enf_signal_sum_kernel, dim3((unsigned)B), dim3(256), 0, st, err, N, scale, loss_b);
  return hipGetLastError() == hipSuccess ? ENF_OK : ENF_ELAUNCH;
}

extern "C" int enf_signal_sum(const float* err, int32_t B, int32_t N, float scale, float* loss_b, void* stream) {
  if (!err || !loss_b || B < 1 || N < 1) return ENF_EINVAL;
  return enf_launch_signal_sum(err, B, N, scale, loss_b, (hipStream_t)stream);
}

static size_t mse_blocks(size_t n) {
  const size_t blocks = (n + 255) / 256;
  return blocks > 1024 ? 1024 : blocks;
}

extern "C" size_t enf_mse_scratch_bytes(size_t n, unsigned flags) {
  if (n == 0 || (flags & ~ENF_MSE_DETERMINISTIC)) return 0;
  return (flags & ENF_MSE_DETERMINISTIC) ? enf_align(sizeof(float) * mse_blocks(n)) : 0;
}

extern "C" int enf_mse_value_grad_w(const float* out, const float* target, const float* weight, size_t n, int32_t O, float grad_scale,
                                    float* dout, float* loss, void* scratch, size_t scratch_bytes, unsigned flags, void* stream) {
  if (!out || !target || !loss || n == 0 || O < 1 || n % (size_t)O != 0 || (flags & ~ENF_MSE_DETERMINISTIC)) return ENF_EINVAL;
  const bool det = (flags & ENF_MSE_DETERMINISTIC) != 0;
  if (det && !scratch) return ENF_EINVAL;
  if (det && scratch_bytes < enf_mse_scratch_bytes(n, flags)) return ENF_EWORKSPACE;
  const size_t blocks = mse_blocks(n);
  float* part = det ? (float*)scratch : nullptr;
  hipLaunchKernelGGL(enf_mse_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, out, target, weight, n, (int)O,
                     1.0f / (float)n, grad_scale, dout, loss, part);
  if (hipGetLastError() != hipSuccess) return ENF_ELAUNCH;
  return det ? enf_launch_loss_sum(part, (int)blocks, loss, (hipStream_t)stream) : ENF_OK;
}

extern "C" int enf_mse_value_grad_cw(const float* out, const float* target, const float* cweight, size_t n, float grad_scale, float* dout,
                                     float* loss, void* scratch, size_t scratch_bytes, unsigned flags, void* stream) {
  if (!out || !target || !cweight || !loss || n == 0 || (flags & ~ENF_MSE_DETERMINISTIC)) return ENF_EINVAL;
  const bool det = (flags & ENF_MSE_DETERMINISTIC) != 0;
  if (det && !scratch) return ENF_EINVAL;
  if (det && scratch_bytes < enf_mse_scratch_bytes(n, flags)) return ENF_EWORKSPACE;
  const size_t blocks = mse_blocks(n);
  float* part = det ? (float*)scratch : nullptr;
  hipLaunchKernelGGL(enf_mse_cw_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, out, target, cweight, n, 1.0f / (float)n,
                     grad_scale, dout, loss, part);
  if (hipGetLastError() != hipSuccess) return ENF_ELAUNCH;
  return det ? enf_launch_loss_sum(part, (int)blocks, loss, (hipStream_t)stream) : ENF_OK;
}

extern "C" int enf_mse_value_grad_ex(const float* out, const float* target, size_t n, float grad_scale, float* dout, float* loss,
                                     void* scratch, size_t scratch_bytes, unsigned flags, void* stream) {
  return enf_mse_value_grad_w(out, target, nullptr, n, 1, grad_scale, dout, loss, scratch, scratch_bytes, flags, stream);
}

extern "C" int enf_mse_value_grad(const float* out, const float* target, size_t n, float grad_scale, float* dout, float* loss,
                                  void* stream) {
  return enf_mse_value_grad_ex(out, target, n, grad_scale, dout, loss, nullptr, 0, 0u, stream);
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

// enf_fit_inputs: the inner loop's setup in one launch (include/enf_hip.h) -- broadcast of the latent initialisation over the signals,
// gather of the S + 1 sampled coordinate / target sets, zeroed loss accumulators.  One flat index space over the five outputs.
struct FitInArgs {
  EnfFitComponent comp[ENF_SGD_MAX_SEGMENTS];
  int ncomp, B, Z, N, Ns, S1, dx, O;
  const float* coords; const float* img; const int64_t* masks;
  float* xs; float* ys; float* losses;
  const float* weight; float* ws;      // both or neither: the loss weights (B, N) and their gather (S1, B, Ns)
                                       // (enf_fit_inputs_cw: per-channel weights (B, N, O) and their gather (S1, B, Ns, O))
};

__global__ __launch_bounds__(256) void enf_fit_inputs_kernel(FitInArgs A) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
  for (int k = 0; k < ENF_SGD_MAX_SEGMENTS; ++k) {
    if (k < A.ncomp) {
      const int64_t per = (int64_t)A.Z * A.comp[k].width, n = per * A.B;
      if (i < n) { A.comp[k].dst[i] = A.comp[k].src[i % per]; return; }
      i -= n;
    }
  }
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
}

extern "C" int enf_fit_inputs(int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t N, int32_t Ns, int32_t S1, int32_t dx,
                              int32_t O, const float* coords, const float* img, const int64_t* masks, float* xs, float* ys, float* losses,
                              void* stream) {
  return enf_fit_inputs_w(ncomp, comps, B, Z, N, Ns, S1, dx, O, coords, img, masks, xs, ys, losses, nullptr, nullptr, stream);
}

extern "C" int enf_fit_inputs_w(int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t N, int32_t Ns, int32_t S1, int32_t dx,
                                int32_t O, const float* coords, const float* img, const int64_t* masks, float* xs, float* ys,
                                float* losses, const float* weight, float* ws, void* stream) {
  if (ncomp < 1 || ncomp > ENF_SGD_MAX_SEGMENTS || !comps || !coords || !img || !masks || !xs || !ys || !losses) return ENF_EINVAL;
  if ((weight == nullptr) != (ws == nullptr)) return ENF_EINVAL;
  if (B < 1 || Z < 1 || N < 1 || Ns < 1 || S1 < 1 || dx < 1 || O < 1) return ENF_EDIM;
  FitInArgs A{};
  int64_t total = 0;
  for (int k = 0; k < ncomp; ++k) {
    if (!comps[k].src || !comps[k].dst || comps[k].width < 1) return ENF_EINVAL;
    A.comp[k] = comps[k];
    total += (int64_t)B * Z * comps[k].width;
  }
  A.ncomp = ncomp; A.B = B; A.Z = Z; A.N = N; A.Ns = Ns; A.S1 = S1; A.dx = dx; A.O = O;
  A.coords = coords; A.img = img; A.masks = masks; A.xs = xs; A.ys = ys; A.losses = losses; A.weight = weight; A.ws = ws;
  total += (int64_t)S1 * Ns * dx + (int64_t)S1 * B * Ns * O + (weight ? (int64_t)S1 * B * Ns : 0) + S1;
  hipLaunchKernelGGL(enf_fit_inputs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? ENF_OK : ENF_ELAUNCH;
}

// enf_fit_inputs_b: the same setup for PER-SIGNAL index sets, masks (B, Ns, S1) (include/enf_hip.h).  A kernel of its own, so that the
// shared-mask kernel above keeps its code object.  One thread per (s, b, i) row of the outputs: it reads its index once and copies the
// dx coordinates, the O target values and the weight of that point; consecutive threads write consecutive rows of xs, ys and ws.  The
// threads after the rows broadcast the latent components and zero the loss accumulators.  An index outside [0, N) is never used as an
// offset: its row is coords[0], zero targets and weight 0 -- by the weighted-loss contract the point does not exist.
__global__ __launch_bounds__(256) void enf_fit_inputs_b_kernel(FitInArgs A) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nrow = (int64_t)A.S1 * A.B * A.Ns;
  if (i < nrow) {
    const int64_t q = i % A.Ns, r = i / A.Ns, b = r % A.B, s = r / A.B;
    const int64_t m = A.masks[(b * A.Ns + q) * A.S1 + s];
    const bool ok = m >= 0 && m < (int64_t)A.N;
    const float* __restrict__ cx = A.coords + (ok ? m : (int64_t)0) * A.dx;
    float* __restrict__ x = A.xs + i * A.dx;
    for (int c = 0; c < A.dx; ++c) x[c] = cx[c];
    float* __restrict__ y = A.ys + i * A.O;
    if (ok) {
      const float* __restrict__ im = A.img + (b * A.N + m) * A.O;
      for (int o = 0; o < A.O; ++o) y[o] = im[o];
      if (A.ws) A.ws[i] = A.weight ? A.weight[b * A.N + m] : 1.0f;
    } else {
      for (int o = 0; o < A.O; ++o) y[o] = 0.f;
      if (A.ws) A.ws[i] = 0.f;
    }
    return;
  }
  i -= nrow;
#pragma unroll
  for (int k = 0; k < ENF_SGD_MAX_SEGMENTS; ++k) {
    if (k < A.ncomp) {
      const int64_t per = (int64_t)A.Z * A.comp[k].width, n = per * A.B;
      if (i < n) { A.comp[k].dst[i] = A.comp[k].src[i % per]; return; }
      i -= n;
    }
  }
  if (i < A.S1) A.losses[i] = 0.f;
}

extern "C" int enf_fit_inputs_b(int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t N, int32_t Ns, int32_t S1, int32_t dx,
                                int32_t O, const float* coords, const float* img, const int64_t* masks, float* xs, float* ys,
                                float* losses, const float* weight, float* ws, void* stream) {
  if (ncomp < 1 || ncomp > ENF_SGD_MAX_SEGMENTS || !comps || !coords || !img || !masks || !xs || !ys || !losses) return ENF_EINVAL;
  if (!ws) return ENF_EINVAL;      // ws is what says that an index outside [0, N) does not exist; without weight it is 1 / 0
  if (B < 1 || Z < 1 || N < 1 || Ns < 1 || S1 < 1 || dx < 1 || O < 1) return ENF_EDIM;
  FitInArgs A{};
  int64_t total = (int64_t)S1 * B * Ns + S1;
  for (int k = 0; k < ncomp; ++k) {
    if (!comps[k].src || !comps[k].dst || comps[k].width < 1) return ENF_EINVAL;
    A.comp[k] = comps[k];
    total += (int64_t)B * Z * comps[k].width;
  }
  if ((total + 255) / 256 > (int64_t)INT_MAX) return ENF_EDIM;
  A.ncomp = ncomp; A.B = B; A.Z = Z; A.N = N; A.Ns = Ns; A.S1 = S1; A.dx = dx; A.O = O;
  A.coords = coords; A.img = img; A.masks = masks; A.xs = xs; A.ys = ys; A.losses = losses; A.weight = weight; A.ws = ws;
  hipLaunchKernelGGL(enf_fit_inputs_b_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? ENF_OK : ENF_ELAUNCH;
}

// enf_fit_inputs_cw: the setup with PER-CHANNEL loss weights, cweight (B, N, O) -> ws (S1, B, Ns, O), for both mask layouts
// (include/enf_hip.h).  A kernel of its own beside the two above.  One thread per (s, b, i) row of ys / ws, as in enf_fit_inputs_b: it
// reads its index once and copies the O targets and the O weights of that point; with per-signal masks also its row of xs, with shared
// masks the threads of signal 0 write xs (S1, Ns, dx).  The index contract of enf_fit_inputs_b holds for both layouts: an index outside
// [0, N) is never used as an offset, its row is coords[0], O zero targets and O zero weights.  All offsets are 64-bit.
__global__ __launch_bounds__(256) void enf_fit_inputs_cw_kernel(FitInArgs A, int per_signal) {
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
    float* __restrict__ y = A.ys + i * A.O;
    float* __restrict__ w = A.ws + i * A.O;
    if (ok) {
      const float* __restrict__ im = A.img + (b * A.N + m) * A.O;
      const float* __restrict__ cw = A.weight + (b * A.N + m) * A.O;
      for (int o = 0; o < A.O; ++o) { y[o] = im[o]; w[o] = cw[o]; }
    } else {
      for (int o = 0; o < A.O; ++o) { y[o] = 0.f; w[o] = 0.f; }
    }
    return;
  }
  i -= nrow;
#pragma unroll
  for (int k = 0; k < ENF_SGD_MAX_SEGMENTS; ++k) {
    if (k < A.ncomp) {
      const int64_t per = (int64_t)A.Z * A.comp[k].width, n = per * A.B;
      if (i < n) { A.comp[k].dst[i] = A.comp[k].src[i % per]; return; }
      i -= n;
    }
  }
  if (i < A.S1) A.losses[i] = 0.f;
}

extern "C" int enf_fit_inputs_cw(int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t N, int32_t Ns, int32_t S1, int32_t dx,
                                 int32_t O, const float* coords, const float* img, const int64_t* masks, float* xs, float* ys,
                                 float* losses, const float* cweight, float* ws, int32_t per_signal_masks, void* stream) {
  if (ncomp < 1 || ncomp > ENF_SGD_MAX_SEGMENTS || !comps || !coords || !img || !masks || !xs || !ys || !losses) return ENF_EINVAL;
  if (!cweight || !ws) return ENF_EINVAL;
  if (B < 1 || Z < 1 || N < 1 || Ns < 1 || S1 < 1 || dx < 1 || O < 1) return ENF_EDIM;
  FitInArgs A{};
  int64_t total = (int64_t)S1 * B * Ns + S1;
  for (int k = 0; k < ncomp; ++k) {
    if (!comps[k].src || !comps[k].dst || comps[k].width < 1) return ENF_EINVAL;
    A.comp[k] = comps[k];
    total += (int64_t)B * Z * comps[k].width;
  }
  if ((total + 255) / 256 > (int64_t)INT_MAX) return ENF_EDIM;
  A.ncomp = ncomp; A.B = B; A.Z = Z; A.N = N; A.Ns = Ns; A.S1 = S1; A.dx = dx; A.O = O;
  A.coords = coords; A.img = img; A.masks = masks; A.xs = xs; A.ys = ys; A.losses = losses; A.weight = cweight; A.ws = ws;
  hipLaunchKernelGGL(enf_fit_inputs_cw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A,
                     per_signal_masks != 0 ? 1 : 0);
  return hipGetLastError() == hipSuccess ? ENF_OK : ENF_ELAUNCH;
}
