// enf_cg.hip -- enf_cg_update (include/enf_hip.h, "Gauss-Newton product"): one conjugate-gradient step for B independent systems in
// one launch.  The Gauss-Newton matrix of a fit is block diagonal over the signals, so a solve is B separate CG iterations with
// per-signal alpha, beta and damping; the vectors are the latent components (p, a, sigma), each (B, Z, width) fp32.
// One workgroup per signal.  Every dot product over all segments is a fixed strided slice per thread plus a fixed LDS tree (the pattern
// of enf_signal_sum_kernel): same inputs, same bits; no atomics, no scratch memory, any Z * width.
#include <hip/hip_runtime.h>
#include <math.h>
#include "enf_launch.h"

namespace {
constexpr int CG_TH = 256;
struct CgArgs {
  EnfCgSegment s[3];
  int nseg, Z;
  const float* lam;
  float* rho;
};

// the workgroup's sum of `v` in a fixed order; every thread gets it
__device__ __forceinline__ float cg_block_sum(float v, float* red) {
  const int tid = threadIdx.x;
  __syncthreads();                       // (the previous sum's readers are done with red)
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = CG_TH / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}
__device__ __forceinline__ bool cg_live(float v) { return v > 0.f && v <= 3.402823466e38f; }      // a finite positive number (NaN fails)

__global__ __launch_bounds__(CG_TH) void enf_cg_update_kernel(CgArgs A) {
  __shared__ float red[CG_TH];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (!A.s[0].q) {                       // INIT: x = 0, d = r, rho = r . r
    float acc = 0.f;
    for (int k = 0; k < A.nseg; ++k) {
      const size_t n = (size_t)A.Z * A.s[k].width, base = (size_t)b * n;
      for (size_t i = tid; i < n; i += CG_TH) {
        const float r = A.s[k].r[base + i];
        A.s[k].x[base + i] = 0.f;
        A.s[k].d[base + i] = r;
        acc = fmaf(r, r, acc);
      }
    }
    const float rho = cg_block_sum(acc, red);
    if (tid == 0) A.rho[b] = rho;
    return;
  }
  const float lam = A.lam ? A.lam[b] : 0.f, rho = A.rho[b];
  float acc = 0.f;
  for (int k = 0; k < A.nseg; ++k) {     // kappa = d . (q + lam d)
    const size_t n = (size_t)A.Z * A.s[k].width, base = (size_t)b * n;
    for (size_t i = tid; i < n; i += CG_TH) {
      const float d = A.s[k].d[base + i];
      acc = fmaf(d, fmaf(lam, d, A.s[k].q[base + i]), acc);
    }
  }
  const float kappa = cg_block_sum(acc, red);
  // a frozen signal (converged, a zero right-hand side, or a numerically indefinite matrix) keeps x, r, d and rho exactly
  if (!cg_live(rho) || !cg_live(kappa)) return;      // (uniform over the workgroup)
  const float alpha = rho / kappa;
  acc = 0.f;
  for (int k = 0; k < A.nseg; ++k) {     // x += alpha d, r -= alpha q', rho' = r . r
    const size_t n = (size_t)A.Z * A.s[k].width, base = (size_t)b * n;
    for (size_t i = tid; i < n; i += CG_TH) {
      const float d = A.s[k].d[base + i];
      const float qd = fmaf(lam, d, A.s[k].q[base + i]);
      const float r = fmaf(-alpha, qd, A.s[k].r[base + i]);
      A.s[k].x[base + i] = fmaf(alpha, d, A.s[k].x[base + i]);
      A.s[k].r[base + i] = r;
      acc = fmaf(r, r, acc);
    }
  }
  const float rho2 = cg_block_sum(acc, red);
  const float beta = rho2 / rho;
  for (int k = 0; k < A.nseg; ++k) {     // d = r + beta d   (every thread re-reads what it wrote itself)
    const size_t n = (size_t)A.Z * A.s[k].width, base = (size_t)b * n;
    for (size_t i = tid; i < n; i += CG_TH) A.s[k].d[base + i] = fmaf(beta, A.s[k].d[base + i], A.s[k].r[base + i]);
  }
  if (tid == 0) A.rho[b] = rho2;
}
}  // namespace

extern "C" int enf_cg_update(int nseg, const EnfCgSegment* segs, int32_t B, int32_t Z, const float* lam, float* rho, void* stream) {
  if (nseg < 1 || nseg > 3 || !segs || B <= 0 || Z <= 0 || !rho) return ENF_EINVAL;
  CgArgs A;
  for (int k = 0; k < nseg; ++k) {
    const EnfCgSegment& s = segs[k];
    if (!s.x || !s.r || !s.d || s.width <= 0 || (s.q == nullptr) != (segs[0].q == nullptr)) return ENF_EINVAL;
    A.s[k] = s;
  }
  for (int k = nseg; k < 3; ++k) A.s[k] = segs[0];
  A.nseg = nseg; A.Z = Z; A.lam = lam; A.rho = rho;
  hipLaunchKernelGGL(enf_cg_update_kernel, dim3(B), dim3(CG_TH), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? ENF_OK : ENF_ELAUNCH;
}
