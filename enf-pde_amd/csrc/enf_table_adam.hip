// enf_table_adam.hip -- enf_table_adam_update: one optax adam step over every component of a latent table in ONE launch, straight
// from the gathered gradient rows a fit step returns (nonmaml_pde_trainer.py:125-126, 159-160: autodecoder_opt = optax.adam over
// the WHOLE table).  Per table element (s, z, c) of a component:
//     g   = sum over j with idx[j] == s of grad[(j, z, c)], in increasing j      (exact 0.0f when no j matches)
//     mu' = b1 mu + (1 - b1) g        nu' = b2 nu + (1 - b2) g g
//     x'  = x - lr (mu' / c1) / (sqrt(nu' / c2) + eps)                           c1 = 1 - b1^count, c2 = 1 - b2^count (the caller's)
// A row outside the batch has g = 0 and moves by its momentum alone, as a dense Adam does -- so every element of the table is
// read and written: a bandwidth kernel of seven streams (x, mu, nu in; x', mu', nu' out; the gradient rows are B of S).
// One thread owns one work unit -- an element, or four consecutive ones (16-byte loads and stores) where a component's width,
// gradient stride and pointers allow -- and scans the nidx batch indices itself: no atomics, no scratch, duplicate indices are
// summed in index order, and in-place use is safe because a unit's inputs are read by its own thread before it stores.  The
// index loads do not depend on the lane, so they go through the scalar cache; an index outside [0, S) equals no row and is
// never used as an offset.  Consecutive threads hold consecutive elements of a component (coalesced along c, then z, then s).
#include <hip/hip_runtime.h>
#include "enf_launch.h"

struct AdamArgs {
  EnfAdamSegment seg[ENF_ADAM_MAX_SEGMENTS];
  int64_t units[ENF_ADAM_MAX_SEGMENTS];   // work units of a segment: S Z width / vec
  int32_t vec[ENF_ADAM_MAX_SEGMENTS];     // elements per unit: 1 or 4
  int64_t total;                          // sum of units
  const int64_t* idx;                     // (nidx) table rows of the gradient's signals, or NULL: row j is table row j
  int32_t nseg, Z, nidx, wide;            // wide: some segment has 2^31 elements or more (64-bit index arithmetic)
  float lr, b1, b2, omb1, omb2, eps, c1, c2;
};

// element e of a (S, Z, width) component -> (s, z, c)
template <typename I>
__device__ __forceinline__ void adam_locate(I e, int width, int Z, int64_t& s, int& z, int& c) {
  const I row = e / (I)width;
  c = (int)(e - row * (I)width);
  const I ss = row / (I)Z;
  z = (int)(row - ss * (I)Z);
  s = (int64_t)ss;
}

__device__ __forceinline__ void adam_element(const AdamArgs& A, float x, float mu, float nu, float g, float& xo, float& muo, float& nuo) {
  muo = fmaf(A.b1, mu, A.omb1 * g);
  nuo = fmaf(A.b2, nu, A.omb2 * (g * g));
  xo = x - A.lr * (muo / A.c1) / (sqrtf(nuo / A.c2) + A.eps);
}

template <int V>
__device__ __forceinline__ void adam_unit(const AdamArgs& A, const EnfAdamSegment& S, int64_t unit) {
  typedef float vec_t __attribute__((ext_vector_type(V)));
  const int64_t e = unit * V;
  int64_t s;
  int z, c;
  if (A.wide) adam_locate<uint64_t>((uint64_t)e, S.width, A.Z, s, z, c);
  else adam_locate<uint32_t>((uint32_t)e, S.width, A.Z, s, z, c);
  vec_t g;
  if (A.idx) {
    g = (vec_t)(0.0f);
    // the constant address space: the loads are lane-independent and nothing in this kernel writes idx, so they are scalar loads
    const __attribute__((address_space(4))) int64_t* idx = (const __attribute__((address_space(4))) int64_t*)A.idx;
    for (int j = 0; j < A.nidx; ++j)
      if (idx[j] == s) g += *reinterpret_cast<const vec_t*>(S.g + ((int64_t)j * A.Z + z) * S.g_stride + c);
  } else {
    g = *reinterpret_cast<const vec_t*>(S.g + (s * A.Z + z) * S.g_stride + c);
  }
  const vec_t x = *reinterpret_cast<const vec_t*>(S.x + e);
  const vec_t mu = *reinterpret_cast<const vec_t*>(S.mu + e);
  const vec_t nu = *reinterpret_cast<const vec_t*>(S.nu + e);
  vec_t xo, muo, nuo;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    float a, b, d;
    adam_element(A, x[k], mu[k], nu[k], g[k], a, b, d);
    xo[k] = a; muo[k] = b; nuo[k] = d;
  }
  *reinterpret_cast<vec_t*>(S.x_out + e) = xo;
  *reinterpret_cast<vec_t*>(S.mu_out + e) = muo;
  *reinterpret_cast<vec_t*>(S.nu_out + e) = nuo;
}

__global__ __launch_bounds__(256) void enf_table_adam_kernel(AdamArgs A) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.total; i += step) {
    int64_t u = i;
    int k = 0;      // the segment of unit i; every A.seg[] below has a constant subscript, so the arguments stay in scalar registers
#pragma unroll
    for (int q = 0; q + 1 < ENF_ADAM_MAX_SEGMENTS; ++q)
      if (k == q && q + 1 < A.nseg && u >= A.units[q]) { u -= A.units[q]; k = q + 1; }
    switch (k) {
      case 0: if (A.vec[0] == 4) adam_unit<4>(A, A.seg[0], u); else adam_unit<1>(A, A.seg[0], u); break;
      case 1: if (A.vec[1] == 4) adam_unit<4>(A, A.seg[1], u); else adam_unit<1>(A, A.seg[1], u); break;
      case 2: if (A.vec[2] == 4) adam_unit<4>(A, A.seg[2], u); else adam_unit<1>(A, A.seg[2], u); break;
      default: if (A.vec[3] == 4) adam_unit<4>(A, A.seg[3], u); else adam_unit<1>(A, A.seg[3], u); break;
    }
  }
}

static bool adam_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

extern "C" int enf_table_adam_update(int nseg, const EnfAdamSegment* segs, int64_t S, int32_t Z, const int64_t* idx, int32_t nidx,
                                     float lr, float b1, float b2, float eps, float c1, float c2, void* stream) {
  if (nseg < 1 || nseg > ENF_ADAM_MAX_SEGMENTS || !segs || S < 1 || Z < 1 || nidx < 1) return ENF_EINVAL;
  if (!(c1 > 0.f) || !(c2 > 0.f)) return ENF_EINVAL;
  for (int k = 0; k < nseg; ++k) {
    const EnfAdamSegment& G = segs[k];
    if (!G.x || !G.mu || !G.nu || !G.g || !G.x_out || !G.mu_out || !G.nu_out || G.width < 1) return ENF_EINVAL;
  }
  if (!idx && (int64_t)nidx != S) return ENF_EDIM;
  AdamArgs A{};
  for (int k = 0; k < nseg; ++k) {
    const EnfAdamSegment& G = segs[k];
    if (G.g_stride < G.width) return ENF_EDIM;
    if (S > INT64_MAX / Z / G.width) return ENF_EDIM;
    const int64_t n = S * Z * G.width;
    const bool v4 = G.width % 4 == 0 && G.g_stride % 4 == 0 && adam_aligned16(G.x) && adam_aligned16(G.mu) && adam_aligned16(G.nu) &&
                    adam_aligned16(G.g) && adam_aligned16(G.x_out) && adam_aligned16(G.mu_out) && adam_aligned16(G.nu_out);
    A.seg[k] = G;
    A.vec[k] = v4 ? 4 : 1;
    A.units[k] = n / A.vec[k];
    A.total += A.units[k];
    if (n > (int64_t)INT_MAX) A.wide = 1;
  }
  A.idx = idx; A.nseg = nseg; A.Z = Z; A.nidx = nidx;
  A.lr = lr; A.b1 = b1; A.b2 = b2; A.omb1 = 1.f - b1; A.omb2 = 1.f - b2; A.eps = eps; A.c1 = c1; A.c2 = c2;
  // a memory-bound pass: at most 8 workgroups per compute unit, the rest by the grid-stride loop
  const int64_t blocks = (A.total + 255) / 256;
  hipLaunchKernelGGL(enf_table_adam_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? ENF_OK : ENF_ELAUNCH;
}
