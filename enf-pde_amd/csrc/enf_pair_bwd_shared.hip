// enf_pair_bwd_shared.hip -- the SHARED instantiations of enf_pair_bwd_kernel (the shared-latent backward of the first inner step)
// and their launcher, in a translation unit of their own: compiled next to them, the per-signal instantiations of enf_pair_bwd.hip
// come out with other register and scratch figures (profiles/step0_resource_usage.txt).  The __global__ template is enf_pair_bwd.hip's.
#define ENF_PAIR_BWD_KERNEL_ONLY 1
#include "enf_pair_bwd.hip"

template <int D, int H, bool BF16, int INV = -1>
static int launch_pair_bwd_shared(const PairBwdArgs& A, hipStream_t st) {
  using SM = PairBwdSmem<D, H, BF16, false>;
  constexpr auto kern = enf_pair_bwd_kernel<D, H, BF16, false, true, INV, false, true>;
  // the slabs of the cross-wave reduce: NWAVES x (D / 16) tiles of 1 KB from LACC on (more than the per-signal partial sums at H = 1)
  constexpr int SLABS = SM::LACC + NWAVES * (D / 16) * 1024, TOTAL = SLABS > SM::TOTAL ? SLABS : SM::TOTAL;
  static_assert(SLABS <= SM::EXTACC || !SM::EXT_OK, "the slabs end before the ext sums");
  static_assert(TOTAL <= 160 * 1024, "K3 LDS budget");
  if (!enf_lds_attr<kern>(TOTAL)) return ENF_ELAUNCH;
  hipLaunchKernelGGL(kern, dim3(A.Z, A.nsplit, (A.SB + 15) / 16), dim3(NTHREADS), TOTAL, st, A);
  return hipGetLastError() == hipSuccess ? 0 : ENF_ELAUNCH;
}

// The shared-latent backward (enf_layout.h: enf_shared_backward_rule; `m` is the whole batch's): one pass over signal 0's (N x Z) pairs
// on the unit-seeded dybar (N, HD) / delta (N, H), contracted with dout (B, N) into all B Z rows of `dlt` (added to: the caller zeroes
// them).  x, lt, lse, wzt, wzb: signal 0's rows.  The instantiations are those of enf_pair_bwd_shared_exists.
int enf_launch_pair_bwd_shared(const EnfDims& m, const EnfLayout& L, const char* blob, const float* x, const float* lt, const float* lse,
                               const float* dybar, const float* delta, const float* dout, float* dlt, const EnfFoldBwd& zs,
                               hipStream_t st) {
  if (!enf_pair_bwd_shared_exists(m) || !enf_pair_bwd_zfold_fits(m) || !zs.wzt || !zs.wzb || !dout) return ENF_EUNSUPPORTED;
  PairBwdArgs A;
  A.dxq = nullptr; A.part = nullptr; A.dxpart = nullptr; A.masks = nullptr; A.mask_B = 1; A.mask_b0 = 0;
  A.wzt = zs.wzt; A.wzb = zs.wzb; A.inv_d = 1.0f / (float)m.Dt;
  A.x = x; A.x_bstride = 0; A.lt = lt; A.blob = blob; A.L = L; A.lse = lse; A.dybar = dybar; A.delta = delta;
  A.dlt = dlt; A.B = 1; A.N = m.N; A.Z = m.Z; A.dx = m.dx; A.inv = m.inv; A.use_window = m.use_window;
  A.nsplit = enf_pair_bwd_shared_nsplit(m); A.xcd_remap = 0;
  A.dout = dout; A.SB = m.B;
  // the invariant as a compile-time constant (enf_layout.h: enf_spec_inv), here for rel_pos_periodic and ponita only
  const int spec = m.inv == ENF_INV_REL_POS_PERIODIC || m.inv == ENF_INV_PONITA ? enf_spec_inv(m) : -1;
  return enf_for_shape(m, [&](auto s) {
    using S = decltype(s);
    if constexpr (!enf_shape_shared_bwd(S::D, S::H)) return (int)ENF_EUNSUPPORTED;
    else return enf_for_spec<S>(spec, [&](auto i) {
      if constexpr (i.INV < 0 || i.INV == ENF_INV_REL_POS_PERIODIC || i.INV == ENF_INV_PONITA) return launch_pair_bwd_shared<S::D, S::H, S::BF16, i.INV>(A, st);
      else return (int)ENF_EUNSUPPORTED;     // (not reached: `spec` is one of the two)
    });
  });
}
