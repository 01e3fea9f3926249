// enf_pair_bwd_shared.hip -- the SHARED instantiations of enf_pair_bwd_kernel (the shared-latent backward of the first inner step)
// and their launcher, in a translation unit of their own: compiled next to them, the per-signal instantiations of enf_pair_bwd.hip
// come out with other register and scratch figures (profiles/step0_resource_usage.txt).  The __global__ template is enf_pair_bwd.hip's.
#define ENF_PAIR_BWD_KERNEL_ONLY 1
#include "enf_pair_bwd.hip"

template <int D, int H, bool BF16, int INV = -1>
static int launch_pair_bwd_shared(const PairBwdArgs& A, hipStream_t st) {
  using SM = PairBwdSmem<D, H, BF16, false>;
  auto kern = enf_pair_bwd_kernel<D, H, BF16, false, true, INV, false, true>;
  static EnfAttrBits attr_done{0};          // one per instantiation, one bit per device
  // the slabs of the cross-wave reduce: NWAVES x (D / 16) tiles of 1 KB from LACC on (more than the per-signal partial sums at H = 1)
  constexpr int SLABS = SM::LACC + NWAVES * (D / 16) * 1024, TOTAL = SLABS > SM::TOTAL ? SLABS : SM::TOTAL;
  static_assert(SLABS <= SM::EXTACC || !SM::EXT_OK, "the slabs end before the ext sums");
  static_assert(TOTAL <= 160 * 1024, "K3 LDS budget");
  if (!enf_lds_attr(reinterpret_cast<const void*>(kern), TOTAL, attr_done)) return ENF_ELAUNCH;
  hipLaunchKernelGGL(kern, dim3(A.Z, A.nsplit, (A.SB + 15) / 16), dim3(NTHREADS), TOTAL, st, A);
  return hipGetLastError() == hipSuccess ? 0 : ENF_ELAUNCH;
}

// The shared-latent backward (enf_layout.h: enf_shared_backward_rule; `m` is the whole batch's): one pass over signal 0's (N x Z) pairs
// on the unit-seeded dybar (N, HD) / delta (N, H), contracted with dout (B, N) into all B Z rows of `dlt` (added to: the caller zeroes
// them).  x, lt, lse, wzt, wzb: signal 0's rows.  The instantiations are those of enf_pair_bwd_shared_exists.
int enf_launch_pair_bwd_shared(const EnfDims& m, const EnfLayout& L, const char* blob, const float* x, const float* lt, const float* lse,
                               const float* dybar, const float* delta, const float* dout, float* dlt, const char* wzt, const float* wzb,
                               hipStream_t st) {
  if (!enf_pair_bwd_shared_exists(m) || !enf_pair_bwd_zfold_fits(m) || !wzt || !wzb || !dout) return ENF_EUNSUPPORTED;
  PairBwdArgs A;
  A.dxq = nullptr; A.part = nullptr; A.dxpart = nullptr; A.masks = nullptr; A.mask_B = 1; A.mask_b0 = 0;
  A.wzt = wzt; A.wzb = wzb; A.inv_d = 1.0f / (float)m.Dt;
  A.x = x; A.x_bstride = 0; A.lt = lt; A.blob = blob; A.L = L; A.lse = lse; A.dybar = dybar; A.delta = delta;
  A.dlt = dlt; A.B = 1; A.N = m.N; A.Z = m.Z; A.dx = m.dx; A.inv = m.inv; A.use_window = m.use_window;
  A.nsplit = enf_pair_bwd_shared_nsplit(m); A.xcd_remap = 0;
  A.dout = dout; A.SB = m.B;
  if (m.bf16 && m.dx == 2) {      // the invariant as a compile-time constant, as for the per-signal kernels of the shipped configs
    if (m.D == 128 && m.H == 2 && m.inv == ENF_INV_REL_POS_PERIODIC) return launch_pair_bwd_shared<128, 2, true, ENF_INV_REL_POS_PERIODIC>(A, st);
    if (m.D == 64 && m.H == 2 && m.inv == ENF_INV_PONITA) return launch_pair_bwd_shared<64, 2, true, ENF_INV_PONITA>(A, st);
  }
#define ENF_CASE(DD, HH) \
  if (m.D == DD && m.H == HH) return m.bf16 ? launch_pair_bwd_shared<DD, HH, true>(A, st) : launch_pair_bwd_shared<DD, HH, false>(A, st);
  ENF_CASE(128, 2)
  ENF_CASE(64, 2)
  ENF_CASE(128, 1)
#undef ENF_CASE
  return ENF_EUNSUPPORTED;
}
