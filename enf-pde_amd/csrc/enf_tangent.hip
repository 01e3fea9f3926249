// enf_tangent.hip -- forward-mode ("tangent") decode along a latent direction (include/enf_hip.h: enf_field_tangent) and, with
// enf_field_tangent_x, along a direction in the query coordinates as well.
//
//   tan[b,n,o] = sum_z  d out[b,n,o] / d (p, a, sigma)[b,z,:]  .  (dp, da, dsigma)[b,z,:]  +  sum_i d out[b,n,o] / d x[b,n,i]  xdot[b,n,i]
//
// the Jacobian-vector product of the decoder with respect to its latents: with (dp, da, dsigma) = dz/dt it is the time derivative of
// the decoded field, and with xdot = a velocity field beside it the material derivative.  The query direction enters in front of the
// first GEMM stage only (pair_invariant_tan: a few terms per pair in (dinv, dwin)); the pair kernel that takes it is an instantiation
// of its own (XD), so the one without it is the code it was.  Three kernels carry a tangent beside every primal activation of the
// forward chain:
//   enf_prologue_tangent_kernel   per latent row, fp32 on the vector ALU: the tangent of the latent table (`ltd`, the table's layout)
//   enf_pair_tangent_kernel       the latent-split layout of K2 (enf_pair_fwd.hip): a wave owns 16 queries and a share of the latents;
//                                 every weight stage in the LDS ring is multiplied twice (primal fragments, tangent fragments with a
//                                 zero start and no bias); the softmax sums Y, C, L get T = sum e (dy + dl y) and S = sum e dl beside
//                                 them and  ybar = (Y - C) / L,  d ybar = T / L - (S / L) ybar
//   enf_tail_tangent_kernel       tail_forward's chain (enf_tail.hip) with the same doubling; writes out (optional) and tan
// The same file holds the Gauss-Newton product (enf_gn_product, at the end): prologue tangent and pair kernel as above -- the pair
// kernel then also stores lse for the backward pair kernel -- and
//   enf_gn_tail_kernel            the tail's chain with tangents, d out = w tan formed in registers, the tail's backward chain
// followed by the backward pair kernel and the prologue backward of the other files.
// There is one copy of each thing the two entry points have in common: the doubled tail chain (tail_forward_tan, which stashes the
// pre-activations for the Gauss-Newton tail only), the panel product (panel_gemm2, whose one-operand form serves the backward chain),
// the launcher and its (D, H) dispatch (launch_pair_tail), and the host sequence (tan_call: refusals, dimensions, workspace;
// tan_launch_prologue; tan_pair_args).  The row moves, the chain's shapes and the constants' load are enf_tail.hip's
// (enf_tail_common.h).  Not shared: the Gauss-Newton tail's backward chain, a copy of enf_tail_bwd_kernel's (see there).
// Register room: at D = 128, H = 2 the accumulators Y and T alone are 128 registers, so these kernels run ONE wave per SIMD
// (workgroups of 4 waves, a 512-register budget) instead of K2's two.  Every output element is written once, by one lane, in a fixed
// order of operations: no atomics, the call is bit-reproducible run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include "enf_launch.h"
#include "enf_device.h"
#include "enf_pair_common.h"
#include "enf_tail_common.h"

namespace {

constexpr int TW = 4;                   // waves per workgroup: one per SIMD
constexpr int TTH = 64 * TW;
constexpr float TWO_PI = 6.283185307179586f;
constexpr int TAN_LDS_MAX = 160 * 1024;

// ---------------------------------------------------------------- staging with four waves
// stage_issue gives a wave PPW consecutive kilobytes, the piece index in the instruction's 12-bit offset field: at most 4 pieces per
// wave.  Four waves therefore issue a stage in chunks of 16 KB.
template <int BYTES> DEV void tan_issue(const Pipe& P, unsigned src, char* dst, int lane) {
  constexpr int CH = BYTES < 16384 ? BYTES : 16384;
  static_assert(BYTES % CH == 0 && BYTES <= STAGE_MAX, "stage size");
#pragma unroll
  for (int o = 0; o < BYTES; o += CH) stage_issue<CH, TW>(P.rs, src + o, dst + o, P.wave, lane);
}
template <int BYTES> DEV void tan_first_stage(Pipe& P, char* ring, unsigned panel, int wave, int lane) {
  P.cur = 0;
  P.wave = __builtin_amdgcn_readfirstlane(wave);
  P.early = false;
  tan_issue<BYTES>(P, panel, ring, lane);
  stage_wait();
  __syncthreads();
}

// The two-operand form of panel_gemm: acc += panel . F (the caller initialised acc), dacc = panel . dF (zero start, no bias), both
// from the SAME staged panel before its slot is released.  Preconditions and `next` / NEXT_BYTES / `active` as in panel_gemm.
// TAN false is the one-operand product in this cadence (four waves issuing): dacc and dF are not touched.
template <int KBIN, int MTOUT, bool BF16, int NEXT_BYTES, bool TAN = true>
DEV void panel_gemm2(f32x4 (&acc)[MTOUT], f32x4 (&dacc)[MTOUT], const Frags<BF16, KBIN>& F, const Frags<BF16, KBIN>& dF, Pipe& P,
                     char* ring, unsigned panel, unsigned next, bool active, int lane) {
  using C = PanelCfg<KBIN, MTOUT, BF16>;
#pragma unroll
  for (int sp = 0; sp < C::SPP; ++sp) {
    if (sp + 1 < C::SPP) tan_issue<C::STAGE>(P, panel + (sp + 1) * C::STAGE, ring + (P.cur ^ 1) * STAGE_MAX, lane);
    else if (next != NO_STAGE) tan_issue<NEXT_BYTES>(P, next, ring + (P.cur ^ 1) * STAGE_MAX, lane);
    const char* slot = ring + P.cur * STAGE_MAX;
    if (active) {
      gemm_stage<BF16, KBIN, C::MTS, INIT_ACC>(&acc[sp * C::MTS], F, slot, lane);
      if constexpr (TAN) gemm_stage<BF16, KBIN, C::MTS, INIT_ZERO>(&dacc[sp * C::MTS], dF, slot, lane);
    } else if constexpr (TAN) {
#pragma unroll
      for (int mt = 0; mt < C::MTS; ++mt) dacc[sp * C::MTS + mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    stage_close(P);
  }
}
// acc += panel . F alone, every wave active (the Gauss-Newton tail's backward chain)
template <int KBIN, int MTOUT, bool BF16, int NEXT_BYTES>
DEV void panel_gemm2(f32x4 (&acc)[MTOUT], const Frags<BF16, KBIN>& F, Pipe& P, char* ring, unsigned panel, unsigned next, int lane) {
  panel_gemm2<KBIN, MTOUT, BF16, NEXT_BYTES, false>(acc, acc, F, F, P, ring, panel, next, true, lane);
}

// gb_panel (enf_pair_common.h) with the tangent: FiLM v = v0 (1 + gamma) + beta,  dv = dv0 (1 + gamma) + v0 dgamma + dbeta,
// [dgamma dbeta] = GB^T dF.
template <int D, bool BF16, int NEXT_BYTES>
DEV void gb_panel2(f32x4 (&v)[D / 16], f32x4 (&dv)[D / 16], const Frags<BF16, D / 32>& F, const Frags<BF16, D / 32>& dF, Pipe& P,
                   char* ring, unsigned panel, unsigned next, bool active, const float* bias, const float* v0vec, const float* dv0vec,
                   int lane, int quad) {
  using C = typename PairCfg<D, BF16>::GB;
  constexpr int KB = D / 32, MTS = C::MTS;
#pragma unroll
  for (int sp = 0; sp < C::SPP; ++sp) {
    if (sp + 1 < C::SPP) tan_issue<C::STAGE>(P, panel + (sp + 1) * C::STAGE, ring + (P.cur ^ 1) * STAGE_MAX, lane);
    else if (next != NO_STAGE) tan_issue<NEXT_BYTES>(P, next, ring + (P.cur ^ 1) * STAGE_MAX, lane);
    const char* slot = ring + P.cur * STAGE_MAX;
    f32x4 t[MTS], dt[MTS];
#pragma unroll
    for (int j = 0; j < MTS; ++j) t[j] = rowvec(bias, sp * MTS + j, quad);
    if (active) {
      gemm_stage<BF16, KB, MTS, INIT_ACC>(t, F, slot, lane);
      gemm_stage<BF16, KB, MTS, INIT_ZERO>(dt, dF, slot, lane);
    } else {
#pragma unroll
      for (int j = 0; j < MTS; ++j) dt[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int g = 0; g < MTS / 4; ++g) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int tile = 2 * (sp * (MTS / 4) + g) + e;
        const f32x4 v0 = rowvec(v0vec, tile, quad), dv0 = rowvec(dv0vec, tile, quad);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float og = 1.0f + t[4 * g + e][i];
          v[tile][i] = fmaf(v0[i], og, t[4 * g + 2 + e][i]);
          dv[tile][i] = fmaf(dv0[i], og, fmaf(v0[i], dt[4 * g + e][i], dt[4 * g + 2 + e][i]));
        }
      }
    }
    stage_close(P);
  }
}

// rff_embed with the tangent, in the kernels' revolutions unit: dt = coeff^T dinv (the same fp32 MFMA, zero start),
// dE = 2 pi [cos(2 pi t) dt ; -sin(2 pi t) dt]
template <int D, bool BF16>
DEV void rff_embed2(f32x4 (&E)[D / 16], f32x4 (&dE)[D / 16], const float (&inv)[4], const float (&dinv)[4], const float* cfrag,
                    int lane, int quad) {
  constexpr int TT = D / 32;
  const float bq = quad == 0 ? inv[0] : quad == 1 ? inv[1] : quad == 2 ? inv[2] : inv[3];
  const float dbq = quad == 0 ? dinv[0] : quad == 1 ? dinv[1] : quad == 2 ? dinv[2] : dinv[3];
#pragma unroll
  for (int tt = 0; tt < TT; ++tt) {
    const float cf = cfrag[tt * 64 + lane];
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    const f32x4 t = __builtin_amdgcn_mfma_f32_16x16x4f32(cf, bq, z4, 0, 0, 0);
    const f32x4 dt = __builtin_amdgcn_mfma_f32_16x16x4f32(cf, dbq, z4, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float s = sin_rev<enf_bf16_valued(BF16)>(t[i]), c = cos_rev<enf_bf16_valued(BF16)>(t[i]);
      E[tt][i] = s; E[TT + tt][i] = c;
      dE[tt][i] = TWO_PI * c * dt[i];
      dE[TT + tt][i] = -TWO_PI * s * dt[i];
    }
  }
}

// X <- gelu(X), dX <- gelu'(X) dX   (one sigmoid per value: gelu_fg_tile)
template <int NT> DEV void gelu_tangent(f32x4 (&X)[NT], f32x4 (&dX)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    f32x4 g;
    gelu_fg_tile(X[t], g);            // X[t] <- gelu'
#pragma unroll
    for (int i = 0; i < 4; ++i) dX[t][i] *= X[t][i];
    X[t] = g;
  }
}
// dX <- 1[X > 0] dX   (the relu itself is applied where X is used)
template <int NT> DEV void relu_tangent(const f32x4 (&X)[NT], f32x4 (&dX)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) dX[t][i] = X[t][i] > 0.f ? dX[t][i] : 0.f;
}
// LayerNorm without affine, y = (g - mu) rstd already applied:  dy = rstd (dg - mean dg - y mean(y dg)), means over the true width
// (exact with the eps).  One fma chain per element with the two row constants folded in.
template <int NT> DEV void ln_tangent(f32x4 (&dg)[NT], const f32x4 (&y)[NT], float rstd, float inv_n) {
  float s, d;
  tiles_sum_dot<NT>(dg, [&](int t) { return y[t]; }, s, d);
  const float c0 = -(xquad_sum(s) * inv_n) * rstd, c1 = -(xquad_sum(d) * inv_n) * rstd;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) dg[t][i] = fmaf(y[t][i], c1, fmaf(dg[t][i], rstd, c0));
}

// Tangent of (invariant, window) along the latent's pose row and window coefficient, both in the latent table's embedded form
// (tp: plain -> dp; ponita -> (dpx, dpy, -sin th dth, cos th dth); sphere -> (dphi, dth, cos th dth, -sin th dth)).  The formulas are
// pair_invariant's (enf_device.h), differentiated; `inv` / `win` are its results for the same pair.
// XD: also along the query's own tangent tq (zero beyond dx), in the coordinates as given (angles on the sphere, no metric factors).
// Wherever the pair depends on x - p (or p - x) alone, that is the pose tangent tp - tq in the position components: the translation
// x += e, p += e then cancels exactly.  What depends on x itself gets its own term: abs_pos' invariant, and theta_x on the sphere
// (through q.sx, q.cx in `dot`, and as latitude_periodic's inv[0]).
template <bool FAST, bool XD>
DEV void pair_invariant_tan(int inv_id, int dx, const QueryPt& q, const f32x4& pz, float wcoef, int use_window, const float (&inv)[4],
                            float win, const f32x4& tpz, float twc, const float (&tq)[3], float (&dinv)[4], float& dwin) {
  const float PI = 3.14159265358979323846f;
  f32x4 tp = tpz;
  if constexpr (XD) {
    const bool sphere = inv_id == ENF_INV_LATITUDE_PERIODIC || inv_id == ENF_INV_POLAR_PERIODIC;
    tp[0] -= tq[0];                                        // phi on the sphere
    if (!sphere) tp[1] -= tq[1];
    if (!sphere && inv_id != ENF_INV_PONITA) tp[2] -= tq[2];   // (ponita: rows 2, 3 are the orientation's)
  }
  dinv[0] = dinv[1] = dinv[2] = dinv[3] = 0.f;
  dwin = 0.f;
  switch (inv_id) {
    case ENF_INV_REL_POS_PERIODIC: {           // inv = [cos pi D0, cos pi D1, sin pi D0, sin pi D1], D = p - x
      dinv[0] = -PI * inv[2] * tp[0]; dinv[1] = -PI * inv[3] * tp[1];
      dinv[2] = PI * inv[0] * tp[0];  dinv[3] = PI * inv[1] * tp[1];
      if (use_window) dwin = twc * (inv[0] * inv[0] + inv[1] * inv[1]) + 2.f * wcoef * (inv[0] * dinv[0] + inv[1] * dinv[1]);
    } break;
    case ENF_INV_LATITUDE_PERIODIC:
    case ENF_INV_POLAR_PERIODIC: {
      const float dphi = (q.x0 - pz[0]) * 0.15915494309189535f;
      const float cd = cos_rev<FAST>(dphi), sd = sin_rev<FAST>(dphi);
      const float dcd = sd * tp[0], dsd = -cd * tp[0];                  // d/d phi_p of cos / sin (phi_x - phi_p)
      const float dot = q.sx * pz[2] * cd + q.cx * pz[3];
      float ddot = q.sx * (tp[2] * cd + pz[2] * dcd) + q.cx * tp[3];
      if constexpr (XD) ddot = fmaf(q.cx * pz[2] * cd - q.sx * pz[3], tq[1], ddot);      // d dot / d theta_x
      if (inv_id == ENF_INV_LATITUDE_PERIODIC) {
        dinv[1] = tp[1]; dinv[2] = dcd; dinv[3] = dsd;
        if constexpr (XD) dinv[0] = tq[1];
      } else dinv[0] = ddot;
      if (use_window) {                         // win = exp(-ang^2 wc), ang = acos(clip(dot))
        const float dc = fminf(fmaxf(dot, -1.f + 1e-6f), 1.f - 1e-6f);
        const float ang = acosf(dc);
        float e = -ang * ang * twc;
        if (dot > -1.f + 1e-6f && dot < 1.f - 1e-6f) e += 2.f * ang * wcoef * ddot * rsqrtf(1.f - dc * dc);
        dwin = win * e;
      }
    } break;
    case ENF_INV_PONITA: {                      // inv = [r . (c, s), r . (-s, c)], r = x - p
      const float r0 = q.x0 - pz[0], r1 = q.x1 - pz[1];
      dinv[0] = -tp[0] * pz[2] - tp[1] * pz[3] + r0 * tp[2] + r1 * tp[3];
      dinv[1] = tp[0] * pz[3] - tp[1] * pz[2] - r0 * tp[3] + r1 * tp[2];
      if (use_window) dwin = -twc * (r0 * r0 + r1 * r1) + 2.f * wcoef * (r0 * tp[0] + r1 * tp[1]);
    } break;
    default: {                                  // abs_pos, rel_pos, norm_rel_pos: r = x - p
      const float r0 = q.x0 - pz[0], r1 = dx > 1 ? q.x1 - pz[1] : 0.f, r2 = dx > 2 ? q.x2 - pz[2] : 0.f;
      const float t0 = tp[0], t1 = dx > 1 ? tp[1] : 0.f, t2 = dx > 2 ? tp[2] : 0.f;
      const float d2 = r0 * r0 + r1 * r1 + r2 * r2, rt = r0 * t0 + r1 * t1 + r2 * t2;
      if (inv_id == ENF_INV_REL_POS) { dinv[0] = -t0; dinv[1] = -t1; dinv[2] = -t2; }
      else if (inv_id == ENF_INV_NORM_REL_POS) dinv[0] = d2 > 0.f ? -rt * rsqrtf(d2) : 0.f;
      else if constexpr (XD) { dinv[0] = tq[0]; dinv[1] = tq[1]; dinv[2] = tq[2]; }       // abs_pos: inv = x
      if (use_window) dwin = -twc * d2 + 2.f * wcoef * rt;
    } break;
  }
}

// ---------------------------------------------------------------- (a) the latent prologue's tangent
// Per latent row, after enf_prologue_kernel (which leaves s, xn, mu, rstd in `an` and k in `kv`):
//   ds = da Ws;  dxn = rstd (ds - mean ds - xn mean(xn ds));  dan = dxn * lna_g;  dk = dan Wk;  dv0 = dan Wv;
//   du_h = MU_h dk_h;  dc_h = cvec_h . dk_h;  pose and window coefficient by the chain rule
// in the scheme of enf_prologue_kernel: PZT rows per block, the output index on the lanes, activations in LDS as [feature][row].
constexpr int PZT = 4;
struct PrologueTanArgs {
  const float* p; const float* sigma; const float* dp; const float* da; const float* dsigma;
  const char* blob; EnfLayout L;
  const float* an; float* ltd;
  int BZ, H, D, C, dp_dim, inv, Dt;
};

DEV float tan_wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void enf_prologue_tangent_kernel(PrologueTanArgs A) {
  extern __shared__ __attribute__((aligned(16))) float psm[];
  const int D = A.D, H = A.H, HD = H * D, C = A.C;
  float* s_a = psm;                  // [C][PZT]   da
  float* s_x = s_a + PZT * C;        // [D][PZT]   ds, then dan
  float* s_k = s_x + PZT * D;        // [HD][PZT]  dk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row0 = blockIdx.x * PZT;
  auto W = [&](size_t off) { return reinterpret_cast<const float*>(A.blob + off); };
  const int stride = enf_lt_stride(H, D);
  for (int i = tid; i < PZT * C; i += 256) {
    const int zz = i / C, c = i % C, r = row0 + zz;
    s_a[c * PZT + zz] = (A.da && r < A.BZ) ? A.da[(size_t)r * C + c] : 0.f;
  }
  __syncthreads();
  for (int d = tid; d < D; d += 256) {
    float acc[PZT];
#pragma unroll
    for (int zz = 0; zz < PZT; ++zz) acc[zz] = 0.f;
#pragma unroll 8
    for (int c = 0; c < C; ++c) {
      const float w = W(A.L.stem_w)[(size_t)c * D + d];
#pragma unroll
      for (int zz = 0; zz < PZT; ++zz) acc[zz] = fmaf(s_a[c * PZT + zz], w, acc[zz]);
    }
#pragma unroll
    for (int zz = 0; zz < PZT; ++zz) s_x[d * PZT + zz] = acc[zz];
  }
  __syncthreads();
  for (int zz = wave; zz < PZT; zz += 4) {           // LayerNorm tangent: one wave per row, means over the true width
    const int r = row0 + zz < A.BZ ? row0 + zz : A.BZ - 1;
    const float* anr = A.an + (size_t)r * (2 * D + 2);
    float v1 = 0.f, v2 = 0.f;
    for (int d = lane; d < A.Dt; d += 64) { const float g = s_x[d * PZT + zz]; v1 += g; v2 += g * anr[D + d]; }
    const float m1 = tan_wave_sum(v1) / A.Dt, m2 = tan_wave_sum(v2) / A.Dt, rstd = anr[2 * D + 1];
    for (int d = lane; d < D; d += 64)
      s_x[d * PZT + zz] = rstd * (s_x[d * PZT + zz] - m1 - anr[D + d] * m2) * W(A.L.lna_g)[d];
  }
  __syncthreads();
  for (int j = tid; j < 2 * HD; j += 256) {          // dk | dv0 (no bias)
    const bool isv = j >= HD;
    const int jj = isv ? j - HD : j;
    const float* Wm = W(isv ? A.L.wv : A.L.wk);
    float acc[PZT];
#pragma unroll
    for (int zz = 0; zz < PZT; ++zz) acc[zz] = 0.f;
#pragma unroll 8
    for (int d = 0; d < D; ++d) {
      const float w = Wm[(size_t)d * HD + jj];
#pragma unroll
      for (int zz = 0; zz < PZT; ++zz) acc[zz] = fmaf(s_x[d * PZT + zz], w, acc[zz]);
    }
#pragma unroll
    for (int zz = 0; zz < PZT; ++zz) {
      const int r = row0 + zz;
      if (!isv) s_k[jj * PZT + zz] = acc[zz];
      else if (r < A.BZ) A.ltd[(size_t)r * stride + enf_lt_off_v0(H, D) + jj] = acc[zz];
    }
  }
  __syncthreads();
  for (int j = tid; j < HD; j += 256) {              // du_h = MU_h dk_h
    const int h = j / D, i = j % D;
    const float* mut = W(A.L.mut) + (size_t)h * D * D + i;
    float acc[PZT];
#pragma unroll
    for (int zz = 0; zz < PZT; ++zz) acc[zz] = 0.f;
#pragma unroll 8
    for (int dd = 0; dd < D; ++dd) {
      const float w = mut[(size_t)dd * D];
#pragma unroll
      for (int zz = 0; zz < PZT; ++zz) acc[zz] = fmaf(s_k[(h * D + dd) * PZT + zz], w, acc[zz]);
    }
#pragma unroll
    for (int zz = 0; zz < PZT; ++zz)
      if (row0 + zz < A.BZ) A.ltd[(size_t)(row0 + zz) * stride + enf_lt_off_u(H, D) + j] = acc[zz];
  }
  for (int t = wave; t < PZT * H; t += 4) {           // dc_h = cvec_h . dk_h
    const int zz = t / H, h = t % H, r = row0 + zz;
    float sacc = 0.f;
    for (int dd = lane; dd < D; dd += 64) sacc = fmaf(W(A.L.cvec)[h * D + dd], s_k[(h * D + dd) * PZT + zz], sacc);
    sacc = tan_wave_sum(sacc);
    if (lane == 0 && r < A.BZ) A.ltd[(size_t)r * stride + enf_lt_off_c(H, D) + h] = sacc;
  }
  if (tid < PZT && row0 + tid < A.BZ) {               // pose row and window coefficient
    const int r = row0 + tid;
    const float* pp = A.p + (size_t)r * A.dp_dim;
    float t[3] = {0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
    if (A.dp)
      for (int i = 0; i < A.dp_dim && i < 3; ++i) t[i] = A.dp[(size_t)r * A.dp_dim + i];
    const bool sphere = A.inv == ENF_INV_LATITUDE_PERIODIC || A.inv == ENF_INV_POLAR_PERIODIC;
    if (A.inv == ENF_INV_PONITA) { q[0] = t[0]; q[1] = t[1]; q[2] = -sinf(pp[2]) * t[2]; q[3] = cosf(pp[2]) * t[2]; }
    else if (sphere) { q[0] = t[0]; q[1] = t[1]; q[2] = cosf(pp[1]) * t[1]; q[3] = -sinf(pp[1]) * t[1]; }
    else { q[0] = t[0]; q[1] = t[1]; q[2] = t[2]; }
    float dwc = 0.f;
    if (A.sigma && A.dsigma) {
      const float sg = A.sigma[r], ds = A.dsigma[r];
      dwc = (sphere ? -1.f : -2.f) * ds / (sg * sg * sg);
    }
    float* o = A.ltd + (size_t)r * stride;
    for (int i = 0; i < 4; ++i) o[enf_lt_off_pose(H, D) + i] = q[i];
    o[enf_lt_off_wcoef(H, D)] = dwc;
  }
}

// ---------------------------------------------------------------- (b) the pair kernel
struct PairTanArgs {
  const float* x; long long x_bstride;
  const float* lt; const float* ltd; const char* blob; EnfLayout L;
  float* ybar; float* ydot;               // (B, N, H D) fp32 each
  float* lse;                             // (B, N, H) in K2's convention (m* + log L) for the backward pair kernel, or nullptr
  float inv_d;                            // 1 / (true num_hidden)
  int B, N, Z, dx, inv, use_window, qg;   // qg: query groups per workgroup (1, 2, 4); ZS = TW / qg latent splits
  const float* xdot; long long xdot_bstride;   // (B, N, dx) query tangent, read by the XD instantiations only (nullptr: the others run)
};

// LDS map: ring (2 slots) | constants | per-wave latent vectors u, v0, du, dv0 | softmax exchange (m, l, c, s)
template <int D, int H> struct TanSmem {
  static constexpr int RING = 0;
  static constexpr int CONSTS = RING + 2 * STAGE_MAX;              // bq1 bv1 bf bm (D each) | bgb (2HD) | acq acv (2D each)
  static constexpr int N_CONST = 4 * D + 2 * H * D + 4 * D;
  static constexpr int ZVEC = CONSTS + 4 * N_CONST;                // TW x 4 H D floats
  static constexpr int XCH = ZVEC + 4 * TW * 4 * H * D;            // TW x H x 4 x 16 floats
  static constexpr int TOTAL = XCH + 4 * TW * H * 4 * 16;
  static constexpr int YBYTES = H * (D / 16) * 4 * 64 * 4;         // one wave's Y (or T) in [reg][lane] order
  static_assert((TW / 2) * 2 * YBYTES <= 2 * STAGE_MAX, "the combine buffer (Y and T of half the waves) must fit in the ring");
  static_assert(TOTAL <= TAN_LDS_MAX, "the tangent pair kernel's LDS exceeds one CU's 160 KiB");
};

#define TAN_BIAS(ACC, PTR)                                                             \
  do {                                                                                 \
    _Pragma("unroll") for (int t_ = 0; t_ < NT; ++t_) ACC[t_] = rowvec(PTR, t_, quad);   \
  } while (0)

template <int D, int H, bool BF16, bool XD>
__global__ __launch_bounds__(TTH, 1) void enf_pair_tangent_kernel(PairTanArgs A) {
  using Cfg = PairCfg<D, BF16>;
  using SM = TanSmem<D, H>;
  constexpr int KB = Cfg::KB, NT = Cfg::NT, HD = H * D;
  constexpr int ST_DD = Cfg::DD::STAGE, ST_GB = Cfg::GB::STAGE, PANEL_GB = Cfg::GB::BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem + SM::RING;
  float* cst = reinterpret_cast<float*>(smem + SM::CONSTS);
  float* c_bq1 = cst, *c_bv1 = cst + D, *c_bf = cst + 2 * D, *c_bm = cst + 3 * D, *c_bgb = cst + 4 * D;
  float* c_acq = c_bgb + 2 * HD, *c_acv = c_acq + 2 * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  float* zv = reinterpret_cast<float*>(smem + SM::ZVEC) + wave * 4 * HD;      // u | v0 | du | dv0
  float* xch = reinterpret_cast<float*>(smem + SM::XCH);
  const int QG = A.qg, ZS = TW / QG;
  const int qgi = wave % QG, zs = wave / QG;
  const char* blob = A.blob;
  auto G = [&](size_t off) { return reinterpret_cast<const float*>(blob + off); };

  for (int i = tid; i < D; i += TTH) { c_bq1[i] = G(A.L.bq1)[i]; c_bv1[i] = G(A.L.bv1)[i]; c_bf[i] = G(A.L.bf)[i]; c_bm[i] = G(A.L.bm)[i]; }
  for (int i = tid; i < 2 * HD; i += TTH) c_bgb[i] = G(A.L.bgb)[i];
  for (int i = tid; i < 2 * D; i += TTH) { c_acq[i] = G(A.L.acq)[i]; c_acv[i] = G(A.L.acv)[i]; }

  const unsigned pQ1 = (unsigned)A.L.aq1, pV1 = (unsigned)A.L.av1, pF = (unsigned)A.L.af, pGB = (unsigned)A.L.agb, pM = (unsigned)A.L.am;
  Pipe P;
  P.rs = make_blob_rsrc(blob, (unsigned)A.L.total);
  P.rs2 = P.rs;

  const int b = blockIdx.y;
  const int n0 = (blockIdx.x * QG + qgi) * 16;
  const int n = min(n0 + col, A.N - 1);                  // tail queries: clamped on load, guarded on store
  const QueryPt q = load_query(A.x + (size_t)b * A.x_bstride + (size_t)n * A.dx, A.dx, A.inv);
  float tq[3] = {0.f, 0.f, 0.f};                         // the query's tangent: x's row, clamped as x is
  if constexpr (XD) {
    const float* xd = A.xdot + (size_t)b * A.xdot_bstride + (size_t)n * A.dx;
    tq[0] = xd[0];
    if (A.dx > 1) tq[1] = xd[1];
    if (A.dx > 2) tq[2] = xd[2];
  }
  tan_first_stage<ST_DD>(P, ring, pQ1, wave, lane);      // (its barrier also publishes the constants)

  // softmax state against a per-column reference logit (the first one seen), as K2: Y = sum e rstd g, C = sum e rstd mu, L = sum e,
  // and beside them T = sum e (dy + dl y), S = sum e dl
  float sm_m[H], sm_l[H], sm_c[H], sm_s[H];
  f32x4 Y[H][NT], T[H][NT];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    sm_m[h] = -INFINITY; sm_l[h] = 0.f; sm_c[h] = 0.f; sm_s[h] = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) { Y[h][t] = f32x4{0.f, 0.f, 0.f, 0.f}; T[h][t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  }

  const int ltstride = enf_lt_stride(H, D);
  // a wave whose share of the latents is empty keeps the staging / barrier cadence and stays at m = -inf, sums 0
  const int iters = (A.Z + ZS - 1) / ZS;
  for (int it = 0; it < iters; ++it) {
    const int z = it * ZS + zs;
    const bool active = z < A.Z;
    const unsigned wrap = it + 1 < iters ? pQ1 : NO_STAGE;
    const size_t lrow = ((size_t)b * A.Z + (active ? z : A.Z - 1)) * ltstride;
    const float* ltrow = A.lt + lrow;
    const float* ltdrow = A.ltd + lrow;
    // per-latent vectors u | v0 and their tangents -> wave-private LDS
#pragma unroll
    for (int i = lane * 4; i < 2 * HD; i += 256) {
      *reinterpret_cast<f32x4*>(zv + i) = *reinterpret_cast<const f32x4*>(ltrow + i);
      *reinterpret_cast<f32x4*>(zv + 2 * HD + i) = *reinterpret_cast<const f32x4*>(ltdrow + i);
    }
    const f32x4 pz = *reinterpret_cast<const f32x4*>(ltrow + enf_lt_off_pose(H, D));
    const f32x4 tpz = *reinterpret_cast<const f32x4*>(ltdrow + enf_lt_off_pose(H, D));
    const float wcoef = ltrow[enf_lt_off_wcoef(H, D)], twc = ltdrow[enf_lt_off_wcoef(H, D)];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    float inv[4], win, dinv[4], dwin;
    pair_invariant<enf_bf16_valued(BF16)>(A.inv, A.dx, q, pz, wcoef, A.use_window, inv, win);
    pair_invariant_tan<enf_bf16_valued(BF16), XD>(A.inv, A.dx, q, pz, wcoef, A.use_window, inv, win, tpz, twc, tq, dinv, dwin);

    float logit[H], dlogit[H];
    Frags<BF16, KB> F, dF;
    {  // ---------------- query branch: h1 = relu(W1q^T E + b), logit_h = h1 . u_h + c_h + win and its tangent
      f32x4 acc[NT], dacc[NT];
      rff_embed2<D, BF16>(acc, dacc, inv, dinv, c_acq, lane, quad);
      make_frags<BF16, KB>(F, acc);
      make_frags<BF16, KB>(dF, dacc);
      TAN_BIAS(acc, c_bq1);
      panel_gemm2<KB, NT, BF16, ST_DD>(acc, dacc, F, dF, P, ring, pQ1, pV1, active, lane);
#pragma unroll
      for (int h = 0; h < H; ++h) {
        float s = 0.f, ds = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const f32x4 u = rowvec(zv + h * D, t, quad), du = rowvec(zv + 2 * HD + h * D, t, quad);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float h1 = relu_f(acc[t][i]);
            const float dh = acc[t][i] > 0.f ? dacc[t][i] : 0.f;
            s = fmaf(h1, u[i], s);
            ds = fmaf(dh, u[i], fmaf(h1, du[i], ds));
          }
        }
        logit[h] = xquad_sum(s) + ltrow[enf_lt_off_c(H, D) + h] + win;
        dlogit[h] = xquad_sum(ds) + ltdrow[enf_lt_off_c(H, D) + h] + dwin;
      }
    }
    {  // ---------------- value branch: RFFNet layer, folded Dense, gelu, LayerNorm
      f32x4 acc[NT], dacc[NT];
      rff_embed2<D, BF16>(acc, dacc, inv, dinv, c_acv, lane, quad);
      make_frags<BF16, KB>(F, acc);
      make_frags<BF16, KB>(dF, dacc);
      TAN_BIAS(acc, c_bv1);
      panel_gemm2<KB, NT, BF16, ST_DD>(acc, dacc, F, dF, P, ring, pV1, pF, active, lane);
      relu_tangent<NT>(acc, dacc);
      make_frags<BF16, KB>(F, acc);
      relu_frags<BF16, KB>(F);
      make_frags<BF16, KB>(dF, dacc);
      TAN_BIAS(acc, c_bf);
      panel_gemm2<KB, NT, BF16, ST_GB>(acc, dacc, F, dF, P, ring, pF, pGB, active, lane);
      gelu_tangent<NT>(acc, dacc);
      float mu, rstd;
      ln_stats<NT>(acc, mu, rstd, A.inv_d);
      ln_apply<NT>(acc, mu, rstd);
      ln_tangent<NT>(dacc, acc, rstd, A.inv_d);
      make_frags<BF16, KB>(F, acc);      // F / dF = normalised f and its tangent, shared by all heads' gamma/beta panels
      make_frags<BF16, KB>(dF, dacc);
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
      f32x4 v[NT], dv[NT];
      gb_panel2<D, BF16, ST_DD>(v, dv, F, dF, P, ring, pGB + h * PANEL_GB, pM, active, c_bgb + 2 * h * D, zv + HD + h * D,
                                zv + 3 * HD + h * D, lane, quad);
      Frags<BF16, KB> FV, dFV;
      make_frags<BF16, KB>(FV, v);
      make_frags<BF16, KB>(dFV, dv);
      TAN_BIAS(v, c_bm);
      if (h + 1 < H) panel_gemm2<KB, NT, BF16, ST_GB>(v, dv, FV, dFV, P, ring, pM, pGB + (h + 1) * PANEL_GB, active, lane);
      else panel_gemm2<KB, NT, BF16, ST_DD>(v, dv, FV, dFV, P, ring, pM, wrap, active, lane);
      gelu_tangent<NT>(v, dv);
      float mu, rstd;
      ln_stats<NT>(v, mu, rstd, A.inv_d);
      f32x4 y[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) y[t] = v[t];
      ln_apply<NT>(y, mu, rstd);
      ln_tangent<NT>(dv, y, rstd, A.inv_d);
      if (active) {
        if (it == 0) sm_m[h] = logit[h];
        const bool far = logit[h] - sm_m[h] > 40.0f;
        if (__any(far)) {                 // the rare "logit far above the reference" case rescales the sums (wave-uniform branch)
          const float alpha = far ? __expf(sm_m[h] - logit[h]) : 1.0f;
          sm_l[h] *= alpha; sm_c[h] *= alpha; sm_s[h] *= alpha;
          if (far) sm_m[h] = logit[h];
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) { Y[h][t][i] *= alpha; T[h][t][i] *= alpha; }
        }
        const float pe = __expf(logit[h] - sm_m[h]);
        const float w = pe * rstd, dl = dlogit[h];
        sm_l[h] += pe;
        sm_c[h] = fmaf(w, mu, sm_c[h]);
        sm_s[h] = fmaf(pe, dl, sm_s[h]);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            Y[h][t][i] = fmaf(w, v[t][i], Y[h][t][i]);
            T[h][t][i] = fmaf(pe, fmaf(dl, y[t][i], dv[t][i]), T[h][t][i]);
          }
      }
    }
  }

  // ---- combine the ZS latent splits of each query group (all staging is finished: the ring is free)
  if (quad == 0) {
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float* e = xch + ((wave * H + h) * 4) * 16 + col;
      e[0] = sm_m[h]; e[16] = sm_l[h]; e[32] = sm_c[h]; e[48] = sm_s[h];
    }
  }
  __syncthreads();
  float cs[H], sb[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    float ms = -INFINITY;
    for (int s = 0; s < ZS; ++s) ms = fmaxf(ms, xch[(((s * QG + qgi) * H + h) * 4) * 16 + col]);
    float L = 0.f, C = 0.f, S = 0.f;
    for (int s = 0; s < ZS; ++s) {
      const float* e = xch + (((s * QG + qgi) * H + h) * 4) * 16 + col;
      const float aw = __expf(e[0] - ms);         // exp(-inf) = 0 for a split that saw no latent
      L = fmaf(aw, e[16], L);
      C = fmaf(aw, e[32], C);
      S = fmaf(aw, e[48], S);
    }
    cs[h] = C / L; sb[h] = S / L;
    if (A.lse && wave < QG && quad == 0 && n0 + col < A.N) A.lse[((size_t)b * A.N + n0 + col) * H + h] = ms + __logf(L);
    const float sc = __expf(sm_m[h] - ms) / L;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) { Y[h][t][i] *= sc; T[h][t][i] *= sc; }
  }
  // deterministic tree over the split index: splits [s, 2s) hand their partial sums to [0, s)
  float* cb = reinterpret_cast<float*>(ring);
  constexpr int YF = SM::YBYTES / 4;
  for (int s = ZS >> 1; s >= 1; s >>= 1) {
    if (zs >= s && zs < 2 * s) {
      float* dst = cb + (size_t)((zs - s) * QG + qgi) * (2 * YF);
#pragma unroll
      for (int h = 0; h < H; ++h)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            dst[((h * NT + t) * 4 + i) * 64 + lane] = Y[h][t][i];
            dst[YF + ((h * NT + t) * 4 + i) * 64 + lane] = T[h][t][i];
          }
    }
    __syncthreads();
    if (zs < s) {
      const float* src = cb + (size_t)(zs * QG + qgi) * (2 * YF);
#pragma unroll
      for (int h = 0; h < H; ++h)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            Y[h][t][i] += src[((h * NT + t) * 4 + i) * 64 + lane];
            T[h][t][i] += src[YF + ((h * NT + t) * 4 + i) * 64 + lane];
          }
    }
    __syncthreads();
  }
  if (zs == 0 && n0 + col < A.N) {
    const size_t row = ((size_t)b * A.N + n0 + col) * HD;
#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        f32x4 o = Y[h][t], d = T[h][t];
#pragma unroll
        for (int i = 0; i < 4; ++i) { o[i] -= cs[h]; d[i] = fmaf(-sb[h], o[i], d[i]); }
        *reinterpret_cast<f32x4*>(A.ybar + row + h * D + 16 * t + 4 * quad) = o;
        *reinterpret_cast<f32x4*>(A.ydot + row + h * D + 16 * t + 4 * quad) = d;
      }
  }
}

// ---------------------------------------------------------------- (c) the tails
// LDS map of both tail kernels: ring (2 slots) | tail_consts' vectors (enf_tail_common.h)
template <int D, int H> struct TailTanSmem {
  static constexpr int CONSTS = 2 * STAGE_MAX;                     // bB bF1 (HD each) | bO0 bO2 (D each) | bO4 (32)
  static constexpr int TOTAL = CONSTS + 4 * (2 * H * D + 2 * D + 32);
  static_assert(TOTAL <= TAN_LDS_MAX, "the tangent tail's LDS exceeds one CU's 160 KiB");
};

// tail_forward's chain (enf_tail.hip) for this wave's 16 queries with a tangent beside every activation: o4 / do4 = the (padded) 32
// network outputs and their tangents.  Precondition: the first stage of L.atb is resident in ring[P.cur] and visible.
// SAVE: stash the primal pre-activations and the LayerNorm's mu, rstd in `act` (TailCfg's layout) for a backward chain.
// next / NEXT_BYTES: the stage that streams behind the last panel (NO_STAGE: nothing follows).
template <int D, int H, bool BF16, bool SAVE, int NEXT_BYTES>
DEV void tail_forward_tan(f32x4 (&o4)[2], f32x4 (&do4)[2], const float* yrow, const float* ydrow, float* act, const EnfLayout& L,
                          const float* cst, Pipe& P, char* ring, unsigned next, int lane, int quad, float inv_hd) {
  using T = TailCfg<D, H, BF16>;
  constexpr int KB = T::KB, KBH = T::KBH, NT = T::NT, NTH = T::NTH, HD = T::HD;
  const float* c_bB = cst, *c_bF1 = cst + HD, *c_bO0 = cst + 2 * HD, *c_bO2 = cst + 2 * HD + D, *c_bO4 = cst + 2 * HD + 2 * D;
  f32x4 a[NTH], da[NTH];
  Frags<BF16, KBH> FH, dFH;
  load_rows<NTH>(a, yrow, quad);
  load_rows<NTH>(da, ydrow, quad);
  make_frags<BF16, KBH>(FH, a);
  make_frags<BF16, KBH>(dFH, da);
#pragma unroll
  for (int t = 0; t < NTH; ++t) a[t] = rowvec(c_bB, t, quad);
  panel_gemm2<KBH, NTH, BF16, T::ST_TB>(a, da, FH, dFH, P, ring, (unsigned)L.atb, (unsigned)L.atf1, true, lane);
  if constexpr (SAVE) store_rows<NTH>(a, act, quad);
  gelu_tangent<NTH>(a, da);
  float mu, rstd;
  ln_stats<NTH>(a, mu, rstd, inv_hd);
  if constexpr (SAVE) {
    if (quad == 0) { act[T::ACT - 2] = mu; act[T::ACT - 1] = rstd; }
  }
  ln_apply<NTH>(a, mu, rstd);
  ln_tangent<NTH>(da, a, rstd, inv_hd);
  make_frags<BF16, KBH>(FH, a);
  make_frags<BF16, KBH>(dFH, da);
#pragma unroll
  for (int t = 0; t < NTH; ++t) a[t] = rowvec(c_bF1, t, quad);
  panel_gemm2<KBH, NTH, BF16, T::ST_O0>(a, da, FH, dFH, P, ring, (unsigned)L.atf1, (unsigned)L.ato0, true, lane);
  if constexpr (SAVE) store_rows<NTH>(a, act + HD, quad);
  gelu_tangent<NTH>(a, da);
  make_frags<BF16, KBH>(FH, a);
  make_frags<BF16, KBH>(dFH, da);
  f32x4 c[NT], dc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) c[t] = rowvec(c_bO0, t, quad);
  panel_gemm2<KBH, NT, BF16, T::ST_O2>(c, dc, FH, dFH, P, ring, (unsigned)L.ato0, (unsigned)L.ato2, true, lane);
  if constexpr (SAVE) store_rows<NT>(c, act + 2 * HD, quad);
  gelu_tangent<NT>(c, dc);
  Frags<BF16, KB> FD, dFD;
  make_frags<BF16, KB>(FD, c);
  make_frags<BF16, KB>(dFD, dc);
#pragma unroll
  for (int t = 0; t < NT; ++t) c[t] = rowvec(c_bO2, t, quad);
  panel_gemm2<KB, NT, BF16, T::ST_O4>(c, dc, FD, dFD, P, ring, (unsigned)L.ato2, (unsigned)L.ato4, true, lane);
  if constexpr (SAVE) store_rows<NT>(c, act + 2 * HD + D, quad);
  gelu_tangent<NT>(c, dc);
  make_frags<BF16, KB>(FD, c);
  make_frags<BF16, KB>(dFD, dc);
  o4[0] = rowvec(c_bO4, 0, quad);
  o4[1] = rowvec(c_bO4, 1, quad);
  panel_gemm2<KB, 2, BF16, NEXT_BYTES>(o4, do4, FD, dFD, P, ring, (unsigned)L.ato4, next, true, lane);
}

// What both tail kernels do before the chain: the LDS constants, the blob's resource, the first stage of the first panel (its barrier
// also publishes the constants).
template <int D, int H, bool BF16>
DEV void tail_tan_open(Pipe& P, char* smem, const char* blob, const EnfLayout& L, int tid) {
  tail_consts<D, H, BF16, TTH>(reinterpret_cast<float*>(smem + TailTanSmem<D, H>::CONSTS), blob, L, tid);
  P.rs = make_blob_rsrc(blob, (unsigned)L.total);
  P.rs2 = P.rs;
  tan_first_stage<TailCfg<D, H, BF16>::ST_TB>(P, smem, (unsigned)L.atb, tid >> 6, tid & 63);
}

struct TailTanArgs {
  const float* ybar; const float* ydot; const char* blob; EnfLayout L;
  float* out;            // (B N, O) or nullptr
  float* tan;            // (B N, O)
  int NQ, O;
  float inv_hd;          // 1 / (true heads * true num_hidden)
};

template <int D, int H, bool BF16>
__global__ __launch_bounds__(TTH, 1) void enf_tail_tangent_kernel(TailTanArgs A) {
  constexpr int HD = H * D;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  const int q0 = blockIdx.x * (16 * TW) + wave * 16;
  const int qi = min(q0 + col, A.NQ - 1);
  Pipe P;
  tail_tan_open<D, H, BF16>(P, smem, A.blob, A.L, tid);
  f32x4 o4[2], do4[2];
  tail_forward_tan<D, H, BF16, false, 1024>(o4, do4, A.ybar + (size_t)qi * HD, A.ydot + (size_t)qi * HD, nullptr, A.L,
                                            reinterpret_cast<const float*>(smem + TailTanSmem<D, H>::CONSTS), P, smem, NO_STAGE, lane,
                                            quad, A.inv_hd);
  if (q0 + col < A.NQ) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int o = 16 * t + 4 * quad + i;
        if (o < A.O) {
          if (A.out) A.out[(size_t)(q0 + col) * A.O + o] = o4[t][i];
          A.tan[(size_t)(q0 + col) * A.O + o] = do4[t][i];
        }
      }
  }
}

// ---------------------------------------------------------------- (d) the Gauss-Newton tail (include/enf_hip.h, "Gauss-Newton product")
// The chain above with the stash, then d out = (w > 0 ? w tan : 0) gs formed in registers where tail_sq_err forms its gradient, then a
// backward chain on the stash: d ybar and delta for the backward pair kernel.  Neither tan nor d out reaches memory and the forward
// chain runs once.  One wave per SIMD, the 2-slot ring with four waves issuing, as every kernel of this file.
// The backward chain MIRRORS enf_tail_bwd_kernel's (enf_tail.hip), line for line, and is kept as a second copy on purpose: that kernel
// runs another ring (three slots or two, eight waves issuing), and a chain shared between the two would either make the hot tail branch
// on its caller or -- tried -- change the code generation of all 220 of its backward instantiations.  A change of the
// arithmetic there belongs here too.

// X <- X * gelu'(pre)
template <int NT> DEV void gelu_back(f32x4 (&X)[NT], const float* pre_row, int quad) {
  f32x4 pre[NT];
  load_rows<NT>(pre, pre_row, quad);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) X[t][i] *= gelu_grad_f(pre[t][i]);
}

struct GnTailArgs {
  const float* ybar; const float* ydot; const char* blob; EnfLayout L;
  const float* weight;   // nullptr, one weight per query (NQ), or with `cw` one per output value (NQ, O)
  float* dybar; float* delta; float* act;      // (NQ, HD), (NQ, H), (NQ, TailCfg::ACT)
  int NQ, O, cw;
  float inv_hd;          // 1 / (true heads * true num_hidden)
  float gs;              // 2 grad_scale / (B N O)
};

template <int D, int H, bool BF16>
__global__ __launch_bounds__(TTH, 1) void enf_gn_tail_kernel(GnTailArgs A) {
  using T = TailCfg<D, H, BF16>;
  constexpr int KB = T::KB, KBH = T::KBH, NT = T::NT, NTH = T::NTH, HD = T::HD, ACT = T::ACT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  const int q0 = blockIdx.x * (16 * TW) + wave * 16;
  const bool qvalid = q0 + col < A.NQ;
  const int qi = min(q0 + col, A.NQ - 1);      // clamped (duplicate) queries stash the same values and store nothing else
  float* act = A.act + (size_t)qi * ACT;
  const float* yrow = A.ybar + (size_t)qi * HD;
  const EnfLayout& L = A.L;
  Pipe P;
  tail_tan_open<D, H, BF16>(P, smem, A.blob, L, tid);

  // ---- forward chain with tangents; the pre-activations this lane stores are re-read by this lane only
  f32x4 g0[2];
  {
    f32x4 o4[2], do4[2];
    tail_forward_tan<D, H, BF16, true, T::ST_G4>(o4, do4, yrow, A.ydot + (size_t)qi * HD, act, L,
                                                 reinterpret_cast<const float*>(smem + TailTanSmem<D, H>::CONSTS), P, ring,
                                                 (unsigned)L.gto4, lane, quad, A.inv_hd);
    // ---- d out = (w > 0 ? w tan : 0) gs: a weight of 0 is a select, as in the fused loss
    const float wq = (A.weight && !A.cw) ? A.weight[qi] : 1.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int o = 16 * t + 4 * quad + i;
        const bool in = o < A.O && qvalid;
        const float w = (in && A.cw) ? A.weight[(size_t)qi * A.O + o] : wq;
        g0[t][i] = (in && w > 0.f) ? w * do4[t][i] * A.gs : 0.f;
      }
  }

  // ---- backward chain (enf_tail_bwd_kernel's) on the stash
  Frags<BF16, 1> F1;
  make_frags<BF16, 1>(F1, g0);
  f32x4 c[NT];
  zero_tiles<NT>(c);
  panel_gemm2<1, NT, BF16, T::ST_O2>(c, F1, P, ring, (unsigned)L.gto4, (unsigned)L.gto2, lane);                   // d g4
  gelu_back<NT>(c, act + 2 * HD + D, quad);                                                                       // d a_O2
  Frags<BF16, KB> FD;
  make_frags<BF16, KB>(FD, c);
  zero_tiles<NT>(c);
  panel_gemm2<KB, NT, BF16, T::ST_G0>(c, FD, P, ring, (unsigned)L.gto2, (unsigned)L.gto0, lane);                  // d g3
  gelu_back<NT>(c, act + 2 * HD, quad);                                                                           // d a_O0
  make_frags<BF16, KB>(FD, c);
  f32x4 a[NTH];
  zero_tiles<NTH>(a);
  panel_gemm2<KB, NTH, BF16, T::ST_TB>(a, FD, P, ring, (unsigned)L.gto0, (unsigned)L.gtf1, lane);                 // d g2
  gelu_back<NTH>(a, act + HD, quad);                                                                              // d a_F1
  Frags<BF16, KBH> FH;
  make_frags<BF16, KBH>(FH, a);
  zero_tiles<NTH>(a);
  panel_gemm2<KBH, NTH, BF16, T::ST_TB>(a, FH, P, ring, (unsigned)L.gtf1, (unsigned)L.gtb, lane);                 // d n
  {     // LayerNorm backward + gelu backward on a_B
    f32x4 pre[NTH];
    load_rows<NTH>(pre, act, quad);
    const float mu = act[ACT - 2], rstd = act[ACT - 1];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < NTH; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float nh = (gelu_f(pre[t][i]) - mu) * rstd;
        s1 += a[t][i]; s2 = fmaf(a[t][i], nh, s2);
      }
    const float m1 = xquad_sum(s1) * A.inv_hd, m2 = xquad_sum(s2) * A.inv_hd;
#pragma unroll
    for (int t = 0; t < NTH; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float nh = (gelu_f(pre[t][i]) - mu) * rstd;
        a[t][i] = rstd * (a[t][i] - m1 - nh * m2) * gelu_grad_f(pre[t][i]);                                       // d a_B
      }
  }
  make_frags<BF16, KBH>(FH, a);
  zero_tiles<NTH>(a);
  panel_gemm2<KBH, NTH, BF16, 1024>(a, FH, P, ring, (unsigned)L.gtb, NO_STAGE, lane);                             // d ybar
  f32x4 y[NTH];
  load_rows<NTH>(y, yrow, quad);
#pragma unroll
  for (int h = 0; h < H; ++h) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) s = fmaf(a[h * NT + t][i], y[h * NT + t][i], s);
    s = xquad_sum(s);
    if (quad == 0 && qvalid) A.delta[(size_t)qi * H + h] = s;
  }
  if (qvalid) store_rows<NTH>(a, A.dybar + (size_t)qi * HD, quad);
}

// ---------------------------------------------------------------- launch: the pair kernel, then the entry point's tail
template <int D, int H, bool BF16> constexpr auto tail_kernel(const TailTanArgs*) { return enf_tail_tangent_kernel<D, H, BF16>; }
template <int D, int H, bool BF16> constexpr auto tail_kernel(const GnTailArgs*) { return enf_gn_tail_kernel<D, H, BF16>; }

// the instantiations: both entry points dispatch here
template <class TailArgsT>
int launch_pair_tail(const EnfDims& m, const PairTanArgs& PA, const TailArgsT& TA, hipStream_t st) {
  return enf_for_shape(m, [&](auto s) {
    constexpr int D = s.D, H = s.H;
    constexpr bool BF16 = s.BF16;
    constexpr int pair_lds = TanSmem<D, H>::TOTAL, tail_lds = TailTanSmem<D, H>::TOTAL;
    constexpr auto pk0 = enf_pair_tangent_kernel<D, H, BF16, false>, pkx = enf_pair_tangent_kernel<D, H, BF16, true>;
    constexpr auto tk = tail_kernel<D, H, BF16>((const TailArgsT*)nullptr);
    if (!(PA.xdot ? enf_lds_attr<pkx>(pair_lds) : enf_lds_attr<pk0>(pair_lds))) return (int)ENF_ELAUNCH;
    if (!enf_lds_attr<tk>(tail_lds)) return (int)ENF_ELAUNCH;
    hipLaunchKernelGGL(PA.xdot ? pkx : pk0, dim3((PA.N + 16 * PA.qg - 1) / (16 * PA.qg), PA.B), dim3(TTH), pair_lds, st, PA);
    if (hipGetLastError() != hipSuccess) return (int)ENF_ELAUNCH;
    hipLaunchKernelGGL(tk, dim3((TA.NQ + 16 * TW - 1) / (16 * TW)), dim3(TTH), tail_lds, st, TA);
    return hipGetLastError() == hipSuccess ? 0 : (int)ENF_ELAUNCH;
  });
}

// ---------------------------------------------------------------- the host sequence of both entry points
// what the calls serve beyond enf_check_desc: the rff embedding, the seven invariants without a per-latent phase, relu masks off
bool tangent_supported(const EnfDesc* d) {
  if (d->embedding != ENF_EMB_RFF || d->mask_mode != ENF_MASK_OFF) return false;
  return d->invariant_id != ENF_INV_BALL && d->invariant_id != ENF_INV_BALL_LAT && d->invariant_id != ENF_INV_PONITA_FULL;
}

// The workspace: the plain workspace's regions at their usual offsets (latent table, an, kv, ybar, ... are used in place), with `det`
// (ENF_BWD_DETERMINISTIC) the deterministic regions behind them (enf_det_workspace: K3's partial rows), then the table's tangent and
// ybar's tangent -- a fit step or an evaluation with the same deterministic bit runs on the same buffer.  enf_field_tangent's layout is
// the one without the deterministic regions.
struct TanWorkspace { size_t ltd, ydot, total; };
TanWorkspace tan_workspace(const EnfDims& m, bool det) {
  const EnfWorkspace W = enf_workspace(m);
  TanWorkspace T;
  T.ltd = det ? enf_det_workspace(m, W).total : W.total;
  T.ydot = T.ltd + enf_align(enf_lt_bytes(m));
  T.total = T.ydot + enf_align(sizeof(float) * (size_t)m.B * m.N * m.HD);
  return T;
}
constexpr unsigned GN_FLAGS = ENF_BWD_DETERMINISTIC | ENF_GN_REUSE_POINT;

// enf_call's context (enf_launch.h) with the regions above and the point's pose rows and window sizes
struct TanCall : EnfCall {
  TanWorkspace T;
  const float* p; const float* sigma;      // sigma: nullptr without a window
};
// Refusals in their order of precedence: the descriptor's (enf_check_desc), ENF_EUNSUPPORTED, then enf_call's -- ENF_EINVAL for a NULL
// pointer (`pointers_ok`: the entry point's own set, p apart) or a window without `sigma` -- then ENF_EWORKSPACE.
int tan_call(TanCall& c, const EnfDesc* d, bool pointers_ok, const float* p, const float* sigma, const void* packed, void* workspace,
             size_t workspace_bytes, bool det, void* stream) {
  int rc = enf_check_desc(d);
  if (rc) return rc;
  if (!tangent_supported(d)) return ENF_EUNSUPPORTED;
  if ((rc = enf_call(c, d, pointers_ok && p, sigma, packed, workspace, ~(size_t)0, stream))) return rc;
  c.T = tan_workspace(c.m, det);
  if (workspace_bytes < c.T.total) return ENF_EWORKSPACE;
  c.p = p;
  c.sigma = d->use_window ? sigma : nullptr;
  return ENF_OK;
}
// the table's tangent along (dp, da, dsigma), behind enf_launch_prologue at the same point
int tan_launch_prologue(const TanCall& c, const float* dp, const float* da, const float* dsigma) {
  const EnfDims& m = c.m;
  PrologueTanArgs A;
  A.p = c.p; A.sigma = c.sigma; A.dp = dp; A.da = da; A.dsigma = dsigma; A.blob = c.blob; A.L = c.L;
  A.an = c.F(c.W.an); A.ltd = c.F(c.T.ltd);
  A.BZ = m.B * m.Z; A.H = m.H; A.D = m.D; A.C = m.C; A.dp_dim = m.dp; A.inv = m.inv; A.Dt = m.Dt;
  const size_t smem = sizeof(float) * PZT * (m.C + m.D + m.HD);
  hipLaunchKernelGGL(enf_prologue_tangent_kernel, dim3((A.BZ + PZT - 1) / PZT), dim3(256), smem, c.st, A);
  return hipGetLastError() == hipSuccess ? 0 : ENF_ELAUNCH;
}
// lse: where the pair kernel leaves the log-sum-exp for a backward pair kernel, or nullptr; xdot: the query tangent, or nullptr
PairTanArgs tan_pair_args(const TanCall& c, const float* x, int64_t x_bstride, float* lse, const float* xdot = nullptr,
                          int64_t xdot_bstride = 0) {
  const EnfDims& m = c.m;
  PairTanArgs PA;
  PA.x = x; PA.x_bstride = x_bstride; PA.lt = c.F(c.W.lt); PA.ltd = c.F(c.T.ltd); PA.blob = c.blob; PA.L = c.L;
  PA.ybar = c.F(c.W.ybar); PA.ydot = c.F(c.T.ydot); PA.lse = lse; PA.inv_d = 1.0f / (float)m.Dt;
  PA.B = m.B; PA.N = m.N; PA.Z = m.Z; PA.dx = m.dx; PA.inv = m.inv; PA.use_window = m.use_window;
  const int zs = enf_latent_splits(m.Z);                 // as many latent splits as there are latents to split, up to one per wave
  PA.qg = TW / (zs < TW ? zs : TW);
  PA.xdot = xdot; PA.xdot_bstride = xdot_bstride;
  return PA;
}

}  // namespace

extern "C" size_t enf_field_tangent_workspace_bytes(const EnfDesc* d) {
  if (enf_check_desc(d) != ENF_OK || !tangent_supported(d)) return 0;
  return tan_workspace(enf_dims(d), false).total;
}

// With xdot alone the prologue tangent still runs, on three NULL tangents: it then writes zeros to every element of `ltd` the pair
// kernel reads (u, v0, the pose row, wcoef, c of every row) -- the workspace is not promised to hold anything.
extern "C" int enf_field_tangent_x(const EnfDesc* d, const float* x, int64_t x_bstride, const float* xdot, int64_t xdot_bstride,
                                   const float* p, const float* a, const float* sigma, const float* dp, const float* da,
                                   const float* dsigma, const void* blob, float* out, float* tan, void* workspace, void* stream) {
  TanCall c;       // (the call takes no workspace size)
  int rc = tan_call(c, d, x && a && tan && (xdot || dp || da || dsigma), p, sigma, blob, workspace, ~(size_t)0, false, stream);
  if (rc) return rc;
  const EnfDims& m = c.m;
  if ((rc = enf_launch_prologue(m, c.L, c.blob, p, a, sigma, c.F(c.W.lt), c.F(c.W.an), c.F(c.W.kv), c.st))) return rc;
  if ((rc = tan_launch_prologue(c, dp, da, dsigma))) return rc;
  const PairTanArgs PA = tan_pair_args(c, x, x_bstride, nullptr, xdot, xdot_bstride);
  TailTanArgs TA;
  TA.ybar = PA.ybar; TA.ydot = PA.ydot; TA.blob = c.blob; TA.L = c.L; TA.out = out; TA.tan = tan;
  TA.NQ = m.B * m.N; TA.O = m.O; TA.inv_hd = 1.0f / (float)(m.Ht * m.Dt);
  return launch_pair_tail(m, PA, TA, c.st);
}

extern "C" int enf_field_tangent(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                                 const float* dp, const float* da, const float* dsigma, const void* blob, float* out, float* tan,
                                 void* workspace, void* stream) {
  return enf_field_tangent_x(d, x, x_bstride, nullptr, 0, p, a, sigma, dp, da, dsigma, blob, out, tan, workspace, stream);
}

// ---------------------------------------------------------------- the Gauss-Newton product (include/enf_hip.h, "Gauss-Newton product")
extern "C" size_t enf_gn_workspace_bytes(const EnfDesc* d, unsigned flags) {
  if (enf_check_desc(d) != ENF_OK || !tangent_supported(d) || (flags & ~GN_FLAGS)) return 0;
  return tan_workspace(enf_dims(d), (flags & ENF_BWD_DETERMINISTIC) != 0).total;
}

extern "C" int enf_gn_product(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                              const float* vp, const float* va, const float* vsigma, const void* packed, const float* weight,
                              const float* cweight, float grad_scale, float* gp, float* ga, float* gsigma, void* workspace,
                              size_t workspace_bytes, unsigned flags, void* stream) {
  const bool det = (flags & ENF_BWD_DETERMINISTIC) != 0, reuse = (flags & ENF_GN_REUSE_POINT) != 0;
  TanCall c;
  int rc = tan_call(c, d, x && a && gp && ga && gsigma && (vp || va || vsigma) && !(weight && cweight) && !(flags & ~GN_FLAGS), p, sigma,
                    packed, workspace, workspace_bytes, det, stream);
  if (rc) return rc;
  const EnfDims& m = c.m;
  const EnfLayout& L = c.L;
  const EnfWorkspace& W = c.W;
  hipStream_t st = c.st;
  const char* pk = c.blob;
  const bool zb = enf_use_zfold_bwd(m);
  if ((rc = enf_side_join_pending(st, workspace))) return rc;
  // the point: latent table, what the prologue backward reads, and the z-fold backward's per-latent matrices -- unless the caller
  // vouches that a fit step or an earlier product at this point left them
  if (!reuse) {
    if ((rc = enf_launch_prologue(m, L, pk, p, a, sigma, c.F(W.lt), c.F(W.an), c.F(W.kv), st))) return rc;
    if (zb && (rc = enf_launch_wz(m, L, pk, c.F(W.lt), nullptr, c.F(W.wzb), nullptr, c.ws + W.wzt, st))) return rc;
  }
  if ((rc = tan_launch_prologue(c, vp, va, vsigma))) return rc;
  const PairTanArgs PA = tan_pair_args(c, x, x_bstride, c.F(W.lse));
  GnTailArgs GA;
  GA.ybar = PA.ybar; GA.ydot = PA.ydot; GA.blob = pk; GA.L = L; GA.weight = cweight ? cweight : weight; GA.cw = cweight != nullptr;
  GA.dybar = c.F(W.dybar); GA.delta = c.F(W.delta); GA.act = c.F(W.tail_act);
  GA.NQ = m.B * m.N; GA.O = m.O; GA.inv_hd = 1.0f / (float)(m.Ht * m.Dt);
  GA.gs = 2.0f * grad_scale / ((float)m.B * (float)m.N * (float)m.O);
  if ((rc = launch_pair_tail(m, PA, GA, st))) return rc;
  // the backward pair kernel without a store, in the variant the descriptor resolves to; deterministic: through the partial rows and
  // the fixed-order reduction, which overwrites the gradient table
  if (!det && hipMemsetAsync(c.F(W.dlt), 0, enf_lt_bytes(m), st) != hipSuccess) return ENF_ELAUNCH;
  if ((rc = enf_launch_pair_bwd(m, L, pk, x, x_bstride, c.F(W.lt), c.F(W.lse), c.F(W.dybar), c.F(W.delta), c.F(W.dlt), nullptr,
                                c.fold_bwd(), nullptr, st, det ? c.F(c.X.part) : nullptr)))
    return rc;
  return enf_launch_prologue_bwd(m, L, pk, p, sigma, c.F(W.an), c.F(W.kv), c.F(W.dlt), gp, ga, gsigma, st);
}
