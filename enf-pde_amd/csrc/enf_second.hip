// enf_second.hip -- the second directional derivative of the decode along a direction in the query coordinates
// (include/enf_hip.h: enf_field_second_x):
//
//   tan2[b,n,o] = sum_ij xdot[b,n,i] xdot[b,n,j]  d^2 out[b,n,o] / d x[b,n,i] d x[b,n,j]
//
// in ONE forward-mode pass that carries a second-order stream d2 beside the primal and the first-order stream d of enf_tangent.hip:
// along x(s) = x + s xdot every activation A has A(s) = A + s dA + s^2/2 d2A, so a linear stage maps the three streams alike (every
// staged weight panel is multiplied three times, d and d2 from a zero start without bias) and a nonlinearity f gives
// d2 f(A) = f'(A) d2A + f''(A) dA^2 ("exactly" as autograd means it: almost everywhere, relu'' = 0).  The direction lives in the query
// coordinates only: the latent table has no tangent here, no prologue tangent runs and no tangent table is read.
//   enf_pair_second_kernel   enf_pair_tangent_kernel's latent-split layout and four-wave cadence (one wave per SIMD).  Register room:
//                            three accumulator sets Y, T, U for H heads do not fit beside the three streams' working set, so the heads
//                            are split over grid.z -- a workgroup serves ONE head and recomputes the branches the heads share (the
//                            query RFFNet for its logit, the value RFFNet and its folded Dense).  The softmax sums Y, C, L, T, S get
//                            U = sum e (d2y + 2 dl dy + (d2l + dl^2) y) and R = sum e (d2l + dl^2) beside them, and
//                            d2 ybar = U / L - 2 (S / L) d ybar - (R / L) ybar
//   enf_tail_tangent_kernel  <.., ORDER = 2> (enf_tangent_common.h): the tangent tail's chain and kernel with the third stream; stores
//                            out (optional), tan (optional) and tan2
// The pair kernel calls the second-order forms of the panel product and of the activation rules directly.  gb_panel3 and rff_embed3
// are its own; panel_gemm3, gelu_second and ln_second sit in enf_tangent_common.h beside their first-order forms, where the tail chain
// picks one by its order.
// Every output element is written once, by one lane, in a fixed order of operations: no atomics, bit-reproducible run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include "enf_launch.h"
#include "enf_device.h"
#include "enf_pair_common.h"
#include "enf_tail_common.h"
#include "enf_tangent_common.h"

namespace {

// gb_panel2 without a tangent of v0 and with the second-order stream: v = v0 (1 + gamma) + beta, dv = v0 dgamma + dbeta,
// d2v = v0 d2gamma + d2beta
template <int D, bool BF16, int NEXT_BYTES>
DEV void gb_panel3(f32x4 (&v)[D / 16], f32x4 (&dv)[D / 16], f32x4 (&d2v)[D / 16], const Frags<BF16, D / 32>& F,
                   const Frags<BF16, D / 32>& dF, const Frags<BF16, D / 32>& d2F, Pipe& P, char* ring, unsigned panel, unsigned next,
                   bool active, const float* bias, const float* v0vec, int lane, int quad) {
  using C = typename PairCfg<D, BF16>::GB;
  constexpr int KB = D / 32, MTS = C::MTS;
#pragma unroll
  for (int sp = 0; sp < C::SPP; ++sp) {
    if (sp + 1 < C::SPP) tan_issue<C::STAGE>(P, panel + (sp + 1) * C::STAGE, ring + (P.cur ^ 1) * STAGE_MAX, lane);
    else if (next != NO_STAGE) tan_issue<NEXT_BYTES>(P, next, ring + (P.cur ^ 1) * STAGE_MAX, lane);
    const char* slot = ring + P.cur * STAGE_MAX;
    f32x4 t[MTS], dt[MTS], d2t[MTS];
#pragma unroll
    for (int j = 0; j < MTS; ++j) t[j] = rowvec(bias, sp * MTS + j, quad);
    if (active) {
      gemm_stage<BF16, KB, MTS, INIT_ACC>(t, F, slot, lane);
      gemm_stage<BF16, KB, MTS, INIT_ZERO>(dt, dF, slot, lane);
      gemm_stage<BF16, KB, MTS, INIT_ZERO>(d2t, d2F, slot, lane);
    } else {
#pragma unroll
      for (int j = 0; j < MTS; ++j) dt[j] = d2t[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int g = 0; g < MTS / 4; ++g) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int tile = 2 * (sp * (MTS / 4) + g) + e;
        const f32x4 v0 = rowvec(v0vec, tile, quad);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[tile][i] = fmaf(v0[i], 1.0f + t[4 * g + e][i], t[4 * g + 2 + e][i]);
          dv[tile][i] = fmaf(v0[i], dt[4 * g + e][i], dt[4 * g + 2 + e][i]);
          d2v[tile][i] = fmaf(v0[i], d2t[4 * g + e][i], d2t[4 * g + 2 + e][i]);
        }
      }
    }
    stage_close(P);
  }
}

// rff_embed2 with the second-order stream: d2t = coeff^T d2inv,
// d2E = [2 pi cos d2t - (2 pi dt)^2 sin ; -2 pi sin d2t - (2 pi dt)^2 cos]
template <int D, bool BF16>
DEV void rff_embed3(f32x4 (&E)[D / 16], f32x4 (&dE)[D / 16], f32x4 (&d2E)[D / 16], const float (&inv)[4], const float (&dinv)[4],
                    const float (&d2inv)[4], const float* cfrag, int lane, int quad) {
  constexpr int TT = D / 32;
  const float bq = quad == 0 ? inv[0] : quad == 1 ? inv[1] : quad == 2 ? inv[2] : inv[3];
  const float dbq = quad == 0 ? dinv[0] : quad == 1 ? dinv[1] : quad == 2 ? dinv[2] : dinv[3];
  const float d2bq = quad == 0 ? d2inv[0] : quad == 1 ? d2inv[1] : quad == 2 ? d2inv[2] : d2inv[3];
#pragma unroll
  for (int tt = 0; tt < TT; ++tt) {
    const float cf = cfrag[tt * 64 + lane];
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    const f32x4 t = __builtin_amdgcn_mfma_f32_16x16x4f32(cf, bq, z4, 0, 0, 0);
    const f32x4 dt = __builtin_amdgcn_mfma_f32_16x16x4f32(cf, dbq, z4, 0, 0, 0);
    const f32x4 d2t = __builtin_amdgcn_mfma_f32_16x16x4f32(cf, d2bq, z4, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float s = sin_rev<enf_bf16_valued(BF16)>(t[i]), c = cos_rev<enf_bf16_valued(BF16)>(t[i]);
      const float w = TWO_PI * dt[i], w2 = w * w;
      E[tt][i] = s; E[TT + tt][i] = c;
      dE[tt][i] = TWO_PI * c * dt[i];
      dE[TT + tt][i] = -TWO_PI * s * dt[i];
      d2E[tt][i] = fmaf(TWO_PI * c, d2t[i], -w2 * s);
      d2E[TT + tt][i] = fmaf(-TWO_PI * s, d2t[i], -w2 * c);
    }
  }
}

// (invariant, window) differentiated twice along the query's own tangent tq (zero beyond dx); the latent has no tangent.  `inv`, `win`
// are pair_invariant's results and `dinv` pair_invariant_tan's (XD, zero pose tangent) for the same pair.  Coordinates as given: angles on
// the sphere, no metric factors.
template <bool FAST>
DEV void pair_invariant_sec(int inv_id, int dx, const QueryPt& q, const f32x4& pz, float wcoef, int use_window, const float (&inv)[4],
                            float win, const float (&tq)[3], const float (&dinv)[4], float (&d2inv)[4], float& d2win) {
  const float PI = 3.14159265358979323846f;
  d2inv[0] = d2inv[1] = d2inv[2] = d2inv[3] = 0.f;
  d2win = 0.f;
  switch (inv_id) {
    case ENF_INV_REL_POS_PERIODIC: {           // inv = [cos pi D0, cos pi D1, sin pi D0, sin pi D1], D = p - x
      const float a0 = PI * PI * tq[0] * tq[0], a1 = PI * PI * tq[1] * tq[1];
      d2inv[0] = -a0 * inv[0]; d2inv[1] = -a1 * inv[1];
      d2inv[2] = -a0 * inv[2]; d2inv[3] = -a1 * inv[3];
      if (use_window)
        d2win = 2.f * wcoef * (fmaf(dinv[0], dinv[0], inv[0] * d2inv[0]) + fmaf(dinv[1], dinv[1], inv[1] * d2inv[1]));
    } break;
    case ENF_INV_LATITUDE_PERIODIC:
    case ENF_INV_POLAR_PERIODIC: {             // dot = sx sp cd + cx cp twice along (t_phi, t_theta)
      const float dphi = (q.x0 - pz[0]) * 0.15915494309189535f;
      const float cd = cos_rev<FAST>(dphi), sd = sin_rev<FAST>(dphi);
      const float tf = tq[0], tt = tq[1];
      const float dot = q.sx * pz[2] * cd + q.cx * pz[3];
      const float ddot = -q.sx * pz[2] * sd * tf + (q.cx * pz[2] * cd - q.sx * pz[3]) * tt;
      const float d2dot = -q.sx * pz[2] * cd * tf * tf - 2.f * q.cx * pz[2] * sd * tf * tt - dot * tt * tt;
      if (inv_id == ENF_INV_LATITUDE_PERIODIC) { d2inv[2] = -cd * tf * tf; d2inv[3] = -sd * tf * tf; }
      else d2inv[0] = d2dot;
      if (use_window && dot > -1.f + 1e-6f && dot < 1.f - 1e-6f) {      // win = exp(g), g = -ang^2 wc, ang = acos(dot); the clip's derivative is 0
        const float ang = acosf(dot), rs = rsqrtf(1.f - dot * dot);
        const float a1 = -ddot * rs, a2 = -d2dot * rs - dot * ddot * ddot * rs * rs * rs;
        const float g1 = -2.f * ang * wcoef * a1, g2 = -2.f * wcoef * (a1 * a1 + ang * a2);
        d2win = win * (g1 * g1 + g2);
      }
    } break;
    case ENF_INV_PONITA: {                      // the invariant is linear in x; win = -wc |x - p|^2
      if (use_window) d2win = -2.f * wcoef * (tq[0] * tq[0] + tq[1] * tq[1]);
    } break;
    default: {                                  // abs_pos, rel_pos, norm_rel_pos: r = x - p
      const float r0 = q.x0 - pz[0], r1 = dx > 1 ? q.x1 - pz[1] : 0.f, r2 = dx > 2 ? q.x2 - pz[2] : 0.f;
      const float t0 = tq[0], t1 = dx > 1 ? tq[1] : 0.f, t2 = dx > 2 ? tq[2] : 0.f;
      const float d2 = r0 * r0 + r1 * r1 + r2 * r2, rt = r0 * t0 + r1 * t1 + r2 * t2, tt = t0 * t0 + t1 * t1 + t2 * t2;
      if (inv_id == ENF_INV_NORM_REL_POS) d2inv[0] = d2 > 0.f ? (tt - rt * rt / d2) * rsqrtf(d2) : 0.f;
      if (use_window) d2win = -2.f * wcoef * tt;
    } break;
  }
}

// ---------------------------------------------------------------- the pair kernel
struct PairSecArgs {
  const float* x; long long x_bstride;
  const float* xdot; long long xdot_bstride;       // (B, N, dx) query direction
  const float* lt; const char* blob; EnfLayout L;
  float* ybar; float* ydot; float* y2;             // (B, N, H D) fp32 each
  float inv_d;                                     // 1 / (true num_hidden)
  int B, N, Z, dx, inv, use_window, qg;            // qg: query groups per workgroup (1, 2, 4); ZS = TW / qg latent splits
};

// LDS map: ring (2 slots) | constants | per-wave latent vectors u_h, v0_h | softmax exchange (m, l, c, s, r)
template <int D> struct SecSmem {
  static constexpr int RING = 0;
  static constexpr int CONSTS = RING + 2 * STAGE_MAX;              // bq1 bv1 bf bm (D each) | bgb of the head (2D) | acq acv (2D each)
  static constexpr int N_CONST = 4 * D + 2 * D + 4 * D;
  static constexpr int ZVEC = CONSTS + 4 * N_CONST;                // TW x 2 D floats
  static constexpr int XCH = ZVEC + 4 * TW * 2 * D;                // TW x 5 x 16 floats
  static constexpr int TOTAL = XCH + 4 * TW * 5 * 16;
  static constexpr int YBYTES = (D / 16) * 4 * 64 * 4;             // one wave's Y (or T, or U) in [reg][lane] order
  static_assert((TW / 2) * 3 * YBYTES <= 2 * STAGE_MAX, "the combine buffer (Y, T and U of half the waves) must fit in the ring");
  static_assert(TOTAL <= TAN_LDS_MAX, "the second-order pair kernel's LDS exceeds one CU's 160 KiB");
};

template <int D, int H, bool BF16>
__global__ __launch_bounds__(TTH, 1) void enf_pair_second_kernel(PairSecArgs A) {
  using Cfg = PairCfg<D, BF16>;
  using SM = SecSmem<D>;
  constexpr int KB = Cfg::KB, NT = Cfg::NT, HD = H * D;
  constexpr int ST_DD = Cfg::DD::STAGE, ST_GB = Cfg::GB::STAGE, PANEL_GB = Cfg::GB::BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem + SM::RING;
  float* cst = reinterpret_cast<float*>(smem + SM::CONSTS);
  float* c_bq1 = cst, *c_bv1 = cst + D, *c_bf = cst + 2 * D, *c_bm = cst + 3 * D, *c_bgb = cst + 4 * D;
  float* c_acq = c_bgb + 2 * D, *c_acv = c_acq + 2 * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  float* zv = reinterpret_cast<float*>(smem + SM::ZVEC) + wave * 2 * D;       // u_h | v0_h
  float* xch = reinterpret_cast<float*>(smem + SM::XCH);
  const int QG = A.qg, ZS = TW / QG;
  const int qgi = wave % QG, zs = wave / QG;
  const int h = blockIdx.z;                                // this workgroup's head
  const char* blob = A.blob;
  auto G = [&](size_t off) { return reinterpret_cast<const float*>(blob + off); };

  for (int i = tid; i < D; i += TTH) { c_bq1[i] = G(A.L.bq1)[i]; c_bv1[i] = G(A.L.bv1)[i]; c_bf[i] = G(A.L.bf)[i]; c_bm[i] = G(A.L.bm)[i]; }
  for (int i = tid; i < 2 * D; i += TTH) { c_bgb[i] = G(A.L.bgb)[2 * h * D + i]; c_acq[i] = G(A.L.acq)[i]; c_acv[i] = G(A.L.acv)[i]; }

  const unsigned pQ1 = (unsigned)A.L.aq1, pV1 = (unsigned)A.L.av1, pF = (unsigned)A.L.af, pM = (unsigned)A.L.am;
  const unsigned pGB = (unsigned)A.L.agb + (unsigned)h * PANEL_GB;
  Pipe P;
  P.rs = make_blob_rsrc(blob, (unsigned)A.L.total);
  P.rs2 = P.rs;

  const int b = blockIdx.y;
  const int n0 = (blockIdx.x * QG + qgi) * 16;
  const int n = min(n0 + col, A.N - 1);                  // tail queries: clamped on load, guarded on store
  const QueryPt q = load_query(A.x + (size_t)b * A.x_bstride + (size_t)n * A.dx, A.dx, A.inv);
  float tq[3] = {0.f, 0.f, 0.f};                         // the query's direction: x's row, clamped as x is
  {
    const float* xd = A.xdot + (size_t)b * A.xdot_bstride + (size_t)n * A.dx;
    tq[0] = xd[0];
    if (A.dx > 1) tq[1] = xd[1];
    if (A.dx > 2) tq[2] = xd[2];
  }
  tan_first_stage<ST_DD>(P, ring, pQ1, wave, lane);      // (its barrier also publishes the constants)

  // softmax state against a per-column reference logit (the first one seen), as enf_pair_tangent_kernel: Y, C, L, T, S and beside them
  // U = sum e (d2y + 2 dl dy + (d2l + dl^2) y), R = sum e (d2l + dl^2)
  float sm_m = -INFINITY, sm_l = 0.f, sm_c = 0.f, sm_s = 0.f, sm_r = 0.f;
  f32x4 Y[NT], T[NT], U[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) { Y[t] = f32x4{0.f, 0.f, 0.f, 0.f}; T[t] = f32x4{0.f, 0.f, 0.f, 0.f}; U[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  const int ltstride = enf_lt_stride(H, D);
  const f32x4 tp0 = {0.f, 0.f, 0.f, 0.f};
  // a wave whose share of the latents is empty keeps the staging / barrier cadence and stays at m = -inf, sums 0
  const int iters = (A.Z + ZS - 1) / ZS;
  for (int it = 0; it < iters; ++it) {
    const int z = it * ZS + zs;
    const bool active = z < A.Z;
    const unsigned wrap = it + 1 < iters ? pQ1 : NO_STAGE;
    const float* ltrow = A.lt + ((size_t)b * A.Z + (active ? z : A.Z - 1)) * ltstride;
    // the head's per-latent vectors u_h | v0_h -> wave-private LDS
#pragma unroll
    for (int i = lane * 4; i < D; i += 256) {
      *reinterpret_cast<f32x4*>(zv + i) = *reinterpret_cast<const f32x4*>(ltrow + enf_lt_off_u(H, D) + h * D + i);
      *reinterpret_cast<f32x4*>(zv + D + i) = *reinterpret_cast<const f32x4*>(ltrow + enf_lt_off_v0(H, D) + h * D + i);
    }
    const f32x4 pz = *reinterpret_cast<const f32x4*>(ltrow + enf_lt_off_pose(H, D));
    const float wcoef = ltrow[enf_lt_off_wcoef(H, D)];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    float inv[4], win, dinv[4], dwin, d2inv[4], d2win;
    pair_invariant<enf_bf16_valued(BF16)>(A.inv, A.dx, q, pz, wcoef, A.use_window, inv, win);
    pair_invariant_tan<enf_bf16_valued(BF16), true>(A.inv, A.dx, q, pz, wcoef, A.use_window, inv, win, tp0, 0.f, tq, dinv, dwin);
    pair_invariant_sec<enf_bf16_valued(BF16)>(A.inv, A.dx, q, pz, wcoef, A.use_window, inv, win, tq, dinv, d2inv, d2win);

    float logit, dlogit, d2logit;
    Frags<BF16, KB> F, dF, d2F;
    {  // ---------------- query branch: h1 = relu(W1q^T E + b), logit = h1 . u_h + c_h + win and its two derivatives
      f32x4 acc[NT], dacc[NT], d2acc[NT];
      rff_embed3<D, BF16>(acc, dacc, d2acc, inv, dinv, d2inv, c_acq, lane, quad);
      make_frags<BF16, KB>(F, acc);
      make_frags<BF16, KB>(dF, dacc);
      make_frags<BF16, KB>(d2F, d2acc);
      TAN_BIAS(acc, c_bq1);
      panel_gemm3<KB, NT, BF16, ST_DD>(acc, dacc, d2acc, F, dF, d2F, P, ring, pQ1, pV1, active, lane);
      float s = 0.f, ds = 0.f, d2s = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const f32x4 u = rowvec(zv, t, quad);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool on = acc[t][i] > 0.f;
          s = fmaf(relu_f(acc[t][i]), u[i], s);
          ds = fmaf(on ? dacc[t][i] : 0.f, u[i], ds);
          d2s = fmaf(on ? d2acc[t][i] : 0.f, u[i], d2s);
        }
      }
      logit = xquad_sum(s) + ltrow[enf_lt_off_c(H, D) + h] + win;
      dlogit = xquad_sum(ds) + dwin;
      d2logit = xquad_sum(d2s) + d2win;
    }
    f32x4 v[NT], dv[NT], d2v[NT];
    {  // ---------------- value branch: RFFNet layer, folded Dense, gelu, LayerNorm
      f32x4 acc[NT], dacc[NT], d2acc[NT];
      rff_embed3<D, BF16>(acc, dacc, d2acc, inv, dinv, d2inv, c_acv, lane, quad);
      make_frags<BF16, KB>(F, acc);
      make_frags<BF16, KB>(dF, dacc);
      make_frags<BF16, KB>(d2F, d2acc);
      TAN_BIAS(acc, c_bv1);
      panel_gemm3<KB, NT, BF16, ST_DD>(acc, dacc, d2acc, F, dF, d2F, P, ring, pV1, pF, active, lane);
      relu_tangent<NT>(acc, dacc);
      relu_tangent<NT>(acc, d2acc);
      make_frags<BF16, KB>(F, acc);
      relu_frags<BF16, KB>(F);
      make_frags<BF16, KB>(dF, dacc);
      make_frags<BF16, KB>(d2F, d2acc);
      TAN_BIAS(acc, c_bf);
      panel_gemm3<KB, NT, BF16, ST_GB>(acc, dacc, d2acc, F, dF, d2F, P, ring, pF, pGB, active, lane);
      gelu_second<NT>(acc, dacc, d2acc);
      float mu, rstd;
      ln_stats<NT>(acc, mu, rstd, A.inv_d);
      ln_apply<NT>(acc, mu, rstd);
      ln_second<NT>(dacc, d2acc, acc, rstd, A.inv_d);
      make_frags<BF16, KB>(F, acc);      // the normalised f and its two streams: the operands of the head's gamma/beta panel
      make_frags<BF16, KB>(dF, dacc);
      make_frags<BF16, KB>(d2F, d2acc);
    }
    gb_panel3<D, BF16, ST_DD>(v, dv, d2v, F, dF, d2F, P, ring, pGB, pM, active, c_bgb, zv + D, lane, quad);
    make_frags<BF16, KB>(F, v);
    make_frags<BF16, KB>(dF, dv);
    make_frags<BF16, KB>(d2F, d2v);
    TAN_BIAS(v, c_bm);
    panel_gemm3<KB, NT, BF16, ST_DD>(v, dv, d2v, F, dF, d2F, P, ring, pM, wrap, active, lane);
    gelu_second<NT>(v, dv, d2v);
    float mu, rstd;
    ln_stats<NT>(v, mu, rstd, A.inv_d);
    if (active) {
      if (it == 0) sm_m = logit;
      const bool far = logit - sm_m > 40.0f;
      if (__any(far)) {                 // the rare "logit far above the reference" case rescales the sums (wave-uniform branch)
        const float alpha = far ? __expf(sm_m - logit) : 1.0f;
        sm_l *= alpha; sm_c *= alpha; sm_s *= alpha; sm_r *= alpha;
        if (far) sm_m = logit;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) { Y[t][i] *= alpha; T[t][i] *= alpha; U[t][i] *= alpha; }
      }
      const float pe = __expf(logit - sm_m);
      const float w = pe * rstd;
      sm_l += pe;
      sm_c = fmaf(w, mu, sm_c);
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) Y[t][i] = fmaf(w, v[t][i], Y[t][i]);
    }
    ln_apply<NT>(v, mu, rstd);                         // v <- y
    ln_second<NT>(dv, d2v, v, rstd, A.inv_d);
    if (active) {
      const float pe = __expf(logit - sm_m);
      const float dl = dlogit, ql = fmaf(dl, dl, d2logit), dl2 = 2.f * dl;
      sm_s = fmaf(pe, dl, sm_s);
      sm_r = fmaf(pe, ql, sm_r);
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          T[t][i] = fmaf(pe, fmaf(dl, v[t][i], dv[t][i]), T[t][i]);
          U[t][i] = fmaf(pe, fmaf(ql, v[t][i], fmaf(dl2, dv[t][i], d2v[t][i])), U[t][i]);
        }
    }
  }

  // ---- combine the ZS latent splits of each query group (all staging is finished: the ring is free)
  if (quad == 0) {
    float* e = xch + (wave * 5) * 16 + col;
    e[0] = sm_m; e[16] = sm_l; e[32] = sm_c; e[48] = sm_s; e[64] = sm_r;
  }
  __syncthreads();
  float cs, sb, rb;
  {
    float ms = -INFINITY;
    for (int s = 0; s < ZS; ++s) ms = fmaxf(ms, xch[((s * QG + qgi) * 5) * 16 + col]);
    float L = 0.f, C = 0.f, S = 0.f, R = 0.f;
    for (int s = 0; s < ZS; ++s) {
      const float* e = xch + ((s * QG + qgi) * 5) * 16 + col;
      const float aw = __expf(e[0] - ms);         // exp(-inf) = 0 for a split that saw no latent
      L = fmaf(aw, e[16], L);
      C = fmaf(aw, e[32], C);
      S = fmaf(aw, e[48], S);
      R = fmaf(aw, e[64], R);
    }
    cs = C / L; sb = S / L; rb = R / L;
    const float sc = __expf(sm_m - ms) / L;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) { Y[t][i] *= sc; T[t][i] *= sc; U[t][i] *= sc; }
  }
  // deterministic tree over the split index: splits [s, 2s) hand their partial sums to [0, s)
  float* cb = reinterpret_cast<float*>(ring);
  constexpr int YF = SM::YBYTES / 4;
  for (int s = ZS >> 1; s >= 1; s >>= 1) {
    if (zs >= s && zs < 2 * s) {
      float* dst = cb + (size_t)((zs - s) * QG + qgi) * (3 * YF);
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          dst[(t * 4 + i) * 64 + lane] = Y[t][i];
          dst[YF + (t * 4 + i) * 64 + lane] = T[t][i];
          dst[2 * YF + (t * 4 + i) * 64 + lane] = U[t][i];
        }
    }
    __syncthreads();
    if (zs < s) {
      const float* src = cb + (size_t)(zs * QG + qgi) * (3 * YF);
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          Y[t][i] += src[(t * 4 + i) * 64 + lane];
          T[t][i] += src[YF + (t * 4 + i) * 64 + lane];
          U[t][i] += src[2 * YF + (t * 4 + i) * 64 + lane];
        }
    }
    __syncthreads();
  }
  if (zs == 0 && n0 + col < A.N) {
    const size_t row = ((size_t)b * A.N + n0 + col) * HD + h * D;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x4 o = Y[t], d = T[t], d2 = U[t];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o[i] -= cs;
        d[i] = fmaf(-sb, o[i], d[i]);
        d2[i] = fmaf(-rb, o[i], fmaf(-2.f * sb, d[i], d2[i]));
      }
      *reinterpret_cast<f32x4*>(A.ybar + row + 16 * t + 4 * quad) = o;
      *reinterpret_cast<f32x4*>(A.ydot + row + 16 * t + 4 * quad) = d;
      *reinterpret_cast<f32x4*>(A.y2 + row + 16 * t + 4 * quad) = d2;
    }
  }
}

// ---------------------------------------------------------------- launch (launch_pair_tail, enf_tangent_common.h) and workspace
// one head per grid.z; the tail is the order-2 instantiation of enf_tail_tangent_kernel
template <class S> bool pair_launch(S, const PairSecArgs& PA, hipStream_t st) {
  constexpr int lds = SecSmem<S::D>::TOTAL;
  constexpr auto pk = enf_pair_second_kernel<S::D, S::H, S::BF16>;
  if (!enf_lds_attr<pk>(lds)) return false;
  hipLaunchKernelGGL(pk, dim3((PA.N + 16 * PA.qg - 1) / (16 * PA.qg), PA.B, S::H), dim3(TTH), lds, st, PA);
  return hipGetLastError() == hipSuccess;
}

// enf_field_tangent_workspace_bytes' regions at their offsets, then d2 ybar: one buffer serves the plain and the tangent calls too
struct SecWorkspace { TanWorkspace T; size_t y2, total; };
SecWorkspace sec_workspace(const EnfDims& m) {
  SecWorkspace S;
  S.T = tan_workspace(m, false);
  S.y2 = S.T.total;
  S.total = S.y2 + enf_align(sizeof(float) * (size_t)m.B * m.N * m.HD);
  return S;
}

}  // namespace

extern "C" size_t enf_field_second_workspace_bytes(const EnfDesc* d) {
  if (enf_check_desc(d) != ENF_OK || !tangent_supported(d)) return 0;
  return sec_workspace(enf_dims(d)).total;
}

extern "C" int enf_field_second_x(const EnfDesc* d, const float* x, int64_t x_bstride, const float* xdot, int64_t xdot_bstride,
                                  const float* p, const float* a, const float* sigma, const void* blob, float* out, float* tan,
                                  float* tan2, void* workspace, void* stream) {
  TanCall c;       // (the call takes no workspace size)
  int rc = tan_call(c, d, x && xdot && a && tan2, p, sigma, blob, workspace, ~(size_t)0, false, stream);
  if (rc) return rc;
  const EnfDims& m = c.m;
  if ((rc = enf_launch_prologue(m, c.L, c.blob, p, a, sigma, c.F(c.W.lt), c.F(c.W.an), c.F(c.W.kv), c.st))) return rc;
  const SecWorkspace S = sec_workspace(m);
  PairSecArgs PA;
  PA.x = x; PA.x_bstride = x_bstride; PA.xdot = xdot; PA.xdot_bstride = xdot_bstride; PA.lt = c.F(c.W.lt); PA.blob = c.blob; PA.L = c.L;
  PA.ybar = c.F(c.W.ybar); PA.ydot = c.F(S.T.ydot); PA.y2 = c.F(S.y2); PA.inv_d = 1.0f / (float)m.Dt;
  PA.B = m.B; PA.N = m.N; PA.Z = m.Z; PA.dx = m.dx; PA.inv = m.inv; PA.use_window = m.use_window;
  const int zs = enf_latent_splits(m.Z);                 // as many latent splits as there are latents to split, up to one per wave
  PA.qg = TW / (zs < TW ? zs : TW);
  TailTanArgs2 TA;
  TA.ybar = PA.ybar; TA.ydot = PA.ydot; TA.y2 = PA.y2; TA.blob = c.blob; TA.L = c.L; TA.out = out; TA.tan = tan; TA.tan2 = tan2;
  TA.NQ = m.B * m.N; TA.O = m.O; TA.inv_hd = 1.0f / (float)(m.Ht * m.Dt);
  return launch_pair_tail(m, PA, TA, c.st);
}
