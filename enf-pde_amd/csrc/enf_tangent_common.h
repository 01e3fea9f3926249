// enf_tangent_common.h -- what the forward-mode kernel families share: the first-order one (enf_tangent.hip: tangent and Gauss-Newton
// kernels) and the second-order one (enf_second.hip).  The four-wave staging cadence; the panel product and the rules of the
// activations, first order and second order side by side; the pair kernel's LDS map; and, ONE copy for both orders: the tail chain
// (tail_forward<.., ORDER, ..>), the tail kernel that stores its outputs (enf_tail_tangent_kernel<.., ORDER, SAVE>), the launcher of a
// pair kernel and its tail (launch_pair_tail), and the host sequence of the entry points (refusals, dimensions, workspace).
// Everything has internal linkage; include it behind enf_launch.h, enf_device.h, enf_pair_common.h and enf_tail_common.h.
#pragma once

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

// ---------------------------------------------------------------- the second-order forms of the rules above
// The three-operand form of panel_gemm2: acc += panel . F (the caller initialised acc), dacc = panel . dF, d2acc = panel . d2F (zero
// start, no bias), all from the SAME staged panel before its slot is released.
template <int KBIN, int MTOUT, bool BF16, int NEXT_BYTES>
DEV void panel_gemm3(f32x4 (&acc)[MTOUT], f32x4 (&dacc)[MTOUT], f32x4 (&d2acc)[MTOUT], const Frags<BF16, KBIN>& F,
                     const Frags<BF16, KBIN>& dF, const Frags<BF16, KBIN>& d2F, Pipe& P, char* ring, unsigned panel, unsigned next,
                     bool active, int lane) {
  using C = PanelCfg<KBIN, MTOUT, BF16>;
#pragma unroll
  for (int sp = 0; sp < C::SPP; ++sp) {
    if (sp + 1 < C::SPP) tan_issue<C::STAGE>(P, panel + (sp + 1) * C::STAGE, ring + (P.cur ^ 1) * STAGE_MAX, lane);
    else if (next != NO_STAGE) tan_issue<NEXT_BYTES>(P, next, ring + (P.cur ^ 1) * STAGE_MAX, lane);
    const char* slot = ring + P.cur * STAGE_MAX;
    if (active) {
      gemm_stage<BF16, KBIN, C::MTS, INIT_ACC>(&acc[sp * C::MTS], F, slot, lane);
      gemm_stage<BF16, KBIN, C::MTS, INIT_ZERO>(&dacc[sp * C::MTS], dF, slot, lane);
      gemm_stage<BF16, KBIN, C::MTS, INIT_ZERO>(&d2acc[sp * C::MTS], d2F, slot, lane);
    } else {
#pragma unroll
      for (int mt = 0; mt < C::MTS; ++mt) dacc[sp * C::MTS + mt] = d2acc[sp * C::MTS + mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    stage_close(P);
  }
}

// gelu_fg2 with the second derivative from the same sigmoid: with s = sigmoid(w), w = 2k(x + c x^3), w' = 2k(1 + 3c x^2), w'' = 12 k c x
//   g' = s + x s(1-s) w',   g'' = 2 s(1-s) w' + x s(1-s) ((1-2s) w'^2 + w'')
DEV void gelu_fgh2(f32x2 x, f32x2& g, f32x2& dg, f32x2& hg) {
  const float c = 0.7978845608028654f;
  const float c2 = -2.0f * c * 1.4426950408889634f;
  const f32x2 x2 = x * x;
  const f32x2 u = x * (x2 * (c2 * 0.044715f) + c2);
  f32x2 e;
  e[0] = __builtin_amdgcn_exp2f(u[0]);
  e[1] = __builtin_amdgcn_exp2f(u[1]);
  e = e + 1.0f;
  f32x2 s;
  s[0] = __builtin_amdgcn_rcpf(e[0]);
  s[1] = __builtin_amdgcn_rcpf(e[1]);
  g = x * s;
  const f32x2 gs = g - g * s, wp = x2 * (6.0f * c * 0.044715f) + 2.0f * c;
  dg = gs * wp + s;
  const f32x2 ss = s - s * s;
  hg = ss * wp * 2.0f + gs * ((1.0f - 2.0f * s) * wp * wp + x * (12.0f * c * 0.044715f));
}
// X <- gelu(X), dX <- gelu'(X) dX, d2X <- gelu'(X) d2X + gelu''(X) dX^2
template <int NT> DEV void gelu_second(f32x4 (&X)[NT], f32x4 (&dX)[NT], f32x4 (&d2X)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    f32x2 g0, d0, h0, g1, d1, h1;
    gelu_fgh2(lo2(X[t]), g0, d0, h0);
    gelu_fgh2(hi2(X[t]), g1, d1, h1);
    const f32x4 g = {g0[0], g0[1], g1[0], g1[1]}, d = {d0[0], d0[1], d1[0], d1[1]}, h = {h0[0], h0[1], h1[0], h1[1]};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      d2X[t][i] = fmaf(d[i], d2X[t][i], h[i] * dX[t][i] * dX[t][i]);
      dX[t][i] *= d[i];
    }
    X[t] = g;
  }
}

// LayerNorm without affine, y = (g - mu) rstd already applied; dg, d2g the raw streams on entry, dy, d2y on exit.  With
// m1 = mean(y dg) and means over the true width (exact with the eps):
//   dy = rstd (dg - mean dg - y m1)                                    (ln_tangent's expression)
//   d2y = rstd (d2g - mean d2g - y mean(y d2g)) - 2 rstd m1 dy - rstd y mean(dy dg)
// Every sum carries a raw stream as a factor, which is zero in zero-padded features: padding adds nothing.
template <int NT> DEV void ln_second(f32x4 (&dg)[NT], f32x4 (&d2g)[NT], const f32x4 (&y)[NT], float rstd, float inv_n) {
  float s, d, s2, dd2;
  tiles_sum_dot<NT>(dg, [&](int t) { return y[t]; }, s, d);
  tiles_sum_dot<NT>(d2g, [&](int t) { return y[t]; }, s2, dd2);
  const float m1 = xquad_sum(d) * inv_n;
  const float c0 = -(xquad_sum(s) * inv_n) * rstd, c1 = -m1 * rstd;
  float q = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float dy = fmaf(y[t][i], c1, fmaf(dg[t][i], rstd, c0));
      q = fmaf(dy, dg[t][i], q);
      dg[t][i] = dy;
    }
  const float mq = xquad_sum(q) * inv_n;
  const float e0 = -(xquad_sum(s2) * inv_n) * rstd, e1 = -(xquad_sum(dd2) * inv_n + mq) * rstd, f = -2.f * rstd * m1;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) d2g[t][i] = fmaf(f, dg[t][i], fmaf(y[t][i], e1, fmaf(d2g[t][i], rstd, e0)));
}

// ---------------------------------------------------------------- the tail chain's jets
// The tail chain carries a jet of order ORDER (1: the tangent and Gauss-Newton tails; 2: the second-order tail) as
// `f32x4 X[ORDER + 1][NT]` beside `Frags F[ORDER + 1]`: stream 0 the primal, stream k its k-th derivative along the call's direction.
// One front per rule picks the order's form above; the two forms stay side by side because the pair kernels call them directly and
// the fp32 D = 128 pair kernels' register allocation does not survive any change of what they call ("Forward-mode jets").
template <int NT> DEV void bias_fill(f32x4 (&acc)[NT], const float* vec, int quad) {
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = rowvec(vec, t, quad);
}
template <int ORDER, bool BF16, int KB> DEV void make_frags_jet(Frags<BF16, KB> (&F)[ORDER + 1], const f32x4 (&X)[ORDER + 1][2 * KB]) {
#pragma unroll
  for (int k = 0; k <= ORDER; ++k) make_frags<BF16, KB>(F[k], X[k]);
}
template <int ORDER, int KBIN, int MTOUT, bool BF16, int NEXT_BYTES>
DEV void panel_gemm_jet(f32x4 (&acc)[ORDER + 1][MTOUT], const Frags<BF16, KBIN> (&F)[ORDER + 1], Pipe& P, char* ring, unsigned panel,
                        unsigned next, int lane) {
  static_assert(ORDER == 1 || ORDER == 2, "order");
  if constexpr (ORDER == 1) panel_gemm2<KBIN, MTOUT, BF16, NEXT_BYTES>(acc[0], acc[1], F[0], F[1], P, ring, panel, next, true, lane);
  else panel_gemm3<KBIN, MTOUT, BF16, NEXT_BYTES>(acc[0], acc[1], acc[2], F[0], F[1], F[2], P, ring, panel, next, true, lane);
}
template <int ORDER, int NT> DEV void gelu_jet(f32x4 (&X)[ORDER + 1][NT]) {
  if constexpr (ORDER == 1) gelu_tangent<NT>(X[0], X[1]);
  else gelu_second<NT>(X[0], X[1], X[2]);
}
// X[0] = y, the LayerNorm's output
template <int ORDER, int NT> DEV void ln_jet(f32x4 (&X)[ORDER + 1][NT], float rstd, float inv_n) {
  if constexpr (ORDER == 1) ln_tangent<NT>(X[1], X[0], rstd, inv_n);
  else ln_second<NT>(X[1], X[2], X[0], rstd, inv_n);
}

// LDS map of every tail kernel: ring (2 slots) | tail_consts' vectors (enf_tail_common.h)
template <int D, int H> struct TailTanSmem {
  static constexpr int CONSTS = 2 * STAGE_MAX;                     // bB bF1 (HD each) | bO0 bO2 (D each) | bO4 (32)
  static constexpr int TOTAL = CONSTS + 4 * (2 * H * D + 2 * D + 32);
  static_assert(TOTAL <= TAN_LDS_MAX, "the tangent tail's LDS exceeds one CU's 160 KiB");
};

// tail_forward's chain (enf_tail.hip) for this wave's 16 queries with a jet beside every activation: o4[0] = the (padded) 32 network
// outputs, o4[k] their k-th derivatives; yrow[k] = the query's row of ybar and of its derivatives.  Precondition: the first stage of
// L.atb is resident in ring[P.cur] and visible.
// SAVE: stash the primal pre-activations and the LayerNorm's mu, rstd in `act` (TailCfg's layout) for a backward chain.
// next / NEXT_BYTES: the stage that streams behind the last panel (NO_STAGE: nothing follows).
template <int D, int H, bool BF16, int ORDER, bool SAVE, int NEXT_BYTES>
DEV void tail_forward(f32x4 (&o4)[ORDER + 1][2], const float* const (&yrow)[ORDER + 1], float* act, const EnfLayout& L, const float* cst,
                      Pipe& P, char* ring, unsigned next, int lane, int quad, float inv_hd) {
  using T = TailCfg<D, H, BF16>;
  constexpr int KB = T::KB, KBH = T::KBH, NT = T::NT, NTH = T::NTH, HD = T::HD;
  const float* c_bB = cst, *c_bF1 = cst + HD, *c_bO0 = cst + 2 * HD, *c_bO2 = cst + 2 * HD + D, *c_bO4 = cst + 2 * HD + 2 * D;
  f32x4 a[ORDER + 1][NTH], c[ORDER + 1][NT];
  Frags<BF16, KBH> FH[ORDER + 1];
  Frags<BF16, KB> FD[ORDER + 1];
#pragma unroll
  for (int k = 0; k <= ORDER; ++k) load_rows<NTH>(a[k], yrow[k], quad);
  make_frags_jet<ORDER, BF16, KBH>(FH, a);
  bias_fill<NTH>(a[0], c_bB, quad);
  panel_gemm_jet<ORDER, KBH, NTH, BF16, T::ST_TB>(a, FH, P, ring, (unsigned)L.atb, (unsigned)L.atf1, lane);
  if constexpr (SAVE) store_rows<NTH>(a[0], act, quad);
  gelu_jet<ORDER, NTH>(a);
  float mu, rstd;
  ln_stats<NTH>(a[0], mu, rstd, inv_hd);
  if constexpr (SAVE) {
    if (quad == 0) { act[T::ACT - 2] = mu; act[T::ACT - 1] = rstd; }
  }
  ln_apply<NTH>(a[0], mu, rstd);
  ln_jet<ORDER, NTH>(a, rstd, inv_hd);
  make_frags_jet<ORDER, BF16, KBH>(FH, a);
  bias_fill<NTH>(a[0], c_bF1, quad);
  panel_gemm_jet<ORDER, KBH, NTH, BF16, T::ST_O0>(a, FH, P, ring, (unsigned)L.atf1, (unsigned)L.ato0, lane);
  if constexpr (SAVE) store_rows<NTH>(a[0], act + HD, quad);
  gelu_jet<ORDER, NTH>(a);
  make_frags_jet<ORDER, BF16, KBH>(FH, a);
  bias_fill<NT>(c[0], c_bO0, quad);
  panel_gemm_jet<ORDER, KBH, NT, BF16, T::ST_O2>(c, FH, P, ring, (unsigned)L.ato0, (unsigned)L.ato2, lane);
  if constexpr (SAVE) store_rows<NT>(c[0], act + 2 * HD, quad);
  gelu_jet<ORDER, NT>(c);
  make_frags_jet<ORDER, BF16, KB>(FD, c);
  bias_fill<NT>(c[0], c_bO2, quad);
  panel_gemm_jet<ORDER, KB, NT, BF16, T::ST_O4>(c, FD, P, ring, (unsigned)L.ato2, (unsigned)L.ato4, lane);
  if constexpr (SAVE) store_rows<NT>(c[0], act + 2 * HD + D, quad);
  gelu_jet<ORDER, NT>(c);
  make_frags_jet<ORDER, BF16, KB>(FD, c);
  bias_fill<2>(o4[0], c_bO4, quad);
  panel_gemm_jet<ORDER, KB, 2, BF16, NEXT_BYTES>(o4, FD, P, ring, (unsigned)L.ato4, next, lane);
}

// What every tail kernel does before the chain: the LDS constants, the blob's resource, the first stage of the first panel (its barrier
// also publishes the constants).
template <int D, int H, bool BF16>
DEV void tail_tan_open(Pipe& P, char* smem, const char* blob, const EnfLayout& L, int tid) {
  tail_consts<D, H, BF16, TTH>(reinterpret_cast<float*>(smem + TailTanSmem<D, H>::CONSTS), blob, L, tid);
  P.rs = make_blob_rsrc(blob, (unsigned)L.total);
  P.rs2 = P.rs;
  tan_first_stage<TailCfg<D, H, BF16>::ST_TB>(P, smem, (unsigned)L.atb, tid >> 6, tid & 63);
}

// ---------------------------------------------------------------- the tail that stores the chain's outputs
struct TailTanArgs {
  const float* ybar; const float* ydot; const char* blob; EnfLayout L;
  float* out;            // (B N, O) or nullptr
  float* tan;            // (B N, O); at order 2: or nullptr
  int NQ, O;
  float inv_hd;          // 1 / (true heads * true num_hidden)
};
// What an instantiation reads beyond that block is appended behind it, as GnTailArgsG (enf_tangent.hip): a longer shared block would
// move the others' scalar loads.  The stash form (enf_gn_product_a):
struct TailTanArgsS : TailTanArgs {
  float* act;            // (NQ, TailCfg::ACT): the pre-activations and the LayerNorm's mu, rstd, as enf_tail_fwd_kernel<.., SAVE> leaves them
};
// order 2 (enf_field_second_x):
struct TailTanArgs2 : TailTanArgs {
  const float* y2;       // (B N, H D): d2 ybar
  float* tan2;           // (B N, O)
};
template <int ORDER, bool SAVE>
using TailTanArgsOf = std::conditional_t<ORDER == 2, TailTanArgs2, std::conditional_t<SAVE, TailTanArgsS, TailTanArgs>>;

// Stores out (optional), tan (optional at order 2) and, at order 2, tan2.
// SAVE (enf_gn_product_a): tail_forward's stash in `act` for enf_tail_bwd_kernel's stash form (enf_tail.hip), which runs behind the two
// operator products on `tan`; stores tan and no out.  Clamped (duplicate) queries stash the same values, as in the other tails.
template <int D, int H, bool BF16, int ORDER = 1, bool SAVE = false>
__global__ __launch_bounds__(TTH, 1) void enf_tail_tangent_kernel(TailTanArgsOf<ORDER, SAVE> A) {
  static_assert(ORDER == 1 || (ORDER == 2 && !SAVE), "the stash belongs to the first-order tail");
  constexpr int HD = H * D;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  const int q0 = blockIdx.x * (16 * TW) + wave * 16;
  const int qi = min(q0 + col, A.NQ - 1);          // tail queries: clamped on load, guarded on store
  Pipe P;
  tail_tan_open<D, H, BF16>(P, smem, A.blob, A.L, tid);
  const float* yrow[ORDER + 1];
  yrow[0] = A.ybar + (size_t)qi * HD;
  yrow[1] = A.ydot + (size_t)qi * HD;
  if constexpr (ORDER >= 2) yrow[2] = A.y2 + (size_t)qi * HD;
  float* act = nullptr;
  if constexpr (SAVE) act = A.act + (size_t)qi * TailCfg<D, H, BF16>::ACT;
  f32x4 o4[ORDER + 1][2];
  tail_forward<D, H, BF16, ORDER, SAVE, 1024>(o4, yrow, act, A.L, reinterpret_cast<const float*>(smem + TailTanSmem<D, H>::CONSTS), P,
                                              smem, NO_STAGE, lane, quad, A.inv_hd);
  if (q0 + col < A.NQ) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int o = 16 * t + 4 * quad + i;
        if (o < A.O) {
          const size_t at = (size_t)(q0 + col) * A.O + o;
          if constexpr (!SAVE) {
            if (A.out) A.out[at] = o4[0][t][i];
          }
          if constexpr (ORDER >= 2) {
            if (A.tan) A.tan[at] = o4[1][t][i];
            A.tan2[at] = o4[2][t][i];
          } else A.tan[at] = o4[1][t][i];
        }
      }
  }
}

// ---------------------------------------------------------------- launch: the entry point's pair kernel, then its tail
// Each file says what is its own by overloads on its argument structs, found through their namespace where launch_pair_tail is
// instantiated: pair_launch(EnfShape, pair arguments, stream) -- the pair kernel's selection, LDS size and grid -- and
// tail_kernel<D, H, BF16>(tail arguments*) for the tails beyond the three above.
template <int D, int H, bool BF16> constexpr auto tail_kernel(const TailTanArgs*) { return enf_tail_tangent_kernel<D, H, BF16>; }
template <int D, int H, bool BF16> constexpr auto tail_kernel(const TailTanArgsS*) { return enf_tail_tangent_kernel<D, H, BF16, 1, true>; }
template <int D, int H, bool BF16> constexpr auto tail_kernel(const TailTanArgs2*) { return enf_tail_tangent_kernel<D, H, BF16, 2>; }

// the instantiations: every entry point dispatches here
template <class PairArgsT, class TailArgsT>
int launch_pair_tail(const EnfDims& m, const PairArgsT& PA, const TailArgsT& TA, hipStream_t st) {
  return enf_for_shape(m, [&](auto s) {
    constexpr int D = s.D, H = s.H;
    constexpr bool BF16 = s.BF16;
    constexpr int tail_lds = TailTanSmem<D, H>::TOTAL;
    constexpr auto tk = tail_kernel<D, H, BF16>((const TailArgsT*)nullptr);
    if (!enf_lds_attr<tk>(tail_lds) || !pair_launch(s, PA, st)) return (int)ENF_ELAUNCH;
    hipLaunchKernelGGL(tk, dim3((TA.NQ + 16 * TW - 1) / (16 * TW)), dim3(TTH), tail_lds, st, TA);
    return hipGetLastError() == hipSuccess ? 0 : (int)ENF_ELAUNCH;
  });
}

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

}  // namespace
