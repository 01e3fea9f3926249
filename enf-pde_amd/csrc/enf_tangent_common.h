// enf_tangent_common.h -- what the forward-mode kernel families share: the first-order one (enf_tangent.hip: tangent and Gauss-Newton
// kernels) and the second-order one (enf_second.hip).  The four-wave staging cadence, the doubled panel product and the first-order
// rules of the activations, the pair kernel's LDS map, the doubled tail chain, and the host sequence of the entry points (refusals,
// dimensions, workspace).  Everything has internal linkage; include it behind enf_launch.h, enf_device.h, enf_pair_common.h and
// enf_tail_common.h.
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
