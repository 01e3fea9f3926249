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
//                                 (enf_tangent_common.h: the order-1 instantiations of the kernel enf_second.hip runs at order 2)
// The same file holds the Gauss-Newton product (enf_gn_product, at the end): prologue tangent and pair kernel as above -- the pair
// kernel then also stores lse for the backward pair kernel -- and
//   enf_gn_tail_kernel            the tail's chain with tangents, d out = w tan formed in registers, the tail's backward chain
// followed by the backward pair kernel and the prologue backward of the other files.  enf_gn_product_g is the same product for grouped
// observations (cell averages): the same host sequence (gn_product_sequence) with the GRP instantiation of the tail, which forms the
// group sum of the tangent over the wave's query lanes in front of d out.  enf_gn_product_a is the product for a sparse observation
// operator: the same host sequence with the tail cut open -- the stash form of enf_tail_tangent_kernel, the two products of enf_obs.hip
// on tan in memory, enf_tail.hip's backward on the stash.
// There is one copy of each thing the entry points have in common, here and in enf_second.hip: the tail chain with its derivative
// streams (tail_forward<.., ORDER, SAVE, ..> of enf_tangent_common.h, which stashes the pre-activations for the Gauss-Newton tails
// only), the panel product (panel_gemm2, whose one-operand form serves the backward chain), the launcher and its (D, H) dispatch
// (launch_pair_tail, which takes this file's pair kernel through pair_launch and its Gauss-Newton tails through tail_kernel), and the
// host sequence (tan_call: refusals, dimensions, workspace; tan_launch_prologue; tan_pair_args).  The row moves, the chain's
// shapes and the constants' load are enf_tail.hip's (enf_tail_common.h).  Not shared: the Gauss-Newton tail's backward chain, a copy
// of enf_tail_bwd_kernel's (see there).
// Register room: at D = 128, H = 2 the accumulators Y and T alone are 128 registers, so these kernels run ONE wave per SIMD
// (workgroups of 4 waves, a 512-register budget) instead of K2's two.  Every output element is written once, by one lane, in a fixed
// order of operations: no atomics, the call is bit-reproducible run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include "enf_launch.h"
#include "enf_device.h"
#include "enf_pair_common.h"
#include "enf_tail_common.h"
#include "enf_tangent_common.h"

namespace {

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

// ---------------------------------------------------------------- (c) the tail: enf_tail_tangent_kernel (enf_tangent_common.h)

// ---------------------------------------------------------------- (d) the Gauss-Newton tail (include/enf_hip.h, "Gauss-Newton product")
// tail_forward's chain (enf_tangent_common.h) at order 1 with the stash, then d out = (w > 0 ? w tan : 0) gs formed in registers where
// tail_sq_err forms its gradient, then a backward chain on the stash: d ybar and delta for the backward pair kernel.  Neither tan nor
// d out reaches memory and the forward chain runs once.  One wave per SIMD, the 2-slot ring with four waves issuing, as every kernel
// of this file.
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
  float gs;              // 2 grad_scale / (B N O); grouped: 2 grad_scale / (B M O), M = N / G
};
// The grouped form's arguments (include/enf_hip.h, "Grouped observations"), appended behind the block every other instantiation takes:
// a longer shared block would move their scalar loads ("Grouped observations").
struct GnTailArgsG : GnTailArgs {
  int G;                 // 1, 2, 4, 8 or 16; NQ % G == 0
  const float* qweight;  // nullptr (every factor is 1 / G), or one quadrature factor per query (NQ floats, finite)
  const float* oweight;  // nullptr (1), or one weight per observation (NQ / G floats, >= 0); the zero-weight select of `weight`
};

// GRP (enf_gn_product_g): the seed is that of a loss on grouped observations.  The wave's 16 rows sit in do4 in the hot tail's lane
// layout (tile start a multiple of 16, lane = (col, quad)), so the tangent of the group sums is tail_sq_err_g's xor tree (enf_tail.hip)
// on do4, in place -- do4 is dead behind the seed -- and d out = q w obs_tan gs in that function's order of operations, contraction off:
// every lane of a group holds the same bits.  As stated there, a group never straddles a tile, a signal or the clamped rows beyond NQ:
// tiles start at multiples of 16, G divides 16 and G divides N.  One instantiation serves every G; `weight` and `cw` are not read.
template <int D, int H, bool BF16, bool GRP = false>
__global__ __launch_bounds__(TTH, 1) void enf_gn_tail_kernel(std::conditional_t<GRP, GnTailArgsG, GnTailArgs> A) {
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
    f32x4 o4[2][2];
    const float* const rows[2] = {yrow, A.ydot + (size_t)qi * HD};
    tail_forward<D, H, BF16, 1, true, T::ST_G4>(o4, rows, act, L, reinterpret_cast<const float*>(smem + TailTanSmem<D, H>::CONSTS), P,
                                                ring, (unsigned)L.gto4, lane, quad, A.inv_hd);
    f32x4 (&do4)[2] = o4[1];
    if constexpr (GRP) {
      // ---- d out = (w > 0 ? q (w obs_tan) : 0) gs,  obs_tan = sum_k q tan over the group: a weight of 0 is a select per observation
#pragma clang fp contract(off)
      const int G = A.G;
      const float q = A.qweight ? A.qweight[qi] : 1.0f / (float)G;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) do4[t][i] = qvalid ? q * do4[t][i] : 0.f;
#define ENF_GROUP_STEP(K_)                                             \
  if (G > K_) {                                                        \
    _Pragma("unroll") for (int t = 0; t < 2; ++t)                      \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) do4[t][i] += __shfl_xor(do4[t][i], K_, 64); \
  }
      ENF_GROUP_STEP(1) ENF_GROUP_STEP(2) ENF_GROUP_STEP(4) ENF_GROUP_STEP(8)
#undef ENF_GROUP_STEP
      const float w = A.oweight ? A.oweight[qi >> __builtin_ctz(G)] : 1.f;
      const bool live = qvalid && w > 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int o = 16 * t + 4 * quad + i;
          g0[t][i] = (o < A.O && live) ? (q * (w * do4[t][i])) * A.gs : 0.f;
        }
    } else {
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

// ---------------------------------------------------------------- launch (launch_pair_tail, enf_tangent_common.h): this file's parts
template <int D, int H, bool BF16> constexpr auto tail_kernel(const GnTailArgs*) { return enf_gn_tail_kernel<D, H, BF16>; }
template <int D, int H, bool BF16> constexpr auto tail_kernel(const GnTailArgsG*) { return enf_gn_tail_kernel<D, H, BF16, true>; }

// the pair kernel with or without the query tangent
template <class S> bool pair_launch(S, const PairTanArgs& PA, hipStream_t st) {
  constexpr int lds = TanSmem<S::D, S::H>::TOTAL;
  constexpr auto pk0 = enf_pair_tangent_kernel<S::D, S::H, S::BF16, false>, pkx = enf_pair_tangent_kernel<S::D, S::H, S::BF16, true>;
  if (!(PA.xdot ? enf_lds_attr<pkx>(lds) : enf_lds_attr<pk0>(lds))) return false;
  hipLaunchKernelGGL(PA.xdot ? pkx : pk0, dim3((PA.N + 16 * PA.qg - 1) / (16 * PA.qg), PA.B), dim3(TTH), lds, st, PA);
  return hipGetLastError() == hipSuccess;
}

// ---------------------------------------------------------------- the host sequence of both entry points
constexpr unsigned GN_FLAGS = ENF_BWD_DETERMINISTIC | ENF_GN_REUSE_POINT;

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

// The one copy of the product's host sequence, seeded by the loss `ls` describes (enf_launch.h: EnfLossSpec): on points the weights
// (B, N) or (B, N, O); on grouped observations the grouped instantiation of the tail with the factors and observation weights,
// 1 / (B M O) in the scale.  What ls.check refuses is ENF_EINVAL, behind ENF_EUNSUPPORTED and before ENF_EWORKSPACE.
// An operator couples rows across tiles and waves, so its tail is cut open as the fit step's: the tangent tail's stash form leaves tan
// and the stash, the two products of enf_obs.hip form d out = gs A^T (w A tan) in memory, and the tail's own backward (enf_tail.hip,
// the stash form) runs on it.  Both tails store TailCfg's layout per query through store_rows, so the one reads the other's stash.
namespace {
// enf_gn_product_a's regions behind tan_workspace(..).total: tan (B, N, O) | r (B, M, O) | d out (B, N, O).  The total is never below
// the deterministic enf_obs_workspace, so one buffer serves the fit step, the products and the evaluation of an LM step.
struct GnObsWorkspace { size_t tan, r, dout, total; };
GnObsWorkspace gn_obs_workspace(const EnfDims& m, bool det, int M) {
  GnObsWorkspace Y;
  const size_t bno = enf_align(sizeof(float) * (size_t)m.B * m.N * m.O);
  Y.tan = tan_workspace(m, det).total;
  Y.r = Y.tan + bno;
  Y.dout = Y.r + enf_align(sizeof(float) * (size_t)m.B * (size_t)M * m.O);
  Y.total = Y.dout + bno;
  const EnfWorkspace W = enf_workspace(m);
  const size_t fit = enf_obs_workspace(m, enf_det_workspace(m, W).total, M).total;
  if (Y.total < fit) Y.total = fit;
  return Y;
}

int gn_product_sequence(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                        const float* vp, const float* va, const float* vsigma, const void* packed, float grad_scale, float* gp, float* ga,
                        float* gsigma, void* workspace, size_t workspace_bytes, unsigned flags, void* stream, const EnfLossSpec& ls) {
  const bool det = (flags & ENF_BWD_DETERMINISTIC) != 0, reuse = (flags & ENF_GN_REUSE_POINT) != 0;
  TanCall c;
  int rc = tan_call(c, d, x && a && gp && ga && gsigma && (vp || va || vsigma) && !(flags & ~GN_FLAGS) && ls.check(d, flags, ENF_LOSS_GN) == ENF_OK,
                    p, sigma, packed, workspace, workspace_bytes, det, stream);
  if (rc) return rc;
  const EnfDims& m = c.m;
  const EnfLayout& L = c.L;
  const EnfWorkspace& W = c.W;
  hipStream_t st = c.st;
  const char* pk = c.blob;
  const bool zb = enf_use_zfold_bwd(m), grp = ls.kind == ENF_LOSS_GROUPS, ao = ls.kind == ENF_LOSS_OPERATOR;
  const GnObsWorkspace Y = gn_obs_workspace(m, det, ao ? ls.op->M : 1);
  if (ao && workspace_bytes < Y.total) return ENF_EWORKSPACE;
  if ((rc = enf_side_join_pending(st, workspace))) return rc;
  // the point: latent table, what the prologue backward reads, and the z-fold backward's per-latent matrices -- unless the caller
  // vouches that a fit step or an earlier product at this point left them
  if (!reuse) {
    if ((rc = enf_launch_prologue(m, L, pk, p, a, sigma, c.F(W.lt), c.F(W.an), c.F(W.kv), st))) return rc;
    if (zb && (rc = enf_launch_wz(m, L, pk, c.F(W.lt), nullptr, c.F(W.wzb), nullptr, c.ws + W.wzt, st))) return rc;
  }
  if ((rc = tan_launch_prologue(c, vp, va, vsigma))) return rc;
  const PairTanArgs PA = tan_pair_args(c, x, x_bstride, c.F(W.lse));
  GnTailArgsG GA;
  GA.ybar = PA.ybar; GA.ydot = PA.ydot; GA.blob = pk; GA.L = L;
  GA.weight = grp ? nullptr : (ls.cweight ? ls.cweight : ls.weight); GA.cw = !grp && ls.cweight != nullptr;
  GA.dybar = c.F(W.dybar); GA.delta = c.F(W.delta); GA.act = c.F(W.tail_act);
  GA.NQ = m.B * m.N; GA.O = m.O; GA.inv_hd = 1.0f / (float)(m.Ht * m.Dt);
  GA.gs = 2.0f * grad_scale / ((float)m.B * (float)ls.rows(m) * (float)m.O);
  if (ao) {
    // tan and the stash -> [kernel 1] r = w (A tan) -> [kernel 2] d out = gs A^T r -> the tail's backward on the stash
    TailTanArgsS TA;
    TA.ybar = PA.ybar; TA.ydot = PA.ydot; TA.blob = pk; TA.L = L; TA.out = nullptr; TA.tan = c.F(Y.tan);
    TA.NQ = GA.NQ; TA.O = m.O; TA.inv_hd = GA.inv_hd; TA.act = GA.act;
    if ((rc = launch_pair_tail(m, PA, TA, st))) return rc;
    if ((rc = enf_launch_obs_weigh(*ls.op, m.N, m.B, m.O, c.F(Y.tan), ls.weight, ls.cweight, c.F(Y.r), st))) return rc;
    if ((rc = enf_launch_obs_transpose(*ls.op, m.N, m.B, m.O, c.F(Y.r), GA.gs, c.F(Y.dout), st))) return rc;
    rc = enf_launch_tail(m, L, pk, PA.ybar, nullptr, c.F(Y.dout), GA.dybar, GA.delta, GA.act, ENF_TAIL_BWD | ENF_TAIL_STASH, st);
  } else if (grp) {
    GA.G = ls.G; GA.qweight = ls.qweight; GA.oweight = ls.weight;
    rc = launch_pair_tail(m, PA, GA, st);
  } else rc = launch_pair_tail(m, PA, static_cast<const GnTailArgs&>(GA), st);
  if (rc) return rc;
  // the backward pair kernel without a store, in the variant the descriptor resolves to; deterministic: through the partial rows and
  // the fixed-order reduction, which overwrites the gradient table
  if (!det && hipMemsetAsync(c.F(W.dlt), 0, enf_lt_bytes(m), st) != hipSuccess) return ENF_ELAUNCH;
  if ((rc = enf_launch_pair_bwd(m, L, pk, x, x_bstride, c.F(W.lt), c.F(W.lse), c.F(W.dybar), c.F(W.delta), c.F(W.dlt), nullptr,
                                c.fold_bwd(), nullptr, st, det ? c.F(c.X.part) : nullptr)))
    return rc;
  return enf_launch_prologue_bwd(m, L, pk, p, sigma, c.F(W.an), c.F(W.kv), c.F(W.dlt), gp, ga, gsigma, st);
}
}  // namespace

extern "C" int enf_gn_product(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                              const float* vp, const float* va, const float* vsigma, const void* packed, const float* weight,
                              const float* cweight, float grad_scale, float* gp, float* ga, float* gsigma, void* workspace,
                              size_t workspace_bytes, unsigned flags, void* stream) {
  return gn_product_sequence(d, x, x_bstride, p, a, sigma, vp, va, vsigma, packed, grad_scale, gp, ga, gsigma, workspace, workspace_bytes, flags,
                             stream, EnfLossSpec{ENF_LOSS_POINTS, weight, cweight});
}

// The product for grouped observations (include/enf_hip.h, "Gauss-Newton product on grouped observations")
extern "C" int enf_gn_product_g(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                                const float* vp, const float* va, const float* vsigma, const void* packed, int32_t G,
                                const float* qweight, const float* oweight, float grad_scale, float* gp, float* ga, float* gsigma,
                                void* workspace, size_t workspace_bytes, unsigned flags, void* stream) {
  return gn_product_sequence(d, x, x_bstride, p, a, sigma, vp, va, vsigma, packed, grad_scale, gp, ga, gsigma, workspace, workspace_bytes, flags,
                             stream, EnfLossSpec{ENF_LOSS_GROUPS, oweight, nullptr, nullptr, nullptr, G, qweight});
}

// The product for sparse linear observations (include/enf_hip.h, "Gauss-Newton product on sparse observations")
extern "C" size_t enf_gn_a_workspace_bytes(const EnfDesc* d, int32_t M, unsigned flags) {
  if (enf_check_desc(d) != ENF_OK || !tangent_supported(d) || M < 1 || (flags & ~GN_FLAGS)) return 0;
  return gn_obs_workspace(enf_dims(d), (flags & ENF_BWD_DETERMINISTIC) != 0, M).total;
}

extern "C" int enf_gn_product_a(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                                const float* vp, const float* va, const float* vsigma, const void* packed, const EnfSparseObs* op,
                                const float* oweight, const float* cweight, float grad_scale, float* gp, float* ga, float* gsigma,
                                void* workspace, size_t workspace_bytes, unsigned flags, void* stream) {
  return gn_product_sequence(d, x, x_bstride, p, a, sigma, vp, va, vsigma, packed, grad_scale, gp, ga, gsigma, workspace, workspace_bytes, flags,
                             stream, EnfLossSpec{ENF_LOSS_OPERATOR, oweight, cweight, nullptr, nullptr, 1, nullptr, op});
}
