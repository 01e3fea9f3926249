// enf_tail.hip -- per-query tail of the decoder, forward and backward.
//
// Input: ybar (B,N,H*D) = softmax-weighted sum of the mixer's normalised gelu output (K2).
// Because softmax weights sum to 1, everything linear after ECA:144 is applied once per query:
//   WB  = blockdiag(diag(LN.scale) Dense_1 [mixer, ECA:19-20]) . attn.out_proj (ECA:150) . ffn.Dense_0 (ECA:17)
//   gelu, LayerNorm (ECA:18-19), WF1 = diag(LN.scale) ffn.Dense_1 (ECA:20)            [block FFN, NEF:66]
//   gelu (NEF:230), out_proj: Dense, gelu, Dense, gelu, Dense (NEF:196-202,233)
// One wave = 16 queries, transposed chain as in enf_device.h; 8 waves share the LDS weight ring.
// The backward kernel recomputes this forward (stashing pre-activations in the workspace),
// then runs dX = W dY through the transposed panels and emits d(ybar) and
// delta[n,h] = sum_d d(ybar)[n,h,d] * ybar[n,h,d]  (the softmax-backward row constant).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <type_traits>
#include "enf_launch.h"
#define ENF_PIPE_ONE_RS 1      // the tail streams from the weight blob only (enf_device.h: stage_issue_p)
#include "enf_device.h"
#include "enf_tail_common.h"     // load_rows, store_rows, zero_tiles, TailCfg, tail_consts

struct TailArgs {
  const float* ybar; const char* blob; EnfLayout L;
  float* out;            // forward: (B*N, O)
  const float* dout;     // backward
  float* dybar; float* delta; float* act;   // backward outputs + scratch (B*N x (2HD + 2D + 2))
  const float* target; float* loss; float gscale, inv_n;     // fused loss (LOSS): d out = 2 (out - target) inv_n gscale, *loss += mean sq. error
  const float* weight;   // LOSS: nullptr, or one loss weight per query (NQ floats, >= 0): se += w (out - target)^2, d out *= w; a query of weight
                         // 0 does not exist -- its target is never used in arithmetic (it may be NaN) and its d out is exactly 0
                         // LOSS + CW (the kernel's template flag): one weight per OUTPUT VALUE instead, (NQ, O) floats, never nullptr;
                         // the same rule per value
  float* err;            // LOSS / EVAL: nullptr, or the weighted squared error of every query, err[n] = sum_o w (out - target)^2 (NQ floats,
                         // OVERWRITTEN; include/enf_hip.h, "Per-signal and per-point errors"): lanes 0..15 of a wave store their 16 queries
  float* loss_part;      // LOSS, deterministic mode: wave w of workgroup g stores its partial in loss_part[g * NWAVES + w] (nullptr: atomic)
  float* tdel;           // weight-gradient backward (WG): per query d a_B | d a_F1 | d a_O0 | d a_O2 (2HD + 2D floats); the layer INPUTS
                         // n^ | gelu(a_F1) | gelu(a_O0) | gelu(a_O2) replace the pre-activations in `act` (enf_train.hip forms X^T delta)
  union {
    int ybar_half;       // forward only (ENF_STAGE_YBAR_HALF): `ybar` holds bf16 rows
    int seed;            // backward, SEED (the kernel's template flag) only: the output channel o of the unit seed d out = e_o
  };
  int NQ, O;             // NQ = B*N queries
  float inv_hd;          // 1 / (H * true num_hidden)
};
// Grouped observations (the kernels' GRP flag / EVAL == 3; include/enf_hip.h, "Grouped observations"): observation m owns the G
// consecutive queries m G .. m G + G - 1; `target` is then (NQ / G, O) and inv_n = 1 / (B M O).  The fields are appended at the END, in a
// struct of their own that only the grouped instantiations take as their argument: the scalar loads a kernel's prologue is compiled to
// depend on the size of its argument block, so the other kernels keep TailArgs as it was, and with it their instructions.
struct TailArgsG : TailArgs {
  const float* qweight;  // nullptr (every factor is 1 / G), or one quadrature factor per query (NQ floats, finite)
  const float* oweight;  // nullptr (1), or one loss weight per observation (NQ / G floats, >= 0); the zero-weight rule of `weight`
  float* err_g;          // nullptr, or the weighted squared error of every observation (NQ / G floats, OVERWRITTEN)
  int G;                 // 1, 2, 4, 8 or 16
};
// Per-value weights on grouped observations (GRP with CW / EVAL == 4; include/enf_hip.h, "Grouped observations": the _gc calls): one
// weight per observed VALUE in place of `oweight`.  Appended in a struct of its own again, for the reason above: only the per-value
// grouped instantiations take it, so TailArgs and TailArgsG keep their layout and the kernels on them their instructions.
struct TailArgsGC : TailArgsG {
  const float* cweight;  // (NQ / G, O) floats, >= 0, never nullptr; the zero-weight rule per value
};
// GROUPED 0: TailArgs; 1: TailArgsG; 2: TailArgsGC
template <int GROUPED> using TailArgsFor = std::conditional_t<GROUPED == 2, TailArgsGC, std::conditional_t<GROUPED == 1, TailArgsG, TailArgs>>;

// load_rows (enf_tail_common.h) from bf16 rows (two values per word, low half first)
template <int NT> DEV void load_rows_half(f32x4 (&X)[NT], const unsigned short* row, int quad) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const uint2 w = *reinterpret_cast<const uint2*>(row + 16 * t + 4 * quad);
    X[t] = f32x4{__builtin_bit_cast(float, w.x << 16), __builtin_bit_cast(float, w.x & 0xffff0000u),
                 __builtin_bit_cast(float, w.y << 16), __builtin_bit_cast(float, w.y & 0xffff0000u)};
  }
}

// ---- LA2: a 3-slot ring with TWO stages in flight.  The tail's GEMM stages are short (0.25 us of MFMAs per 32 KB
// stage) against ~1.1 us from LDS-DMA issue to landing, so with one stage in flight (panel_gemm) a small grid -- the fit
// shape has 64 workgroups, one per CU -- spends its time waiting for weights.  Here stage s + 2 of the kernel's stage
// stream is issued at the start of stage s; the end-of-stage wait lets that newest stage stay outstanding
// (s_waitcnt vmcnt(its per-wave instruction count)) and only requires stage s + 1.  One barrier per stage as before:
// a wave writes slot (s + 2) % 3 = (s - 1) % 3 only after every wave has left stage s - 1.
// (Large grids keep the 2-slot kernel: two workgroups per CU hide the latency there and need the LDS.)
template <int BYTES> struct La2Cnt { static constexpr int K = BYTES > 0 ? (BYTES / 1024) / NWAVES : 0; };
template <int K> DEV void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(K) : "memory"); }
template <int BYTES> DEV void la2_issue(const Pipe& P, unsigned off, char* ring, int slot, int lane) {
  stage_issue<BYTES>(P.rs, off, ring + slot * STAGE_MAX, P.wave, lane);
}
// panel descriptor for the stream: offset at run time, shape at compile time
template <int KBIN, int MTOUT, bool BF16> struct Pan {
  using C = PanelCfg<KBIN, MTOUT, BF16>;
  static constexpr int SPP = C::SPP, STAGE = C::STAGE;
};
struct NoPan { static constexpr int SPP = 0, STAGE = 0; };

// One stage step: issue the stage two ahead (own panel, else next panel N1, else the one after, N2), multiply, wait, barrier.
// ACTIVE false (the code path of a wave without queries, tail_cadence): issue this wave's share of the stage, wait, meet the barrier.
template <int SP, int KBIN, int MTOUT, bool BF16, typename N1, typename N2, int INIT, bool ACTIVE>
DEV void la2_step(f32x4 (&acc)[MTOUT], const Frags<BF16, KBIN>& F, Pipe& P, char* ring, unsigned panel, unsigned n1, unsigned n2,
                  int lane, const float* bias) {
  using C = PanelCfg<KBIN, MTOUT, BF16>;
  constexpr int AHEAD = SP + 2 - C::SPP;          // < 0: own panel; 0.. : stage AHEAD of the following panels
  const int slot2 = (P.cur + 2) % 3;
  constexpr int ISSUED = AHEAD < 0 ? C::STAGE : (AHEAD < N1::SPP ? N1::STAGE : (AHEAD == N1::SPP && N1::SPP <= 1 ? N2::STAGE : 0));
  if constexpr (AHEAD < 0) la2_issue<C::STAGE>(P, panel + (SP + 2) * C::STAGE, ring, slot2, lane);
  else if constexpr (AHEAD < N1::SPP) la2_issue<N1::STAGE>(P, n1 + AHEAD * N1::STAGE, ring, slot2, lane);
  else if constexpr (AHEAD == N1::SPP && N1::SPP <= 1 && N2::STAGE > 0) la2_issue<N2::STAGE>(P, n2, ring, slot2, lane);
  if constexpr (ACTIVE) gemm_stage<BF16, KBIN, C::MTS, INIT>(&acc[SP * C::MTS], F, ring + P.cur * STAGE_MAX, lane, bias + 16 * SP * C::MTS);
  wait_vm<La2Cnt<ISSUED>::K>();
  __syncthreads();
  P.cur = (P.cur + 1) % 3;
}
template <int KBIN, int MTOUT, bool BF16, typename N1, typename N2, bool ACTIVE = true, int INIT = INIT_ACC>
DEV void panel_gemm_la2(f32x4 (&acc)[MTOUT], const Frags<BF16, KBIN>& F, Pipe& P, char* ring, unsigned panel, unsigned n1,
                        unsigned n2, int lane, const float* bias = nullptr) {
  using C = PanelCfg<KBIN, MTOUT, BF16>;
  static_assert(C::SPP <= 8, "unrolled by hand");
#define LA2_STEP(SP_) if constexpr (C::SPP > SP_) la2_step<SP_, KBIN, MTOUT, BF16, N1, N2, INIT, ACTIVE>(acc, F, P, ring, panel, n1, n2, lane, bias);
  LA2_STEP(0) LA2_STEP(1) LA2_STEP(2) LA2_STEP(3) LA2_STEP(4) LA2_STEP(5) LA2_STEP(6) LA2_STEP(7)
#undef LA2_STEP
}
// stream start: stage 0 and stage 1 (of the first panel A, or of the second panel B when A has one stage)
template <typename A0, typename B0>
DEV void la2_first(Pipe& P, char* ring, unsigned a, unsigned b, int wave, int lane) {
  P.cur = 0;
  P.wave = __builtin_amdgcn_readfirstlane(wave);
  P.early = false;
  la2_issue<A0::STAGE>(P, a, ring, 0, lane);
  constexpr int S1 = A0::SPP > 1 ? A0::STAGE : B0::STAGE;
  if constexpr (A0::SPP > 1) la2_issue<A0::STAGE>(P, a + A0::STAGE, ring, 1, lane);
  else if constexpr (B0::STAGE > 0) la2_issue<B0::STAGE>(P, b, ring, 1, lane);
  wait_vm<La2Cnt<S1>::K>();
  __syncthreads();
}
// dispatch: LA2 or the 2-slot panel_gemm
template <bool LA2, int KBIN, int MTOUT, bool BF16, typename N1, typename N2, int NEXT_BYTES, bool ACTIVE = true>
DEV void tail_gemm(f32x4 (&acc)[MTOUT], const Frags<BF16, KBIN>& F, Pipe& P, char* ring, unsigned panel, unsigned n1, unsigned n2,
                   int lane) {
  if constexpr (LA2) panel_gemm_la2<KBIN, MTOUT, BF16, N1, N2, ACTIVE>(acc, F, P, ring, panel, n1, n2, lane);
  else panel_gemm<KBIN, MTOUT, BF16, NEXT_BYTES>(acc, F, P, ring, panel, n1, ACTIVE, lane);
}

// Forward chain for this wave's 16 queries.  o4 = the (padded) 32 network outputs.
// SAVE: stash pre-activations + LN stats to `act` (row per query) for the backward chain.
// NX1 / NX2 (Pan<..> or NoPan) + next / next2: the two panels that follow the forward chain (the backward chain's first
// two, or nothing); the 2-slot pipeline only uses the first stage of NX1.
template <int D, int H, bool BF16, bool SAVE, bool LA2, typename NX1, typename NX2>
DEV void tail_forward(f32x4 (&o4)[2], const float* yrow, float* act, const EnfLayout& L, const float* cst, Pipe& P,
                      char* ring, unsigned next, unsigned next2, int lane, int quad, float inv_hd, bool save_ok = true, bool y_half = false) {
  using T = TailCfg<D, H, BF16>;
  constexpr int KB = T::KB, KBH = T::KBH, NT = T::NT, NTH = T::NTH, HD = T::HD;
  using PTB = Pan<KBH, NTH, BF16>; using PO0 = Pan<KBH, NT, BF16>; using PO2 = Pan<KB, NT, BF16>; using PO4 = Pan<KB, 2, BF16>;
  constexpr int NEXT_BYTES = NX1::STAGE > 0 ? NX1::STAGE : 1024;
  const float* c_bB = cst, *c_bF1 = cst + HD, *c_bO0 = cst + 2 * HD, *c_bO2 = cst + 2 * HD + D, *c_bO4 = cst + 2 * HD + 2 * D;
  Frags<BF16, KBH> FH;
  f32x4 a[NTH];
  if (y_half) load_rows_half<NTH>(a, reinterpret_cast<const unsigned short*>(yrow), quad);     // (yrow: the caller's row pointer in bf16 units)
  else load_rows<NTH>(a, yrow, quad);
  make_frags<BF16, KBH>(FH, a);
#pragma unroll
  for (int t = 0; t < NTH; ++t) a[t] = rowvec(c_bB, t, quad);
  tail_gemm<LA2, KBH, NTH, BF16, PTB, PO0, T::ST_TB>(a, FH, P, ring, (unsigned)L.atb, (unsigned)L.atf1, (unsigned)L.ato0, lane);
  if (SAVE && save_ok) store_rows<NTH>(a, act, quad);
#pragma unroll
  for (int t = 0; t < NTH; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) a[t][i] = gelu_f(a[t][i]);
  float mu, rstd;
  ln_stats<NTH>(a, mu, rstd, inv_hd);
  if (SAVE && save_ok && quad == 0) { act[T::ACT - 2] = mu; act[T::ACT - 1] = rstd; }
  ln_apply<NTH>(a, mu, rstd);          // (scalar fmas on purpose: enf_device.h)
  make_frags<BF16, KBH>(FH, a);
#pragma unroll
  for (int t = 0; t < NTH; ++t) a[t] = rowvec(c_bF1, t, quad);
  tail_gemm<LA2, KBH, NTH, BF16, PO0, PO2, T::ST_O0>(a, FH, P, ring, (unsigned)L.atf1, (unsigned)L.ato0, (unsigned)L.ato2, lane);
  if (SAVE && save_ok) store_rows<NTH>(a, act + HD, quad);
#pragma unroll
  for (int t = 0; t < NTH; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) a[t][i] = gelu_f(a[t][i]);       // NEF:230
  make_frags<BF16, KBH>(FH, a);
  f32x4 c[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) c[t] = rowvec(c_bO0, t, quad);
  tail_gemm<LA2, KBH, NT, BF16, PO2, PO4, T::ST_O2>(c, FH, P, ring, (unsigned)L.ato0, (unsigned)L.ato2, (unsigned)L.ato4, lane);
  if (SAVE && save_ok) store_rows<NT>(c, act + 2 * HD, quad);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) c[t][i] = gelu_f(c[t][i]);
  Frags<BF16, KB> FD;
  make_frags<BF16, KB>(FD, c);
#pragma unroll
  for (int t = 0; t < NT; ++t) c[t] = rowvec(c_bO2, t, quad);
  tail_gemm<LA2, KB, NT, BF16, PO4, NX1, T::ST_O4>(c, FD, P, ring, (unsigned)L.ato2, (unsigned)L.ato4, next, lane);
  if (SAVE && save_ok) store_rows<NT>(c, act + 2 * HD + D, quad);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) c[t][i] = gelu_f(c[t][i]);
  make_frags<BF16, KB>(FD, c);
  o4[0] = rowvec(c_bO4, 0, quad);
  o4[1] = rowvec(c_bO4, 1, quad);
  tail_gemm<LA2, KB, 2, BF16, NX1, NX2, NEXT_BYTES>(o4, FD, P, ring, (unsigned)L.ato4, next, next2, lane);
}

// The code path of a wave WITHOUT queries in the kernels with fewer than NWAVES active waves (LA2 only): its part of the constants, then
// the stage cadence of the kernel's whole chain -- this wave's share of every LDS-DMA stage, the wait, the barrier -- and nothing else:
// no load, no store, no MFMA, no epilogue.  FWD: the forward chain (tail_forward); BWD: the backward chain of enf_tail_bwd_kernel behind
// it, or alone.  The GEMM calls below are those of the two chains, panel for panel, with the same look-ahead arguments: they must
// change together (tests/test_gpu_tail_active_waves.py compares every form with the eight-wave kernel, whose waves all run the chain).
// The waves with queries run the kernel's own code, which is the eight-wave kernel's, instruction for instruction.
template <int D, int H, bool BF16, bool FWD, bool BWD>
DEV void tail_cadence(const TailArgs& A, char* smem) {
  using T = TailCfg<D, H, BF16>;
  constexpr int KB = T::KB, KBH = T::KBH, NT = T::NT, NTH = T::NTH;
  using PTB = Pan<KBH, NTH, BF16>; using PO0 = Pan<KBH, NT, BF16>; using PO2 = Pan<KB, NT, BF16>; using PO4 = Pan<KB, 2, BF16>;
  using PG4 = Pan<1, NT, BF16>; using PG2 = Pan<KB, NT, BF16>; using PG0 = Pan<KB, NTH, BF16>; using PGH = Pan<KBH, NTH, BF16>;
  using NX1 = std::conditional_t<BWD, PG4, NoPan>; using NX2 = std::conditional_t<BWD, PG2, NoPan>;
  char* ring = smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const EnfLayout& L = A.L;
  tail_consts<D, H, BF16>(reinterpret_cast<float*>(smem + 3 * STAGE_MAX), A.blob, L, tid);
  Pipe P;
  P.rs = make_blob_rsrc(A.blob, (unsigned)L.total);
  P.rs2 = P.rs;
  __syncthreads();
  f32x4 a[NTH], c[NT], o4[2];            // never read: ACTIVE is false in every call
  Frags<BF16, KBH> FH; Frags<BF16, KB> FD; Frags<BF16, 1> F1;
  const unsigned next = BWD ? (unsigned)L.gto4 : NO_STAGE, next2 = BWD ? (unsigned)L.gto2 : NO_STAGE;
  if constexpr (FWD) {
    la2_first<PTB, PTB>(P, ring, (unsigned)L.atb, (unsigned)L.atf1, wave, lane);
    tail_gemm<true, KBH, NTH, BF16, PTB, PO0, T::ST_TB, false>(a, FH, P, ring, (unsigned)L.atb, (unsigned)L.atf1, (unsigned)L.ato0, lane);
    tail_gemm<true, KBH, NTH, BF16, PO0, PO2, T::ST_O0, false>(a, FH, P, ring, (unsigned)L.atf1, (unsigned)L.ato0, (unsigned)L.ato2, lane);
    tail_gemm<true, KBH, NT, BF16, PO2, PO4, T::ST_O2, false>(c, FH, P, ring, (unsigned)L.ato0, (unsigned)L.ato2, (unsigned)L.ato4, lane);
    tail_gemm<true, KB, NT, BF16, PO4, NX1, T::ST_O4, false>(c, FD, P, ring, (unsigned)L.ato2, (unsigned)L.ato4, next, lane);
    tail_gemm<true, KB, 2, BF16, NX1, NX2, 1024, false>(o4, FD, P, ring, (unsigned)L.ato4, next, next2, lane);
  } else la2_first<PG4, PG2>(P, ring, (unsigned)L.gto4, (unsigned)L.gto2, wave, lane);
  if constexpr (BWD) {
    tail_gemm<true, 1, NT, BF16, PG2, PG0, T::ST_O2, false>(c, F1, P, ring, (unsigned)L.gto4, (unsigned)L.gto2, (unsigned)L.gto0, lane);
    tail_gemm<true, KB, NT, BF16, PG0, PGH, T::ST_G0, false>(c, FD, P, ring, (unsigned)L.gto2, (unsigned)L.gto0, (unsigned)L.gtf1, lane);
    tail_gemm<true, KB, NTH, BF16, PGH, PGH, T::ST_TB, false>(a, FD, P, ring, (unsigned)L.gto0, (unsigned)L.gtf1, (unsigned)L.gtb, lane);
    tail_gemm<true, KBH, NTH, BF16, PGH, NoPan, T::ST_TB, false>(a, FH, P, ring, (unsigned)L.gtf1, (unsigned)L.gtb, NO_STAGE, lane);
    tail_gemm<true, KBH, NTH, BF16, NoPan, NoPan, 1024, false>(a, FH, P, ring, (unsigned)L.gtb, NO_STAGE, NO_STAGE, lane);
  }
}

// The fused loss of one wave's 16 queries (enf_loss.hip's arithmetic on the forward chain's outputs, in registers): this lane's share of
// sum_o w (out - target)^2 and, in g0, d out = 2 w (out - target) inv_n gscale (gs = 2 inv_n gscale).  CW: `weight` holds one value per
// output element, else nullptr or one per query.  A weight of 0 is a select, never 0 * target: the NaN of a missing value reaches neither
// the sum nor d out.
template <bool CW>
DEV float tail_sq_err(const f32x4 (&o4)[2], f32x4 (&g0)[2], const TailArgs& A, int qi, bool qvalid, int quad, float gs) {
  float se = 0.f;
  if constexpr (CW) {      // the lane that holds output o of query n reads weight[n][o]; the zero test is per value
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int o = 16 * t + 4 * quad + i;
        const bool in = o < A.O && qvalid;
        const float w = in ? A.weight[(size_t)qi * A.O + o] : 0.f;
        const float dd = (in && w > 0.f) ? o4[t][i] - A.target[(size_t)qi * A.O + o] : 0.f;
        const float wd = w * dd;
        se = fmaf(wd, dd, se);
        g0[t][i] = wd * gs;
      }
  } else if (A.weight) {          // (wave-uniform; the unweighted arithmetic below stays as it was, bit for bit)
    const float w = A.weight[qi];
    const bool live = qvalid && w > 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int o = 16 * t + 4 * quad + i;
        const float dd = (o < A.O && live) ? o4[t][i] - A.target[(size_t)qi * A.O + o] : 0.f;
        const float wd = w * dd;
        se = fmaf(wd, dd, se);
        g0[t][i] = wd * gs;
      }
  } else {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int o = 16 * t + 4 * quad + i;
        const float dd = (o < A.O && qvalid) ? o4[t][i] - A.target[(size_t)qi * A.O + o] : 0.f;
        se = fmaf(dd, dd, se);
        g0[t][i] = dd * gs;
      }
  }
  return se;
}
// The fused loss against GROUPED observations (include/enf_hip.h, "Grouped observations"): obs[m] = sum_{k < G} q[m G + k] out[m G + k]
// is compared with target[m].  The 16 queries of the tile sit in the 16 `col` lanes of each quad and a group is G consecutive, G-aligned
// cols (the tile starts at a multiple of 16 and G divides 16 and N), so the group sum is an xor tree over col bits: shuffles by 1, 2, ..
// G / 2 under wave-uniform tests of G, which never mix two quads.  Each step adds the same two values in both lanes, so every lane of a
// group ends with the same bits.  (Contraction is off in here: a fused q * out + partner would round differently in the two lanes.)
// A group is wholly valid or wholly beyond NQ; lanes beyond NQ contribute zeros.  The squared error is counted once per observation, by
// the lane with col % G == 0; g0 = d out = q w (obs - target) gs in every lane.  w == 0 is a select, as in tail_sq_err.
// Returns this lane's share of sum_o w (obs - target)^2.
// CW (A is then a TailArgsGC): one weight per observed value.  After the tree every lane of a group holds obs for its eight channels, so
// the lane reads cweight[m][o] where the per-observation form reads oweight[m] and applies the select per value, as tail_sq_err<CW> does;
// the arithmetic per value and its order are those of the per-observation form.
template <bool CW, class Args>
DEV float tail_sq_err_g(const f32x4 (&o4)[2], f32x4 (&g0)[2], const Args& A, int qi, bool qvalid, int col, int quad, float gs) {
#pragma clang fp contract(off)
  const int G = A.G;
  const float q = A.qweight ? A.qweight[qi] : 1.0f / (float)G;
  f32x4 s[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) s[t][i] = qvalid ? q * o4[t][i] : 0.f;
#define ENF_GROUP_STEP(K_)                                             \
  if (G > K_) {                                                        \
    _Pragma("unroll") for (int t = 0; t < 2; ++t)                      \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) s[t][i] += __shfl_xor(s[t][i], K_, 64); \
  }
  ENF_GROUP_STEP(1) ENF_GROUP_STEP(2) ENF_GROUP_STEP(4) ENF_GROUP_STEP(8)
#undef ENF_GROUP_STEP
  const int m = qi >> __builtin_ctz(G);
  const bool head = (col & (G - 1)) == 0;
  float se = 0.f;
  if constexpr (CW) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int o = 16 * t + 4 * quad + i;
        const bool in = o < A.O && qvalid;
        const float w = in ? A.cweight[(size_t)m * A.O + o] : 0.f;
        const float dd = (in && w > 0.f) ? s[t][i] - A.target[(size_t)m * A.O + o] : 0.f;
        const float wd = w * dd;
        se = head ? fmaf(wd, dd, se) : se;
        g0[t][i] = (q * wd) * gs;
      }
  } else {
    const float w = A.oweight ? A.oweight[m] : 1.f;
    const bool live = qvalid && w > 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int o = 16 * t + 4 * quad + i;
        const float dd = (o < A.O && live) ? s[t][i] - A.target[(size_t)m * A.O + o] : 0.f;
        const float wd = w * dd;
        se = head ? fmaf(wd, dd, se) : se;
        g0[t][i] = (q * wd) * gs;
      }
  }
  return se;
}
// The wave's reduction of `se` in the order it always had (xor 32, 16, 8, 4, 2, 1).  After the first two steps the four quads are
// folded: lanes 0..15 hold one weighted squared error per query, and with `err` they store it (one 64-byte store per wave; rows beyond
// NQ -- clamped duplicate lanes -- do not).  No atomic and nothing that depends on which signals a wave straddles.  `want_sum` false:
// the per-query values were all that was asked for.
DEV float tail_err_reduce(float se, float* err, int q, bool qvalid, int quad, bool want_sum = true) {
  se += __shfl_xor(se, 32, 64);
  se += __shfl_xor(se, 16, 64);
  if (err && quad == 0 && qvalid) err[q] = se;
  if (want_sum) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
  }
  return se;
}
DEV void tail_loss_add(float se, const TailArgs& A, int qtile) {      // qtile: the wave's global query-tile index
  if (A.loss_part) A.loss_part[qtile] = se * A.inv_n;     // deterministic mode: summed in index order afterwards
  else atomicAdd(A.loss, se * A.inv_n);          // (one per wave, nobody waits for it; the caller zeroed *loss)
}

// EVAL (1: unweighted or per-point weights, 2: per-channel weights, 3: grouped observations, 4: grouped with per-value weights; never with SAVE): the evaluation tail -- the epilogue forms err and,
// with A.loss, the scalar loss from the output accumulators instead of storing `out` (enf_eval_loss): no backward chain, no stash, no
// `out` in HBM.
//
// AW (active waves; 8, 4, 2 or 1): a launch whose grid would be far below the CU count runs workgroups in which only the first AW of
// the eight waves carry queries (q0 = 16 AW blockIdx.x + 16 wave; tail_active_waves below picks AW).  A stage costs the same ~2.5 us
// whether 4 or 64 workgroups run it -- the eight waves of a workgroup queue two per SIMD on one vector ALU and one LDS port between the
// stage barriers -- so the same queries spread over 8 / AW times as many CUs finish every stage sooner.  The other waves leave for
// tail_cadence: they keep issuing their share of every LDS-DMA stage and keep the wait / barrier cadence (stage_issue's piece split, the
// 12-bit offsets and La2Cnt are those of eight waves) and run nothing else.  The waves with queries run the code below unchanged, so
// their arithmetic does not depend on AW: the results are bit-equal.
template <int D, int H, bool BF16, bool LA2, bool SAVE, int EVAL = 0, int AW = NWAVES>
__global__ __launch_bounds__(NTHREADS, 2) void enf_tail_fwd_kernel(TailArgsFor<EVAL == 4 ? 2 : (EVAL == 3 ? 1 : 0)> A) {
  static_assert(!(SAVE && EVAL != 0), "the evaluation tail has no backward to stash for");
  static_assert(AW == NWAVES || (LA2 && (AW == 4 || AW == 2 || AW == 1)), "fewer active waves: small grids, the 3-slot ring");
  using T = TailCfg<D, H, BF16>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem;
  float* cst = reinterpret_cast<float*>(smem + (LA2 ? 3 : 2) * STAGE_MAX);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  if constexpr (AW < NWAVES) {
    if (__builtin_amdgcn_readfirstlane(wave) >= AW) { tail_cadence<D, H, BF16, true, false>(A, smem); return; }
  }
  const int q0 = blockIdx.x * (16 * AW) + wave * 16;
  const int qi = min(q0 + col, A.NQ - 1);
  tail_consts<D, H, BF16>(cst, A.blob, A.L, tid);
  Pipe P;
  P.rs = make_blob_rsrc(A.blob, (unsigned)A.L.total);
  P.rs2 = P.rs;
  if constexpr (LA2) {
    __syncthreads();                                   // the LDS constants, for waves that run ahead of the first stage barrier
    la2_first<Pan<T::KBH, T::NTH, BF16>, Pan<T::KBH, T::NTH, BF16>>(P, ring, (unsigned)A.L.atb, (unsigned)A.L.atf1, wave, lane);
  } else first_stage<T::ST_TB>(P, ring, (unsigned)A.L.atb, wave, lane);
  f32x4 o4[2];
  // SAVE: the pre-activations go to the workspace so that the backward that follows need not recompute this chain
  const bool yh = !SAVE && A.ybar_half;
  const float* yrow = yh ? reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(A.ybar) + (size_t)qi * T::HD)
                         : A.ybar + (size_t)qi * T::HD;
  tail_forward<D, H, BF16, SAVE, LA2, NoPan, NoPan>(o4, yrow, SAVE ? A.act + (size_t)qi * T::ACT : nullptr, A.L,
                                                    cst, P, ring, NO_STAGE, NO_STAGE, lane, quad, A.inv_hd, true, yh);
  if constexpr (EVAL >= 3) {      // grouped observations: err_g per observation, stored by the group's first lane
    const bool qvalid = q0 + col < A.NQ;
    f32x4 g0[2];       // (dead code, as below)
    float se = tail_sq_err_g<EVAL == 4>(o4, g0, A, qi, qvalid, col, quad, 0.f);
    se = tail_err_reduce(se, A.err_g, qi >> __builtin_ctz(A.G), qvalid && (col & (A.G - 1)) == 0, quad, A.loss != nullptr);
    if (A.loss && lane == 0) tail_loss_add(se, A, blockIdx.x * AW + wave);
  } else if constexpr (EVAL != 0) {
    const bool qvalid = q0 + col < A.NQ;
    f32x4 g0[2];       // (d out is not wanted: dead code)
    float se = tail_sq_err<EVAL == 2>(o4, g0, A, qi, qvalid, quad, 0.f);
    se = tail_err_reduce(se, A.err, q0 + col, qvalid, quad, A.loss != nullptr);
    if (A.loss && lane == 0) tail_loss_add(se, A, blockIdx.x * AW + wave);
  } else if (q0 + col < A.NQ) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int o = 16 * t + 4 * quad + i;
        if (o < A.O) A.out[(size_t)(q0 + col) * A.O + o] = o4[t][i];
      }
  }
}

// LOSS (with RECOMP): the inner step's tail in ONE kernel -- forward chain, the reconstruction loss and its gradient
// (pde_trainer.py:185: mean squared error over all B N O outputs; enf_loss.hip's arithmetic) formed in registers from the forward's
// outputs, backward chain: no `out` / `d out` round trip and two launches less between the pair kernels of an inner step.
// CW (with LOSS): `weight` holds one value per output element (include/enf_hip.h, "Weighted loss": per-channel weights).  An
// instantiation of its own: the per-point and the unweighted kernels keep their code.
// SEED (never with WG or LOSS): the seeded backward of enf_field_grad -- d out is the unit vector e_o of output channel
// o = A.seed (a run-time argument: one instantiation serves every channel), formed in registers where LOSS forms its gradient; no
// `d out` is read and no (B, N, O) one-hot tensor exists.  The pre-activations come from the forward's stash.
// SEED with RECOMP: the shared-latent fit step's tail in one kernel -- the unit seed does not depend on the loss, so the forward chain
// (stash as ever, `out` stored where A.out is given) and the seeded backward chain need no launch between them.
// AW: as in enf_tail_fwd_kernel.
// GRP (with LOSS): the loss against grouped observations (tail_sq_err_g) -- means over G consecutive queries, formed by
// cross-lane adds in front of the squared error.  An instantiation of its own, one for every G; the other fused-loss kernels keep their code.
// GRP with CW: one weight per observed value (TailArgsGC), an instantiation of its own again.
template <int D, int H, bool BF16, bool LA2, bool RECOMP, bool WG = false, bool LOSS = false, bool CW = false, bool SEED = false,
          int AW = NWAVES, bool GRP = false>
__global__ __launch_bounds__(NTHREADS, 2) void enf_tail_bwd_kernel(TailArgsFor<GRP ? (CW ? 2 : 1) : 0> A) {
  static_assert(!LOSS || RECOMP, "the fused loss needs the forward chain's outputs");
  static_assert(!CW || LOSS, "per-channel weights belong to the fused loss");
  static_assert(!GRP || LOSS, "grouped observations are a form of the fused loss (CW: their weights are per value, else per observation)");
  static_assert(!SEED || (!WG && !LOSS), "the seeded backward writes d ybar and delta (and, with the forward chain, out) only");
  static_assert(AW == NWAVES || (LA2 && !WG && (AW == 4 || AW == 2 || AW == 1)), "fewer active waves: small grids, the 3-slot ring");
  using T = TailCfg<D, H, BF16>;
  constexpr int KB = T::KB, KBH = T::KBH, NT = T::NT, NTH = T::NTH, HD = T::HD;
  using PG4 = Pan<1, NT, BF16>; using PG2 = Pan<KB, NT, BF16>; using PG0 = Pan<KB, NTH, BF16>; using PGH = Pan<KBH, NTH, BF16>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem;
  float* cst = reinterpret_cast<float*>(smem + (LA2 ? 3 : 2) * STAGE_MAX);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  if constexpr (AW < NWAVES) {
    if (__builtin_amdgcn_readfirstlane(wave) >= AW) { tail_cadence<D, H, BF16, RECOMP, true>(A, smem); return; }
  }
  const int q0 = blockIdx.x * (16 * AW) + wave * 16;
  const bool qvalid = q0 + col < A.NQ;
  const int qi = min(q0 + col, A.NQ - 1);
  // clamped (duplicate) queries write the same scratch values: benign
  float* act = A.act + (size_t)qi * T::ACT;
  float* tdel = WG ? A.tdel + (size_t)qi * (2 * HD + 2 * D) : nullptr;
  const float* yrow = A.ybar + (size_t)qi * HD;
  tail_consts<D, H, BF16>(cst, A.blob, A.L, tid);
  Pipe P;
  P.rs = make_blob_rsrc(A.blob, (unsigned)A.L.total);
  P.rs2 = P.rs;
  f32x4 o4[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  if constexpr (RECOMP) {
    if constexpr (LA2) {
      __syncthreads();
      la2_first<PGH, PGH>(P, ring, (unsigned)A.L.atb, (unsigned)A.L.atf1, wave, lane);
    } else first_stage<T::ST_TB>(P, ring, (unsigned)A.L.atb, wave, lane);
    // WG: the rows of `act` are rewritten in place below (layer inputs over pre-activations), so a clamped duplicate lane -- it shares
    // its row with the query's own lane in another wave -- must not store: its late pre-activation would land on the finished row
    tail_forward<D, H, BF16, true, LA2, PG4, PG2>(o4, yrow, act, A.L, cst, P, ring, (unsigned)A.L.gto4, (unsigned)A.L.gto2, lane, quad,
                                                  A.inv_hd, !WG || qvalid);
    if constexpr (SEED) {      // the forward's output row, for the loss kernel that follows
      if (qvalid && A.out) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int o = 16 * t + 4 * quad + i;
            if (o < A.O) A.out[(size_t)(q0 + col) * A.O + o] = o4[t][i];
          }
      }
    }
  } else {      // the forward of this step stashed the pre-activations (enf_tail_fwd_kernel<.., SAVE>): start at the backward chain
    if constexpr (LA2) {
      __syncthreads();
      la2_first<PG4, PG2>(P, ring, (unsigned)A.L.gto4, (unsigned)A.L.gto2, wave, lane);
    } else first_stage<T::ST_G4>(P, ring, (unsigned)A.L.gto4, wave, lane);
  }
  // the pre-activations this lane stored are re-read by this lane only (same addresses)

  // ---- backward chain
  f32x4 g0[2];
  if constexpr (LOSS && GRP) {
    float se = tail_sq_err_g<CW>(o4, g0, A, qi, qvalid, col, quad, 2.0f * A.inv_n * A.gscale);
    se = tail_err_reduce(se, A.err_g, qi >> __builtin_ctz(A.G), qvalid && (col & (A.G - 1)) == 0, quad);
    if (lane == 0) tail_loss_add(se, A, blockIdx.x * AW + wave);
  } else if constexpr (LOSS) {
    float se = tail_sq_err<CW>(o4, g0, A, qi, qvalid, quad, 2.0f * A.inv_n * A.gscale);
    se = tail_err_reduce(se, A.err, q0 + col, qvalid, quad);
    if (lane == 0) tail_loss_add(se, A, blockIdx.x * AW + wave);
  } else if constexpr (SEED) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) g0[t][i] = (16 * t + 4 * quad + i == A.seed && qvalid) ? 1.f : 0.f;
  } else {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = 16 * t + 4 * quad + i;
      g0[t][i] = (o < A.O && qvalid) ? A.dout[(size_t)qi * A.O + o] : 0.f;
    }
  }
  Frags<BF16, 1> F1;
  make_frags<BF16, 1>(F1, g0);
  f32x4 c[NT];
  zero_tiles<NT>(c);
  tail_gemm<LA2, 1, NT, BF16, PG2, PG0, T::ST_O2>(c, F1, P, ring, (unsigned)A.L.gto4, (unsigned)A.L.gto2, (unsigned)A.L.gto0, lane);   // d g4
  {
    f32x4 pre[NT];
    load_rows<NT>(pre, act + 2 * HD + D, quad);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) c[t][i] *= gelu_grad_f(pre[t][i]);                                            // d a_O2
    if constexpr (WG) {
      if (qvalid) store_rows<NT>(c, tdel + 2 * HD + D, quad);      // (a clamped duplicate lane holds zeros: only the query's own lane writes)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) pre[t][i] = gelu_f(pre[t][i]);
      if (qvalid) store_rows<NT>(pre, act + 2 * HD + D, quad);                                                  // input of out_proj.layers_4
    }
  }
  Frags<BF16, KB> FD;
  make_frags<BF16, KB>(FD, c);
  zero_tiles<NT>(c);
  tail_gemm<LA2, KB, NT, BF16, PG0, PGH, T::ST_G0>(c, FD, P, ring, (unsigned)A.L.gto2, (unsigned)A.L.gto0, (unsigned)A.L.gtf1, lane);  // d g3
  {
    f32x4 pre[NT];
    load_rows<NT>(pre, act + 2 * HD, quad);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) c[t][i] *= gelu_grad_f(pre[t][i]);                                            // d a_O0
    if constexpr (WG) {
      if (qvalid) store_rows<NT>(c, tdel + 2 * HD, quad);
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) pre[t][i] = gelu_f(pre[t][i]);
      if (qvalid) store_rows<NT>(pre, act + 2 * HD, quad);                                                      // input of out_proj.layers_2
    }
  }
  make_frags<BF16, KB>(FD, c);
  f32x4 a[NTH];
  zero_tiles<NTH>(a);
  tail_gemm<LA2, KB, NTH, BF16, PGH, PGH, T::ST_TB>(a, FD, P, ring, (unsigned)A.L.gto0, (unsigned)A.L.gtf1, (unsigned)A.L.gtb, lane);  // d g2
  {
    f32x4 pre[NTH];
    load_rows<NTH>(pre, act + HD, quad);
#pragma unroll
    for (int t = 0; t < NTH; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) a[t][i] *= gelu_grad_f(pre[t][i]);                                            // d a_F1
    if constexpr (WG) {
      if (qvalid) store_rows<NTH>(a, tdel + HD, quad);
#pragma unroll
      for (int t = 0; t < NTH; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) pre[t][i] = gelu_f(pre[t][i]);
      if (qvalid) store_rows<NTH>(pre, act + HD, quad);                                                         // input of out_proj.layers_0
    }
  }
  Frags<BF16, KBH> FH;
  make_frags<BF16, KBH>(FH, a);
  zero_tiles<NTH>(a);
  tail_gemm<LA2, KBH, NTH, BF16, PGH, NoPan, T::ST_TB>(a, FH, P, ring, (unsigned)A.L.gtf1, (unsigned)A.L.gtb, NO_STAGE, lane);          // d n
  {
    // LayerNorm backward + gelu backward on a_B
    f32x4 pre[NTH];
    load_rows<NTH>(pre, act, quad);
    const float mu = act[T::ACT - 2], rstd = act[T::ACT - 1];
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
        a[t][i] = rstd * (a[t][i] - m1 - nh * m2) * gelu_grad_f(pre[t][i]);                                     // d a_B
        if constexpr (WG) pre[t][i] = nh;
      }
    if constexpr (WG) {
      if (qvalid) store_rows<NTH>(a, tdel, quad);
      if (qvalid) store_rows<NTH>(pre, act, quad);                                                              // n^: input of the (folded) FFN Dense_1
    }
  }
  make_frags<BF16, KBH>(FH, a);
  zero_tiles<NTH>(a);
  tail_gemm<LA2, KBH, NTH, BF16, NoPan, NoPan, 1024>(a, FH, P, ring, (unsigned)A.L.gtb, NO_STAGE, NO_STAGE, lane);                       // d ybar
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

// The active waves of a tail launch of nq queries (enf_tail_fwd_kernel): the largest AW whose grid ceil(tiles / AW) still reaches the
// 256 CUs the shapes are tuned for, else 1.  512 queries: 32 workgroups of one active wave; 8192: 256 workgroups of two.
static int tail_active_waves(int nq) {
  const int tiles = (nq + 15) / 16;
  for (int aw = NWAVES; aw > 1; aw >>= 1)
    if ((tiles + aw - 1) / aw >= 256) return aw;
  return 1;
}
// The fused-loss tail keeps eight active waves: on four (128 workgroups beside the fold kernel's 128) the step measured slower
// (DESIGN.md section 5).  The test library has it in every AW, as one more form whose bits must not depend on AW.
#ifdef ENF_TEST_HOOKS
// Test library only: enf_test_tail_active_waves(aw) makes every following tail launch of a form that has the instantiation run with
// `aw` active waves (1, 2, 4 or 8; 0: the launcher's own rule again).  Returns the previous setting.
static int g_test_tail_aw = 0;
extern "C" int enf_test_tail_active_waves(int aw) {
  const int was = g_test_tail_aw;
  g_test_tail_aw = (aw == 1 || aw == 2 || aw == 4 || aw == NWAVES) ? aw : 0;
  return was;
}
constexpr bool TAIL_LOSS_AW_ALL = true;       // the fused loss in every AW (tests/test_gpu_tail_active_waves.py)
#else
constexpr bool TAIL_LOSS_AW_ALL = false;
#endif

// ---- the launch forms: which kernel template, with which template arguments
enum TailForm {
  TF_FWD, TF_FWD_STASH, TF_EVAL, TF_EVAL_CW,                    // enf_tail_fwd_kernel
  TF_BWD, TF_BWD_STASH, TF_WG, TF_WG_STASH,                     // enf_tail_bwd_kernel on d out: recompute / from the stash
  TF_LOSS, TF_LOSS_CW, TF_SEED_STASH, TF_FWD_SEED,              // fused loss; seeded from the stash / behind its own forward chain
  TF_LOSS_G, TF_EVAL_G,                                         // grouped observations: the fused loss and the evaluation tail
  TF_LOSS_GC, TF_EVAL_GC,                                       // the same with one weight per observed value
  TF_COUNT
};
// bwd: enf_tail_bwd_kernel; chain: SAVE of the forward kernel (stash the pre-activations), RECOMP of the backward kernel (run the forward
// chain first); eval: EVAL; wg / loss / cw / seed / grp: the backward kernel's flags
struct TailFormCfg { bool bwd, chain; int eval; bool wg, loss, cw, seed, grp; };
constexpr TailFormCfg tail_form_cfg(TailForm f) {
  switch (f) {
    case TF_FWD: return {false, false, 0, false, false, false, false, false};
    case TF_FWD_STASH: return {false, true, 0, false, false, false, false, false};
    case TF_EVAL: return {false, false, 1, false, false, false, false, false};
    case TF_EVAL_CW: return {false, false, 2, false, false, false, false, false};
    case TF_BWD: return {true, true, 0, false, false, false, false, false};
    case TF_BWD_STASH: return {true, false, 0, false, false, false, false, false};
    case TF_WG: return {true, true, 0, true, false, false, false, false};
    case TF_WG_STASH: return {true, false, 0, true, false, false, false, false};
    case TF_LOSS: return {true, true, 0, false, true, false, false, false};
    case TF_LOSS_CW: return {true, true, 0, false, true, true, false, false};
    case TF_SEED_STASH: return {true, false, 0, false, false, false, true, false};
    case TF_LOSS_G: return {true, true, 0, false, true, false, false, true};
    case TF_EVAL_G: return {false, false, 3, false, false, false, false, false};
    case TF_LOSS_GC: return {true, true, 0, false, true, true, false, true};
    case TF_EVAL_GC: return {false, false, 4, false, false, false, false, false};
    default: return {true, true, 0, false, false, false, true, false};      // TF_FWD_SEED
  }
}
// the forms the launcher's own rule runs on fewer active waves: the forward forms and the seeded backward forms (the d out and the
// weight-gradient backward never, the fused loss in the test library only)
constexpr bool tail_form_small(TailForm f) { return !tail_form_cfg(f).bwd || tail_form_cfg(f).seed; }
constexpr bool tail_form_has_aw(TailForm f) { return tail_form_small(f) || (TAIL_LOSS_AW_ALL && tail_form_cfg(f).loss); }

// THE place that names the kernels
template <int D, int H, bool BF16, TailForm F, bool LA2, int AW> constexpr auto tail_kernel() {
  constexpr TailFormCfg c = tail_form_cfg(F);
  if constexpr (c.bwd) return enf_tail_bwd_kernel<D, H, BF16, LA2, c.chain, c.wg, c.loss, c.cw, c.seed, AW, c.grp>;
  else return enf_tail_fwd_kernel<D, H, BF16, LA2, c.chain, c.eval, AW>;
}
template <int D, int H, bool BF16, TailForm F, bool LA2, int AW>
static int launch_tail_kernel(const TailArgsGC& A, dim3 grid, hipStream_t st) {
  constexpr auto kern = tail_kernel<D, H, BF16, F, LA2, AW>();
  // (the kernel's own argument block: the per-value grouped forms take the whole struct, the grouped forms its TailArgsG part, the others
  // its TailArgs part)
  constexpr TailFormCfg c = tail_form_cfg(F);
  using Args = TailArgsFor<(c.grp && c.cw) || c.eval == 4 ? 2 : (c.grp || c.eval == 3 ? 1 : 0)>;
  constexpr int smem = LA2 ? TailCfg<D, H, BF16>::SMEM3 : TailCfg<D, H, BF16>::SMEM;
  if (!enf_lds_attr<kern>(smem)) return ENF_ELAUNCH;
  hipLaunchKernelGGL(kern, grid, dim3(NTHREADS), smem, st, static_cast<const Args&>(A));
  return hipGetLastError() == hipSuccess ? 0 : ENF_ELAUNCH;
}

template <int D, int H, bool BF16, TailForm F>
static int launch_tail_form(const TailArgsGC& A, hipStream_t st) {
  constexpr TailFormCfg c = tail_form_cfg(F);
  // fewer active waves: deterministic mode keeps eight (the partial-sum slots enf_launch_loss_sum reads are those of the 8-wave grid)
  int aw = NWAVES;
  if (tail_form_small(F) && !A.loss_part) aw = tail_active_waves(A.NQ);
#ifdef ENF_TEST_HOOKS
  if (g_test_tail_aw && tail_form_has_aw(F) && !A.loss_part) aw = g_test_tail_aw;
#endif
  const dim3 grid((A.NQ + 16 * aw - 1) / (16 * aw));
  // few workgroups (at most one per CU): the deeper weight pipeline (LA2) instead of a second workgroup per CU
  const bool la2 = grid.x <= 256 || aw < NWAVES;
  if (c.seed && (A.seed < 0 || A.seed >= A.O)) return ENF_EINVAL;
  if ((c.eval || c.loss) && !A.target) return ENF_EINVAL;
  if ((c.eval == 2 || (c.cw && !c.grp)) && !A.weight) return ENF_EINVAL;
  if ((c.eval == 4 || (c.cw && c.grp)) && !A.cweight) return ENF_EINVAL;
  if ((c.eval >= 3 || c.grp) && (A.G < 1 || A.G > 16 || (A.G & (A.G - 1)) || A.NQ % A.G)) return ENF_EINVAL;
  // (run-time la2, aw) -> template arguments; the instantiations with fewer active waves run the 3-slot ring only
  if constexpr (tail_form_has_aw(F)) {
    if (aw == 4) return launch_tail_kernel<D, H, BF16, F, true, 4>(A, grid, st);
    if (aw == 2) return launch_tail_kernel<D, H, BF16, F, true, 2>(A, grid, st);
    if (aw == 1) return launch_tail_kernel<D, H, BF16, F, true, 1>(A, grid, st);
  }
  return la2 ? launch_tail_kernel<D, H, BF16, F, true, NWAVES>(A, grid, st) : launch_tail_kernel<D, H, BF16, F, false, NWAVES>(A, grid, st);
}

// run-time form and shape -> launch_tail_form
template <class S, int F = 0> static int launch_tail_shape(const TailArgsGC& A, TailForm form, hipStream_t st) {
  if (form == F) return launch_tail_form<S::D, S::H, S::BF16, (TailForm)F>(A, st);
  if constexpr (F + 1 < TF_COUNT) return launch_tail_shape<S, F + 1>(A, form, st);
  else return ENF_EINVAL;
}
static int launch_tail(const EnfDims& m, const TailArgsGC& A, TailForm form, hipStream_t st) {
  if (m.OB != 1) return ENF_EUNSUPPORTED;
  return enf_for_shape(m, [&](auto s) { return launch_tail_shape<decltype(s)>(A, form, st); });
}
// what every form's arguments share; the entry points below set what differs
static TailArgsGC tail_args(const EnfDims& m, const EnfLayout& L, const char* blob, const float* ybar) {
  TailArgsGC A{};
  A.ybar = ybar; A.blob = blob; A.L = L;
  A.NQ = m.B * m.N; A.O = m.O; A.inv_hd = 1.0f / (float)(m.Ht * m.Dt);
  return A;
}

int enf_launch_tail(const EnfDims& m, const EnfLayout& L, const char* blob, const float* ybar, float* out,
                    const float* dout, float* dybar, float* delta, float* act, unsigned flags, hipStream_t st) {
  return enf_launch_tail_wg(m, L, blob, ybar, out, dout, dybar, delta, act, nullptr, flags, st);
}
int enf_launch_tail_wg(const EnfDims& m, const EnfLayout& L, const char* blob, const float* ybar, float* out,
                       const float* dout, float* dybar, float* delta, float* act, float* tdel, unsigned flags, hipStream_t st) {
  const bool bwd = flags & ENF_TAIL_BWD, stash = flags & ENF_TAIL_STASH;
  TailArgsGC A = tail_args(m, L, blob, ybar);
  A.out = out; A.dout = dout; A.dybar = dybar; A.delta = delta; A.act = act; A.tdel = tdel;
  A.ybar_half = (!bwd && (flags & ENF_TAIL_YBAR_HALF) && m.bf16) ? 1 : 0;
  const TailForm form = !bwd ? (stash ? TF_FWD_STASH : TF_FWD) : tdel ? (stash ? TF_WG_STASH : TF_WG) : (stash ? TF_BWD_STASH : TF_BWD);
  return launch_tail(m, A, form, st);
}

int enf_launch_tail_seed(const EnfDims& m, const EnfLayout& L, const char* blob, const float* ybar, int seed, float* dybar, float* delta,
                         float* act, hipStream_t st) {
  TailArgsGC A = tail_args(m, L, blob, ybar);
  A.seed = seed; A.dybar = dybar; A.delta = delta; A.act = act;
  return launch_tail(m, A, TF_SEED_STASH, st);
}
// Forward chain (stash in `act`, `out` (B N, O) stored if given) and the seeded backward in one launch: what enf_launch_tail with the
// stash followed by enf_launch_tail_seed compute, bit for bit.
int enf_launch_tail_fwd_seed(const EnfDims& m, const EnfLayout& L, const char* blob, const float* ybar, float* out, int seed, float* dybar,
                             float* delta, float* act, hipStream_t st) {
  TailArgsGC A = tail_args(m, L, blob, ybar);
  A.out = out; A.seed = seed; A.dybar = dybar; A.delta = delta; A.act = act;
  return launch_tail(m, A, TF_FWD_SEED, st);
}

int enf_tail_loss_parts(const EnfDims& m) {
  return (int)(((long long)m.B * m.N + 16 * NWAVES - 1) / (16 * NWAVES)) * NWAVES;
}

// the fused loss and the evaluation tail: target, weights, the loss and its deterministic partials, the per-point errors
static int tail_loss_kernel(const EnfDims& m, TailArgsGC& A, TailForm form, const float* target, const float* weight, float gscale, float* loss,
                            float* loss_part, float* err, hipStream_t st, int G = 1) {
  // (G: the grouped forms' group size -- the mean is over the B M O observed values, M = N / G)
  A.target = target; A.weight = weight; A.loss = loss; A.gscale = gscale; A.inv_n = 1.0f / ((float)m.B * (float)(m.N / G) * (float)m.O);
  A.loss_part = loss_part; A.err = err;
  if (int rc = launch_tail(m, A, form, st)) return rc;
  return loss_part ? enf_launch_loss_sum(loss_part, enf_tail_loss_parts(m), loss, st) : 0;
}

int enf_launch_tail_loss(const EnfDims& m, const EnfLayout& L, const char* blob, const float* ybar, const float* target,
                         const float* weight, float gscale, float* loss, float* dybar, float* delta, float* act, hipStream_t st, float* loss_part,
                         bool per_value, float* err) {
  TailArgsGC A = tail_args(m, L, blob, ybar);
  A.dybar = dybar; A.delta = delta; A.act = act;
  return tail_loss_kernel(m, A, per_value ? TF_LOSS_CW : TF_LOSS, target, weight, gscale, loss, loss_part, err, st);
}

int enf_launch_tail_eval(const EnfDims& m, const EnfLayout& L, const char* blob, const float* ybar, const float* target,
                         const float* weight, bool per_value, float* loss, float* err, hipStream_t st, float* loss_part) {
  TailArgsGC A = tail_args(m, L, blob, ybar);
  return tail_loss_kernel(m, A, per_value ? TF_EVAL_CW : TF_EVAL, target, weight, 0.f, loss, loss ? loss_part : nullptr, err, st);
}

// Grouped observations: the fused loss (dybar != NULL) or the evaluation tail (dybar == NULL) against target (B, N / G, O).
int enf_launch_tail_group(const EnfDims& m, const EnfLayout& L, const char* blob, const float* ybar, const float* target, const EnfGroupObs& g,
                          float gscale, float* loss, float* dybar, float* delta, float* act, hipStream_t st, float* loss_part) {
  if (!enf_group_size_ok(g.G) || m.N % g.G) return ENF_EINVAL;
  TailArgsGC A = tail_args(m, L, blob, ybar);
  A.dybar = dybar; A.delta = delta; A.act = act;
  A.G = g.G; A.qweight = g.qweight; A.oweight = g.oweight; A.err_g = g.err_g; A.cweight = g.cweight;
  // (per-value weights: the forms of their own; without them the calls run the instantiations they always ran)
  const TailForm form = g.cweight ? (dybar ? TF_LOSS_GC : TF_EVAL_GC) : (dybar ? TF_LOSS_G : TF_EVAL_G);
  return tail_loss_kernel(m, A, form, target, nullptr, gscale, loss, loss ? loss_part : nullptr, nullptr, st, g.G);
}

#ifdef ENF_TEST_HOOKS
// Test library only: one tail launch on the caller's buffers (tests/test_gpu_tail_active_waves.py).  ybar (B N, H D); act (B N,
// 2 H D + 2 D + 2) is the stash.  form 0: forward -> out; 1: forward with the stash -> out, act; 2: evaluation -> err, *loss; 3: seeded
// backward from the stash -> dybar, delta; 4: forward + seeded backward in one launch -> out, act, dybar, delta; 5: fused loss -> act,
// dybar, delta, err, *loss.  weight: nullptr, one per query, or with per_value one per output value; loss_part: nullptr, or the
// deterministic mode's partial sums (enf_tail_loss_parts floats); the caller zeroes *loss.
extern "C" int enf_test_tail_parts(const EnfDesc* d) { return enf_check_desc(d) ? -1 : enf_tail_loss_parts(enf_dims(d)); }
extern "C" int enf_test_tail(const EnfDesc* d, const void* packed, int form, int seed, const float* ybar, const float* target,
                             const float* weight, int per_value, float* out, float* act, float* dybar, float* delta, float* err, float* loss,
                             float* loss_part, void* stream) {
  if (int rc = enf_check_desc(d)) return rc;
  const EnfDims m = enf_dims(d);
  const EnfLayout L = enf_layout(m);
  const char* blob = (const char*)packed;
  hipStream_t st = (hipStream_t)stream;
  switch (form) {
    case 0: return enf_launch_tail(m, L, blob, ybar, out, nullptr, nullptr, nullptr, nullptr, ENF_TAIL_FWD, st);
    case 1: return enf_launch_tail(m, L, blob, ybar, out, nullptr, nullptr, nullptr, act, ENF_TAIL_FWD | ENF_TAIL_STASH, st);
    case 2: return enf_launch_tail_eval(m, L, blob, ybar, target, weight, per_value != 0, loss, err, st, loss_part);
    case 3: return enf_launch_tail_seed(m, L, blob, ybar, seed, dybar, delta, act, st);
    case 4: return enf_launch_tail_fwd_seed(m, L, blob, ybar, out, seed, dybar, delta, act, st);
    case 5: return enf_launch_tail_loss(m, L, blob, ybar, target, weight, 1.0f, loss, dybar, delta, act, st, loss_part, per_value != 0, err);
  }
  return ENF_EINVAL;
}
#endif
