// enf_pair_fwd.hip -- K2: fused per-pair chain + cross-attention over the latent set.
//
// One workgroup = 8 waves (2 per SIMD).  A wave owns 16 queries (columns) of one signal and a
// share of the Z latents: the 8 waves form QG query groups x ZS latent splits (ZS = 8 for Z >= 8,
// so a workgroup covers 16 queries; fewer splits / more query groups for tiny Z).  For each
// (16 queries) x (one latent) the wave runs, entirely in registers and in the transposed
// "acc layout" of enf_device.h:
//   invariant (INV/*)                -> inv (I<=4)                              ECA:86
//   t = coeff^T inv (fp32 MFMA), [sin,cos]                                      RFF:86-93
//   h1 = relu(W1q^T e + b)           (query RFFNet layer)                       RFF:63-64
//   logit_h = h1.u_h + c_h + window  (RFF linear_final, inv_emb_to_q and the q.k dot folded
//                                     into the per-latent vector u_h)            RFF:46, ECA:92,134,139
//   g1 = relu(W1v^T e_v + b); f = gelu(AF^T g1 + b); n = LayerNorm(f)           RFF:63-64,46; ECA:17-19
//   [gamma_h; beta_h] = AGB^T n + b ; v_h = v0_h (1+gamma_h) + beta_h           ECA:20,115-121
//   g = gelu(AM^T v_h + b); (mu, rstd) = LN stats of g                          ECA:122 -> ECA:17-19
//   softmax over z of logit_h; ybar_h += softmax * (g - mu) * rstd              ECA:141-144
// The mixer's LayerNorm affine and Dense_1, attn.out_proj and the block FFN's Dense_0 are
// linear in the softmax-weighted sum and are applied once per query by the tail kernel.
// Weight panels stream L2 -> LDS by LDS-DMA through a 2-slot ring shared by the 8 waves; the shared panels that fit behind the
// ring stay resident in LDS for the workgroup's lifetime (PairSmem).
#include <hip/hip_runtime.h>
#include "enf_launch.h"
#include "enf_device.h"
#include "enf_pair_common.h"

struct PairFwdArgs {
  const float* x; long long x_bstride;
  const float* lt; const char* blob; EnfLayout L;
  float* ybar; float* lse;
  const char* wz; const float* wzb; const char* wzu;   // z-fold only: per-latent mixer-input panels / biases (enf_wz.hip)
  float inv_d;                            // 1 / (true num_hidden)
  int xcd_remap;                          // z-fold: 1 when B % 8 == 0 (see the kernel)
  unsigned* masks; int mask_mode, mask_B; // relu masks (ENF_MASK_*): buffer, 0 off / 1 write / 2 read, signals per mask set
  int B, N, Z, dx, inv, use_window, qg;   // qg: query groups per workgroup (1,2,4,8); ZS = 8/qg
  int zsplit;                             // z-fold, ENF_VARIANT_ZFOLD_ZSPLIT: the most parts a query tile's latents are cut into (1: no split)
  int sk_len;                             // zsplit > 1: latent steps per workgroup -- workgroup c walks steps [c sk_len, (c + 1) sk_len) of the
                                          // flattened (signal, query tile, latent) space (enf_layout.h: enf_zfold_streamk)
  int ybar_half;                          // ENF_STAGE_YBAR_HALF: `ybar` is written as bf16 rows (H D x 2 bytes) for the tail kernel of the same call
  float* ysplit;                          // zsplit > 1: [zsplit][B N HD] partial sums | [zsplit][B N H][3] (m, l, c), merged by enf_zsplit_merge_kernel
  // the shared-latent forward of the latent-split kernel (enf_layout.h: enf_shared_fwd_parts), NULL / 1 / 1 otherwise: the grid is
  // (query tiles, parts) for signal 0, the partial sums go to [parts][N HD] | [parts][N H][3] (m*, L, C) in `spart` and
  // enf_shared_merge_kernel writes ybar / lse of all `bcast` signals
  float* spart;
  int parts, bcast;
};

// Debug build only (-DENF_STAMPS): s_memtime stamps of the first iterations of workgroup 0, one row per
// wave, read back with enf_debug_read_stamps(); the buffer is read by no kernel code (MI355X_MICROARCH.md).
#ifdef ENF_STAMPS
__device__ unsigned long long enf_stamps[8 * 4 * 24];
#define STAMP(k)                                                                                              \
  do {                                                                                                        \
    if (blockIdx.x == 7 && blockIdx.y == 0 && lane == 0 && it < 4)                                            \
      enf_stamps[(wave * 4 + it) * 24 + (k)] = __builtin_amdgcn_s_memtime();                                  \
  } while (0)
extern "C" int enf_debug_read_stamps(unsigned long long* dst) {
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(enf_stamps), sizeof(enf_stamps)) == hipSuccess ? 0 : -1;
}
#else
#define STAMP(k) do {} while (0)
#endif

// accumulators start from the bias row vector, loaded here (INIT_ACC; inside the asm stage measured 1.19 vs 1.135 ms)
#define K2_BIAS(ACC, PTR)                                                              \
  do {                                                                                 \
    _Pragma("unroll") for (int t_ = 0; t_ < NT; ++t_) ACC[t_] = rowvec(PTR, t_, quad);   \
  } while (0)
// relu-mask modes live in their own instantiation (MASKS): as wave-uniform runtime branches in the one kernel they cost
// the default path 1.3 % (measured)
#define K2_MASK_MODE (MASKS && !FFN ? A.mask_mode : 0)

// The shared D x D weight panels of a latent step, in the order the step multiplies by them.  (The gamma/beta panels are one per
// head and twice the size, the z-fold's W_zh are per latent: both always stream.)
enum { RP_Q1 = 0, RP_V1 = 1, RP_F = 2, RP_M = 3, RP_COUNT = 4 };
constexpr int LDS_PER_CU = 160 * 1024;
// The resident set (a bit per RP_*): greedily the candidate that saves the most ring loads per latent step, then the smaller one,
// then the earlier one, as long as it fits in `room` bytes.  saved[i] = 0: the step has no such panel.
constexpr unsigned pair_resident_set(const int (&saved)[RP_COUNT], const int (&bytes)[RP_COUNT], int room) {
  unsigned set = 0;
  for (int n = 0; n < RP_COUNT; ++n) {
    int best = -1;
    for (int i = 0; i < RP_COUNT; ++i) {
      if ((set >> i & 1u) || saved[i] <= 0 || bytes[i] > room) continue;
      if (best < 0 || saved[i] > saved[best] || (saved[i] == saved[best] && bytes[i] < bytes[best])) best = i;
    }
    if (best < 0) break;
    set |= 1u << best;
    room -= bytes[best];
  }
  return set;
}
// where the resident panels in front of panel `p` end, the first of them at `base`
constexpr int pair_resident_end(unsigned set, const int (&bytes)[RP_COUNT], int p, int base) {
  for (int i = 0; i < p; ++i) base += (set >> i & 1u) ? bytes[i] : 0;
  return base;
}

// LDS map (bytes from 0): ring, 2 slots of 32 KB | constants | per-wave latent vectors | softmax exchange | resident panels.
// RES = false leaves the resident set empty (every panel streams through the ring): the test library's reference, not a product path.
template <int D, int H, bool BF16, int NW, bool FFN = false, bool ZFOLD = false, bool RES = true> struct PairSmem {
  static constexpr int RING = 0;                                   // 2 slots
  static constexpr int EW = FFN ? 4 * D : 2 * D;                   // embedding of one branch: coefficient A-operands / Dense_0 rows
  static constexpr int CONSTS = RING + 2 * STAGE_MAX;              // bq1 bv1 bf bm (D each) | bgb (2HD) | acq acv (EW each)
  static constexpr int N_CONST = 4 * D + 2 * H * D + 2 * EW;
  static constexpr int ZVEC = CONSTS + 4 * N_CONST;                // NWAVES x 2*H*D floats
  static constexpr int XCH = ZVEC + 4 * NW * 2 * H * D;            // NW x H x 3 x 16 floats
  static constexpr int RESIDENT = XCH + 4 * NW * H * 3 * 16;       // the resident panels, in RP_* order
  static constexpr int YBYTES = H * (D / 16) * 4 * 64 * 4;         // one wave's Y in [reg][lane] order
  static_assert(4 * YBYTES <= 2 * STAGE_MAX, "combine buffer must fit in the ring");   // (so it ends below the resident panels)
  // ring loads a resident panel saves per latent step: the relu-layer panels exist without the ffn embedding only, the mixer panel
  // AM is multiplied once per head and only in the latent-split variant (the z-fold has it folded into W_zh).  Single-stage panels
  // only: a two-stage one (fp32, D = 128: 64 KB) would take all the room for one panel, and unrolled over both stages without a
  // barrier between them its GEMM spills (84-356 bytes of scratch per lane where the streamed kernel has none)
  static constexpr int PANEL = PanelCfg<D / 32, D / 16, BF16>::BYTES, SPP = PanelCfg<D / 32, D / 16, BF16>::SPP;
  static constexpr int ONE = SPP == 1 ? 1 : 0;
  static constexpr int SAVED[RP_COUNT] = {FFN ? 0 : ONE, FFN ? 0 : ONE, ONE, ZFOLD ? 0 : H * ONE};
  static constexpr int BYTES[RP_COUNT] = {PANEL, PANEL, PANEL, PANEL};
  static constexpr unsigned SET = RES && RESIDENT <= LDS_PER_CU ? pair_resident_set(SAVED, BYTES, LDS_PER_CU - RESIDENT) : 0u;
  static constexpr bool has(int p) { return SET >> p & 1u; }
  static constexpr int off(int p) { return pair_resident_end(SET, BYTES, p, RESIDENT); }    // byte offset of resident panel p
  static constexpr int TOTAL = pair_resident_end(SET, BYTES, RP_COUNT, RESIDENT);
  static_assert(TOTAL <= LDS_PER_CU, "K2's LDS (ring + constants + resident panels) exceeds one CU's");
};

// ZFOLD: qg = 8 (every wave walks all latents, the 8 waves in step), and per head the gamma/beta GEMM, FiLM
// and the mixer's first Dense are ONE D x D GEMM with the per-latent matrix W_zh of enf_wz.hip:
//   a5_h = W_zh^T n + c_zh      (5 D x D GEMMs per pair instead of 9 D x D equivalents)
// INV >= 0: the invariant as a compile-time constant (the shipped configs' instantiations, launch code below): the per-latent step then
// carries no switch over the invariant (as in K3, enf_pair_bwd.hip)
// FFN: the ffn embedding (ENF_EMB_FFN) in both branches: h = gelu(W0^T inv + b0) takes the place of the relu layer's output, so
// a latent step starts at the AF panel (the relu-layer panels aq1 / av1 and the relu masks do not exist)
// RES: keep the resident set of PairSmem in LDS for the workgroup's lifetime and stream only the other panels through the ring
template <int D, int H, bool BF16, bool ZFOLD, bool MASKS, int INV = -1, bool FFN = false, bool RES = true>
__global__ __launch_bounds__(NTHREADS, 2) void enf_pair_fwd_kernel(PairFwdArgs A) {
  const int inv_id = INV >= 0 ? INV : A.inv;
  const int dx_ = INV >= 0 ? 2 : A.dx;
  using Cfg = PairCfg<D, BF16>;
  constexpr int NW = NWAVES, NTH = NTHREADS;
  using SM = PairSmem<D, H, BF16, NW, FFN, ZFOLD, RES>;
  constexpr int KB = Cfg::KB, NT = Cfg::NT;
  constexpr int ST_DD = Cfg::DD::STAGE, ST_GB = Cfg::GB::STAGE, PANEL_GB = Cfg::GB::BYTES, PANEL_DD = Cfg::DD::BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem + SM::RING;
  float* cst = reinterpret_cast<float*>(smem + SM::CONSTS);
  float* c_bq1 = cst, *c_bv1 = cst + D, *c_bf = cst + 2 * D, *c_bm = cst + 3 * D, *c_bgb = cst + 4 * D;
  float* c_acq = c_bgb + 2 * H * D, *c_acv = c_acq + SM::EW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  float* zv = reinterpret_cast<float*>(smem + SM::ZVEC) + wave * 2 * H * D;
  float* xch = reinterpret_cast<float*>(smem + SM::XCH);
  const int QG = A.qg, ZS = NW / QG;
  const int qgi = wave % QG, zs = wave / QG;
  // XCD-aware placement (z-fold, B % 8 == 0): workgroup ids go round-robin over the 8 XCDs, and every workgroup of
  // a signal streams that signal's per-latent panels, so all of a signal's workgroups are given ids of ONE residue
  // mod 8: its 64 KB x Z of panels then enter one XCD's L2 instead of eight (HBM/fabric fetches 540 -> ~70 MB).
  int bx = blockIdx.x, by = blockIdx.y;
  if (ZFOLD && A.xcd_remap) {
    const int id = blockIdx.y * gridDim.x + blockIdx.x, xcd = id & 7, slot = id >> 3;
    by = xcd + 8 * (slot / (int)gridDim.x);
    bx = slot % (int)gridDim.x;
  }
  // ENF_VARIANT_ZFOLD_ZSPLIT ("stream-K" over the latents): this workgroup owns the latent steps [f0, f1) of the flattened
  // (signal, query tile, latent) space -- the same count for every workgroup, so one round of <= 256 workgroups ends together -- and
  // walks them as one or more SEGMENTS, each a run of latents of one query tile that leaves partial sums in that tile's slot `part`
  const bool split = ZFOLD && A.zsplit > 1;
  const bool shared = !ZFOLD && A.spart != nullptr;    // blockIdx.y is then a part of signal 0's latents, not a signal
  const int tiles_n = (A.N + 16 * QG - 1) / (16 * QG);
  int f0 = split ? (int)blockIdx.x * A.sk_len : 0;
  const int f1 = split ? min(f0 + A.sk_len, tiles_n * A.B * A.Z) : 0;
  const char* blob = A.blob;
  auto G = [&](size_t off) { return reinterpret_cast<const float*>(blob + off); };

  // ---- constants -> LDS
  for (int i = tid; i < D; i += NTH) { c_bq1[i] = G(A.L.bq1)[i]; c_bv1[i] = G(A.L.bv1)[i]; c_bf[i] = G(A.L.bf)[i]; c_bm[i] = G(A.L.bm)[i]; }
  for (int i = tid; i < 2 * H * D; i += NTH) c_bgb[i] = G(A.L.bgb)[i];
  for (int i = tid; i < SM::EW; i += NTH) { c_acq[i] = G(A.L.acq)[i]; c_acv[i] = G(A.L.acv)[i]; }

  const unsigned pQ1 = (unsigned)A.L.aq1, pV1 = (unsigned)A.L.av1, pF = (unsigned)A.L.af, pGB = (unsigned)A.L.agb, pM = (unsigned)A.L.am;
  Pipe P;
  P.rs = make_blob_rsrc(blob, (unsigned)A.L.total);
  // ---- resident panels -> LDS, once per workgroup: retired by the wait + barrier of the first first_stage below
  constexpr bool rQ1 = SM::has(RP_Q1), rV1 = SM::has(RP_V1), rF = SM::has(RP_F), rM = SM::has(RP_M);
  constexpr int oQ1 = SM::off(RP_Q1), oV1 = SM::off(RP_V1), oF = SM::off(RP_F), oM = SM::off(RP_M);
  {
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    if constexpr (rQ1) resident_load<PANEL_DD, NW>(P.rs, pQ1, smem + oQ1, wv, lane);
    if constexpr (rV1) resident_load<PANEL_DD, NW>(P.rs, pV1, smem + oV1, wv, lane);
    if constexpr (rF) resident_load<PANEL_DD, NW>(P.rs, pF, smem + oF, wv, lane);
    if constexpr (rM) resident_load<PANEL_DD, NW>(P.rs, pM, smem + oM, wv, lane);
  }
  // The ring carries the streamed panels only, each stage naming the next STREAMED one.  A step multiplies in the order
  // Q1, V1, F (positions 0, 1, 2; the ffn embedding has no Q1 / V1) and then per head W_zh (z-fold) or GB_h, M (latent-split);
  // W_zh and GB_h always stream, so position 3 ends the search.  first_from(pos): the first streamed panel at or behind `pos`
  // (`at3`: the one at position 3), ST_FROM<pos>: its stage size.
  constexpr bool sQ1 = !FFN && !rQ1, sV1 = !FFN && !rV1, sF = !rF;
  auto first_from = [&](int pos, unsigned at3) { return sQ1 && pos <= 0 ? pQ1 : sV1 && pos <= 1 ? pV1 : sF && pos <= 2 ? pF : at3; };
  constexpr int ST_3 = ZFOLD ? ST_DD : ST_GB;
  constexpr int ST_FROM0 = sQ1 || sV1 || sF ? ST_DD : ST_3, ST_FROM1 = sV1 || sF ? ST_DD : ST_3, ST_FROM2 = sF ? ST_DD : ST_3;
  float sm_m[H], sm_l[H], sm_c[H];     // softmax state against a per-column reference logit (the first one seen); fp32 accumulators
  f32x4 Y[H][NT];
  int b, n0;
 for (;;) {                            // one pass per segment (exactly one without the split)
  int z_lo = 0, seg_iters = 0, part = 0;
  if (split) {
    const int tf = f0 / A.Z;
    z_lo = f0 - tf * A.Z;
    seg_iters = min(A.Z - z_lo, f1 - f0);
    part = (int)blockIdx.x - (tf * A.Z) / A.sk_len;
    by = tf / tiles_n;
    bx = tf - by * tiles_n;
    f0 += seg_iters;
  }
  b = shared ? 0 : by;
  n0 = (bx * QG + qgi) * 16;
  const int n = min(n0 + col, A.N - 1);
  const QueryPt q = load_query(A.x + (size_t)b * A.x_bstride + (size_t)n * dx_, dx_, inv_id);
  if constexpr (ZFOLD) P.rs2 = make_blob_rsrc(A.wz + (size_t)b * A.Z * H * PANEL_DD, (unsigned)(A.Z * H * PANEL_DD));
  else P.rs2 = P.rs;
  auto wzp = [&](int zz, int h_) { return STAGE_RS2 | (unsigned)((zz * H + h_) * PANEL_DD); };    // z-fold: W_zh of latent zz
  first_stage<ST_FROM0, NW>(P, ring, first_from(0, ZFOLD ? wzp(z_lo, 0) : pGB), wave, lane);
  // the z-fold stages of this kernel: 2-slot staging (look-ahead and antiphase 3-slot staging measured 3 % / 2 % slower)
  auto zgemm = [&](f32x4 (&acc_)[NT], const Frags<BF16, KB>& F_, unsigned panel_, unsigned next_, bool active_, const float* bias_) {
    panel_gemm<KB, NT, BF16, ST_DD, NW, INIT_ACC>(acc_, F_, P, ring, panel_, next_, active_, lane, bias_);
  };
  auto rgemm = [&](f32x4 (&acc_)[NT], const Frags<BF16, KB>& F_, int off_, bool active_, const float* bias_) {
    resident_gemm<KB, NT, BF16, INIT_ACC>(acc_, F_, smem + off_, active_, lane, bias_);
  };

#pragma unroll
  for (int h = 0; h < H; ++h) {
    sm_m[h] = -INFINITY; sm_l[h] = 0.f; sm_c[h] = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) Y[h][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int ltstride = enf_lt_stride(H, D);
  // latent-split: this workgroup's latents [z_first, z_end) -- all of them, or with `shared` part `by`: a contiguous ceil(Z / parts),
  // the last part the rest; a wave whose share of them is empty stays at m = -inf, l = c = 0, Y = 0.  The helper's P ZS <= Z keeps
  // every wave of a FULL part busy, but the last part may be short (Z = 65, P = 8: 2 latents, six empty waves), and from P = 16 on
  // whole trailing parts can be empty ((P - 1) ceil(Z / P) >= Z, e.g. Z = 129: part 15 starts at 135): such a workgroup walks its
  // passes inactive and stores m* = -inf, L = C = 0, Y = 0
  const int zpart = shared ? (A.Z + A.parts - 1) / A.parts : A.Z;
  const int z_first = shared ? by * zpart : 0, z_end = shared ? min(z_first + zpart, A.Z) : A.Z;
  const int iters = split ? seg_iters : ZFOLD ? A.Z : (zpart + ZS - 1) / ZS;
  for (int it = 0; it < iters; ++it) {
    const int z = ZFOLD ? z_lo + it : z_first + it * ZS + zs;
    const bool active = z < z_end;
    const unsigned at3 = ZFOLD ? wzp(z, 0) : pGB;                                              // this step's first per-head panel
    const unsigned wrap = it + 1 < iters ? first_from(0, ZFOLD ? wzp(z + 1, 0) : pGB) : NO_STAGE;   // the next step's first stage
    const float* ltrow = A.lt + ((size_t)b * A.Z + (active ? z : A.Z - 1)) * ltstride;
    STAMP(0);
    // per-latent vectors u | v0 -> wave-private LDS
    if constexpr (ZFOLD) {      // u (bf16: as A-operand rows) and c_zh from the fold kernel
      const float* czrow = A.wzb + ((size_t)b * A.Z + z) * (H * D);
#pragma unroll
      for (int i = lane * 4; i < H * D; i += 256) {
        if constexpr (!BF16) *reinterpret_cast<f32x4*>(zv + i) = *reinterpret_cast<const f32x4*>(ltrow + i);
        *reinterpret_cast<f32x4*>(zv + H * D + i) = *reinterpret_cast<const f32x4*>(czrow + i);
      }
      if constexpr (BF16) {
        if (lane < KB * 4 * H)
          *reinterpret_cast<f32x4*>(zv + lane * 4) =
              *reinterpret_cast<const f32x4*>(A.wzu + ((size_t)b * A.Z + z) * enf_wzu_bytes(H, D) + lane * 16);
      }
    } else {
#pragma unroll
      for (int i = lane * 4; i < 2 * H * D; i += 256)
        *reinterpret_cast<f32x4*>(zv + i) = *reinterpret_cast<const f32x4*>(ltrow + i);
    }
    const f32x4 pz = *reinterpret_cast<const f32x4*>(ltrow + enf_lt_off_pose(H, D));
    const float wcoef = ltrow[enf_lt_off_wcoef(H, D)];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    float inv[4], win;
    const bool has_ph = INV < 0 && D == 64 && enf_inv_has_phase(inv_id);   // ball / ball_lat (64-wide only): rotation matrix and RFF phases of the latent
    pair_invariant<enf_bf16_valued(BF16)>(inv_id, dx_, q, pz, wcoef, A.use_window, inv, win, ltrow + enf_lt_off_ext(H, D));

    float logit[H];
    Frags<BF16, KB> F;
    {  // ---------------- query branch
      f32x4 acc[NT];
      if constexpr (FFN) {
        ffn_pre<D>(acc, inv, c_acq, c_bq1, col, quad);
        gelu_tiles<NT>(acc);
      } else {
        rff_embed<D, BF16>(acc, inv, c_acq, lane, quad, has_ph ? ltrow + enf_lt_off_phq(H, D) : nullptr);
        make_frags<BF16, KB>(F, acc);
        K2_BIAS(acc, c_bq1);
        STAMP(1);
        if constexpr (rQ1) rgemm(acc, F, oQ1, active, c_bq1);
        else panel_gemm<KB, NT, BF16, ST_FROM1, NW, INIT_ACC>(acc, F, P, ring, pQ1, first_from(1, at3), active, lane, c_bq1);
      }
      STAMP(2);
      const bool mread = FFN || K2_MASK_MODE == 2;                // wave-uniform; also: no relu to apply (ffn)
      if (K2_MASK_MODE) {
        const size_t mrow = relu_mask_index(b % A.mask_B, A.Z, active ? z : A.Z - 1, (A.N + 15) / 16, n0 / 16, 0, lane);
        if (K2_MASK_MODE == 1 && active && n0 < A.N) A.masks[mrow] = relu_mask_of<NT>(acc);
        if (mread) relu_apply_mask<NT>(acc, n0 < A.N ? A.masks[mrow] : 0u);
      }
      if constexpr (ZFOLD && BF16) {
        // logits on the matrix pipe: rows 0..H-1 of the A operand are u_zh (bf16, packed by enf_wz_kernel),
        // B = relu(a1) fragments; lane (col, quad 0) register h then holds h1 . u_h of query `col`
        static_assert(H <= 4, "logit rows live in one quad");
        make_frags<BF16, KB>(F, acc);
        if (!mread) relu_frags<BF16, KB>(F);
        f32x4 lg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int blk = 0; blk < KB; ++blk) {
          bf16x8 ua = __builtin_bit_cast(bf16x8, f32x4{0.f, 0.f, 0.f, 0.f});
          if (col < H) ua = *reinterpret_cast<const bf16x8*>(zv + ((blk * 4 + quad) * H + col) * 4);
          lg = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ua, F.f[blk], lg, 0, 0, 0);
        }
#pragma unroll
        for (int h = 0; h < H; ++h) logit[h] = __shfl(lg[h], col, 64) + ltrow[enf_lt_off_c(H, D) + h] + win;
      } else
#pragma unroll
      for (int h = 0; h < H; ++h) {
        float s = 0.f;           // (as a packed-pair sum -- tiles_dot, enf_device.h -- this loop measured 0.6 % SLOWER on the fit-shape forward)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if constexpr (ZFOLD && enf_bf16_valued(BF16)) {     // fp32 layout, the matrix-pipe branch's bf16 values: rounded h1 and u
            const f32x4 u = bf16_round4(rowvec(zv + h * D, t, quad)), a = bf16_round4(acc[t]);
#pragma unroll
            for (int i = 0; i < 4; ++i) s = fmaf(mread ? a[i] : relu_f(a[i]), u[i], s);
          } else {
            const f32x4 u = rowvec(zv + h * D, t, quad);
#pragma unroll
            for (int i = 0; i < 4; ++i) s = fmaf(mread ? acc[t][i] : relu_f(acc[t][i]), u[i], s);
          }
        }
        logit[h] = xquad_sum(s) + ltrow[enf_lt_off_c(H, D) + h] + win;
      }
    }
    STAMP(3);
    {  // ---------------- value branch: RFFNet layer (ffn: Dense_0 + gelu), folded (linear_final . Dense_0), gelu, LN
      f32x4 acc[NT];
      if constexpr (FFN) {
        ffn_pre<D>(acc, inv, c_acv, c_bv1, col, quad);
        gelu_tiles<NT>(acc);
      } else {
        rff_embed<D, BF16>(acc, inv, c_acv, lane, quad, has_ph ? ltrow + enf_lt_off_phv(H, D) : nullptr);
        make_frags<BF16, KB>(F, acc);
        K2_BIAS(acc, c_bv1);
        STAMP(4);
        if constexpr (rV1) rgemm(acc, F, oV1, active, c_bv1);
        else panel_gemm<KB, NT, BF16, ST_FROM2, NW, INIT_ACC>(acc, F, P, ring, pV1, first_from(2, at3), active, lane, c_bv1);
      }
      STAMP(5);
      const bool mread = FFN || K2_MASK_MODE == 2;
      if (K2_MASK_MODE) {
        const size_t mrow = relu_mask_index(b % A.mask_B, A.Z, active ? z : A.Z - 1, (A.N + 15) / 16, n0 / 16, 1, lane);
        if (K2_MASK_MODE == 1 && active && n0 < A.N) A.masks[mrow] = relu_mask_of<NT>(acc);
        if (mread) relu_apply_mask<NT>(acc, n0 < A.N ? A.masks[mrow] : 0u);
      }
      make_frags<BF16, KB>(F, acc);
      if (!mread) relu_frags<BF16, KB>(F);
      K2_BIAS(acc, c_bf);
      STAMP(6);
      if constexpr (rF) rgemm(acc, F, oF, active, c_bf);
      else panel_gemm<KB, NT, BF16, ST_3, NW, INIT_ACC>(acc, F, P, ring, pF, at3, active, lane, c_bf);
      STAMP(7);
      gelu_tiles<NT>(acc);
      float mu, rstd;
      ln_stats<NT>(acc, mu, rstd, A.inv_d);
      ln_apply<NT>(acc, mu, rstd);
      make_frags<BF16, KB>(F, acc);   // F = normalised f, shared by all heads' gamma/beta panels
      STAMP(8);
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
      f32x4 v[NT];
      if constexpr (ZFOLD) {
        const unsigned wzh = STAGE_RS2 | (unsigned)((z * H + h) * PANEL_DD);
        K2_BIAS(v, zv + H * D + h * D);
        STAMP(10 + 4 * h);
        zgemm(v, F, wzh, h + 1 < H ? wzh + PANEL_DD : wrap, active, zv + H * D + h * D);
      } else {
        f32x4 dummy[1];
        const float* gbias = c_bgb + 2 * h * D, *v0 = zv + H * D + h * D;
        if constexpr (!rM) gb_panel<D, BF16, ST_DD, false, NW>(v, dummy, F, P, ring, pGB + h * PANEL_GB, pM, active, gbias, v0, lane, quad);
        else if (h + 1 < H) gb_panel<D, BF16, ST_GB, false, NW>(v, dummy, F, P, ring, pGB + h * PANEL_GB, pGB + (h + 1) * PANEL_GB, active, gbias, v0, lane, quad);
        else gb_panel<D, BF16, ST_FROM0, false, NW>(v, dummy, F, P, ring, pGB + h * PANEL_GB, wrap, active, gbias, v0, lane, quad);
        STAMP(9 + 4 * h);
        Frags<BF16, KB> FV;
        make_frags<BF16, KB>(FV, v);
        K2_BIAS(v, c_bm);
        STAMP(10 + 4 * h);
        if constexpr (rM) rgemm(v, FV, oM, active, c_bm);
        else if (h + 1 < H) panel_gemm<KB, NT, BF16, ST_GB, NW, INIT_ACC>(v, FV, P, ring, pM, pGB + (h + 1) * PANEL_GB, active, lane, c_bm);
        else panel_gemm<KB, NT, BF16, ST_FROM0, NW, INIT_ACC>(v, FV, P, ring, pM, wrap, active, lane, c_bm);
      }
      STAMP(11 + 4 * h);
      gelu_tiles<NT>(v);
      float mu, rstd;
      ln_stats<NT>(v, mu, rstd, A.inv_d);
      if (active) {
        // softmax over this wave's latents (ECA:141-144).  The rare "logit far above the
        // reference" case rescales the accumulators (wave-uniform branch).
        if (it == 0) sm_m[h] = logit[h];
        const bool far = logit[h] - sm_m[h] > 40.0f;
        if (__any(far)) {
          const float alpha = far ? __expf(sm_m[h] - logit[h]) : 1.0f;
          sm_l[h] *= alpha; sm_c[h] *= alpha;
          if (far) sm_m[h] = logit[h];
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) Y[h][t][i] *= alpha;
        }
        const float pe = __expf(logit[h] - sm_m[h]);
        const float w = pe * rstd;
        sm_l[h] += pe;
        sm_c[h] = fmaf(w, mu, sm_c[h]);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) Y[h][t][i] = fmaf(w, v[t][i], Y[h][t][i]);
      }
      STAMP(12 + 4 * h);
    }
  }

  pipe_finish(P);
  if constexpr (ZFOLD) {
    if (split) {               // partial weighted sums against this segment's own reference logit + (m, l, c): merged afterwards
      if (n0 + col < A.N) {
        const size_t BN = (size_t)A.B * A.N, row = (size_t)b * A.N + n0 + col;
        float* yo = A.ysplit + ((size_t)part * BN + row) * (H * D);
        float* so = A.ysplit + (size_t)A.zsplit * BN * (H * D) + ((size_t)part * BN + row) * (H * 3);
#pragma unroll
        for (int h = 0; h < H; ++h) {
#pragma unroll
          for (int t = 0; t < NT; ++t) *reinterpret_cast<f32x4*>(yo + h * D + 16 * t + 4 * quad) = Y[h][t];
          if (quad == 0) { so[h * 3] = sm_m[h]; so[h * 3 + 1] = sm_l[h]; so[h * 3 + 2] = sm_c[h]; }
        }
      }
      if (f0 >= f1) return;
      continue;                // (the closing barrier of the last stage is behind every wave: the ring and zv are free again)
    }
  }
  break;
 }
  // ---- combine the ZS latent splits of each query group (all staging is finished: ring is free)
  if (quad == 0) {
#pragma unroll
    for (int h = 0; h < H; ++h) {
      xch[((wave * H + h) * 3 + 0) * 16 + col] = sm_m[h];
      xch[((wave * H + h) * 3 + 1) * 16 + col] = sm_l[h];
      xch[((wave * H + h) * 3 + 2) * 16 + col] = sm_c[h];
    }
  }
  __syncthreads();
  float Ltot[H], Ctot[H], mstar[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    float ms = -INFINITY;
    for (int s = 0; s < ZS; ++s) ms = fmaxf(ms, xch[(((s * QG + qgi) * H + h) * 3 + 0) * 16 + col]);
    float L = 0.f, C = 0.f;
    for (int s = 0; s < ZS; ++s) {
      const int w = s * QG + qgi;
      const float aw = __expf(xch[((w * H + h) * 3 + 0) * 16 + col] - ms);
      L = fmaf(aw, xch[((w * H + h) * 3 + 1) * 16 + col], L);
      C = fmaf(aw, xch[((w * H + h) * 3 + 2) * 16 + col], C);
    }
    if (shared && ms == -INFINITY) { L = 0.f; C = 0.f; }     // a part without a latent (the merge skips it)
    mstar[h] = ms; Ltot[h] = L; Ctot[h] = C;
    float sc = __expf(sm_m[h] - ms) / L;           // exp(-inf) = 0 for a split that saw no latent
    if (shared) sc = ms == -INFINITY ? 0.f : __expf(sm_m[h] - ms);      // un-normalised: the merge divides by the parts' L
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) Y[h][t][i] *= sc;
  }
  // deterministic tree over the split index: splits [s, 2s) hand their partial sums to [0, s)
  float* cb = reinterpret_cast<float*>(ring);
  for (int s = ZS >> 1; s >= 1; s >>= 1) {
    if (zs >= s && zs < 2 * s) {
      float* dst = cb + (size_t)((zs - s) * QG + qgi) * (SM::YBYTES / 4);
#pragma unroll
      for (int h = 0; h < H; ++h)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) dst[((h * NT + t) * 4 + i) * 64 + lane] = Y[h][t][i];
    }
    __syncthreads();
    if (zs < s) {
      const float* src = cb + (size_t)(zs * QG + qgi) * (SM::YBYTES / 4);
#pragma unroll
      for (int h = 0; h < H; ++h)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) Y[h][t][i] += src[((h * NT + t) * 4 + i) * 64 + lane];
    }
    __syncthreads();
  }
  if (shared) {                // this part's partial sums against its reference m* and (m*, L, C): enf_shared_merge_kernel
    if (zs == 0 && n0 + col < A.N) {
      const size_t row = (size_t)by * A.N + n0 + col;
      float* yo = A.spart + row * (H * D);
      float* so = A.spart + (size_t)A.parts * A.N * (H * D) + row * (H * 3);
#pragma unroll
      for (int h = 0; h < H; ++h) {
#pragma unroll
        for (int t = 0; t < NT; ++t) *reinterpret_cast<f32x4*>(yo + h * D + 16 * t + 4 * quad) = Y[h][t];
        if (quad == 0) { so[h * 3] = mstar[h]; so[h * 3 + 1] = Ltot[h]; so[h * 3 + 2] = Ctot[h]; }
      }
    }
    return;
  }
  if (zs == 0 && n0 + col < A.N) {
    float* yo = A.ybar + ((size_t)b * A.N + n0 + col) * (H * D);
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const float cs = Ctot[h] / Ltot[h];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        f32x4 o = Y[h][t];
        o[0] -= cs; o[1] -= cs; o[2] -= cs; o[3] -= cs;
        if (!MASKS && BF16 && A.ybar_half) {      // (wave-uniform; masked passes are training passes) round to nearest even, as the tail's make_frags would
          unsigned short* yh = reinterpret_cast<unsigned short*>(A.ybar) + ((size_t)b * A.N + n0 + col) * (H * D);
          *reinterpret_cast<uint2*>(yh + h * D + 16 * t + 4 * quad) = uint2{bf16_pack2(o[0], o[1]), bf16_pack2(o[2], o[3])};
        } else {
          *reinterpret_cast<f32x4*>(yo + h * D + 16 * t + 4 * quad) = o;
        }
      }
      if (quad == 0) A.lse[((size_t)b * A.N + n0 + col) * H + h] = mstar[h] + __logf(Ltot[h]);
    }
  }
}

// ENF_VARIANT_ZFOLD_ZSPLIT: ybar[row][h][:] = sum_s e^{m_s - m*} Y_s / L - C / L,  lse = m* + log L  with  L = sum_s e^{m_s - m*} l_s (C alike):
// exactly the in-kernel combine of the latent-split variant, across workgroups.  One thread per (row, feature).
__global__ __launch_bounds__(256) void enf_zsplit_merge_kernel(const float* __restrict__ ysplit, int S, long long BN, int H, int D,
                                                              int N, int Z, int sk_len, float* __restrict__ ybar, float* __restrict__ lse) {
  const int HD = H * D;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= BN * HD) return;
  const long long row = e / HD;
  const int c = (int)(e % HD), h = c / D;
  // the parts of this row's query tile: the workgroups whose runs meet its latent steps [tf Z, (tf + 1) Z)
  const int tiles_n = (N + 127) / 128, tf = (int)(row / N) * tiles_n + (int)(row % N) / 128;
  const int parts = (tf * Z + Z - 1) / sk_len - (tf * Z) / sk_len + 1;
  const float* st = ysplit + (size_t)S * BN * HD;
  float ms = -INFINITY;
  for (int s = 0; s < parts; ++s) ms = fmaxf(ms, st[((size_t)s * BN + row) * (H * 3) + h * 3]);
  float L = 0.f, C = 0.f, y = 0.f;
  for (int s = 0; s < parts; ++s) {
    const float* q = st + ((size_t)s * BN + row) * (H * 3) + h * 3;
    const float aw = __expf(q[0] - ms);
    L = fmaf(aw, q[1], L);
    C = fmaf(aw, q[2], C);
    y = fmaf(aw, ysplit[((size_t)s * BN + row) * HD + c], y);
  }
  ybar[(size_t)row * HD + c] = (y - C) / L;
  if (c % D == 0) lse[(size_t)row * H + h] = ms + __logf(L);
}

// The shared-latent forward's merge: the parts of signal 0's row -> ybar / lse of that row in all `bcast` signals, by the formula of
// the in-kernel combine (and of enf_zsplit_merge_kernel): ybar = (sum_r e^{m_r - m*} Y_r - C) / L, lse = m* + log L with
// L = sum_r e^{m_r - m*} L_r (C alike); a part with m_r = -inf saw no latent and adds nothing.  One thread per (row, 4 features);
// blockIdx.y strides over the signals.
__global__ __launch_bounds__(256) void enf_shared_merge_kernel(const float* __restrict__ part, int P, int N, int H, int D, int bcast,
                                                              float* __restrict__ ybar, float* __restrict__ lse) {
  const int HD = H * D, Q = HD / 4;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)N * Q) return;
  const int row = (int)(e / Q), c = (int)(e % Q) * 4, h = c / D;
  const float* st = part + (size_t)P * N * HD;
  float ms = -INFINITY;
  for (int r = 0; r < P; ++r) ms = fmaxf(ms, st[((size_t)r * N + row) * (H * 3) + h * 3]);
  float L = 0.f, C = 0.f;
  f32x4 y = {0.f, 0.f, 0.f, 0.f};
  for (int r = 0; r < P; ++r) {
    const float* q = st + ((size_t)r * N + row) * (H * 3) + h * 3;
    const float aw = q[0] == -INFINITY ? 0.f : __expf(q[0] - ms);
    const f32x4 yr = *reinterpret_cast<const f32x4*>(part + ((size_t)r * N + row) * HD + c);
    L = fmaf(aw, q[1], L);
    C = fmaf(aw, q[2], C);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = fmaf(aw, yr[i], y[i]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = (y[i] - C) / L;
  const float ls = ms + __logf(L);
  for (int b = blockIdx.y; b < bcast; b += gridDim.y) {
    *reinterpret_cast<f32x4*>(ybar + ((size_t)b * N + row) * HD + c) = y;
    if (c % D == 0) lse[((size_t)b * N + row) * H + h] = ls;
  }
}

#ifdef ENF_TEST_HOOKS
// Test library only: enf_test_pair_fwd_streamed(1) makes every following pair forward run with an EMPTY resident set (all panels
// through the ring), the reference tests/test_gpu_resident_panels.py compares the resident kernels with; (0) switches back.
static int g_test_streamed = 0;
extern "C" int enf_test_pair_fwd_streamed(int on) { const int was = g_test_streamed; g_test_streamed = on != 0; return was; }
#endif

template <int D, int H, bool BF16, bool ZFOLD, bool MASKS = false, int INV = -1, bool FFN = false, bool RES = true>
static int launch_pair_fwd(const PairFwdArgs& A, hipStream_t st) {
  if constexpr (!MASKS && !FFN) {
    if (A.mask_mode) return launch_pair_fwd<D, H, BF16, ZFOLD, true>(A, st);       // (the masked passes keep the run-time invariant)
  }
#ifdef ENF_TEST_HOOKS
  if constexpr (RES) {
    if (g_test_streamed) return launch_pair_fwd<D, H, BF16, ZFOLD, MASKS, INV, FFN, false>(A, st);
  }
#endif
  using SM = PairSmem<D, H, BF16, NWAVES, FFN, ZFOLD, RES>;
  constexpr auto kern = enf_pair_fwd_kernel<D, H, BF16, ZFOLD, MASKS, INV, FFN, RES>;
  if (!enf_lds_attr<kern>(SM::TOTAL)) return ENF_ELAUNCH;
  dim3 grid((A.N + 16 * A.qg - 1) / (16 * A.qg), A.B);
  if (ZFOLD && A.zsplit > 1) grid = dim3((unsigned)(((long long)grid.x * A.B * A.Z + A.sk_len - 1) / A.sk_len));
  const bool shared = !ZFOLD && A.spart != nullptr;
  if (shared) grid.y = (unsigned)A.parts;
  hipLaunchKernelGGL(kern, grid, dim3(NTHREADS), SM::TOTAL, st, A);
  if (shared) {
    const long long tot = (long long)A.N * (H * D / 4);
    hipLaunchKernelGGL(enf_shared_merge_kernel, dim3((unsigned)((tot + 255) / 256), (unsigned)(A.bcast < 4 ? A.bcast : 4)), dim3(256), 0, st,
                       (const float*)A.spart, A.parts, A.N, H, D, A.bcast, A.ybar, A.lse);
  }
  if (ZFOLD && A.zsplit > 1) {
    const long long BN = (long long)A.B * A.N, tot = BN * H * D;
    hipLaunchKernelGGL(enf_zsplit_merge_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const float*)A.ysplit, A.zsplit, BN, H, D,
                       A.N, A.Z, A.sk_len, A.ybar, A.lse);
  }
  return hipGetLastError() == hipSuccess ? 0 : ENF_ELAUNCH;
}

// relu masks: per call (EnfDims.masks / mask_mode / mask_B, from the descriptor)
int enf_launch_pair_fwd(const EnfDims& m, const EnfLayout& L, const char* blob, const float* x, long long x_bstride,
                        const float* lt, float* ybar, float* lse, const EnfFoldFwd& zs, unsigned flags, hipStream_t st, float* spart) {
  const bool run_pair = flags & ENF_PAIR_PAIR, yhalf = flags & ENF_PAIR_YBAR_HALF;
  PairFwdArgs A;
  A.x = x; A.x_bstride = x_bstride; A.lt = lt; A.blob = blob; A.L = L; A.ybar = ybar; A.lse = lse; A.wz = zs.wz; A.wzb = zs.wzb; A.wzu = zs.wzu; A.inv_d = 1.0f / (float)m.Dt;
  A.B = m.B; A.N = m.N; A.Z = m.Z; A.dx = m.dx; A.inv = m.inv; A.use_window = m.use_window;
  A.masks = m.masks; A.mask_mode = run_pair && !m.ffn ? m.mask_mode : 0; A.mask_B = m.mask_B;   // (ffn: no relu, no masks)
  // the bf16 hand-off is the caller's decision, made once for this launcher and the tail's (enf_api.hip: yhalf).  The masked
  // instantiations store fp32 rows only: a caller that asks for both has decided wrongly -- refused, not answered with fp32 rows
  // that its tail would read as bf16
  if (yhalf && A.mask_mode) return ENF_EINVAL;
  // as many latent splits as there are latents to split (up to 8); the rest of the 8 waves take more queries
  static_assert(NWAVES == 8, "enf_latent_splits (enf_layout.h) splits 8 waves");
  A.qg = NWAVES / enf_latent_splits(m.Z);
  const bool zfold = zs.wz && zs.wzb && zs.wzu && enf_pair_fwd_zfold_fits(m);
  const EnfStreamK sk = enf_zfold_streamk(m);
  A.zsplit = zfold && zs.ysplit && sk.parts > 1 ? sk.parts : 1;
  A.sk_len = A.zsplit > 1 ? sk.len : 0;
  A.ysplit = zs.ysplit;
  A.ybar_half = yhalf && A.zsplit == 1 && m.bf16;
  A.xcd_remap = zfold && m.B % 8 == 0 && A.zsplit == 1;
  // the shared-latent forward is a permission: it runs on the latent-split kernel, without relu masks, with ybar in fp32
  const int sparts = spart && !zfold && !A.mask_mode && run_pair && !yhalf ? enf_shared_fwd_parts(m) : 0;
  A.spart = sparts ? spart : nullptr; A.parts = sparts ? sparts : 1; A.bcast = sparts ? m.B : 1;
  if (zfold) {
    A.qg = NWAVES;
    if (flags & ENF_PAIR_FOLD) {
      int rc = enf_launch_wz(m, L, blob, lt, zs.wz, zs.wzb, zs.wzu, nullptr, st);
      if (rc) return rc;
    }
  }
  if (!run_pair) return 0;
  // the ffn embedding: every shape, run-time invariant; rff: the shipped configs' bf16 kernels with the invariant fixed at compile
  // time (enf_layout.h: enf_spec_inv), here without relu masks only
  const int spec = m.ffn || A.mask_mode ? -1 : enf_spec_inv(m);
  return enf_for_shape(m, [&](auto s) {
    using S = decltype(s);
    if (m.ffn)
      return zfold ? launch_pair_fwd<S::D, S::H, S::BF16, true, false, -1, true>(A, st) : launch_pair_fwd<S::D, S::H, S::BF16, false, false, -1, true>(A, st);
    return enf_for_spec<S>(spec, [&](auto i) {
      return zfold ? launch_pair_fwd<S::D, S::H, S::BF16, true, false, i.INV>(A, st) : launch_pair_fwd<S::D, S::H, S::BF16, false, false, i.INV>(A, st);
    });
  });
}
