// enf_tail_common.h -- what the per-query tail kernels of enf_tail.hip and the tangent / Gauss-Newton tails of enf_tangent.hip share:
// the row <-> accumulator moves, the shapes of the tail's chain and the constants' load.  Device code only; include it behind
// enf_device.h (enf_tail.hip sets ENF_PIPE_ONE_RS first).
#pragma once
#include "enf_layout.h"
#include "enf_device.h"

// row-per-query global <-> acc layout (feature f = 16 t + 4 quad + i lives in tile t register i)
template <int NT> DEV void load_rows(f32x4 (&X)[NT], const float* row, int quad) {
#pragma unroll
  for (int t = 0; t < NT; ++t) X[t] = *reinterpret_cast<const f32x4*>(row + 16 * t + 4 * quad);
}
template <int NT> DEV void store_rows(const f32x4 (&X)[NT], float* row, int quad) {
#pragma unroll
  for (int t = 0; t < NT; ++t) *reinterpret_cast<f32x4*>(row + 16 * t + 4 * quad) = X[t];
}
template <int NT> DEV void zero_tiles(f32x4 (&X)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) X[t] = f32x4{0.f, 0.f, 0.f, 0.f};
}

template <int D, int H, bool BF16> struct TailCfg {
  static constexpr int KB = D / 32, KBH = H * D / 32, NT = D / 16, NTH = H * D / 16, HD = H * D;
  static constexpr int ACT = 2 * HD + 2 * D + 2;   // a_B | a_F1 | a_O0 | a_O2 | mu | rstd
  static constexpr int ST_TB = PanelCfg<KBH, NTH, BF16>::STAGE;   // HD x HD
  static constexpr int ST_O0 = PanelCfg<KBH, NT, BF16>::STAGE;    // out D, in HD
  static constexpr int ST_O2 = PanelCfg<KB, NT, BF16>::STAGE;     // D x D
  static constexpr int ST_O4 = PanelCfg<KB, 2, BF16>::STAGE;      // out 32 (O padded), in D
  static constexpr int ST_G4 = PanelCfg<1, NT, BF16>::STAGE;      // gto4: out D, in 32
  static constexpr int ST_G0 = PanelCfg<KB, NTH, BF16>::STAGE;    // gto0: out HD, in D
  static constexpr int SMEM = 2 * STAGE_MAX + 4 * (2 * HD + 2 * D + 32);
  static constexpr int SMEM3 = 3 * STAGE_MAX + 4 * (2 * HD + 2 * D + 32);      // LA2: three ring slots
};

// the chain's bias vectors -> LDS: bB bF1 (HD each) | bO0 bO2 (D each) | bO4 (32), by the NT threads of the workgroup
template <int D, int H, bool BF16, int NT = NTHREADS>
DEV void tail_consts(float* cst, const char* blob, const EnfLayout& L, int tid) {
  constexpr int HD = H * D;
  auto G = [&](size_t off) { return reinterpret_cast<const float*>(blob + off); };
  for (int i = tid; i < HD; i += NT) { cst[i] = G(L.bB)[i]; cst[HD + i] = G(L.bF1)[i]; }
  for (int i = tid; i < D; i += NT) { cst[2 * HD + i] = G(L.bO0)[i]; cst[2 * HD + D + i] = G(L.bO2)[i]; }
  for (int i = tid; i < 32; i += NT) cst[2 * HD + 2 * D + i] = G(L.bO4)[i];
}
