// enf_pack.hip -- K0: weight packing + exact folds.
//
// K0 turns the Flax weight tree of EquivariantCrossAttentionNeF into the packed
// blob described in enf_layout.h.  Among the folds is the one of inv_emb_to_q into the keys (ECA:92 + ECA:134), which
// the latent prologue (K1, enf_prologue.hip) applies per latent:
//   att[n,z,h] = scale * q[n,z,h,:] . k[z,h,:]
//              = h1[n,z,:] . u[z,h,:] + c[z,h],   u = scale * W2 Wq_h k_h,  c = scale * (b2 Wq_h + bq_h) . k_h
// where h1 is the relu layer of the query RFFNet and (W2, b2) its linear_final (RFF:46).
#include <hip/hip_runtime.h>
#include <math.h>
#include "enf_launch.h"

#define CK(x) do { if ((x) != hipSuccess) return ENF_ELAUNCH; } while (0)

// ---------------------------------------------------------------- small dense helpers (fp32)
// C[i][j] = (acc ? C[i][j] : 0) + alpha * (sum_k A[i*lda+k] * B[k*ldb+j] + (addv ? addv[j] : 0))
__global__ __launch_bounds__(256) void mm_kernel(float* C, int ldc, const float* A, int lda, const float* B, int ldb, int M, int N, int K,
                                                 float alpha, const float* addv, int acc) {
  // 16 x 16 output tile per workgroup, operands through LDS (the one-thread-per-output form read A uncoalesced: 32 us per call)
  __shared__ float sa[16][17], sb[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i = blockIdx.y * 16 + ty, j = blockIdx.x * 16 + tx;
  float s = 0.f;
  for (int k0 = 0; k0 < K; k0 += 16) {
    sa[ty][tx] = (i < M && k0 + tx < K) ? A[(size_t)i * lda + k0 + tx] : 0.f;
    sb[ty][tx] = (k0 + ty < K && j < N) ? B[(size_t)(k0 + ty) * ldb + j] : 0.f;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) s = fmaf(sa[ty][k], sb[k][tx], s);
    __syncthreads();
  }
  if (i >= M || j >= N) return;
  if (addv) s += addv[j];
  s *= alpha;
  C[(size_t)i * ldc + j] = acc ? C[(size_t)i * ldc + j] + s : s;
}
// dst[i][j] = g[i] * src[i][j]
__global__ void rowscale_kernel(float* dst, const float* src, const float* g, int rows, int cols) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j < cols && i < rows) dst[(size_t)i * cols + j] = g[i] * src[(size_t)i * cols + j];
}
// gamma/beta column reorder (ECA:115 split: gamma = first HD columns, beta = last HD): per head h the
// 32-wide blocks alternate [g_h blk0 | b_h blk0 | g_h blk1 | b_h blk1 ..] so that one staged slice of the
// panel holds gamma AND beta of the same features:
//   dst col h*2D + (2m+t)*32 + i  <-  src col t*HD + h*D + 32m + i      (t: 0 gamma, 1 beta); rows scaled by g
__global__ void reorder_gb_kernel(float* dst, const float* src, const float* g, int rows, int H, int D) {
  const int jj = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  const int HD = H * D;
  if (jj >= 2 * HD || i >= rows) return;
  const int h = jj / (2 * D), w = jj % (2 * D), blk = w / 32, ii = w % 32, m = blk >> 1, t = blk & 1;
  dst[(size_t)i * 2 * HD + jj] = (g ? g[i] : 1.f) * src[(size_t)i * 2 * HD + t * HD + h * D + 32 * m + ii];
}
// dst (cols x rows) = src (rows x cols)^T
__global__ void transpose_kernel(float* dst, const float* src, int rows, int cols) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j < cols && i < rows) dst[(size_t)j * rows + i] = src[(size_t)i * cols + j];
}
// zero-padded copy of a (rows x cols) matrix into (rows x cols_pad)
__global__ void padcopy_kernel(float* dst, const float* src, int rows, int cols, int cols_pad) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j < cols_pad && i < rows) dst[(size_t)i * cols_pad + j] = j < cols ? src[(size_t)i * cols + j] : 0.f;
}
// RFF coefficient A-operand of t = coeff^T inv (v_mfma_f32_16x16x4_f32, K = 4 = the I <= 4 invariant
// components): [t-tile][lane], lane (i = lane&15, q = lane>>4) holds coeff[q][16 tt + i]
__global__ void coef_frag_kernel(float* dst, const float* coeff, int I, int Dh /*D/2*/) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = (Dh / 16) * 64;
  if (idx >= total) return;
  const int lane = idx & 63, tt = idx >> 6;
  const int c = lane >> 4, t = 16 * tt + (lane & 15);
  dst[idx] = c < I ? coeff[(size_t)c * Dh + t] : 0.f;
}

// coefficient rows in kernel order: dst (8 x Dh) = [the <= 4 per-pair rows | the <= 2 latent-only rows | 0] (enf_inv_rows)
__global__ void coef_perm_kernel(float* dst, const float* coeff, int inv, int I, int Dh) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (t >= Dh) return;
  int pair[4], lat[2], np, nl;
  enf_inv_rows(inv, I, pair, np, lat, nl);
  const int src = r < 4 ? (r < np ? pair[r] : -1) : (r - 4 < nl ? lat[r - 4] : -1);
  dst[(size_t)r * Dh + t] = src >= 0 ? coeff[(size_t)src * Dh + t] : 0.f;
}

// ---------------------------------------------------------------- MFMA A-operand panel packer
// A[r][k] (R x K; R multiple of 16, K multiple of 32) = scale * (trans ? W[r*ldw + k] : W[k*ldw + r]).
// bf16 (v_mfma_f32_16x16x32_bf16): byte ((mt*KB+blk)*64+lane)*16 + 2j
//        <- A[16mt + (lane&15)][32blk + 16(j>>2) + 4(lane>>4) + (j&3)]
// fp32 (v_mfma_f32_16x16x4_f32):   byte ((mt*2KB+tin)*64+lane)*16 + 4i
//        <- A[16mt + (lane&15)][16tin + 4(lane>>4) + i]
// (the k order is the one in which 16x16 accumulator tiles present their rows as the next B operand)
__global__ void pack_panel_kernel(void* dst, const float* W, int ldw, int R, int K, int trans, int bf16,
                                  int Rvalid, int Kvalid, float scale) {
  const size_t total = (size_t)R * K;
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  int r, k;
  if (bf16) {
    const int KB = K / 32;
    const int j = e & 7, lane = (e >> 3) & 63;
    const size_t g = e >> 9;  // mt*KB + blk
    const int blk = g % KB, mt = g / KB;
    r = 16 * mt + (lane & 15);
    k = 32 * blk + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3);
  } else {
    const int KT = K / 16;
    const int i = e & 3, lane = (e >> 2) & 63;
    const size_t g = e >> 8;  // mt*KT + tin
    const int tin = g % KT, mt = g / KT;
    r = 16 * mt + (lane & 15);
    k = 16 * tin + 4 * (lane >> 4) + i;
  }
  float v = 0.f;
  if (r < Rvalid && k < Kvalid) v = scale * (trans ? W[(size_t)r * ldw + k] : W[(size_t)k * ldw + r]);
  if (bf16) reinterpret_cast<__bf16*>(dst)[e] = (__bf16)v;
  else reinterpret_cast<float*>(dst)[e] = enf_bf16_valued(false) ? (float)(__bf16)v : v;      // (fp32 layout, bf16 values: ENF_F32_ROUNDED)
}

// gamma half of one head out of the [g g b b]-interleaved D x 2HD matrix: dst[i][j] = Wgamma_h[i][j]
__global__ void gamma_extract_kernel(float* dst, const float* agb, int h, int H, int D) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j < D) dst[(size_t)i * D + j] = agb[(size_t)i * 2 * H * D + h * 2 * D + 64 * (j >> 5) + (j & 31)];
}

// latent-independent parts of the per-latent fold W_zh = (Wgamma_h diag(v0) + Wbeta_h) AM (enf_wz.hip):
//   wbmt[h][k][i] = sum_j Wbeta_h[i][j] AM[j][k];  cb[h][k] = sum_j bbeta_h[j] AM[j][k] + bm[k];  opbg[h][j] = 1 + bgamma_h[j]
// agb / bgb are in the [g g b b] interleaved column order of reorder_gb_kernel.
__global__ void wz_const_kernel(float* wbmt, float* wbm, float* cb, float* opbg, const float* agb, const float* bgb, const float* am,
                                const float* bm, int H, int D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y, h = blockIdx.z;
  if (i >= D) return;
  const int HD2 = 2 * H * D;
  auto bcol = [&](int j) { return h * 2 * D + 64 * (j >> 5) + 32 + (j & 31); };   // beta column of feature j
  float s = 0.f;
  for (int j = 0; j < D; ++j) s = fmaf(agb[(size_t)i * HD2 + bcol(j)], am[(size_t)j * D + k], s);
  wbmt[((size_t)h * D + k) * D + i] = s;
  wbm[((size_t)h * D + i) * D + k] = s;
  if (i == 0) {
    float c = bm[k];
    for (int j = 0; j < D; ++j) c = fmaf(bgb[bcol(j)], am[(size_t)j * D + k], c);
    cb[h * D + k] = c;
  }
  if (k == 0) opbg[h * D + i] = 1.0f + bgb[h * 2 * D + 64 * (i >> 5) + (i & 31)];
}

static inline int mm(hipStream_t st, float* C, int ldc, const float* A, int lda, const float* B, int ldb, int M, int N,
                     int K, float alpha, const float* addv, int acc) {
  dim3 g((N + 15) / 16, (M + 15) / 16);
  hipLaunchKernelGGL(mm_kernel, g, dim3(256), 0, st, C, ldc, A, lda, B, ldb, M, N, K, alpha, addv, acc);
  return hipGetLastError() == hipSuccess ? 0 : ENF_ELAUNCH;
}
static inline int pack_panel(hipStream_t st, char* blob, size_t off, const float* W, int ldw, int R, int K, int trans,
                             int bf16, int Rvalid = -1, int Kvalid = -1, float scale = 1.0f) {
  const size_t total = (size_t)R * K;
  hipLaunchKernelGGL(pack_panel_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (void*)(blob + off), W,
                     ldw, R, K, trans, bf16, Rvalid < 0 ? R : Rvalid, Kvalid < 0 ? K : Kvalid, scale);
  return hipGetLastError() == hipSuccess ? 0 : ENF_ELAUNCH;
}

// Panels of the per-pair chain (forward: A[out][in] = W[in][out]; backward: A[in][out] = W[in][out], dX = W dY)
// from plain (in, out) matrices; `agb` is D x 2HD in the [g g b b] interleaved column order.
static int pack_pair_panels(hipStream_t st, char* blob, const EnfLayout& L, const EnfDims& m, const float* aq1,
                            const float* av1, const float* af, const float* agb, const float* am, const float* coefq,
                            const float* coefv) {
  const int D = m.D, H = m.H, HD = m.HD, I = m.I, bf = m.bf16;
  int rc;
  if (m.ffn) {
    // Dense_0 of both branches (I x D, in the R?_COEF slots) as 4 rows of D (zero rows below I): the pre-activation's A operand
    // and the rows of d inv = W0 d P in the pair kernels.  No ball invariant (enf_check_desc): the rows are in reference order.
    if (hipMemsetAsync(blob + L.acq, 0, sizeof(float) * 4 * D, st) != hipSuccess) return ENF_ELAUNCH;
    if (hipMemsetAsync(blob + L.acv, 0, sizeof(float) * 4 * D, st) != hipSuccess) return ENF_ELAUNCH;
    if (hipMemcpyAsync(blob + L.acq, coefq, sizeof(float) * I * D, hipMemcpyDeviceToDevice, st) != hipSuccess) return ENF_ELAUNCH;
    if (hipMemcpyAsync(blob + L.acv, coefv, sizeof(float) * I * D, hipMemcpyDeviceToDevice, st) != hipSuccess) return ENF_ELAUNCH;
  } else {
    // coefficient rows permuted to [per-pair rows | latent-only rows] (identity except for ball / ball_lat)
    float* cq = reinterpret_cast<float*>(blob + L.p_tmp);
    float* cv = cq + 8 * (D / 2);
    hipLaunchKernelGGL(coef_perm_kernel, dim3((D / 2 + 63) / 64, 8), dim3(64), 0, st, cq, coefq, m.inv, I, D / 2);
    hipLaunchKernelGGL(coef_perm_kernel, dim3((D / 2 + 63) / 64, 8), dim3(64), 0, st, cv, coefv, m.inv, I, D / 2);
    const int tot = (D / 32) * 64;
    hipLaunchKernelGGL(coef_frag_kernel, dim3((tot + 255) / 256), dim3(256), 0, st, reinterpret_cast<float*>(blob + L.acq), cq, 4, D / 2);
    hipLaunchKernelGGL(coef_frag_kernel, dim3((tot + 255) / 256), dim3(256), 0, st, reinterpret_cast<float*>(blob + L.acv), cv, 4, D / 2);
    if (hipGetLastError() != hipSuccess) return ENF_ELAUNCH;
    if (hipMemcpyAsync(blob + L.cphq, cq + 4 * (D / 2), sizeof(float) * D, hipMemcpyDeviceToDevice, st) != hipSuccess) return ENF_ELAUNCH;
    if (hipMemcpyAsync(blob + L.cphv, cv + 4 * (D / 2), sizeof(float) * D, hipMemcpyDeviceToDevice, st) != hipSuccess) return ENF_ELAUNCH;
    // d inv[c] = sum_t 2 pi coeff[c][t] d t[t]  (RFF:92), rows in the same order (latent-only rows 4, 5)
    if ((rc = pack_panel(st, blob, L.gcq, cq, D / 2, 16, D / 2, 1, bf, 8, D / 2, 6.283185307179586f))) return rc;
    if ((rc = pack_panel(st, blob, L.gcv, cv, D / 2, 16, D / 2, 1, bf, 8, D / 2, 6.283185307179586f))) return rc;
  }
  if (!m.ffn) {       // the relu layers' panels (rff only)
    if ((rc = pack_panel(st, blob, L.aq1, aq1, D, D, D, 0, bf))) return rc;
    if ((rc = pack_panel(st, blob, L.av1, av1, D, D, D, 0, bf))) return rc;
    if ((rc = pack_panel(st, blob, L.gq1, aq1, D, D, D, 1, bf))) return rc;
    if ((rc = pack_panel(st, blob, L.gv1, av1, D, D, D, 1, bf))) return rc;
  }
  if ((rc = pack_panel(st, blob, L.af, af, D, D, D, 0, bf))) return rc;
  if ((rc = pack_panel(st, blob, L.agb, agb, 2 * HD, 2 * HD, D, 0, bf))) return rc;
  if ((rc = pack_panel(st, blob, L.am, am, D, D, D, 0, bf))) return rc;
  if ((rc = pack_panel(st, blob, L.gf, af, D, D, D, 1, bf))) return rc;
  for (int h = 0; h < H; ++h)   // one K-slice (that head's [g g b b ..] 2D columns) per head
    if ((rc = pack_panel(st, blob, L.ggb + (size_t)h * enf_panel_bytes(D, 2 * D, bf), agb + h * 2 * D, 2 * HD, D, 2 * D, 1, bf))) return rc;
  if ((rc = pack_panel(st, blob, L.gm, am, D, D, D, 1, bf))) return rc;
  auto F = [&](size_t off) { return reinterpret_cast<float*>(blob + off); };
  hipLaunchKernelGGL(wz_const_kernel, dim3((D + 63) / 64, D, H), dim3(64), 0, st, F(L.p_wbmt), F(L.p_wbm), F(L.p_cb), F(L.p_opbg), agb,
                     F(L.bgb), am, F(L.bm), H, D);
  if (hipGetLastError() != hipSuccess) return ENF_ELAUNCH;
  for (int h = 0; h < H; ++h) {      // gamma-only forward panels (z-fold backward: flipped 1 + gamma for d v0)
    hipLaunchKernelGGL(gamma_extract_kernel, dim3((D + 63) / 64, D), dim3(64), 0, st, F(L.p_tmp), agb, h, H, D);
    if (hipGetLastError() != hipSuccess) return ENF_ELAUNCH;
    if ((rc = pack_panel(st, blob, L.awg + (size_t)h * enf_panel_bytes(D, D, bf), F(L.p_tmp), D, D, D, 0, bf))) return rc;
  }
  return ENF_OK;
}

// Pack ONLY what the pair kernels (enf_pair_forward / enf_pair_backward) read, from the "effective"
// per-pair parameters (ENF_P_* order, include/enf_hip.h): used by the training path, where folds,
// latent prologue and tail run as differentiable host-framework ops around the HIP pair kernels.
extern "C" int enf_pack_pair(const EnfDesc* d, const float* const* T, void* packed, void* stream) {
  if (!d || !T || !packed) return ENF_EINVAL;
  int rc = enf_check_desc(d);
  if (rc) return rc;
  if (d->embedding == ENF_EMB_FFN) return ENF_EUNSUPPORTED;          // the training path's pair blob: rff only
  for (int i = 0; i < ENF_NUM_PAIR_TENSORS; ++i)
    if (!T[i]) return ENF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const EnfDims m = enf_dims(d);
  const EnfLayout L = enf_layout(m);
  char* blob = (char*)packed;
  auto F = [&](size_t off) { return reinterpret_cast<float*>(blob + off); };
  const int D = m.D, H = m.H, HD = m.HD;
  const size_t f = sizeof(float);
  auto cp = [&](size_t off, const float* src, size_t n) {
    return hipMemcpyAsync(blob + off, src, n * f, hipMemcpyDeviceToDevice, st);
  };
  CK(cp(L.bq1, T[ENF_P_BQ1], D)); CK(cp(L.bv1, T[ENF_P_BV1], D)); CK(cp(L.bf, T[ENF_P_BF], D)); CK(cp(L.bm, T[ENF_P_BM], D));
  hipLaunchKernelGGL(reorder_gb_kernel, dim3((2 * HD + 127) / 128, 1), dim3(128), 0, st, F(L.bgb), T[ENF_P_BGB], (const float*)nullptr, 1, H, D);
  hipLaunchKernelGGL(reorder_gb_kernel, dim3((2 * HD + 127) / 128, D), dim3(128), 0, st, F(L.p_agb), T[ENF_P_AGB], (const float*)nullptr, D, H, D);
  if (hipGetLastError() != hipSuccess) return ENF_ELAUNCH;
  return pack_pair_panels(st, blob, L, m, T[ENF_P_AQ1], T[ENF_P_AV1], T[ENF_P_AF], F(L.p_agb), T[ENF_P_AM], T[ENF_P_COEFQ],
                          T[ENF_P_COEFV]);
}

#ifdef ENF_TEST_HOOKS
// test-only build (libenf_hip_test.so): pack a plain fp32 (K x M row-major, W[k][m]) matrix as the A operand A[m][k] = W[k][m]
extern "C" int enf_debug_pack(void* dst, const float* W, int M, int K, int bf16, void* stream) {
  const size_t total = (size_t)M * K;
  hipLaunchKernelGGL(pack_panel_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dst, W, M,
                     M, K, 0, bf16, M, K, 1.0f);
  return hipGetLastError() == hipSuccess ? 0 : ENF_ELAUNCH;
}
#endif

extern "C" int enf_pack_weights(const EnfDesc* d, const float* const* T, void* packed, void* stream) {
  if (!d || !T || !packed) return ENF_EINVAL;
  int rc = enf_check_desc(d);
  if (rc) return rc;
  const bool ffn = d->embedding == ENF_EMB_FFN;
  for (int i = 0; i < ENF_NUM_TENSORS; ++i)
    if (!T[i] && !(ffn && (i == ENF_W_RQ_W1 || i == ENF_W_RV_W1))) return ENF_EINVAL;   // ffn: the R?_W1 slots are unused
  hipStream_t st = (hipStream_t)stream;
  const EnfDims m = enf_dims(d);
  const EnfLayout L = enf_layout(m);
  char* blob = (char*)packed;
  auto F = [&](size_t off) { return reinterpret_cast<float*>(blob + off); };
  const int D = m.D, H = m.H, HD = m.HD, C = m.C, O = m.O, OP = 32 * m.OB;
  const size_t f = sizeof(float);
  const float scale = 1.0f / sqrtf((float)m.Dt);  // ECA:59 (num_hidden, not a padded width)
  auto cp = [&](size_t off, const float* src, size_t n) {
    return hipMemcpyAsync(blob + off, src, n * f, hipMemcpyDeviceToDevice, st);
  };
  // ---- prologue tensors
  CK(cp(L.stem_w, T[ENF_W_STEM_W], (size_t)C * D)); CK(cp(L.stem_b, T[ENF_W_STEM_B], D));
  CK(cp(L.lna_g, T[ENF_W_LNA_G], D)); CK(cp(L.lna_b, T[ENF_W_LNA_B], D));
  CK(cp(L.wk, T[ENF_W_K_W], (size_t)D * HD)); CK(cp(L.bk, T[ENF_W_K_B], HD));
  CK(cp(L.wv, T[ENF_W_V_W], (size_t)D * HD)); CK(cp(L.bv, T[ENF_W_V_B], HD));
  for (int h = 0; h < H; ++h) {
    if ((rc = mm(st, F(L.mu) + (size_t)h * D * D, D, T[ENF_W_RQ_W2], D, T[ENF_W_Q_W] + h * D, HD, D, D, D, scale, nullptr, 0))) return rc;
    if ((rc = mm(st, F(L.cvec) + (size_t)h * D, D, T[ENF_W_RQ_B2], D, T[ENF_W_Q_W] + h * D, HD, 1, D, D, scale, T[ENF_W_Q_B] + h * D, 0))) return rc;
  }
  for (int h = 0; h < H; ++h)
    hipLaunchKernelGGL(transpose_kernel, dim3((D + 127) / 128, D), dim3(128), 0, st, F(L.mut) + (size_t)h * D * D,
                       F(L.mu) + (size_t)h * D * D, D, D);
  hipLaunchKernelGGL(transpose_kernel, dim3((HD + 127) / 128, D), dim3(128), 0, st, F(L.wkt), T[ENF_W_K_W], D, HD);
  hipLaunchKernelGGL(transpose_kernel, dim3((HD + 127) / 128, D), dim3(128), 0, st, F(L.wvt), T[ENF_W_V_W], D, HD);
  if (hipGetLastError() != hipSuccess) return ENF_ELAUNCH;
  // ---- per-pair biases
  CK(cp(L.bq1, T[ENF_W_RQ_B1], D)); CK(cp(L.bv1, T[ENF_W_RV_B1], D)); CK(cp(L.bm, T[ENF_W_MX_B0], D));
  if ((rc = mm(st, F(L.bf), D, T[ENF_W_RV_B2], D, T[ENF_W_F1_W0], D, 1, D, D, 1.f, T[ENF_W_F1_B0], 0))) return rc;
  // bgb = LN.bias @ Dense_1 + Dense_1.bias, reordered like the panel (see reorder_gb_kernel)
  if ((rc = mm(st, F(L.p_tmp), 2 * HD, T[ENF_W_F1_BE], D, T[ENF_W_F1_W1], 2 * HD, 1, 2 * HD, D, 1.f, T[ENF_W_F1_B1], 0))) return rc;
  hipLaunchKernelGGL(reorder_gb_kernel, dim3((2 * HD + 127) / 128, 1), dim3(128), 0, st, F(L.bgb), F(L.p_tmp), (const float*)nullptr, 1, H, D);
  // ---- folded plain matrices
  if ((rc = mm(st, F(L.p_af), D, T[ENF_W_RV_W2], D, T[ENF_W_F1_W0], D, D, D, D, 1.f, nullptr, 0))) return rc;
  hipLaunchKernelGGL(reorder_gb_kernel, dim3((2 * HD + 127) / 128, D), dim3(128), 0, st, F(L.p_agb), T[ENF_W_F1_W1], T[ENF_W_F1_G], D, H, D);
  hipLaunchKernelGGL(rowscale_kernel, dim3((D + 127) / 128, D), dim3(128), 0, st, F(L.p_mxw), T[ENF_W_MX_W1], T[ENF_W_MX_G], D, D);
  if ((rc = mm(st, F(L.p_mxb), D, T[ENF_W_MX_BE], D, T[ENF_W_MX_W1], D, 1, D, D, 1.f, T[ENF_W_MX_B1], 0))) return rc;
  if ((rc = mm(st, F(L.p_tmp), HD, T[ENF_W_AO_W], HD, T[ENF_W_FF_W0], HD, HD, HD, HD, 1.f, nullptr, 0))) return rc;
  if ((rc = mm(st, F(L.bB), HD, T[ENF_W_AO_B], HD, T[ENF_W_FF_W0], HD, 1, HD, HD, 1.f, T[ENF_W_FF_B0], 0))) return rc;
  for (int h = 0; h < H; ++h) {
    if ((rc = mm(st, F(L.p_wb) + (size_t)h * D * HD, HD, F(L.p_mxw), D, F(L.p_tmp) + (size_t)h * D * HD, HD, D, HD, D, 1.f, nullptr, 0))) return rc;
    if ((rc = mm(st, F(L.bB), HD, F(L.p_mxb), D, F(L.p_tmp) + (size_t)h * D * HD, HD, 1, HD, D, 1.f, nullptr, 1))) return rc;
  }
  hipLaunchKernelGGL(rowscale_kernel, dim3((HD + 127) / 128, HD), dim3(128), 0, st, F(L.p_wf1), T[ENF_W_FF_W1], T[ENF_W_FF_G], HD, HD);
  if ((rc = mm(st, F(L.bF1), HD, T[ENF_W_FF_BE], HD, T[ENF_W_FF_W1], HD, 1, HD, HD, 1.f, T[ENF_W_FF_B1], 0))) return rc;
  CK(cp(L.bO0, T[ENF_W_O0_B], D)); CK(cp(L.bO2, T[ENF_W_O2_B], D));
  hipLaunchKernelGGL(padcopy_kernel, dim3((OP + 127) / 128, 1), dim3(128), 0, st, F(L.bO4), T[ENF_W_O4_B], 1, O, OP);
  hipLaunchKernelGGL(padcopy_kernel, dim3((OP + 127) / 128, D), dim3(128), 0, st, F(L.p_o4), T[ENF_W_O4_W], D, O, OP);
  if (hipGetLastError() != hipSuccess) return ENF_ELAUNCH;
  // ---- panels
  const int bf = m.bf16;
  if ((rc = pack_pair_panels(st, blob, L, m, T[ENF_W_RQ_W1], T[ENF_W_RV_W1], F(L.p_af), F(L.p_agb), T[ENF_W_MX_W0],
                             T[ENF_W_RQ_COEF], T[ENF_W_RV_COEF]))) return rc;
  // tail, forward: A[out][in] = W[in][out]; backward: A[in][out] = W[in][out]  (dX = W dY)
  if ((rc = pack_panel(st, blob, L.atb, F(L.p_wb), HD, HD, HD, 0, bf))) return rc;
  if ((rc = pack_panel(st, blob, L.atf1, F(L.p_wf1), HD, HD, HD, 0, bf))) return rc;
  if ((rc = pack_panel(st, blob, L.ato0, T[ENF_W_O0_W], D, D, HD, 0, bf))) return rc;
  if ((rc = pack_panel(st, blob, L.ato2, T[ENF_W_O2_W], D, D, D, 0, bf))) return rc;
  if ((rc = pack_panel(st, blob, L.ato4, F(L.p_o4), OP, OP, D, 0, bf))) return rc;
  if ((rc = pack_panel(st, blob, L.gtb, F(L.p_wb), HD, HD, HD, 1, bf))) return rc;
  if ((rc = pack_panel(st, blob, L.gtf1, F(L.p_wf1), HD, HD, HD, 1, bf))) return rc;
  if ((rc = pack_panel(st, blob, L.gto0, T[ENF_W_O0_W], D, HD, D, 1, bf))) return rc;
  if ((rc = pack_panel(st, blob, L.gto2, T[ENF_W_O2_W], D, D, D, 1, bf))) return rc;
  if ((rc = pack_panel(st, blob, L.gto4, F(L.p_o4), OP, D, OP, 1, bf))) return rc;
  return ENF_OK;
}
