// enf_launch.h -- everything host-side that one .hip file of the library uses from another: the kernel launchers, the call
// context of the C-ABI entry points and the shared launch helpers (with enf_layout.h).  Every .hip file includes it, the file
// that defines a function too, and the functions have C++ linkage: a definition that drifts from its declaration here is a
// link error.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include "enf_layout.h"

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) holds per DEVICE and per kernel: every kernel (the template argument: one
// instantiation of this function, so one `done` each, with no index to compute) keeps one bit per device ordinal of the calling
// thread's current device (ordinals beyond 63 set the attribute on every launch).  Safe from concurrent host threads:
// setting the attribute twice is harmless, the bit is set only after it succeeded.
template <auto Kern> inline bool enf_lds_attr(int bytes) {
  static std::atomic<unsigned long long> done{0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  if (dev >= 0 && dev < 64 && ((done.load(std::memory_order_acquire) >> dev) & 1ull)) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
  if (dev >= 0 && dev < 64) done.fetch_or(1ull << dev, std::memory_order_release);
  return true;
}

// ---- deterministic mode (ENF_BWD_DETERMINISTIC / ENF_FIT_DETERMINISTIC): K3 and the loss kernels store their partial sums in
// scratch and a fixed-order pass adds them; no result depends on the order in which workgroups finish.
// K3's query split (grid.y): one workgroup per CU is resident (LDS), so the query tiles are split until all 256 CUs have one.
// `zfold` = the launch runs the z-fold form (one workgroup per latent; otherwise one wave per latent, 8 per workgroup).
inline int enf_pair_bwd_nsplit(const EnfDims& m, bool zfold) {
  const long long wgs = zfold ? (long long)m.B * m.Z : ((long long)m.B * m.Z + 7) / 8;
  const int ntiles = (m.N + 15) / 16;
  int ns = 1;
  while (wgs * ns < 256 && ns * 2 <= ntiles) ns *= 2;
  return ns;
}
// the shared-latent backward's query split (grid.y; grid.x = the Z latents of signal 0): where Z ceil(N / 128) workgroups fit one round
// of 256 CUs every wave gets at most one tile, so the launch is one tile step deep; larger shapes follow the sweep above on Z latents
inline int enf_pair_bwd_shared_nsplit(const EnfDims& m) {
  const int ntiles = (m.N + 15) / 16;
  if ((long long)m.Z * ((m.N + 127) / 128) <= 256) return (ntiles + 7) / 8;
  EnfDims m1 = m;
  m1.B = 1;
  return enf_pair_bwd_nsplit(m1, true);
}
// K3's partial rows of d lt, [nsplit][B Z][lt stride] floats, and its per-latent shares of the query gradient, (B, Z, N, dx)
inline size_t enf_det_part_bytes(const EnfDims& m, bool zfold) {
  return enf_align(sizeof(float) * (size_t)enf_pair_bwd_nsplit(m, zfold) * m.B * m.Z * enf_lt_stride(m.H, m.D));
}
inline size_t enf_det_dx_bytes(const EnfDims& m) { return enf_align(sizeof(float) * (size_t)m.B * m.Z * m.N * m.dx); }
// the fused tail's loss partials: one per wave (enf_tail.hip)
int enf_tail_loss_parts(const EnfDims& m);
// *loss += part[0] + ... + part[n - 1], one workgroup, fixed order (enf_loss.hip)
int enf_launch_loss_sum(const float* part, int n, float* loss, hipStream_t st);
// out[e] (+)= part[0][e] + ... + part[nwg - 1][e], e < n: the fixed-order sum of per-workgroup partials (enf_ode.hip)
void enf_launch_sum_partials(const float* part, int nwg, int n, float* out, int accumulate, hipStream_t st);
struct EnfDetWorkspace { size_t part, loss, total; };      // byte offsets in the workspace, behind EnfWorkspace::total
inline EnfDetWorkspace enf_det_workspace(const EnfDims& m, const EnfWorkspace& W) {
  EnfDetWorkspace X;
  X.part = W.total;
  X.loss = X.part + enf_det_part_bytes(m, enf_use_zfold_bwd(m) && enf_pair_bwd_zfold_fits(m));
  X.total = X.loss + enf_align(sizeof(float) * (size_t)enf_tail_loss_parts(m));
  return X;
}

// ---- the scratch of the z-fold pair kernels as their launchers take it (regions of EnfWorkspace, or enf_pair_forward's own)
// forward: all NULL for the latent-split variant; ysplit: the partial sums of ENF_VARIANT_ZFOLD_ZSPLIT, or NULL
struct EnfFoldFwd { char* wz; float* wzb; char* wzu; float* ysplit; };
// backward: the [forward | backward] panel pairs and the bias vectors; NULL: the latent-split form
struct EnfFoldBwd { const char* wzt; const float* wzb; };

// ---- what the entry points that run on a workspace (enf_forward_stages, enf_backward_latents_ex, enf_fit_step,
// enf_backward_all) derive from their arguments
struct EnfCall {
  EnfDims m;
  EnfLayout L;
  EnfWorkspace W;
  EnfDetWorkspace X;    // what a deterministic call carves behind W.total (enf_workspace_bytes_ex)
  hipStream_t st;
  char* ws;             // the workspace (also the key of its pending side-stream work)
  const char* blob;     // the packed weights
  float* F(size_t off) const { return reinterpret_cast<float*>(ws + off); }
  // the workspace's scratch of the z-fold pair kernels, where the shape resolves to them (all NULL otherwise)
  EnfFoldFwd fold_fwd() const {
    const bool zf = enf_use_zfold(m);
    return {zf ? ws + W.wz : nullptr, zf ? F(W.wzb) : nullptr, zf ? ws + W.wzu : nullptr, enf_zfold_split(m) > 1 ? F(W.ysplit) : nullptr};
  }
  EnfFoldBwd fold_bwd() const {
    const bool zb = enf_use_zfold_bwd(m);
    return {zb ? ws + W.wzt : nullptr, zb ? F(W.wzb) : nullptr};
  }
};
// Errors in their order of precedence: the descriptor's (enf_check_desc), ENF_EINVAL for a NULL pointer (`pointers_ok` is the
// entry point's own set; `packed` and `workspace` are everybody's) or for a window without `sigma`, ENF_EWORKSPACE.
inline int enf_call(EnfCall& c, const EnfDesc* d, bool pointers_ok, const float* sigma, const void* packed, void* workspace,
                    size_t workspace_bytes, void* stream, bool deterministic = false) {
  const int rc = enf_check_desc(d);
  if (rc) return rc;
  if (!pointers_ok || !packed || !workspace) return ENF_EINVAL;
  if (d->use_window && !sigma) return ENF_EINVAL;
  c.m = enf_dims(d);
  c.L = enf_layout(c.m);
  c.W = enf_workspace(c.m);
  c.X = enf_det_workspace(c.m, c.W);
  if (workspace_bytes < (deterministic ? c.X.total : c.W.total)) return ENF_EWORKSPACE;
  c.st = (hipStream_t)stream;
  c.ws = (char*)workspace;
  c.blob = (const char*)packed;
  return ENF_OK;
}

// join the side-stream work an earlier ENF_STAGE_PREPARE_BWD left pending on THIS workspace (no matching backward
// came) before `st` touches the regions it writes (enf_api.hip)
int enf_side_join_pending(hipStream_t st, const void* workspace);

// ---- K1, the latent prologue (enf_prologue.hip): p, a, sigma -> the latent table `lt` and what its backward reads (`an`, `kv`)
int enf_launch_prologue(const EnfDims& m, const EnfLayout& L, const char* blob, const float* p, const float* a, const float* sigma,
                        float* lt, float* an, float* kv, hipStream_t st);
// d lt -> d p, d a, d sigma; _wg: with pg != NULL also the operand rows of the prologue's weight gradients (enf_train.hip)
int enf_launch_prologue_bwd(const EnfDims& m, const EnfLayout& L, const char* blob, const float* p, const float* sigma,
                            const float* an, const float* kv, const float* dlt, float* dp, float* da, float* dsigma, hipStream_t st);
int enf_launch_prologue_bwd_wg(const EnfDims& m, const EnfLayout& L, const char* blob, const float* p, const float* sigma,
                               const float* an, const float* kv, const float* dlt, float* dp, float* da, float* dsigma, float* pg,
                               hipStream_t st);

// ---- the per-latent folded matrices of the z-fold pair kernels (enf_wz.hip)
// wzt == NULL: forward panels only, packed back to back in `wz`, and the logit rows `wzu` (the z-fold forward kernel's layout);
// wzt != NULL: `wzt` holds [forward | backward] panel pairs per (latent, head), `wz` is ignored.  `wzb`: the bias vectors.
int enf_launch_wz(const EnfDims& m, const EnfLayout& L, const char* blob, const float* lt, char* wz, float* wzb, char* wzu,
                  char* wzt, hipStream_t st);

// ---- K2, the forward pair kernel (enf_pair_fwd.hip).  zs: the scratch of the z-fold variant.  flags:
//   ENF_PAIR_FOLD       the z-fold variant first builds its per-latent matrices (enf_launch_wz)
//   ENF_PAIR_PAIR       run the pair stage (without it the call is the fold alone)
//   ENF_PAIR_YBAR_HALF  hand ybar to the tail as bf16 (the caller passes the same decision to the tail's ENF_TAIL_YBAR_HALF; with relu
//                       masks on a call that runs the masked kernels: ENF_EINVAL)
//   spart      != NULL: the caller vouches that all B signals hold the same latent rows and query points (x_bstride == 0) and lends
//              B N (HD + H) floats: where the call runs the latent-split kernel without relu masks and without the bf16 hand-off, and
//              B > 1, it computes signal 0 alone, its latents in enf_shared_fwd_parts(m) parts (enf_layout.h), and a merge kernel
//              writes every signal's rows of ybar / lse; elsewhere the argument is ignored
enum EnfPairFwdFlags : unsigned { ENF_PAIR_FOLD = 1u, ENF_PAIR_PAIR = 2u, ENF_PAIR_YBAR_HALF = 4u };
int enf_launch_pair_fwd(const EnfDims& m, const EnfLayout& L, const char* blob, const float* x, long long x_bstride, const float* lt,
                        float* ybar, float* lse, const EnfFoldFwd& zs, unsigned flags, hipStream_t st, float* spart = nullptr);

// ---- K3, the backward pair kernel (enf_pair_bwd.hip): ADDS to `dlt`.  store != NULL: the activation-store form (the K4 operands
// of ENF_NUM_STORE(H) buffers); otherwise zs.wzt / zs.wzb != NULL selects the z-fold form.  dxq: d x per query (added to), or NULL.
// part != NULL: deterministic mode -- the kernel stores its partial rows in `part` (enf_det_part_bytes) and, with dxq, its
// per-latent query-gradient shares in `dxpart` (enf_det_dx_bytes); two reduction kernels then OVERWRITE `dlt` (splits in
// order) and `dxq` (latents in order): no float atomic runs, `dlt` need not be zeroed.
int enf_launch_pair_bwd(const EnfDims& m, const EnfLayout& L, const char* blob, const float* x, long long x_bstride, const float* lt,
                        const float* lse, const float* dybar, const float* delta, float* dlt, void* const* store, const EnfFoldBwd& zs,
                        float* dxq, hipStream_t st, float* part = nullptr, float* dxpart = nullptr);

// the shared-latent backward (enf_layout.h: enf_shared_backward_rule): signal 0's pairs once, on the unit-seeded dybar / delta, contracted
// with dout (B, N) into all B Z rows of `dlt` (ADDS); ENF_EUNSUPPORTED where there is no such instantiation
int enf_launch_pair_bwd_shared(const EnfDims& m, const EnfLayout& L, const char* blob, const float* x, const float* lt, const float* lse,
                               const float* dybar, const float* delta, const float* dout, float* dlt, const EnfFoldBwd& zs,
                               hipStream_t st);

// ---- K4, X^T delta over the activation store (enf_xtd.hip)
size_t enf_xtd_part_bytes(const EnfDims& m, long long P);       // slice partials of a pass over P rows (256-aligned)
// store: the ENF_NUM_STORE(H) device buffers K3 wrote for P rows; dpair: ENF_NUM_PAIR_TENSORS fp32 device pointers in
// ENF_P_* order (the two coefficient entries are not touched); accumulate = add to what dpair holds (later chunks)
int enf_launch_xtd(const EnfDims& m, void* const* store, long long P, float* const* dpair, float* part, int accumulate,
                   hipStream_t st);

// The weight-gradient pass of the per-pair chain, chunked over signals: zero `dlt`, then per chunk of `cb` signals K3 with
// the activation store and K4.  `scratch` holds enf_wgrad_scratch_bytes(m, cb); x .. dx are the whole batch's (dx may be NULL).
// part / dxpart: deterministic mode as in enf_launch_pair_bwd, sized for the chunks (enf_wgrad_det_part_bytes, cb signals' dx shares).
size_t enf_wgrad_scratch_bytes(const EnfDims& m, int cb);
size_t enf_wgrad_det_part_bytes(const EnfDims& m, int cb);
int enf_launch_wgrad_chunks(const EnfDims& m, const EnfLayout& L, const char* blob, int cb, const float* x, long long x_bstride,
                            const float* lt, const float* lse, const float* dybar, const float* delta, float* dlt, float* dx,
                            char* scratch, float* const* dpair, hipStream_t st, float* part = nullptr, float* dxpart = nullptr);
// the largest chunk of signals whose scratch, bytes(cb), fits in `avail` (0: none does); with relu masks, whole groups of
// mask_signals (signal b replays b % mask_signals)
template <class Bytes>
inline int enf_wgrad_chunk(const EnfDims& m, size_t avail, Bytes bytes) {
  const int step = m.mask_mode == ENF_MASK_READ && m.mask_B < m.B ? m.mask_B : 1;
  int cb = m.B;
  while (cb > step && bytes(cb) > avail) cb = (cb - 1) / step * step;
  return cb >= 1 && bytes(cb) <= avail ? cb : 0;
}

// ---- the per-query tail (enf_tail.hip)
//   ENF_TAIL_BWD        backward (dout -> dybar, delta); without it forward (ybar -> out)
//   ENF_TAIL_STASH      forward: stash the pre-activations in `act`; backward: `act` holds them, skip the recompute
//   ENF_TAIL_YBAR_HALF  forward only: ybar is bf16 (the pair kernel's ENF_PAIR_YBAR_HALF)
// _wg: tdel != NULL (backward only) is the weight-gradient form -- it also leaves every layer's input (in `act`, in place of
// the pre-activations) and delta (in `tdel`) for the X^T delta products of enf_train.hip
enum EnfTailFlags : unsigned { ENF_TAIL_FWD = 0u, ENF_TAIL_BWD = 1u, ENF_TAIL_STASH = 2u, ENF_TAIL_YBAR_HALF = 4u };
int enf_launch_tail(const EnfDims& m, const EnfLayout& L, const char* blob, const float* ybar, float* out, const float* dout,
                    float* dybar, float* delta, float* act, unsigned flags, hipStream_t st);
int enf_launch_tail_wg(const EnfDims& m, const EnfLayout& L, const char* blob, const float* ybar, float* out, const float* dout,
                       float* dybar, float* delta, float* act, float* tdel, unsigned flags, hipStream_t st);
// the seeded tail backward (enf_field_grad): d out = the unit vector of output channel `seed` (0 <= seed < O), formed in registers --
// no d out in memory; `act` holds the pre-activations a forward with ENF_TAIL_STASH stashed; writes d ybar and delta
int enf_launch_tail_seed(const EnfDims& m, const EnfLayout& L, const char* blob, const float* ybar, int seed, float* dybar, float* delta,
                         float* act, hipStream_t st);
// forward chain with the stash (and `out`, if given) and the seeded backward in ONE launch (the shared-latent fit step): the results of
// enf_launch_tail(.., ENF_TAIL_STASH) followed by enf_launch_tail_seed, bit for bit
int enf_launch_tail_fwd_seed(const EnfDims& m, const EnfLayout& L, const char* blob, const float* ybar, float* out, int seed, float* dybar,
                             float* delta, float* act, hipStream_t st);
// the inner step's tail as one kernel: forward chain -> mean squared error against `target` (added to *loss) and its gradient ->
// backward chain -> d ybar, delta
// weight: NULL, or one loss weight per query (B N floats, include/enf_hip.h "Weighted loss"); per_value: `weight` (not NULL) holds one
// weight per output value instead, B N O floats (enf_fit_step_cw) -- a kernel instantiation of its own
// loss_part != NULL (enf_tail_loss_parts(m) floats): every wave stores its partial there and enf_launch_loss_sum adds them to *loss
// err != NULL (B N floats): the same kernels also store every query's weighted squared error, err[b,n] = sum_o w (out - target)^2
// (include/enf_hip.h, "Per-signal and per-point errors"); the loss, the partials and d out keep their arithmetic
int enf_launch_tail_loss(const EnfDims& m, const EnfLayout& L, const char* blob, const float* ybar, const float* target,
                         const float* weight, float gscale, float* loss, float* dybar, float* delta, float* act, hipStream_t st,
                         float* loss_part = nullptr, bool per_value = false, float* err = nullptr);
// the evaluation tail: the forward chain whose epilogue forms err (B N floats, or NULL) and, with loss != NULL, adds the scalar loss to
// *loss (through loss_part in deterministic mode) instead of storing `out`; weight / per_value as above.  ybar is fp32.
int enf_launch_tail_eval(const EnfDims& m, const EnfLayout& L, const char* blob, const float* ybar, const float* target,
                         const float* weight, bool per_value, float* loss, float* err, hipStream_t st, float* loss_part = nullptr);
// grouped observations (include/enf_hip.h, "Grouped observations"): observation m of a signal is the q-weighted sum of the decode at
// queries m G .. m G + G - 1.  qweight (B, N) or NULL (1 / G); oweight (B, N / G) or NULL (1); err_g (B, N / G) or NULL.
// cweight (B, N / G, O) or NULL: one weight per observed VALUE in place of oweight (the _gc calls) -- the tail's per-value grouped forms.
struct EnfGroupObs { int G; const float* qweight; const float* oweight; float* err_g; const float* cweight = nullptr; };
inline bool enf_group_size_ok(int G) { return G == 1 || G == 2 || G == 4 || G == 8 || G == 16; }
// the fused-loss tail (dybar != NULL: arguments as enf_launch_tail_loss) or the evaluation tail (dybar, delta, act NULL: as
// enf_launch_tail_eval) against target (B, N / G, O); ENF_EINVAL for a G outside the set or N % G != 0
int enf_launch_tail_group(const EnfDims& m, const EnfLayout& L, const char* blob, const float* ybar, const float* target, const EnfGroupObs& g,
                          float gscale, float* loss, float* dybar, float* delta, float* act, hipStream_t st, float* loss_part = nullptr);
// the shared-latent backward's loss (enf_loss.hip): ONE row out1 (N values, O = 1) against all B signals' targets and weights (B, N;
// weight may be NULL): *loss += the mean squared error, dout (B, N) = its gradient times gscale -- enf_mse_kernel's arithmetic
int enf_launch_mse_shared(const float* out1, const float* target, const float* weight, int B, int N, float gscale, float* dout,
                          float* loss, hipStream_t st);
// its grouped form (enf_fit_step_gs): the one row against all B signals' observations target (B, N / G) and weights oweight (B, N / G) or
// NULL, with signal 0's factors q0 (N) or NULL (1 / G); dout (B, N) -- enf_mse_group_kernel's arithmetic
int enf_launch_mse_group_shared(const float* out1, const float* target, const float* q0, const float* oweight, int B, int N, int G,
                                float gscale, float* dout, float* loss, hipStream_t st);
// loss_b[b] = scale * (err[b, 0] + ... + err[b, N - 1]): one workgroup per signal, fixed order, no atomics (enf_loss.hip)
int enf_launch_signal_sum(const float* err, int B, int N, float scale, float* loss_b, hipStream_t st);

// ---- sparse linear observations (include/enf_hip.h, "Sparse linear observations"; enf_obs.hip)
enum { ENF_OBS_TREE_MIN = 65,        // rows of at least this many entries are summed by their whole wave (lane-strided partials, xor tree)
       ENF_OBS_MAX_BLOCKS = 1024 };  // the grid's cap = the loss partials of a deterministic call
// what every entry point checks of an operator (M >= 1, 0 <= nnz < 2^31, the CSR's pointers; transposed: the CSC's too)
bool enf_obs_op_ok(const EnfSparseObs* op, bool transposed);
// kernel 1, the forward product with the loss on out (B, N, O): r = w (obs - target) (B, M, O) and err_a (B, M), each NULL or stored;
// loss NULL or *loss += the loss -- with part != NULL (ENF_OBS_MAX_BLOCKS floats) through it and enf_launch_loss_sum
int enf_launch_obs_loss(const EnfSparseObs& op, int N, int B, int O, const float* out, const float* target, const float* oweight,
                        const float* cweight, float* r, float* err_a, float* loss, float* part, hipStream_t st);
// kernel 1 with weights and no target (enf_gn_product_a): r (B, M, O) = (w > 0 ? w (A x) : 0) of x (B, N, O), every element written;
// oweight (B, M), cweight (B, M, O), or neither (1); no loss, no atomic
int enf_launch_obs_weigh(const EnfSparseObs& op, int N, int B, int O, const float* x, const float* oweight, const float* cweight, float* r,
                         hipStream_t st);
// kernel 2, the transposed product: dout (B, N, O) = gs * A^T r, every element written
int enf_launch_obs_transpose(const EnfSparseObs& op, int N, int B, int O, const float* r, float gs, float* dout, hipStream_t st);
// the regions enf_fit_step_a / enf_eval_loss_a carve behind the plain or deterministic workspace (`base` = its total), byte offsets
struct EnfObsWorkspace { size_t out, dout, r, err, loss, total; };
inline EnfObsWorkspace enf_obs_workspace(const EnfDims& m, size_t base, int M) {
  EnfObsWorkspace Y;
  const size_t bno = enf_align(sizeof(float) * (size_t)m.B * m.N * m.O), bm = (size_t)m.B * (size_t)M;
  Y.out = base;
  Y.dout = Y.out + bno;
  Y.r = Y.dout + bno;
  Y.err = Y.r + enf_align(sizeof(float) * bm * m.O);
  Y.loss = Y.err + enf_align(sizeof(float) * bm);
  Y.total = Y.loss + enf_align(sizeof(float) * ENF_OBS_MAX_BLOCKS);
  return Y;
}

// ---- what the loss of a host sequence is: fit_step_sequence and eval_loss_sequence (enf_api.hip), gn_product_sequence
// (enf_tangent.hip).  An entry point fills one and calls its sequence; which forms exist and what each refuses is check()'s.
enum EnfLossKind { ENF_LOSS_POINTS,      // every query is an observation (include/enf_hip.h, "Weighted loss")
                   ENF_LOSS_GROUPS,      // observation m is the q-weighted sum of G consecutive queries ("Grouped observations")
                   ENF_LOSS_OPERATOR };  // obs = A out of a CSR operator, the tail unfused ("Sparse linear observations")
enum EnfLossCall { ENF_LOSS_FIT, ENF_LOSS_EVAL, ENF_LOSS_GN };
struct EnfLossSpec {
  EnfLossKind kind = ENF_LOSS_POINTS;
  const float* weight = nullptr;      // one weight per observation, (B, rows), or NULL (1)
  const float* cweight = nullptr;     // one per observed VALUE in its place, (B, rows, O); never both
  float* err = nullptr;               // the per-observation errors (B, rows), or NULL
  float* loss_b = nullptr;            // the per-signal losses (B), or NULL
  int G = 1;                          // groups: the group size and the factors (B, N) or NULL (1 / G)
  const float* qweight = nullptr;
  const EnfSparseObs* op = nullptr;   // operator
  // what differs between the entry points of one kind
  bool need_cweight = false;          // the per-value calls (_cw, _gc): cweight is required
  bool need_err = false;              // enf_fit_step_e: err is required
  bool shared_entry = false;          // groups: the call that may carry ENF_FIT_SHARED_LATENTS (enf_fit_step_gs)
  // the values a signal's loss is the mean of: its points, or its observations
  int rows(const EnfDims& m) const { return kind == ENF_LOSS_OPERATOR ? op->M : kind == ENF_LOSS_GROUPS ? m.N / G : m.N; }
  // the grouped tail's argument, the errors going to `e`
  EnfGroupObs group(float* e) const { return {G, qweight, weight, e, cweight}; }
  // ENF_OK, or what the call answers BEHIND the descriptor's errors and before any launch: ENF_EINVAL, or ENF_EUNSUPPORTED for the
  // per-value grouped fit with ENF_FIT_SHARED_LATENTS (the shared loss kernel has no per-value form), which the sequence answers
  // ahead of its own ENF_EINVAL.  The flag is the fit's alone: on points a permission, on groups _gs's (the shared backward's loss
  // is another kernel), on an operator refused.
  int check(const EnfDesc* d, unsigned flags, EnfLossCall call) const {
    const bool shared = call == ENF_LOSS_FIT && (flags & ENF_FIT_SHARED_LATENTS);
    if (shared && kind == ENF_LOSS_GROUPS && need_cweight) return ENF_EUNSUPPORTED;
    if (shared && (kind == ENF_LOSS_OPERATOR || (kind == ENF_LOSS_GROUPS && !shared_entry))) return ENF_EINVAL;
    if ((weight && cweight) || (need_cweight && !cweight) || (need_err && !err)) return ENF_EINVAL;
    if (kind == ENF_LOSS_GROUPS && !(enf_group_size_ok(G) && d && d->N % G == 0)) return ENF_EINVAL;
    // (the grouped fit has no region of its workspace free for the errors)
    if (kind == ENF_LOSS_GROUPS && call == ENF_LOSS_FIT && loss_b && !err) return ENF_EINVAL;
    // an operator that enf_obs_op_ok refuses (the fit and the product read the CSC too)
    if (kind == ENF_LOSS_OPERATOR && !enf_obs_op_ok(op, call != ENF_LOSS_EVAL)) return ENF_EINVAL;
    return ENF_OK;
  }
};
