// enf_api.hip -- the C-ABI of include/enf_hip.h: validation, workspace carving, kernel sequencing.
// No device allocation, no host synchronisation, no settings: a call depends on its arguments only.  The host-side
// bookkeeping that exists -- one side stream per device and the pending side-stream work per (device, workspace) -- is
// keyed by what the caller passes, so calls on different workspaces / streams / devices / threads do not interact.
#include <hip/hip_runtime.h>
#include <mutex>
#include <unordered_map>
#include "enf_launch.h"

extern "C" int enf_abi_version(void) { return ENF_ABI_VERSION; }

extern "C" const char* enf_strerror(int code) {
  switch (code) {
    case ENF_OK: return "ok";
    case ENF_EINVAL: return "invalid argument (null pointer or non-positive size)";
    case ENF_EINVARIANT: return "Unknown invariant type";
    case ENF_EUNSUPPORTED: return "shape not in the compiled kernel set (num_hidden 64 or 128 after padding; num_heads 1, 2, or 4 at num_hidden 64; "
                                  "num_out <= 32; ball / ball_lat at num_hidden 64 only)";
    case ENF_EWORKSPACE: return "workspace too small";
    case ENF_ELAUNCH: return "HIP launch failed";
    case ENF_EDIM: return "coordinate / pose width inconsistent with the invariant";
    default: return "unknown error";
  }
}

extern "C" int enf_invariant_dim(int inv, int dx) {
  const int i = enf_inv_dim(inv, dx);
  return i < 0 ? ENF_EINVARIANT : i;
}
extern "C" int enf_invariant_pose_dim(int inv, int dx) {
  const int i = enf_inv_pose_dim(inv, dx);
  return i < 0 ? ENF_EINVARIANT : i;
}

extern "C" int enf_check_desc(const EnfDesc* d) {
  if (!d) return ENF_EINVAL;
  if (d->B <= 0 || d->N <= 0 || d->Z <= 0 || d->C <= 0 || d->O <= 0 || d->H <= 0 || d->D <= 0) return ENF_EINVAL;
  if (d->invariant_id < 0 || d->invariant_id >= ENF_INV_COUNT) return ENF_EINVARIANT;
  if (d->dx < 1 || d->dx > 3) return ENF_EDIM;
  const bool two_d = d->invariant_id == ENF_INV_REL_POS_PERIODIC || d->invariant_id == ENF_INV_PONITA ||
                     d->invariant_id == ENF_INV_LATITUDE_PERIODIC || d->invariant_id == ENF_INV_POLAR_PERIODIC;
  if (two_d && d->dx != 2) return ENF_EDIM;     // reference: assert cfg.num_in == 2 (invariant/__init__.py:62,65)
  if (d->invariant_id == ENF_INV_PONITA_FULL && d->dx != 3) return ENF_EDIM;   // queries (pos_x, pos_y, theta)
  if (enf_inv_has_phase(d->invariant_id) && d->D != 64) return ENF_EUNSUPPORTED;   // (the 128-wide backward kernel has no LDS left)
  if (enf_inv_has_phase(d->invariant_id) && d->dx != 3) return ENF_EDIM;   // ball, ball_lat: (phi, theta, r) coordinates
  if (!enf_width_compiled(d->D)) return ENF_EUNSUPPORTED;
  if (d->d_true < 0 || d->d_true > d->D || (d->d_true & 1)) return ENF_EINVAL;
  if (!enf_shape_compiled(d->D, d->H)) return ENF_EUNSUPPORTED;   // enf_layout.h: ENF_SHAPES (4 heads: 64-wide kernels only)
  if (d->h_true < 0 || d->h_true > d->H) return ENF_EINVAL;
  if (d->O > 32) return ENF_EUNSUPPORTED;
  if (d->precision != ENF_PREC_F32 && d->precision != ENF_PREC_BF16) return ENF_EINVAL;
  if (d->pair_fwd_variant < ENF_VARIANT_AUTO || d->pair_fwd_variant > ENF_VARIANT_ZFOLD_ZSPLIT) return ENF_EINVAL;
  if (d->pair_bwd_variant < ENF_VARIANT_AUTO || d->pair_bwd_variant > ENF_VARIANT_ZFOLD) return ENF_EINVAL;
  if (d->mask_mode < ENF_MASK_OFF || d->mask_mode > ENF_MASK_READ || d->mask_signals < 0) return ENF_EINVAL;
  if (d->mask_mode != ENF_MASK_OFF && !d->relu_masks) return ENF_EINVAL;
  if (d->embedding != ENF_EMB_RFF && d->embedding != ENF_EMB_FFN) return ENF_EINVAL;
  if (d->embedding == ENF_EMB_FFN && enf_inv_has_phase(d->invariant_id)) return ENF_EUNSUPPORTED;
  return ENF_OK;
}

extern "C" size_t enf_packed_weight_bytes(const EnfDesc* d) {
  if (enf_check_desc(d) != ENF_OK) return 0;
  return enf_layout(enf_dims(d)).total;
}

extern "C" size_t enf_workspace_bytes(const EnfDesc* d) {
  if (enf_check_desc(d) != ENF_OK) return 0;
  return enf_workspace(enf_dims(d)).total;
}

// the workspace of a call with these flags: ENF_BWD_DETERMINISTIC (= ENF_FIT_DETERMINISTIC) adds K3's partial rows and the fused
// tail's loss partials behind the plain workspace (enf_launch.h: enf_det_workspace); ENF_FIT_SHARED_LATENTS adds nothing (its parts
// borrow the d ybar | delta region)
extern "C" size_t enf_workspace_bytes_ex(const EnfDesc* d, unsigned flags) {
  if (enf_check_desc(d) != ENF_OK || (flags & ~(ENF_BWD_DETERMINISTIC | ENF_BWD_QUERY_GRAD | ENF_FIT_SHARED_LATENTS))) return 0;
  const EnfDims m = enf_dims(d);
  const EnfWorkspace W = enf_workspace(m);
  return (flags & ENF_BWD_DETERMINISTIC) ? enf_det_workspace(m, W).total : W.total;
}

// Side streams.  Work that can overlap the caller's stream (the z-fold backward's per-latent matrices) runs on ONE side
// stream per device, created at the first call that needs it on that device.  Fork / join is by events, so the caller's stream order is preserved.  What a forward leaves pending for
// its backward (ENF_STAGE_PREPARE_BWD) is recorded against the WORKSPACE it was prepared in, with an event of its own:
// only a call on that workspace sees it.  One mutex per device keeps host threads from interleaving their record / wait
// pairs on the shared fork event.
struct SidePending { hipEvent_t join = nullptr; bool pending = false; };
struct SideStream {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr;
  std::mutex mu;
  std::unordered_map<const void*, SidePending> ws;     // by workspace base address
  // the entry of a workspace (created on demand; entries without pending work are recycled beyond 64 workspaces)
  SidePending* entry(const void* workspace) {
    auto it = ws.find(workspace);
    if (it != ws.end()) return &it->second;
    if (ws.size() >= 64)
      for (auto j = ws.begin(); j != ws.end();) {
        if (!j->second.pending) { (void)hipEventDestroy(j->second.join); j = ws.erase(j); } else ++j;
      }
    SidePending e;
    if (hipEventCreateWithFlags(&e.join, hipEventDisableTiming) != hipSuccess) return nullptr;
    return &ws.emplace(workspace, e).first->second;
  }
};
static constexpr int ENF_MAX_DEVICES = 64;
static SideStream* side_stream() {      // of the calling thread's current device, or nullptr
  static std::mutex table_mu;
  static SideStream* table[ENF_MAX_DEVICES] = {};
  static bool tried[ENF_MAX_DEVICES] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= ENF_MAX_DEVICES) return nullptr;
  std::lock_guard<std::mutex> lk(table_mu);
  if (!tried[dev]) {
    tried[dev] = true;
    SideStream* t = new SideStream();
    if (hipStreamCreateWithFlags(&t->s, hipStreamNonBlocking) == hipSuccess &&
        hipEventCreateWithFlags(&t->fork, hipEventDisableTiming) == hipSuccess)
      table[dev] = t;
    else
      delete t;
  }
  return table[dev];
}

int enf_side_join_pending(hipStream_t st, const void* workspace) {
  SideStream* side = side_stream();
  if (!side) return 0;
  std::lock_guard<std::mutex> lk(side->mu);
  auto it = side->ws.find(workspace);
  if (it != side->ws.end() && it->second.pending) {
    if (hipStreamWaitEvent(st, it->second.join, 0) != hipSuccess) return ENF_ELAUNCH;
    it->second.pending = false;
  }
  return 0;
}

// What the z-fold backward pair kernel needs from the latent table alone -- its per-latent folded matrices (enf_wz_kernel, both
// orientations) and, with `zero_dlt`, the zeroed gradient table -- on the side stream behind what `c.st` holds now: fork, the
// work, the workspace's join event, pending until enf_side_join_pending.  Returns 1 if it forked, 0 (and nothing has been done)
// where there is no side stream (`side` NULL) or no entry for the workspace, or an error (< 0): one after the fork returns at
// once, the entry is pending only once the join event is recorded.  The three callers differ, on purpose:
//   ENF_STAGE_PREPARE_BWD     z-fold backward only; zeroes on the side stream; not forked: nothing at all (the backward prepares
//                             for itself later)
//   enf_backward_latents_ex   z-fold backward only; does NOT zero here (its memset follows the tail backward on the caller's
//                             stream); not forked: enf_launch_wz on the caller's stream
//   enf_fit_step              zeroes on the side stream; not forked (or not the z-fold backward): enf_launch_wz (z-fold only) and
//                             the memset on the caller's stream; with the shared-latent backward (wz_signals = 1) the matrices
//                             of signal 0's Z latents only -- the zero-fill stays whole
static int side_prepare_bwd(SideStream* side, const EnfCall& c, bool zero_dlt, int wz_signals = 0) {
  if (!side) return 0;
  EnfDims mw = c.m;
  if (wz_signals > 0) mw.B = wz_signals;
  std::lock_guard<std::mutex> lk(side->mu);
  SidePending* e = side->entry(c.ws);
  if (!e) return 0;
  if (hipEventRecord(side->fork, c.st) != hipSuccess || hipStreamWaitEvent(side->s, side->fork, 0) != hipSuccess) return ENF_ELAUNCH;
  if (int rc = enf_launch_wz(mw, c.L, c.blob, c.F(c.W.lt), nullptr, c.F(c.W.wzb), nullptr, c.ws + c.W.wzt, side->s)) return rc;
  if (zero_dlt && hipMemsetAsync(c.F(c.W.dlt), 0, enf_lt_bytes(c.m), side->s) != hipSuccess) return ENF_ELAUNCH;
  if (hipEventRecord(e->join, side->s) != hipSuccess) return ENF_ELAUNCH;
  e->pending = true;              // until joined: a failure in between leaves it for the next call's join
  return 1;
}

extern "C" int enf_forward_stages(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a,
                                  const float* sigma, const void* packed, float* out, float* ybar, float* lse,
                                  void* workspace, size_t workspace_bytes, unsigned stages, void* stream) {
  EnfCall c;
  // ENF_STAGE_SHARED_LATENTS: the caller's statement that the signals share latents and points -- a batch stride contradicts it
  const bool shared = (stages & ENF_STAGE_SHARED_LATENTS) && d && d->B > 1;
  int rc = enf_call(c, d, x && p && a && out && !(shared && x_bstride != 0), sigma, packed, workspace, workspace_bytes, stream);
  if (rc) return rc;
  const EnfDims& m = c.m;
  const EnfWorkspace& W = c.W;
  float* yb = ybar ? ybar : c.F(W.ybar);
  float* ls = lse ? lse : c.F(W.lse);
  // ENF_STAGE_YBAR_HALF: the hand-off to the tail as bf16 (the launchers' ..._YBAR_HALF flags), decided HERE, once, for the pair kernel that writes
  // the rows and the tail that reads them.  Not with relu masks: the masked pair kernels (training passes) store fp32 only
  const bool yhalf = (stages & ENF_STAGE_YBAR_HALF) && m.bf16 && !ybar && (stages & ENF_STAGE_PAIR) && (stages & ENF_STAGE_TAIL) &&
                     !(stages & ENF_STAGE_TAIL_SAVE) && enf_zfold_split(m) <= 1 && m.mask_mode == ENF_MASK_OFF;
  if ((rc = enf_side_join_pending(c.st, workspace))) return rc;
  if ((stages & ENF_STAGE_PROLOGUE) && (rc = enf_launch_prologue(m, c.L, c.blob, p, a, sigma, c.F(W.lt), c.F(W.an), c.F(W.kv), c.st))) return rc;
  if ((stages & (ENF_STAGE_PAIR | ENF_STAGE_FOLD)) &&
      (rc = enf_launch_pair_fwd(m, c.L, c.blob, x, x_bstride, c.F(W.lt), yb, ls, c.fold_fwd(),
                                (stages & ENF_STAGE_FOLD ? ENF_PAIR_FOLD : 0u) | (stages & ENF_STAGE_PAIR ? ENF_PAIR_PAIR : 0u) |
                                    (yhalf ? ENF_PAIR_YBAR_HALF : 0u),
                                c.st, shared ? c.F(W.dybar) : nullptr)))
    return rc;
  // starts behind the pair kernel, beside the tail, the caller's loss and the tail backward
  if ((stages & ENF_STAGE_PREPARE_BWD) && enf_use_zfold_bwd(m) && (rc = side_prepare_bwd(side_stream(), c, true)) < 0) return rc;
  const bool tsave = (stages & ENF_STAGE_TAIL_SAVE) != 0;      // stash the tail's pre-activations for the backward that follows
  if ((stages & ENF_STAGE_TAIL) &&
      (rc = enf_launch_tail(m, c.L, c.blob, yb, out, nullptr, nullptr, nullptr, tsave ? c.F(W.tail_act) : nullptr,
                            ENF_TAIL_FWD | (tsave ? ENF_TAIL_STASH : 0u) | (yhalf ? ENF_TAIL_YBAR_HALF : 0u), c.st)))
    return rc;
  return ENF_OK;
}

extern "C" int enf_forward(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a,
                           const float* sigma, const void* packed, float* out, float* ybar, float* lse, void* workspace,
                           size_t workspace_bytes, void* stream) {
  return enf_forward_stages(d, x, x_bstride, p, a, sigma, packed, out, ybar, lse, workspace, workspace_bytes,
                            ENF_STAGE_PROLOGUE | ENF_STAGE_FOLD | ENF_STAGE_PAIR | ENF_STAGE_TAIL, stream);
}

extern "C" int enf_backward_latents(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a,
                                    const float* sigma, const void* packed, const float* ybar, const float* lse,
                                    const float* dout, float* dp, float* da, float* dsigma, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  return enf_backward_latents_ex(d, x, x_bstride, p, a, sigma, packed, ybar, lse, dout, dp, da, dsigma, workspace,
                                 workspace_bytes, 0u, stream);
}

// the backward pair kernel on the workspace's dybar / delta / dlt, in the z-fold form where the shape resolves to it;
// det: through the workspace's partial rows and the fixed-order reduction (which overwrites dlt) instead of float atomics
static int pair_bwd_on_workspace(const EnfCall& c, const float* x, int64_t x_bstride, const float* lse, bool det = false) {
  return enf_launch_pair_bwd(c.m, c.L, c.blob, x, x_bstride, c.F(c.W.lt), lse, c.F(c.W.dybar), c.F(c.W.delta), c.F(c.W.dlt), nullptr,
                             c.fold_bwd(), nullptr, c.st, det ? c.F(c.X.part) : nullptr);
}

extern "C" int enf_backward_latents_ex(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a,
                                       const float* sigma, const void* packed, const float* ybar, const float* lse,
                                       const float* dout, float* dp, float* da, float* dsigma, void* workspace,
                                       size_t workspace_bytes, unsigned flags, void* stream) {
  EnfCall c;
  const bool det = (flags & ENF_BWD_DETERMINISTIC) != 0;
  const bool known = !(flags & ~(ENF_BWD_REUSE_PROLOGUE | ENF_BWD_REUSE_TAIL | ENF_BWD_REUSE_PREPARED | ENF_BWD_ONLY_PAIR | ENF_BWD_DETERMINISTIC));
  int rc = enf_call(c, d, known && x && p && a && ybar && lse && dout && dp && da && dsigma, sigma, packed, workspace, workspace_bytes,
                    stream, det);
  if (rc) return rc;
  const EnfDims& m = c.m;
  const EnfWorkspace& W = c.W;
  hipStream_t st = c.st;
  const bool zb = enf_use_zfold_bwd(m);
  if (flags & ENF_BWD_ONLY_PAIR) {      // measurement hook: the pair kernel alone, on what a complete backward left behind
    if ((rc = enf_side_join_pending(st, workspace))) return rc;
    if (!det && hipMemsetAsync(c.F(W.dlt), 0, enf_lt_bytes(m), st) != hipSuccess) return ENF_ELAUNCH;
    return pair_bwd_on_workspace(c, x, x_bstride, lse, det);
  }
  // the latent table is recomputed (cheap) so the call does not depend on workspace contents, unless the
  // caller vouches that nothing has touched the workspace since the matching enf_forward
  if (!(flags & ENF_BWD_REUSE_PROLOGUE) && (rc = enf_launch_prologue(m, c.L, c.blob, p, a, sigma, c.F(W.lt), c.F(W.an), c.F(W.kv), st)))
    return rc;
  // z-fold backward: the per-latent matrices depend on the latent table only, so enf_wz_kernel runs on a side stream
  // (fork / join by events) beside the tail backward instead of in front of the pair kernel
  SideStream* side = zb ? side_stream() : nullptr;
  bool prepared = false;
  if (zb && side && (flags & ENF_BWD_REUSE_PREPARED) && (flags & ENF_BWD_REUSE_PROLOGUE)) {
    std::lock_guard<std::mutex> lk(side->mu);
    auto it = side->ws.find(workspace);
    prepared = it != side->ws.end() && it->second.pending;   // launched by the matching forward ON THIS WORKSPACE
  }
  if (!prepared && (rc = enf_side_join_pending(st, workspace))) return rc;
  if (zb && !prepared) {
    if ((rc = side_prepare_bwd(side, c, false)) < 0) return rc;
    if (!rc && (rc = enf_launch_wz(m, c.L, c.blob, c.F(W.lt), nullptr, c.F(W.wzb), nullptr, c.ws + W.wzt, st))) return rc;
  }
  const bool treuse = (flags & ENF_BWD_REUSE_TAIL) && (flags & ENF_BWD_REUSE_PROLOGUE);
  if ((rc = enf_launch_tail(m, c.L, c.blob, ybar, nullptr, dout, c.F(W.dybar), c.F(W.delta), c.F(W.tail_act),
                            ENF_TAIL_BWD | (treuse ? ENF_TAIL_STASH : 0u), st)))
    return rc;
  // (deterministic mode: the reduction overwrites the gradient table, nothing to zero)
  if (!prepared && !det && hipMemsetAsync(c.F(W.dlt), 0, enf_lt_bytes(m), st) != hipSuccess) return ENF_ELAUNCH;
  if ((rc = enf_side_join_pending(st, workspace))) return rc;      // the per-latent matrices (and, if prepared, the zeroed table)
  if ((rc = pair_bwd_on_workspace(c, x, x_bstride, lse, det))) return rc;
  return enf_launch_prologue_bwd(m, c.L, c.blob, p, sigma, c.F(W.an), c.F(W.kv), c.F(W.dlt), dp, da, dsigma, st);
}


// One inner step of the MAML loop in one call (SURVEY.md 8d's unit of work; pde_trainer.py:175-207): forward on the sampled points,
// mean squared error against `target` and its gradient, backward to the latents.  Same kernels as enf_forward_stages +
// enf_mse_value_grad + enf_backward_latents_ex with every REUSE flag, except that the tail runs ONCE (forward chain, loss and
// backward chain in one kernel, enf_tail.hip: LOSS) and neither `out` nor `d out` exists.
// The one copy of the fit-step sequence, against the loss `ls` describes (enf_launch.h: EnfLossSpec; `target` is (B, rows, O)).
// With ls.err the tail also stores the per-observation errors, and with ls.loss_b the per-signal sums follow at the end of the sequence
// on the same stream.  ENF_FIT_DETERMINISTIC: the same kernels; the loss partials and K3's gradient rows go through the workspace's
// partial buffers and are added in a fixed order (no float atomic, no zero-fill of the gradient table).
// An operator: the tail runs forward with its stash and backward on it, the two products of enf_obs.hip between them, on the regions of
// enf_obs_workspace behind the workspace.
static int fit_step_sequence(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                             const void* packed, const float* target, float grad_scale, float* loss, float* dp, float* da,
                             float* dsigma, void* workspace, size_t workspace_bytes, unsigned flags, void* stream, const EnfLossSpec& ls) {
  EnfCall c;
  const bool det = (flags & ENF_FIT_DETERMINISTIC) != 0;
  // ENF_FIT_SHARED_LATENTS (include/enf_hip.h): a permission for the forward pair kernel; with one signal it says nothing
  const bool shared = (flags & ENF_FIT_SHARED_LATENTS) && d && d->B > 1;
  const int refusal = ls.check(d, flags, ENF_LOSS_FIT);
  if (refusal == ENF_EUNSUPPORTED) {
    const int drc = enf_check_desc(d);
    return drc ? drc : refusal;
  }
  int rc = enf_call(c, d, !(flags & ~(ENF_FIT_DETERMINISTIC | ENF_FIT_SHARED_LATENTS)) && !(shared && x_bstride != 0) && x && p && a && target &&
                    loss && dp && da && dsigma && refusal == ENF_OK, sigma, packed, workspace, workspace_bytes, stream, det);
  if (rc) return rc;
  const EnfDims& m = c.m;
  const EnfWorkspace& W = c.W;
  hipStream_t st = c.st;
  const bool zb = enf_use_zfold_bwd(m);
  const bool grp = ls.kind == ENF_LOSS_GROUPS, ao = ls.kind == ENF_LOSS_OPERATOR;
  const int rows = ls.rows(m);
  float* err = ls.err;
  const EnfObsWorkspace Y = enf_obs_workspace(m, det ? c.X.total : W.total, ao ? rows : 1);
  if (ao && workspace_bytes < Y.total) return ENF_EWORKSPACE;
  if ((rc = enf_side_join_pending(st, workspace))) return rc;
  if ((rc = enf_launch_prologue(m, c.L, c.blob, p, a, sigma, c.F(W.lt), c.F(W.an), c.F(W.kv), st))) return rc;
  // (shared: the parts of the one forward borrow d ybar | delta, which this step's tail overwrites afterwards)
  if ((rc = enf_launch_pair_fwd(m, c.L, c.blob, x, x_bstride, c.F(W.lt), c.F(W.ybar), c.F(W.lse), c.fold_fwd(), ENF_PAIR_FOLD | ENF_PAIR_PAIR, st,
                                shared ? c.F(W.dybar) : nullptr)))
    return rc;
  // the shared-latent backward (enf_layout.h: enf_shared_backward_rule): tail, loss and backward pair kernel run ONCE, on signal 0
  const bool sbwd = enf_shared_backward_rule(m, flags, ls.cweight != nullptr, err != nullptr) == 1;
  EnfDims m1 = m;
  if (sbwd) m1.B = 1;
  // what the backward pair kernel needs from the latent table alone runs on the side stream beside the tail
  if ((rc = side_prepare_bwd(zb ? side_stream() : nullptr, c, !det, sbwd ? 1 : 0)) < 0) return rc;
  if (!rc) {
    if (zb && (rc = enf_launch_wz(m1, c.L, c.blob, c.F(W.lt), nullptr, c.F(W.wzb), nullptr, c.ws + W.wzt, st))) return rc;
    if (!det && hipMemsetAsync(c.F(W.dlt), 0, enf_lt_bytes(m), st) != hipSuccess) return ENF_ELAUNCH;
  }
  if (sbwd) {
    // signal 0's tail forward and unit-seeded tail backward in one launch (the seed does not depend on the loss), the loss of that one
    // row against all B targets and weights with d out (B, N), then the one pair pass contracted with d out.  d out and the row of
    // outputs borrow the d ybar region behind signal 0's rows, which nothing else of this step uses: [N HD | d out: B N | out: N].
    float* dout = c.F(W.dybar) + (size_t)m.N * m.HD;
    float* out1 = dout + (size_t)m.B * m.N;
    if ((rc = enf_launch_tail_fwd_seed(m1, c.L, c.blob, c.F(W.ybar), out1, 0, c.F(W.dybar), c.F(W.delta), c.F(W.tail_act), st))) return rc;
    // (grouped: the one row's group sums with signal 0's factors against all B signals' observations and observation weights)
    if (grp) rc = enf_launch_mse_group_shared(out1, target, ls.qweight, ls.weight, m.B, m.N, ls.G, grad_scale, dout, loss, st);
    else rc = enf_launch_mse_shared(out1, target, ls.weight, m.B, m.N, grad_scale, dout, loss, st);
    if (rc) return rc;
    if ((rc = enf_side_join_pending(st, workspace))) return rc;
    if ((rc = enf_launch_pair_bwd_shared(m, c.L, c.blob, x, c.F(W.lt), c.F(W.lse), c.F(W.dybar), c.F(W.delta), dout, c.F(W.dlt),
                                         c.fold_bwd(), st)))
      return rc;
    return enf_launch_prologue_bwd(m, c.L, c.blob, p, sigma, c.F(W.an), c.F(W.kv), c.F(W.dlt), dp, da, dsigma, st);
  }
  if (ao) {
    // out -> [kernel 1] obs, r, err_a, loss -> [kernel 2] d out; loss_b without err_a: the errors go through the workspace's own region
    if (ls.loss_b && !err) err = c.F(Y.err);
    const float gs = 2.0f * (1.0f / ((float)m.B * (float)rows * (float)m.O)) * grad_scale;
    if ((rc = enf_launch_tail(m, c.L, c.blob, c.F(W.ybar), c.F(Y.out), nullptr, nullptr, nullptr, c.F(W.tail_act), ENF_TAIL_FWD | ENF_TAIL_STASH, st)))
      return rc;
    if ((rc = enf_launch_obs_loss(*ls.op, m.N, m.B, m.O, c.F(Y.out), target, ls.weight, ls.cweight, c.F(Y.r), err, loss,
                                  det ? c.F(Y.loss) : nullptr, st)))
      return rc;
    if ((rc = enf_launch_obs_transpose(*ls.op, m.N, m.B, m.O, c.F(Y.r), gs, c.F(Y.dout), st))) return rc;
    rc = enf_launch_tail(m, c.L, c.blob, c.F(W.ybar), nullptr, c.F(Y.dout), c.F(W.dybar), c.F(W.delta), c.F(W.tail_act),
                         ENF_TAIL_BWD | ENF_TAIL_STASH, st);
  } else if (grp) rc = enf_launch_tail_group(m, c.L, c.blob, c.F(W.ybar), target, ls.group(err), grad_scale, loss, c.F(W.dybar), c.F(W.delta),
                                             c.F(W.tail_act), st, det ? c.F(c.X.loss) : nullptr);
  else rc = enf_launch_tail_loss(m, c.L, c.blob, c.F(W.ybar), target, ls.cweight ? ls.cweight : ls.weight, grad_scale, loss, c.F(W.dybar),
                                 c.F(W.delta), c.F(W.tail_act), st, det ? c.F(c.X.loss) : nullptr, ls.cweight != nullptr, err);
  if (rc) return rc;
  if ((rc = enf_side_join_pending(st, workspace))) return rc;
  if ((rc = pair_bwd_on_workspace(c, x, x_bstride, c.F(W.lse), det))) return rc;
  if ((rc = enf_launch_prologue_bwd(m, c.L, c.blob, p, sigma, c.F(W.an), c.F(W.kv), c.F(W.dlt), dp, da, dsigma, st))) return rc;
  // (behind the gradients: nothing of the step waits for the per-signal sums)
  return err && ls.loss_b ? enf_launch_signal_sum(err, m.B, rows, 1.0f / ((float)rows * (float)m.O), ls.loss_b, st) : ENF_OK;
}

extern "C" int enf_fit_step(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                            const void* packed, const float* target, float grad_scale, float* loss, float* dp, float* da,
                            float* dsigma, void* workspace, size_t workspace_bytes, void* stream) {
  return fit_step_sequence(d, x, x_bstride, p, a, sigma, packed, target, grad_scale, loss, dp, da, dsigma, workspace, workspace_bytes, 0u, stream,
                           EnfLossSpec{});
}

extern "C" int enf_fit_step_ex(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                               const void* packed, const float* target, float grad_scale, float* loss, float* dp, float* da,
                               float* dsigma, void* workspace, size_t workspace_bytes, unsigned flags, void* stream) {
  return fit_step_sequence(d, x, x_bstride, p, a, sigma, packed, target, grad_scale, loss, dp, da, dsigma, workspace, workspace_bytes, flags, stream,
                           EnfLossSpec{});
}

// one loss weight per signal and query, weight (B, N) or NULL (include/enf_hip.h, "Weighted loss")
extern "C" int enf_fit_step_w(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                              const void* packed, const float* target, float grad_scale, float* loss, float* dp, float* da,
                              float* dsigma, void* workspace, size_t workspace_bytes, const float* weight, unsigned flags,
                              void* stream) {
  return fit_step_sequence(d, x, x_bstride, p, a, sigma, packed, target, grad_scale, loss, dp, da, dsigma, workspace, workspace_bytes, flags, stream,
                           EnfLossSpec{ENF_LOSS_POINTS, weight});
}

// per-channel loss weights, cweight (B, N, O), required
extern "C" int enf_fit_step_cw(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                               const void* packed, const float* target, float grad_scale, float* loss, float* dp, float* da,
                               float* dsigma, void* workspace, size_t workspace_bytes, const float* cweight, unsigned flags,
                               void* stream) {
  EnfLossSpec ls{ENF_LOSS_POINTS, nullptr, cweight};
  ls.need_cweight = true;
  return fit_step_sequence(d, x, x_bstride, p, a, sigma, packed, target, grad_scale, loss, dp, da, dsigma, workspace, workspace_bytes, flags, stream, ls);
}

// enf_fit_step_w / _cw plus the per-point errors and, with loss_b, the per-signal losses (include/enf_hip.h, "Per-signal and per-point
// errors"): the same kernel instantiations with the `err` pointer set, so loss and gradients are those calls', bit for bit
extern "C" int enf_fit_step_e(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                              const void* packed, const float* target, float grad_scale, float* loss, float* dp, float* da,
                              float* dsigma, void* workspace, size_t workspace_bytes, const float* weight, const float* cweight,
                              float* err, float* loss_b, unsigned flags, void* stream) {
  EnfLossSpec ls{ENF_LOSS_POINTS, weight, cweight, err, loss_b};
  ls.need_err = true;
  return fit_step_sequence(d, x, x_bstride, p, a, sigma, packed, target, grad_scale, loss, dp, da, dsigma, workspace, workspace_bytes, flags, stream, ls);
}

// Evaluation without a decode, against the loss `ls` describes: prologue, forward pair kernel (whatever variant the descriptor resolves
// to), the evaluation tail -- for an operator the plain forward tail into the workspace, then the forward product with the loss --, the
// per-signal sums.  loss_b without err: the errors go through the workspace's (unused) d ybar region, B N HD floats, or the
// operator's own region.
static int eval_loss_sequence(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                              const void* packed, const float* target, float* loss, void* workspace, size_t workspace_bytes,
                              unsigned flags, void* stream, const EnfLossSpec& ls) {
  EnfCall c;
  const bool det = (flags & ENF_FIT_DETERMINISTIC) != 0;
  int rc = enf_call(c, d, !(flags & ~ENF_FIT_DETERMINISTIC) && x && p && a && target && (loss || ls.err || ls.loss_b) &&
                    ls.check(d, flags, ENF_LOSS_EVAL) == ENF_OK, sigma, packed, workspace, workspace_bytes, stream, det);
  if (rc) return rc;
  const EnfDims& m = c.m;
  const EnfWorkspace& W = c.W;
  hipStream_t st = c.st;
  const bool ao = ls.kind == ENF_LOSS_OPERATOR;
  const int rows = ls.rows(m);
  const EnfObsWorkspace Y = enf_obs_workspace(m, det ? c.X.total : W.total, ao ? rows : 1);
  if (ao && workspace_bytes < Y.total) return ENF_EWORKSPACE;
  if ((rc = enf_side_join_pending(st, workspace))) return rc;
  if ((rc = enf_launch_prologue(m, c.L, c.blob, p, a, sigma, c.F(W.lt), c.F(W.an), c.F(W.kv), st))) return rc;
  if ((rc = enf_launch_pair_fwd(m, c.L, c.blob, x, x_bstride, c.F(W.lt), c.F(W.ybar), c.F(W.lse), c.fold_fwd(), ENF_PAIR_FOLD | ENF_PAIR_PAIR, st)))
    return rc;
  float* e = ls.err ? ls.err : (ls.loss_b ? c.F(ao ? Y.err : W.dybar) : nullptr);
  if (ao) {
    if ((rc = enf_launch_tail(m, c.L, c.blob, c.F(W.ybar), c.F(Y.out), nullptr, nullptr, nullptr, nullptr, ENF_TAIL_FWD, st))) return rc;
    rc = enf_launch_obs_loss(*ls.op, m.N, m.B, m.O, c.F(Y.out), target, ls.weight, ls.cweight, nullptr, e, loss, det ? c.F(Y.loss) : nullptr, st);
  } else if (ls.kind == ENF_LOSS_GROUPS)
    rc = enf_launch_tail_group(m, c.L, c.blob, c.F(W.ybar), target, ls.group(e), 0.f, loss, nullptr, nullptr, nullptr, st, det ? c.F(c.X.loss) : nullptr);
  else
    rc = enf_launch_tail_eval(m, c.L, c.blob, c.F(W.ybar), target, ls.cweight ? ls.cweight : ls.weight, ls.cweight != nullptr, loss, e, st,
                              det ? c.F(c.X.loss) : nullptr);
  if (rc) return rc;
  return ls.loss_b ? enf_launch_signal_sum(e, m.B, rows, 1.0f / ((float)rows * (float)m.O), ls.loss_b, st) : ENF_OK;
}

extern "C" int enf_eval_loss(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                             const void* packed, const float* target, const float* weight, const float* cweight, float* loss,
                             float* err, float* loss_b, void* workspace, size_t workspace_bytes, unsigned flags, void* stream) {
  return eval_loss_sequence(d, x, x_bstride, p, a, sigma, packed, target, loss, workspace, workspace_bytes, flags, stream,
                            EnfLossSpec{ENF_LOSS_POINTS, weight, cweight, err, loss_b});
}

// ---- grouped observations (include/enf_hip.h, "Grouped observations"): the two sequences with the tail's grouped forms; target
// (B, N / G, O), weights and errors per observation.
extern "C" int enf_fit_step_g(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                              const void* packed, const float* target, int32_t G, const float* qweight, const float* oweight, float grad_scale,
                              float* loss, float* dp, float* da, float* dsigma, float* err_g, float* loss_b, void* workspace,
                              size_t workspace_bytes, unsigned flags, void* stream) {
  const EnfLossSpec ls{ENF_LOSS_GROUPS, oweight, nullptr, err_g, loss_b, G, qweight};
  return fit_step_sequence(d, x, x_bstride, p, a, sigma, packed, target, grad_scale, loss, dp, da, dsigma, workspace, workspace_bytes, flags, stream, ls);
}

// enf_fit_step_g that may carry ENF_FIT_SHARED_LATENTS (the first inner step of a fit on cells): the flag clear, the call above; set,
// the one shared forward and -- where enf_shared_backward_rule holds and err_g is NULL -- the one shared backward, its d out (B, N) from
// the grouped SHARED loss kernel; elsewhere the ordinary grouped tail behind the shared forward.
extern "C" int enf_fit_step_gs(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                               const void* packed, const float* target, int32_t G, const float* qweight, const float* oweight, float grad_scale,
                               float* loss, float* dp, float* da, float* dsigma, float* err_g, float* loss_b, void* workspace,
                               size_t workspace_bytes, unsigned flags, void* stream) {
  EnfLossSpec ls{ENF_LOSS_GROUPS, oweight, nullptr, err_g, loss_b, G, qweight};
  ls.shared_entry = true;
  return fit_step_sequence(d, x, x_bstride, p, a, sigma, packed, target, grad_scale, loss, dp, da, dsigma, workspace, workspace_bytes, flags, stream, ls);
}

extern "C" int enf_eval_loss_g(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                               const void* packed, const float* target, int32_t G, const float* qweight, const float* oweight, float* loss,
                               float* err_g, float* loss_b, void* workspace, size_t workspace_bytes, unsigned flags, void* stream) {
  return eval_loss_sequence(d, x, x_bstride, p, a, sigma, packed, target, loss, workspace, workspace_bytes, flags, stream,
                            EnfLossSpec{ENF_LOSS_GROUPS, oweight, nullptr, err_g, loss_b, G, qweight});
}

// per-value weights on grouped observations: cweight_g (B, M, O), required, in place of oweight -- the tail's per-value grouped forms
extern "C" int enf_fit_step_gc(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                               const void* packed, const float* target, int32_t G, const float* qweight, const float* cweight_g, float grad_scale,
                               float* loss, float* dp, float* da, float* dsigma, float* err_g, float* loss_b, void* workspace,
                               size_t workspace_bytes, unsigned flags, void* stream) {
  EnfLossSpec ls{ENF_LOSS_GROUPS, nullptr, cweight_g, err_g, loss_b, G, qweight};
  ls.need_cweight = true;
  return fit_step_sequence(d, x, x_bstride, p, a, sigma, packed, target, grad_scale, loss, dp, da, dsigma, workspace, workspace_bytes, flags, stream, ls);
}

extern "C" int enf_eval_loss_gc(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                                const void* packed, const float* target, int32_t G, const float* qweight, const float* cweight_g, float* loss,
                                float* err_g, float* loss_b, void* workspace, size_t workspace_bytes, unsigned flags, void* stream) {
  EnfLossSpec ls{ENF_LOSS_GROUPS, nullptr, cweight_g, err_g, loss_b, G, qweight};
  ls.need_cweight = true;
  return eval_loss_sequence(d, x, x_bstride, p, a, sigma, packed, target, loss, workspace, workspace_bytes, flags, stream, ls);
}

// ---- sparse linear observations (include/enf_hip.h, "Sparse linear observations"): the two sequences with the tail run unfused and
// the two products of enf_obs.hip in the loss's place; target (B, M, O), weights and errors per observation.
extern "C" size_t enf_obs_workspace_bytes(const EnfDesc* d, int32_t M, unsigned flags) {
  if (enf_check_desc(d) != ENF_OK || M < 1 || (flags & ~ENF_FIT_DETERMINISTIC)) return 0;
  const EnfDims m = enf_dims(d);
  const EnfWorkspace W = enf_workspace(m);
  return enf_obs_workspace(m, (flags & ENF_FIT_DETERMINISTIC) ? enf_det_workspace(m, W).total : W.total, M).total;
}

extern "C" int enf_fit_step_a(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                              const void* packed, const float* target, const EnfSparseObs* op, const float* oweight, const float* cweight,
                              float grad_scale, float* loss, float* dp, float* da, float* dsigma, float* err_a, float* loss_b, void* workspace,
                              size_t workspace_bytes, unsigned flags, void* stream) {
  const EnfLossSpec ls{ENF_LOSS_OPERATOR, oweight, cweight, err_a, loss_b, 1, nullptr, op};
  return fit_step_sequence(d, x, x_bstride, p, a, sigma, packed, target, grad_scale, loss, dp, da, dsigma, workspace, workspace_bytes, flags, stream, ls);
}

extern "C" int enf_eval_loss_a(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                               const void* packed, const float* target, const EnfSparseObs* op, const float* oweight, const float* cweight,
                               float* loss, float* err_a, float* loss_b, void* workspace, size_t workspace_bytes, unsigned flags, void* stream) {
  return eval_loss_sequence(d, x, x_bstride, p, a, sigma, packed, target, loss, workspace, workspace_bytes, flags, stream,
                            EnfLossSpec{ENF_LOSS_OPERATOR, oweight, cweight, err_a, loss_b, 1, nullptr, op});
}

// ---- derivative fields: the Jacobian of a decode w.r.t. the query coordinates (include/enf_hip.h, "Derivative fields")
// The workspace of enf_field_grad / enf_query_vjp: the plain one; with ENF_BWD_DETERMINISTIC the deterministic one (K3's partial rows)
// followed by the per-latent shares of the query gradient, (B, Z, N, dx) floats, reused by every channel's pass.
extern "C" size_t enf_field_grad_workspace_bytes(const EnfDesc* d, unsigned flags) {
  if (enf_check_desc(d) != ENF_OK || d->mask_mode != ENF_MASK_OFF || (flags & ~ENF_BWD_DETERMINISTIC)) return 0;
  const EnfDims m = enf_dims(d);
  const EnfWorkspace W = enf_workspace(m);
  return (flags & ENF_BWD_DETERMINISTIC) ? enf_det_workspace(m, W).total + enf_det_dx_bytes(m) : W.total;
}

// The one copy of the sequence.  dout == NULL: the Jacobian -- one seeded tail backward and one backward pair kernel per output channel,
// channel o's query gradient into grad + o B N dx; dout != NULL: one pass of the tail backward on `dout`, the vector-Jacobian product
// into grad (B, N, dx).  Prologue, the z-fold backward's per-latent matrices, forward pair kernel and the forward tail with its stash run
// once.  Everything is on the caller's stream.
static int field_grad_sequence(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                               const void* packed, const float* dout, float* out, float* grad, bool args_ok, void* workspace,
                               size_t workspace_bytes, unsigned flags, void* stream) {
  int rc = enf_check_desc(d);
  if (rc) return rc;
  if (d->mask_mode != ENF_MASK_OFF) return ENF_EUNSUPPORTED;      // relu masks belong to the meta-gradient, not to a decode
  EnfCall c;
  const bool det = (flags & ENF_BWD_DETERMINISTIC) != 0;
  if ((rc = enf_call(c, d, !(flags & ~ENF_BWD_DETERMINISTIC) && x && p && a && grad && args_ok, sigma, packed, workspace, workspace_bytes,
                     stream, det)))
    return rc;
  const EnfDims& m = c.m;
  const EnfWorkspace& W = c.W;
  hipStream_t st = c.st;
  if (det && workspace_bytes < c.X.total + enf_det_dx_bytes(m)) return ENF_EWORKSPACE;
  float* part = det ? c.F(c.X.part) : nullptr;
  float* dxpart = det ? c.F(c.X.total) : nullptr;
  const bool zb = enf_use_zfold_bwd(m);
  const size_t per = (size_t)m.B * m.N * m.dx;                    // one channel's query gradient
  const int passes = dout ? 1 : m.O;
  if ((rc = enf_side_join_pending(st, workspace))) return rc;
  if ((rc = enf_launch_prologue(m, c.L, c.blob, p, a, sigma, c.F(W.lt), c.F(W.an), c.F(W.kv), st))) return rc;
  if (zb && (rc = enf_launch_wz(m, c.L, c.blob, c.F(W.lt), nullptr, c.F(W.wzb), nullptr, c.ws + W.wzt, st))) return rc;
  if ((rc = enf_launch_pair_fwd(m, c.L, c.blob, x, x_bstride, c.F(W.lt), c.F(W.ybar), c.F(W.lse), c.fold_fwd(), ENF_PAIR_FOLD | ENF_PAIR_PAIR, st)))
    return rc;
  // the forward tail with the stash; without `out` its B N O values land in the workspace's d ybar region (B N HD floats, O <= 32 <= HD),
  // which the first backward pass overwrites
  if ((rc = enf_launch_tail(m, c.L, c.blob, c.F(W.ybar), out ? out : c.F(W.dybar), nullptr, nullptr, nullptr, c.F(W.tail_act),
                            ENF_TAIL_FWD | ENF_TAIL_STASH, st)))
    return rc;
  // default mode: K3 adds to d lt (scratch of this call, never returned: zeroed once, the passes pile up in it) and to the query gradient
  // with float atomics; deterministic mode: the fixed-order reductions overwrite both
  if (!det && (hipMemsetAsync(c.F(W.dlt), 0, enf_lt_bytes(m), st) != hipSuccess ||
               hipMemsetAsync(grad, 0, sizeof(float) * per * passes, st) != hipSuccess))
    return ENF_ELAUNCH;
  for (int o = 0; o < passes; ++o) {
    if (dout) rc = enf_launch_tail(m, c.L, c.blob, c.F(W.ybar), nullptr, dout, c.F(W.dybar), c.F(W.delta), c.F(W.tail_act),
                                    ENF_TAIL_BWD | ENF_TAIL_STASH, st);
    else rc = enf_launch_tail_seed(m, c.L, c.blob, c.F(W.ybar), o, c.F(W.dybar), c.F(W.delta), c.F(W.tail_act), st);
    if (rc) return rc;
    if ((rc = enf_launch_pair_bwd(m, c.L, c.blob, x, x_bstride, c.F(W.lt), c.F(W.lse), c.F(W.dybar), c.F(W.delta), c.F(W.dlt), nullptr,
                                  c.fold_bwd(), grad + (size_t)o * per, st, part, dxpart)))
      return rc;
  }
  return ENF_OK;
}

extern "C" int enf_field_grad(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                              const void* packed, float* out, float* jac, void* workspace, size_t workspace_bytes, unsigned flags,
                              void* stream) {
  return field_grad_sequence(d, x, x_bstride, p, a, sigma, packed, nullptr, out, jac, true, workspace, workspace_bytes, flags, stream);
}

extern "C" int enf_query_vjp(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                             const void* packed, const float* dout, float* out, float* dx, void* workspace, size_t workspace_bytes,
                             unsigned flags, void* stream) {
  return field_grad_sequence(d, x, x_bstride, p, a, sigma, packed, dout, out, dx, dout != nullptr, workspace, workspace_bytes, flags, stream);
}

extern "C" int enf_lt_layout(const EnfDesc* d, int* stride, int* off_u, int* off_v0, int* off_pose, int* off_wcoef, int* off_c) {
  int rc = enf_check_desc(d);
  if (rc) return rc;
  if (stride) *stride = enf_lt_stride(d->H, d->D);
  if (off_u) *off_u = enf_lt_off_u(d->H, d->D);
  if (off_v0) *off_v0 = enf_lt_off_v0(d->H, d->D);
  if (off_pose) *off_pose = enf_lt_off_pose(d->H, d->D);
  if (off_wcoef) *off_wcoef = enf_lt_off_wcoef(d->H, d->D);
  if (off_c) *off_c = enf_lt_off_c(d->H, d->D);
  return ENF_OK;
}

extern "C" int enf_lt_layout_ext(const EnfDesc* d, int* off_ext, int* off_phase_q, int* off_phase_v) {
  int rc = enf_check_desc(d);
  if (rc) return rc;
  if (off_ext) *off_ext = enf_lt_off_ext(d->H, d->D);
  if (off_phase_q) *off_phase_q = enf_lt_off_phq(d->H, d->D);
  if (off_phase_v) *off_phase_v = enf_lt_off_phv(d->H, d->D);
  return ENF_OK;
}

// What ENF_VARIANT_AUTO resolves to is a function of the shape alone (enf_layout.h); per call the caller chooses with
// EnfDesc.pair_fwd_variant / pair_bwd_variant.
extern "C" int enf_pair_variant(const EnfDesc* d, int backward) {
  const int rc = enf_check_desc(d);
  if (rc) return rc;
  const EnfDims m = enf_dims(d);
  if (backward) return enf_use_zfold_bwd(m) ? ENF_VARIANT_ZFOLD : ENF_VARIANT_LATENT_SPLIT;
  const int sp = enf_zfold_split(m);
  return sp > 1 ? ENF_VARIANT_ZFOLD_ZSPLIT : (sp == 1 ? ENF_VARIANT_ZFOLD : ENF_VARIANT_LATENT_SPLIT);
}

// the shared-latent forward's parts (enf_layout.h: enf_shared_fwd_parts): 1 and *parts = P where a call with ENF_FIT_SHARED_LATENTS /
// ENF_STAGE_SHARED_LATENTS on this descriptor runs the one shared forward, 0 (and *parts = 1) where it runs the ordinary sequence
extern "C" int enf_shared_forward_parts(const EnfDesc* d, int32_t* parts) {
  const int rc = enf_check_desc(d);
  if (rc) return rc;
  if (!parts) return ENF_EINVAL;
  const EnfDims m = enf_dims(d);
  const int P = enf_use_zfold(m) || (m.mask_mode != ENF_MASK_OFF && !m.ffn) ? 0 : enf_shared_fwd_parts(m);
  *parts = P ? P : 1;
  return P ? 1 : 0;
}

// 1 where a fit step with these flags on this descriptor takes the shared-latent backward (enf_layout.h: enf_shared_backward_rule; a
// call that carries per-channel weights or wants the per-point errors never does), 0 where it runs the ordinary sequence
extern "C" int enf_shared_backward_applies(const EnfDesc* d, unsigned flags) {
  const int rc = enf_check_desc(d);
  if (rc) return rc;
  if (flags & ~(ENF_FIT_DETERMINISTIC | ENF_FIT_SHARED_LATENTS)) return ENF_EINVAL;
  return enf_shared_backward_rule(enf_dims(d), flags, false, false);
}

extern "C" int enf_pair_partition(const EnfDesc* d, int32_t* run, int32_t* workgroups, int32_t* parts) {
  const int rc = enf_check_desc(d);
  if (rc) return rc;
  if (!run || !workgroups || !parts) return ENF_EINVAL;
  const EnfDims m = enf_dims(d);
  if (enf_zfold_split(m) < 2) return 0;
  const EnfStreamK k = enf_zfold_streamk(m);
  *run = k.len; *workgroups = k.wgs; *parts = k.parts;
  return 1;
}

// the z-fold forward's scratch outside a workspace (byte offsets; total 0: the latent-split variant, no scratch)
struct PairScratch { size_t wz, wzb, wzu, ysplit, total; };
static PairScratch pair_scratch(const EnfDims& m) {
  PairScratch s{0, 0, 0, 0, 0};
  if (!enf_use_zfold(m)) return s;
  const size_t BZ = (size_t)m.B * m.Z, BN = (size_t)m.B * m.N;
  const int split = enf_zfold_split(m);
  s.wzb = s.wz + enf_align(BZ * m.H * enf_panel_bytes(m.D, m.D, m.bf16));
  s.wzu = s.wzb + enf_align(sizeof(float) * BZ * m.HD);
  s.ysplit = s.wzu + enf_align(BZ * enf_wzu_bytes(m.H, m.D));
  s.total = s.ysplit + (split > 1 ? sizeof(float) * split * (BN * m.HD + BN * m.H * 3) : 0);
  return s;
}

extern "C" size_t enf_pair_scratch_bytes(const EnfDesc* d) {
  if (enf_check_desc(d)) return 0;
  return pair_scratch(enf_dims(d)).total;
}

extern "C" int enf_pair_forward(const EnfDesc* d, const float* x, int64_t x_bstride, const float* lt, const void* packed,
                                float* ybar, float* lse, void* scratch, size_t scratch_bytes, void* stream) {
  int rc = enf_check_desc(d);
  if (rc) return rc;
  if (!x || !lt || !packed || !ybar || !lse) return ENF_EINVAL;
  const EnfDims m = enf_dims(d);
  const PairScratch S = pair_scratch(m);
  const bool zf = S.total != 0;
  if (zf && (!scratch || scratch_bytes < S.total)) return ENF_EWORKSPACE;
  char* sc = (char*)scratch;
  EnfFoldFwd zs{};
  if (zf) zs = {sc + S.wz, reinterpret_cast<float*>(sc + S.wzb), sc + S.wzu, enf_zfold_split(m) > 1 ? reinterpret_cast<float*>(sc + S.ysplit) : nullptr};
  return enf_launch_pair_fwd(m, enf_layout(m), (const char*)packed, x, x_bstride, lt, ybar, lse, zs, ENF_PAIR_FOLD | ENF_PAIR_PAIR, (hipStream_t)stream);
}

extern "C" size_t enf_relu_mask_bytes(const EnfDesc* d) {
  if (enf_check_desc(d) != ENF_OK) return 0;
  const size_t signals = d->mask_signals > 0 ? d->mask_signals : d->B;
  return signals * d->Z * ((d->N + 15) / 16) * 2 * 64 * sizeof(unsigned);
}

extern "C" int enf_pair_backward(const EnfDesc* d, const float* x, int64_t x_bstride, const float* lt, const void* packed,
                                 const float* lse, const float* dybar, const float* delta, float* dlt, void* const* store,
                                 void* stream) {
  return enf_pair_backward_ex(d, x, x_bstride, lt, packed, lse, dybar, delta, dlt, store, nullptr, stream);
}

extern "C" int enf_pair_backward_ex(const EnfDesc* d, const float* x, int64_t x_bstride, const float* lt, const void* packed,
                                    const float* lse, const float* dybar, const float* delta, float* dlt, void* const* store,
                                    float* dx, void* stream) {
  return enf_pair_backward_ex2(d, x, x_bstride, lt, packed, lse, dybar, delta, dlt, store, dx, nullptr, 0, 0u, stream);
}

// scratch of enf_pair_backward_ex2: [K3's partial rows | with ENF_BWD_QUERY_GRAD the per-latent shares of d x]; 0 without the
// deterministic flag (the stand-alone entry point always runs the latent-split kernel)
extern "C" size_t enf_pair_backward_scratch_bytes(const EnfDesc* d, unsigned flags) {
  if (enf_check_desc(d) != ENF_OK || (flags & ~(ENF_BWD_DETERMINISTIC | ENF_BWD_QUERY_GRAD))) return 0;
  if (!(flags & ENF_BWD_DETERMINISTIC)) return 0;
  const EnfDims m = enf_dims(d);
  return enf_det_part_bytes(m, false) + ((flags & ENF_BWD_QUERY_GRAD) ? enf_det_dx_bytes(m) : 0);
}

extern "C" int enf_pair_backward_ex2(const EnfDesc* d, const float* x, int64_t x_bstride, const float* lt, const void* packed,
                                     const float* lse, const float* dybar, const float* delta, float* dlt, void* const* store,
                                     float* dx, void* scratch, size_t scratch_bytes, unsigned flags, void* stream) {
  int rc = enf_check_desc(d);
  if (rc) return rc;
  if ((flags & ~ENF_BWD_DETERMINISTIC) || !x || !lt || !packed || !lse || !dybar || !delta || !dlt) return ENF_EINVAL;
  const bool det = (flags & ENF_BWD_DETERMINISTIC) != 0;
  if (det && !scratch) return ENF_EINVAL;
  const EnfDims m = enf_dims(d);
  if (store)
    for (int i = 0; i < ENF_NUM_STORE(m.H); ++i)
      if (!store[i]) return ENF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (det) {
    const size_t pb = enf_det_part_bytes(m, false);
    if (scratch_bytes < pb + (dx ? enf_det_dx_bytes(m) : 0)) return ENF_EWORKSPACE;
    return enf_launch_pair_bwd(m, enf_layout(m), (const char*)packed, x, x_bstride, lt, lse, dybar, delta, dlt, store, EnfFoldBwd{}, dx, st,
                               (float*)scratch, dx ? reinterpret_cast<float*>((char*)scratch + pb) : nullptr);
  }
  if (hipMemsetAsync(dlt, 0, enf_lt_bytes(m), st) != hipSuccess) return ENF_ELAUNCH;
  return enf_launch_pair_bwd(m, enf_layout(m), (const char*)packed, x, x_bstride, lt, lse, dybar, delta, dlt, store, EnfFoldBwd{}, dx, st);
}

// ---- weight gradients of the per-pair chain: K3 (STORE) -> K4, chunked over signals (enf_xtd.hip)
extern "C" size_t enf_backward_weights_scratch_bytes(const EnfDesc* d, int chunk_signals) {
  if (enf_check_desc(d) != ENF_OK || chunk_signals < 1 || chunk_signals > d->B) return 0;
  return enf_wgrad_scratch_bytes(enf_dims(d), chunk_signals);
}

extern "C" int enf_backward_weights(const EnfDesc* d, const float* x, int64_t x_bstride, const float* lt, const void* packed,
                                    const float* lse, const float* dybar, const float* delta, float* dlt,
                                    float* const* dpair, float* dx, void* scratch, size_t scratch_bytes, void* stream) {
  return enf_backward_weights_ex(d, x, x_bstride, lt, packed, lse, dybar, delta, dlt, dpair, dx, scratch, scratch_bytes, 0u, stream);
}

// scratch with flags: [the plain scratch | K3's partial rows | with ENF_BWD_QUERY_GRAD a chunk's shares of d x]
static size_t wgrad_scratch_ex(const EnfDims& m, int cb, unsigned flags) {
  size_t n = enf_wgrad_scratch_bytes(m, cb);
  if (flags & ENF_BWD_DETERMINISTIC) {
    n += enf_wgrad_det_part_bytes(m, cb);
    if (flags & ENF_BWD_QUERY_GRAD) n += enf_align(sizeof(float) * (size_t)cb * m.Z * m.N * m.dx);
  }
  return n;
}
extern "C" size_t enf_backward_weights_scratch_bytes_ex(const EnfDesc* d, int chunk_signals, unsigned flags) {
  if (enf_check_desc(d) != ENF_OK || chunk_signals < 1 || chunk_signals > d->B) return 0;
  if (flags & ~(ENF_BWD_DETERMINISTIC | ENF_BWD_QUERY_GRAD)) return 0;
  return wgrad_scratch_ex(enf_dims(d), chunk_signals, flags);
}

extern "C" int enf_backward_weights_ex(const EnfDesc* d, const float* x, int64_t x_bstride, const float* lt, const void* packed,
                                       const float* lse, const float* dybar, const float* delta, float* dlt,
                                       float* const* dpair, float* dx, void* scratch, size_t scratch_bytes, unsigned flags,
                                       void* stream) {
  int rc = enf_check_desc(d);
  if (rc) return rc;
  if (d->embedding == ENF_EMB_FFN) return ENF_EUNSUPPORTED;       // the ENF_P_* (composed) path: rff only; ffn trains through enf_backward_all
  if ((flags & ~ENF_BWD_DETERMINISTIC) || !x || !lt || !packed || !lse || !dybar || !delta || !dlt || !dpair || !scratch) return ENF_EINVAL;
  for (int i = 0; i < ENF_NUM_PAIR_TENSORS; ++i)
    if (i != ENF_P_COEFQ && i != ENF_P_COEFV && !dpair[i]) return ENF_EINVAL;
  const EnfDims m = enf_dims(d);
  const unsigned sflags = flags ? (ENF_BWD_DETERMINISTIC | (dx ? ENF_BWD_QUERY_GRAD : 0u)) : 0u;
  const int cb = enf_wgrad_chunk(m, scratch_bytes, [&](int n) { return wgrad_scratch_ex(m, n, sflags); });
  if (!cb) return ENF_EWORKSPACE;
  char* sc = (char*)scratch;
  float* part = sflags ? reinterpret_cast<float*>(sc + enf_wgrad_scratch_bytes(m, cb)) : nullptr;
  float* dxpart = sflags && dx ? reinterpret_cast<float*>(sc + enf_wgrad_scratch_bytes(m, cb) + enf_wgrad_det_part_bytes(m, cb)) : nullptr;
  return enf_launch_wgrad_chunks(m, enf_layout(m), (const char*)packed, cb, x, x_bstride, lt, lse, dybar, delta, dlt, dx, sc, dpair,
                                 (hipStream_t)stream, part, dxpart);
}
