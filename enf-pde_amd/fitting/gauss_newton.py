"""Second-order fits of the latents to observations: a batched conjugate-gradient solve on the native Gauss-Newton product and a
Levenberg-Marquardt loop on top of it.

  cg_solve(matvec, rhs, lam, iters)   (G_b + lam_b I) x_b = rhs_b for B independent systems, on enf_cg_update (include/enf_hip.h):
                                      one launch per iteration beside the product, per-signal alpha / beta, frozen signals
  lm_fit_latents(nef, ...)            per signal: gradient and loss from one fit step, a damped Gauss-Newton step by cg_solve on
                                      EquivariantCrossAttentionNeF.gn_product, accept where the signal's loss fell
  lm_fit_cell_averages(nef, ...)      the same loop against cell averages (grouped observations): the grouped fit step, the grouped
                                      product EquivariantCrossAttentionNeF.gn_cell_product, the grouped evaluation
  lm_fit_linear_observations(nef, ...)  the same loop against a sparse linear observation operator (fitting/operators.py): the operator
                                      fit step, the product EquivariantCrossAttentionNeF.gn_operator_product, the operator evaluation

The loss is a sum over signals and the latents of different signals do not interact, so the Gauss-Newton matrix is block diagonal:
every quantity below (damping, step length, acceptance) is per signal, and nothing in a loop iteration reads a value back to the host.
The three fits are one loop, ``_lm_loop``, on the calls half of an observation kind (inner_loop.py: _Observed); the public functions
only check and batch their arguments and name the kind.
"""
import torch

from .. import _lib
from .inner_loop import Points, _batched
from .cells import Cells
from .operators import LinearObservations, check_operator

__all__ = ["cg_solve", "lm_fit_latents", "lm_fit_cell_averages", "lm_fit_linear_observations"]


def _cg_update(segs, B, Z, lam, rho, q=None):
    """One enf_cg_update launch on the segments ``segs`` = [(x, r, d)], with ``q`` = the matching products or None (INIT)."""
    dev = rho.device
    if not rho.is_cuda:
        raise _lib.EnfError("cg_solve needs CUDA/HIP tensors: there is no CPU path")
    arr = (_lib.EnfCgSegment * _lib.ENF_CG_MAX_SEGMENTS)()
    for k, (x, r, d) in enumerate(segs):
        arr[k].x, arr[k].r, arr[k].d = x.data_ptr(), r.data_ptr(), d.data_ptr()
        arr[k].q = q[k].data_ptr() if q is not None else None
        arr[k].width = x.shape[2]
    _lib.launch(dev, _lib.load().enf_cg_update, len(segs), arr, B, Z, _lib.ptr(lam), _lib.ptr(rho), _lib.stream(dev))


@torch.no_grad()
def cg_solve(matvec, rhs, lam, iters):
    """``iters`` conjugate-gradient iterations from x = 0 on (G_b + lam_b I) x_b = rhs_b, b = 0 .. B - 1, in one batch.
    ``rhs``: a tuple of one to three float32 (B, Z, width) device tensors -- the components of the vectors; ``matvec``: a callable that
    takes such a tuple d and returns G d in the same shapes (undamped; symmetric positive semi-definite per signal); ``lam``: (B,)
    damping, or None.  Returns the tuple x.  A signal whose residual is zero, or whose curvature d . (G + lam) d is not a finite
    positive number, stops moving and leaves the others alone.  Same inputs and a reproducible ``matvec`` give the same bits."""
    if not 1 <= len(rhs) <= _lib.ENF_CG_MAX_SEGMENTS:
        raise ValueError(f"cg_solve takes one to {_lib.ENF_CG_MAX_SEGMENTS} components, got {len(rhs)}")
    B, Z = rhs[0].shape[:2]
    for t in rhs:
        if t.dim() != 3 or tuple(t.shape[:2]) != (B, Z) or t.dtype != torch.float32:
            raise ValueError("cg_solve: every component must be a float32 (B, Z, width) tensor with the same B and Z")
    dev = rhs[0].device
    lam_ = None if lam is None else lam.to(device=dev, dtype=torch.float32).contiguous()
    if lam_ is not None and tuple(lam_.shape) != (B,):
        raise ValueError(f"lam has shape {tuple(lam_.shape)}, expected {(B,)}")
    segs = [(torch.empty_like(t, memory_format=torch.contiguous_format), t.clone(memory_format=torch.contiguous_format),
             torch.empty_like(t, memory_format=torch.contiguous_format)) for t in rhs]
    rho = torch.empty((B,), device=dev, dtype=torch.float32)
    _cg_update(segs, B, Z, lam_, rho)
    for _ in range(int(iters)):
        q = matvec(tuple(d for _, _, d in segs))
        if len(q) != len(segs):
            raise ValueError("matvec must return as many components as it was given")
        q = [qi.float().contiguous() for qi in q]
        _cg_update(segs, B, Z, lam_, rho, q)
    return tuple(x for x, _, _ in segs)


_COMPONENTS = ("p", "a", "window")


def _lm_loop(nef, params, obs, xs, qs, target, wkw, p, a, window, steps, cg_iters, damping, down, up, components):
    """The one copy of the Levenberg-Marquardt loop, on any kind of observation ``obs`` (inner_loop.py: _Observed; its calls half is
    all the loop needs): the batched query rows ``xs`` (B, N, dx) with the kind's factors ``qs`` or None, ``target`` and the weight
    keywords ``wkw`` (obs.weights_kw) go to three calls at the current latents ``cur`` = {"p", "a", "window"}:
      obs.fit_step    at gradient scale B with return_errors: the gradient and the per-signal losses
      obs.gn_product  at the same scale along v = {component: tensor}, with ``reuse`` the workspace tag behind the last call there
      obs.loss_b      the per-signal losses at a trial point
    The buffer is reserved first, with what the kind's product needs beside the sizes (obs.reserve_kw: the operator).
    Returns what lm_fit_latents documents."""
    comps = tuple(components)
    if not comps or any(c not in _COMPONENTS for c in comps) or len(set(comps)) != len(comps):
        raise ValueError(f"components must be a non-empty subset of {_COMPONENTS}, got {components}")
    if "window" in comps and window is None:
        raise ValueError("components names the window, but the model has none")
    comps = tuple(c for c in _COMPONENTS if c in comps)
    B, Z = p.shape[0], p.shape[1]
    dev = p.device
    cur = {"p": p.detach().float().contiguous(), "a": a.detach().float().contiguous(),
           "window": None if window is None else window.detach().float().reshape(B, Z, 1).contiguous()}
    at = lambda lat: (nef, params, xs, qs, lat["p"], lat["a"], lat["window"])
    lam = torch.full((B,), float(damping), device=dev, dtype=torch.float32)
    loss_b = torch.empty((int(steps) + 1, B), device=dev, dtype=torch.float32)
    accepted = torch.zeros((int(steps), B), device=dev, dtype=torch.bool)
    nef.gn_reserve(B, xs.shape[1], Z, dev, **obs.reserve_kw())      # the fit step below must already run on the buffer the products reuse
    last = None
    for k in range(int(steps)):
        res = obs.fit_step(*at(cur), target, None, False, grad_scale=float(B), return_errors=True, **wkw)
        grads, lb = dict(zip(_COMPONENTS, res[1:4])), res[5]
        loss_b[k] = lb
        tag = [nef.workspace_tag(dev)]

        def matvec(d, tag=tag):
            v = dict(zip(comps, d))
            out = obs.gn_product(*at(cur), vp=v.get("p"), va=v.get("a"), vwindow=v.get("window"), grad_scale=float(B), reuse=tag[0], **wkw)
            tag[0] = nef.workspace_tag(dev)
            g = dict(zip(_COMPONENTS, out))
            return tuple(g[c] for c in comps)

        delta = cg_solve(matvec, tuple(-grads[c] for c in comps), lam, cg_iters)
        trial = dict(cur)
        for c, dlt in zip(comps, delta):
            trial[c] = cur[c] + dlt
        lb_t = obs.loss_b(*at(trial), target, **wkw)
        acc = lb_t < lb                      # (a NaN trial loss is a rejection)
        for c in comps:
            cur[c] = torch.where(acc[:, None, None], trial[c], cur[c])
        lam = torch.where(acc, lam * down, lam * up)
        accepted[k] = acc
        last = torch.where(acc, lb_t, lb)
    if last is None:
        last = obs.loss_b(*at(cur), target, **wkw)
    loss_b[int(steps)] = last
    return (cur["p"], cur["a"], cur["window"]), loss_b, lam, accepted


@torch.no_grad()
def lm_fit_latents(nef, params, x, target, p, a, window, steps, cg_iters=8, damping=1e-2, down=1.0 / 3.0, up=4.0, components=("p", "a"),
                   weight=None, channel_weight=None):
    """Levenberg-Marquardt fit of the latents (p, a, window) of B signals to ``target`` (B, N, O) at the points ``x`` (B, N, dx).
    Per step: one ``nef.mse_value_and_latent_grads(return_errors=True, grad_scale=B)`` for the per-signal losses and the gradient;
    ``cg_iters`` products ``nef.gn_product`` at that point (the latent prologue reused) inside ``cg_solve`` with the per-signal damping;
    one ``nef.eval_loss`` at the trial point; then per signal: where the loss fell the trial point is accepted and the damping is
    multiplied by ``down``, elsewhere the old latents stay and it is multiplied by ``up``.  Selection is by torch.where: no host
    synchronisation inside the loop.
    ``components``: which of "p", "a", "window" move -- the block of the Gauss-Newton matrix that is solved with; the others are held.
    ``weight`` / ``channel_weight``: the loss weights of the fit step.
    Returns ((p, a, window), loss_b (steps + 1, B), damping (B,), accepted (steps, B) bool), all on the device; loss_b[k] is the loss
    before step k, loss_b[steps] the final one."""
    obs = Points.given()
    return _lm_loop(nef, params, obs, x, None, target, obs.weights_kw(weight, channel_weight), p, a, window, steps, cg_iters, damping, down,
                    up, components)


@torch.no_grad()
def lm_fit_cell_averages(nef, params, x, q, group, target, p, a, window, steps, cg_iters=8, damping=1e-2, down=1.0 / 3.0, up=4.0,
                         components=("p", "a"), obs_weight=None):
    """Levenberg-Marquardt fit of the latents of B signals to CELL AVERAGES (fitting/cells.py; include/enf_hip.h, "Grouped
    observations"): ``target`` (B, M, O) are observations obs[m] = sum_k q[m group + k] out[m group + k] over the ``group`` consecutive
    quadrature points of cell m.  ``x``: the points, (N, dx) shared by the signals or (B, N, dx), a stride-0 batch included; ``q``: the
    factors (N,), (B, N), or None for 1 / group (cell_quadrature gives both); ``obs_weight``: None or (B, M), an observation of weight 0
    does not exist.  An observation is linear in the decode, so the Gauss-Newton matrix is exact up to the residual's curvature.
    lm_fit_latents' loop on the grouped calls.  Per step: one ``nef.mse_value_and_cell_grads(return_errors=True, grad_scale=B)``;
    ``cg_iters`` products ``nef.gn_cell_product`` at that point (the latent prologue reused) inside ``cg_solve``; one
    ``nef.eval_cell_loss`` at the trial point; per-signal acceptance and damping by torch.where, no host synchronisation in the loop.
    The other arguments and the return values are lm_fit_latents'."""
    obs = Cells.given(rows=int(group))
    xb, qb = _batched(x, q, p.shape[0])
    return _lm_loop(nef, params, obs, xb, qb, target, obs.weights_kw(obs_weight), p, a, window, steps, cg_iters, damping, down, up, components)


@torch.no_grad()
def lm_fit_linear_observations(nef, params, x, op, target, p, a, window, steps, cg_iters=8, damping=1e-2, down=1.0 / 3.0, up=4.0,
                               components=("p", "a"), obs_weight=None, obs_channel_weight=None):
    """Levenberg-Marquardt fit of the latents of B signals to LINEAR OBSERVATIONS obs = A out of a sparse operator ``op``
    (fitting/operators.py: SparseObservations; include/enf_hip.h, "Sparse linear observations"), shared by the signals: ``target``
    (B, M, O), M = op.M.  ``x``: the operator's query points, (N, dx) shared by the signals or (B, N, dx), a stride-0 batch included,
    N = op.N; ``obs_weight``: None or (B, M), ``obs_channel_weight``: None or (B, M, O), one weight per observed value (both:
    ValueError) -- what has weight 0 does not exist.  An observation is linear in the decode, so the Gauss-Newton matrix is exact up
    to the residual's curvature.
    lm_fit_latents' loop on the operator calls.  Per step: one ``nef.mse_value_and_operator_grads(return_errors=True, grad_scale=B)``;
    ``cg_iters`` products ``nef.gn_operator_product`` at that point (the latent prologue reused) inside ``cg_solve``; one
    ``nef.eval_operator_loss`` at the trial point; per-signal acceptance and damping by torch.where, no host synchronisation in the loop.
    The other arguments and the return values are lm_fit_latents'."""
    B = p.shape[0]
    check_operator(x, op, B, target, "target has shape {shape}, expected ({B}, {M}, O)")
    obs = LinearObservations.given(op=op)
    return _lm_loop(nef, params, obs, _batched(x, None, B)[0], None, target, obs.weights_kw(obs_weight, obs_channel_weight), p, a, window,
                    steps, cg_iters, damping, down, up, components)
