"""What a fit observes: point values of the field, or cell averages of it (fitting/cells.py; include/enf_hip.h, "Grouped observations").

``Points(coords)`` and ``Cells(x, q, group, num)`` answer, each for its kind, the questions the inner loop and both trainers ask of
their data -- how many observations there are and how many query rows each owns, how a step's inputs are gathered, which call of the
decoder is its fit step, its evaluation and the loss of a decode, and how the frames of a roll-out are sampled -- so that the code
above the decoder has one body per step instead of one per kind.  The keyword a decoder call takes sampled weights by is chosen in
``fit_step`` / ``eval`` / ``loss_of_decode`` and nowhere else.  Where the two kinds truly differ, the difference lives here:
  - the loop's final loss without ``per_signal_loss`` is a decode plus the loss kernel on points, always nef.eval_cell_loss on cells;
  - the shared-latent hint of step 0 is given for every weight form on points, on cells only without per-value weights;
  - the forward sweep of meta_gradients differentiates nef.apply with autograd on points and runs the grouped fit step on cells.
``LinearObservations(x, op)`` -- any sparse linear operator on the decode (fitting/operators.py) -- answers the step and the final loss
for fit_linear_observations only; ``observed`` and the trainers refuse it.
``observed`` is the one parser of a public step's four keywords (weights, channel_weights, cells, cell_channel_weights): it refuses
what is not served and returns the observation value with the prepared LossWeights.
"""
import torch

from .. import _lib
from .inner_loop import FUSED_FIT_INPUTS, _gather_inputs, _pose, gather_signal_points, make_signal_masks, split_latent_grads
from .cells import _batched, _cell_inputs, check_cells, gather_cell_samples
from .weights import LossWeights, loop_kw

_NO_CHANNEL_WEIGHTS_ON_CELLS = ("cells= takes per-observation weights= (M,) / (B, M) or cell_channel_weights= (M, O) / (B, M, O); "
                                "channel_weights are not served on cells")


class _Observed:
    """What the two kinds share: the keyword of sampled weights, and the loss of the decode at step ``s``'s sample."""

    def _weight_kw(self, ws, channel, always=False):
        return {self.WEIGHT_KW[bool(channel)]: ws} if ws is not None or always else {}

    def decode_loss(self, nef, params, img, masks, s, lat, weights, mse):
        xs, qs, ys, ws = self.sampled(img, masks, s, weights)                      # pde_trainer.py:193-197
        out = nef.apply(params, xs, _pose(lat, nef.cross_attn_invariant.num_z_ori_dims), lat["a"], lat.get("gaussian_window"))
        return self.loss_of_decode(nef, out, ys, qs, ws, mse)


class Points(_Observed):
    """Values of the field at the N grid points ``coords`` (N, dx): one query row per observation."""
    rows, STEP, WEIGHT_KW = 1, "mse_value_and_latent_grads", ("weight", "channel_weight")

    def __init__(self, coords):
        self.x, self.num = coords, coords.shape[0]

    def num_sampled(self, max_points):
        return max_points

    def hints(self, channel):
        return True

    def step_kw(self, lw):
        """The keywords a public step takes this observation and its prepared weights by."""
        return loop_kw(lw)

    def loop_args(self, img, masks, lw, decode_free=False):
        """What inner_loop takes after the learning rates, and by keyword, to fit these points with the prepared weights ``lw``;
        ``decode_free``: its last loss is to come from enf_eval_loss."""
        return (self.x, img, masks), dict(loop_kw(lw), **({"per_signal_loss": True} if decode_free else {}))

    def gather(self, latents0, img, masks, w, channel):
        lat, xs_all, ys_all, losses, ws_all = _gather_inputs(latents0, self.x, img, masks, w, channel)
        return lat, xs_all, None, ys_all, losses, ws_all

    def step_inputs(self, xs_all, qs_all, ws_all, s, B, per_signal):
        return xs_all[s] if per_signal else xs_all[s][None].expand(B, -1, -1), None, None if ws_all is None else ws_all[s]

    def sampled(self, img, masks, s, weights, copies=1):
        """The points of step ``s``: (xs (copies * B, N_s, dx), None, ys (B, N_s, O), weights (B, N_s) or None).  Shared masks (N_s, S+1)
        give the reference's gather (pde_trainer.py:193-197) with a stride-0 batch; per-signal masks (B, N_s, S+1) give every signal its
        own points and always weights (0 where the sampler padded with -1; gather_signal_points).  Per-channel ``weights`` (B, N, O) come
        back as (B, N_s, O); weighted_mse tells the two apart by their rank."""
        if masks.dim() == 2:
            m = masks[:, s]
            return self.x[m][None].expand(copies * img.shape[0], -1, -1), None, img[:, m], (None if weights is None else weights[:, m])
        xs, ys, ws = gather_signal_points(self.x, img, masks[:, :, s:s + 1], weights)
        return (xs[0] if copies == 1 else xs[0].repeat(copies, 1, 1)), None, ys[0].to(img.dtype), ws[0]

    def fit_step(self, nef, params, xs, qs, p, a, window, ys, ws, channel, always=False, **kw):
        return nef.mse_value_and_latent_grads(params, xs, p, a, window, ys, **kw, **self._weight_kw(ws, channel, always))

    def eval(self, nef, params, part, n, p, a, window, ys, ws, channel):
        """(loss_b or None, err (n, |part|)) of ``n`` signals on the slice ``part`` of the grid, without a decode (nef.eval_loss)."""
        return nef.eval_loss(params, self.x[part][None].expand(n, -1, -1), p, a, window, ys, per_signal=False, **self._weight_kw(ws, channel))

    def loss_of_decode(self, nef, out, ys, qs, ws, mse):
        """``mse``: the calling module's weighted_mse (fitting/weights.py), formed only where there are weights."""
        return ((out - ys) ** 2).mean() if ws is None else mse(out, ys, ws)         # pde_trainer.py:185

    def final_loss(self, nef, params, xs, qs, p, a, window, ys, ws, channel, loss_out, per_signal_loss):
        """The loop's loss on the last mask, added to ``loss_out``: enf_eval_loss with ``per_signal_loss`` (returns loss_b), else the
        reference's decode (pde_trainer.py:225-235) and the loss kernel of the weight form (returns None)."""
        if per_signal_loss:
            return nef.eval_loss(params, xs, p, a, window, ys, loss_out=loss_out, **self._weight_kw(ws, channel, True))[0]
        with torch.no_grad():
            out = nef.apply(params, xs, p, a, window).float().contiguous()
            if out.shape != ys.shape:
                raise AssertionError(f"targets have shape {tuple(ys.shape)}, expected {tuple(out.shape)}")
            lib, n, loss = _lib.load(), out.numel(), loss_out.data_ptr()
            if ws is None:
                fn, args = lib.enf_mse_value_grad, (n, 1.0, None, loss)
            elif channel:
                fn, args = lib.enf_mse_value_grad_cw, (ws.data_ptr(), n, 1.0, None, loss, None, 0, 0)
            else:
                fn, args = lib.enf_mse_value_grad_w, (ws.data_ptr(), n, out.shape[-1], 1.0, None, loss, None, 0, 0)
            _lib.launch(out.device, fn, out.data_ptr(), ys.data_ptr(), *args, _lib.stream(out.device))

    def latent_grads(self, nef, params, img, masks, s, lat, keys, weights, mse):
        """d loss_s / d lat[keys] of meta_gradients' forward sweep: autograd through nef.apply."""
        leaves = {k: lat[k].detach().requires_grad_(True) for k in lat}
        g = torch.autograd.grad(self.decode_loss(nef, params, img, masks, s, leaves, weights, mse), [leaves[k] for k in keys], allow_unused=True)
        return {k: (torch.zeros_like(lat[k]) if gk is None else gk) for k, gk in zip(keys, g)}

    def subset(self, img, mask, lw, max_points, rng, per_signal):
        """What a step of the auto-decoder trainer fits on (nonmaml_pde_trainer.py:311-335): (targets (B, n, O), xs (B, n, dx), None,
        the LossWeights of these points or None) -- ``mask`` first (:321-323), then at most ``max_points`` points, one subset for the
        batch drawn from ``rng`` (a stride-0 xs, :326-335), or with ``per_signal`` and weights every signal's own observed points (the
        sampler's -1 padding has weight 0) with the weights rescaled for that draw.  With channel weights a point counts as observed
        where any of its channels is."""
        coords = self.x
        if mask is not None:
            img, coords, lw = img[:, mask], coords[mask], lw and lw.points(mask)
        if per_signal and lw is not None:
            m = make_signal_masks(lw.support(), min(max_points, coords.shape[0]), 0, generator=rng, device=coords.device)
            # (the factor n_b / N of a draw from the observed points: the loss keeps the scale of the shared subset's)
            xs, img, ws = (t[0] for t in gather_signal_points(coords, img, m, lw.drawn_on(m).w))
            return img, xs, None, LossWeights(ws, lw.channel)
        if max_points < coords.shape[0]:
            sub = torch.randperm(coords.shape[0], generator=rng)[:max_points].to(coords.device)
            img, coords, lw = img[:, sub], coords[sub], lw and lw.points(sub)
        return img, coords[None].expand(img.shape[0], -1, -1), None, lw

    def sample_frames(self, traj, point_masks=None, weights=None):
        """Queries and targets of the B T signal-frames: ``traj`` (B, T, N, O), ``point_masks`` (T, n_s) long or None for the full grid.
        Returns xs (B T, n, dx), None, ys (B T, n, O), signal-major like the flattened roll-out, and the gather of ``weights`` (B, T, N)
        -> ws (B T, n), per-channel (B, T, N, O) -> (B T, n, O), or None."""
        B, T, N, O = traj.shape
        if point_masks is None:
            return (self.x[None].expand(B * T, -1, -1), None, traj.reshape(B * T, N, O),
                    None if weights is None else weights.reshape(B * T, N, *weights.shape[3:]))
        n_s = point_masks.shape[1]
        xs = self.x[point_masks][None].expand(B, -1, -1, -1).reshape(B * T, n_s, -1)
        return xs, None, *_gather_frames(traj, point_masks, weights)


def _gather_frames(traj, masks, weights):
    """ys (B T, n, O) and ws -- None, (B T, n) or (B T, n, O) -- of ``traj`` (B, T, num, O) at the per-frame index sets ``masks`` (T, n)."""
    B, T, _, O = traj.shape
    n = masks.shape[1]
    ys = torch.gather(traj, 2, masks[None, :, :, None].expand(B, -1, -1, O)).reshape(B * T, n, O)
    if weights is None:
        return ys, None
    if weights.dim() == 4:
        return ys, torch.gather(weights, 2, masks[None, :, :, None].expand(B, -1, -1, O)).reshape(B * T, n, O)
    return ys, torch.gather(weights, 2, masks[None].expand(B, -1, -1)).reshape(B * T, n)


class Cells(_Observed):
    """Averages of the field over ``num`` cells: quadrature points ``x`` (num * group, dx) and factors ``q`` (num * group,) or None for
    the plain mean, ``group`` query rows per observation.  The constructor is where ``cells=`` is validated (check_cells)."""
    STEP, WEIGHT_KW = "mse_value_and_cell_grads", ("obs_weight", "obs_channel_weight")

    def __init__(self, x, q, group, num):
        self.x, self.q, self.rows = check_cells((x, q, group), num)
        self.num = num

    def num_sampled(self, max_points):
        return max(1, max_points // self.rows)

    def hints(self, channel):
        return not channel

    def step_kw(self, lw):
        return {"cells": (self.x, self.q, self.rows), **({} if lw is None else {"cell_channel_weights" if lw.channel else "weights": lw.w})}

    def loop_args(self, img, masks, lw, decode_free=False):
        """What inner_loop_cells takes after the learning rates, and by keyword (its last loss never decodes)."""
        return (self.x, self.q, self.rows, img, masks), {} if lw is None else {"obs_channel_weight" if lw.channel else "obs_weights": lw.w}

    def gather(self, latents0, img, masks, w, channel):
        """One launch (enf_fit_inputs_g / _gc), or gather_cell_samples where the tensors are not what the kernel takes."""
        fused = _cell_inputs(latents0, self.x, self.q, self.rows, img, masks, w, channel) if FUSED_FIT_INPUTS else None
        if fused is not None:
            return fused
        dev = img.device
        lat = {k: v.detach().repeat_interleave(img.shape[0], dim=0) for k, v in latents0.items()}
        losses = torch.zeros(masks.shape[-1], device=dev, dtype=torch.float32)
        xs_all, qs_all, ys_all, ws_all = gather_cell_samples(self.x.to(dev), None if self.q is None else self.q.to(dev), self.rows, img,
                                                             masks.to(dev), **self._weight_kw(w, channel, True))
        return lat, xs_all, qs_all, ys_all, losses, ws_all

    def step_inputs(self, xs_all, qs_all, ws_all, s, B, per_signal):
        xs, qs = xs_all[s], None if qs_all is None else qs_all[s]
        if not per_signal:
            xs, qs = _batched(xs, qs, B)
        return xs, qs, None if ws_all is None else ws_all[s]

    def sampled(self, img, masks, s, weights, copies=1):
        """The cells of step ``s`` (masks hold CELL indices): (xs (copies * B, Ms G, dx), qs (B, Ms G) or None, ys (B, Ms, O), ws (B, Ms)
        or None) -- gather_cell_samples on column s, shared masks as a stride-0 batch; per-signal masks give every signal its own cells
        and always weights (0 where the sampler padded with -1).  Per-value ``weights`` (B, M, O) come back as (B, Ms, O)."""
        B = img.shape[0]
        xs, qs, ys, ws = gather_cell_samples(self.x, self.q, self.rows, img, masks[..., s:s + 1],
                                             **self._weight_kw(weights, weights is not None and weights.dim() == 3))
        xs, qs = xs[0], None if qs is None else qs[0]
        if masks.dim() == 2:
            xs, qs = _batched(xs, qs, B)
            xs = xs if copies == 1 else xs[:1].expand(copies * B, -1, -1)
        elif copies > 1:
            xs = xs.repeat(copies, 1, 1)
        return xs, qs, ys[0].to(img.dtype), None if ws is None else ws[0]

    def fit_step(self, nef, params, xs, qs, p, a, window, ys, ws, channel, always=False, **kw):
        return nef.mse_value_and_cell_grads(params, xs, p, a, window, ys, self.rows, qweight=qs, **kw, **self._weight_kw(ws, channel, always))

    def eval(self, nef, params, part, n, p, a, window, ys, ws, channel):
        """(loss_b or None, err_g (n, |part|)) of ``n`` signals on the cells ``part``, without a decode (nef.eval_cell_loss)."""
        rows = slice(part.start * self.rows, part.stop * self.rows)
        xs, qs = _batched(self.x[rows], None if self.q is None else self.q[rows], n)
        return nef.eval_cell_loss(params, xs, p, a, window, ys, self.rows, qweight=qs, per_signal=False, **self._weight_kw(ws, channel))

    def loss_of_decode(self, nef, out, ys, qs, ws, mse=None):
        """The grouped loss of a decode at the cells' quadrature rows (nef.cell_mse: one kernel).  Sampled weights (B, Ms) are per
        observation, (B, Ms, O) per value: on cells the two kinds differ by rank."""
        return nef.cell_mse(out, ys, self.rows, qs, **self._weight_kw(ws, ws is not None and ws.dim() == 3))

    def fused_loss(self, nef, params, xs, qs, p, a, window, ys, ws):
        """The same loss without a decode (nef.cell_fit_loss: one grouped fit step whose latent gradients the backward scales)."""
        return nef.cell_fit_loss(params, xs, p, a, window, ys, self.rows, qweight=qs, **self._weight_kw(ws, ws is not None and ws.dim() == 3))

    def final_loss(self, nef, params, xs, qs, p, a, window, ys, ws, channel, loss_out, per_signal_loss):
        return nef.eval_cell_loss(params, xs, p, a, window, ys, self.rows, qweight=qs, loss_out=loss_out, per_signal=per_signal_loss,
                                  **self._weight_kw(ws, channel, True))[0]

    def latent_grads(self, nef, params, img, masks, s, lat, keys, weights, mse=None):
        """d loss_s / d lat[keys] of meta_gradients' forward sweep: ONE grouped fit step (no decode, no autograd graph), whose forward
        pair kernel records the relu masks when the caller has set them to "write"."""
        xs, qs, ys, ws = self.sampled(img, masks, s, weights)
        _, dp, da, dsig = self.fit_step(nef, params, xs, qs, _pose(lat, nef.cross_attn_invariant.num_z_ori_dims), lat["a"],
                                        lat.get("gaussian_window"), ys, ws, ws is not None and ws.dim() == 3)
        g = split_latent_grads(dp, da, dsig, lat["p_pos"].shape[-1])
        return {k: (torch.zeros_like(lat[k]) if g.get(k) is None else g[k].reshape(lat[k].shape)) for k in keys}

    def subset(self, img, mask, lw, max_points, rng, per_signal):
        """Points.subset on cell means ``img`` (B, M, O), ``mask`` and ``lw`` per observation: (targets (B, m, O), xs (B, m G, dx), qs
        (B, m G) or None, the LossWeights of these cells or None) -- at most num_sampled(max_points) cells, one subset for the batch (a
        stride-0 xs) or, with ``per_signal`` and weights, every signal's own observed cells with the weights rescaled for that draw.
        With weights per observed value a cell is observed where any of its values is."""
        x, q, G = self.x, self.q, self.rows
        B, M, O = img.shape
        pick = None
        if mask is not None:
            pick = torch.as_tensor(mask, device=img.device)
            pick = pick.nonzero().reshape(-1) if pick.dtype == torch.bool else pick.long()
        n = self.num_sampled(max_points)
        if per_signal and lw is not None:
            if pick is not None:
                keep = torch.zeros(M, dtype=torch.bool, device=img.device)
                keep[pick] = True
                lw = lw.keep(keep[None].expand(B, -1))
            m = make_signal_masks(lw.support(), min(n, M), 0, generator=rng, device=img.device)
            xs, qs, ys, ws = gather_cell_samples(x, q, G, img, m, **self._weight_kw(lw.drawn_on(m).w, lw.channel))
            return ys[0].to(img.dtype), xs[0], None if qs is None else qs[0], LossWeights(ws[0], lw.channel)
        if pick is None and n < M:
            pick = torch.arange(M, device=img.device)
        if pick is not None and n < pick.numel():
            pick = pick[torch.randperm(pick.numel(), generator=rng)[:n].to(pick.device)]
        if pick is not None:
            rows = (pick[:, None] * G + torch.arange(G, device=pick.device)).reshape(-1)
            img, x, q, lw = img[:, pick], x[rows], None if q is None else q[rows], lw and lw.points(pick)
        return img, *_batched(x, q, B), lw

    def sample_frames(self, traj, cell_masks=None, weights=None):
        """sample_frames on cell averages: ``traj`` (B, T, M, O) cell means, ``cell_masks`` (T, m_s) long CELL indices or None for all M.
        Returns xs (B T, m G, dx), qs (B T, m G) or None, ys (B T, m, O) and ws -- None, (B T, m) from ``weights`` (B, T, M), or
        (B T, m, O) from per-value weights (B, T, M, O); row i G + k of a frame's set is row c G + k of its cell c, signal-major like
        the flattened roll-out."""
        x, q, G = self.x, self.q, self.rows
        B, T, M, O = traj.shape
        if cell_masks is None:
            xs, qs = _batched(x, q, B * T)
            return xs, qs, traj.reshape(B * T, M, O), None if weights is None else weights.reshape(B * T, M, *weights.shape[3:])
        m_s = cell_masks.shape[1]
        rows = (cell_masks[..., None] * G + torch.arange(G, device=cell_masks.device)).reshape(T, m_s * G)
        xs = x[rows][None].expand(B, -1, -1, -1).reshape(B * T, m_s * G, -1)
        qs = None if q is None else q[rows][None].expand(B, -1, -1).reshape(B * T, m_s * G)
        return xs, qs, *_gather_frames(traj, cell_masks, weights)


class LinearObservations(_Observed):
    """Linear functionals of the field given by a sparse operator (fitting/operators.py: SparseObservations) on the query points ``x``
    (N, dx): observation m owns the entries of row m, of any number, shared or not.  It answers what fit_linear_observations asks -- the
    step and the final loss -- and nothing else yet: ``observed`` and the trainers' steps refuse it, there is no sampling of rows.  (The
    Levenberg-Marquardt fit, gauss_newton.lm_fit_linear_observations, takes x and the operator themselves.)"""
    STEP, WEIGHT_KW = "mse_value_and_operator_grads", ("obs_weight", "obs_channel_weight")
    REFUSAL = ("a linear observation operator is served by fitting.fit_linear_observations and fitting.lm_fit_linear_observations only: "
               "the trainers' steps and inner_loop sampling do not take it yet")

    def __init__(self, x, op):
        if x.dim() != 2 or x.shape[0] != op.N:
            raise ValueError(f"x must be (N, dx) = ({op.N}, dx) for this operator, got {tuple(x.shape)}")
        self.x, self.op, self.num = x, op, op.M

    def hints(self, channel):
        return False

    def fit_step(self, nef, params, xs, qs, p, a, window, ys, ws, channel, always=False, **kw):
        return nef.mse_value_and_operator_grads(params, xs, p, a, window, ys, self.op, **kw, **self._weight_kw(ws, channel, always))

    def final_loss(self, nef, params, xs, qs, p, a, window, ys, ws, channel, loss_out, per_signal_loss):
        return nef.eval_operator_loss(params, xs, p, a, window, ys, self.op, loss_out=loss_out, per_signal=per_signal_loss,
                                      **self._weight_kw(ws, channel, True))[0]


def cell_loss_weights(weights, cell_channel_weights, B, M, O, **kw):
    """LossWeights.build for data on cells: ``weights`` per observation, ``cell_channel_weights`` per observed value; both at once is
    a ValueError that names them."""
    if weights is not None and cell_channel_weights is not None:
        raise ValueError("pass weights= (one per observation) or cell_channel_weights= (one per observed value), not both")
    return LossWeights.build(weights, cell_channel_weights, B, M, O, **kw)


def observed(coords, weights, channel_weights, cells, cell_channel_weights, B, num, O, T=None, normalize=True, frames=None, device=None,
             nef=None):
    """What every public step does first with its four keywords: (obs, lw), the observation value -- ``Points(coords)``, or ``Cells``
    of ``cells`` = (x (M G, dx), q (M G,) or None, group) checked against ``num`` = M -- and the prepared LossWeights over (B, num[, O])
    (``T``: (B, T, num[, O]); ``frames``: cut first; LossWeights.build) or None.  The refusals, in this order: on points,
    ``cell_channel_weights``; on cells ``channel_weights``, a decoder with self-attention layers (``nef``: the grouped calls are built
    for num_layers = 0), a group or a number of quadrature rows that is not served; then both weight kinds at once and wrong shapes."""
    if cells is None:
        if cell_channel_weights is not None:
            raise ValueError("cell_channel_weights= goes with cells=")
        lw = LossWeights.build(weights, channel_weights, B, num, O, T=T, normalize=normalize, device=device, frames=frames)
        return Points(coords), lw
    from .operators import SparseObservations        # (operators imports this module)
    if isinstance(cells, LinearObservations) or any(isinstance(c, SparseObservations) for c in (cells if isinstance(cells, (tuple, list)) else ())):
        raise NotImplementedError(LinearObservations.REFUSAL)
    if channel_weights is not None:
        raise ValueError(_NO_CHANNEL_WEIGHTS_ON_CELLS)
    if getattr(nef, "num_layers", 0) > 0:
        raise NotImplementedError("cells= is built for num_layers = 0 (the fused decoder)")
    return Cells(*cells, num), cell_loss_weights(weights, cell_channel_weights, B, num, O, T=T, normalize=normalize, device=device, frames=frames)
