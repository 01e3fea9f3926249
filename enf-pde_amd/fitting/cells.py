"""Fits against cell averages (include/enf_hip.h, "Grouped observations"; no counterpart in the reference).

Data on a coarse grid are mostly not point values: a finite-volume solver gives cell means, a reanalysis box means, a satellite a
footprint's weighted mean.  Such an observation is a fixed linear functional of the decoded field,
    obs[m] = sum_k q[m G + k] u(x[m G + k]),
a quadrature rule over G points of cell m.  ``cell_quadrature`` builds the points and factors, ``decode_cell_averages`` applies the
functional to a decode in torch ops, and ``fit_cell_averages`` runs the inner loop's update rule on the fused grouped step
(nef.mse_value_and_cell_grads: the group sums are formed in the tail's registers, no decode exists in memory).
``Cells`` is the observation value of this kind (inner_loop.py: _Observed).  ``inner_loop_cells`` is inner_loop on sampled cells -- the
same loop (inner_loop.py: _fit_loop) given a ``Cells`` value: one gather launch (enf_fit_inputs_g), the shared-latent hint at step 0 --
and what the trainers run with ``cells=``; ``fit_cell_averages`` chooses its inputs itself (all cells, or samples it gathers in torch
ops) and runs the same body on them (inner_loop.py: _fit_given).  ``check_cells`` and ``check_obs_weights`` are the one copy of the
argument checks.  ``gather_cell_samples`` and ``cell_mse_torch`` are the torch-op mirrors of the gather kernel and of the unfused
grouped loss (nef.cell_mse)."""
import numpy as np
import torch

from .. import _lib
from .inner_loop import _Observed, _batched, _fit_given, _fit_loop, _fresh, _gather_frames, _pose, make_signal_masks, split_latent_grads
from .inner_loop import _shared_kw      # noqa: F401  (tests/test_gpu_cells_train.py asks this module for the hint of the grouped step)
from .weights import LossWeights

GROUP_SIZES = (1, 2, 4, 8, 16)


def check_cells(cells, num_cells, x_wrong=None, q_wrong=None):
    """The one check of cells shared by the signals: (x (M G, dx), q (M G,) or None, group) with group a size the fused tail serves and
    M = ``num_cells``, the cells the data hold.  Returns (x, q, int(group)); ValueError otherwise, group first, then x, then q.
    ``x_wrong(x)`` / ``q_wrong(q)``: the words of a caller that names its arguments otherwise than ``cells=`` does."""
    x, q, G = cells[0], cells[1], int(cells[2])
    if G not in GROUP_SIZES:
        raise ValueError(f"group must be one of {GROUP_SIZES}, got {cells[2]}")
    if x.dim() != 2 or x.shape[0] != num_cells * G:
        raise ValueError(x_wrong(x) if x_wrong else f"cells hold {tuple(x.shape)} quadrature points, img {num_cells} cells of {G}")
    if q is not None and tuple(q.shape) != (x.shape[0],):
        raise ValueError(q_wrong(q) if q_wrong else f"cells hold {x.shape[0]} quadrature points and factors of shape {tuple(q.shape)}")
    return x, q, G


def _rule_1d(k, rule):
    """Nodes in (-1, 1) and weights that sum to 1 of a k-point rule on the reference interval."""
    if k < 1:
        raise ValueError(f"k must be >= 1, got {k}")
    if rule == "gauss":
        t, w = np.polynomial.legendre.leggauss(k)
        return t, w / 2.0
    if rule == "midpoint":
        return (2.0 * np.arange(k) + 1.0) / k - 1.0, np.full(k, 1.0 / k)
    raise ValueError(f"rule must be 'gauss' or 'midpoint', got {rule!r}")


def _edges(cells):
    """One fp64 edge array per axis: a TUPLE is the uniform box (lo, hi, shape), scalars or one value per axis; a LIST holds the edge
    arrays themselves."""
    if isinstance(cells, tuple):
        if len(cells) != 3:
            raise ValueError("a tuple of cells is (lo, hi, shape)")
        shape = np.atleast_1d(np.asarray(cells[2]))
        lo, hi = (np.broadcast_to(np.asarray(c, dtype=np.float64), shape.shape) for c in cells[:2])
        if shape.ndim != 1 or np.any(shape < 1) or np.any(shape != shape.astype(np.int64)) or not np.all(hi > lo):
            raise ValueError("(lo, hi, shape) needs hi > lo and whole cell counts >= 1")
        return [np.linspace(l, h, int(n) + 1) for l, h, n in zip(lo, hi, shape)]
    edges = [np.asarray(e, dtype=np.float64) for e in cells]
    for e in edges:
        if e.ndim != 1 or e.size < 2 or not np.all(np.diff(e) > 0):
            raise ValueError("every axis needs a 1-D array of at least two increasing edges")
    return edges


def cell_quadrature(cells, k, rule="gauss", kind="cartesian", dtype=torch.float32, device=None):
    """Quadrature points and factors for the mean over every cell of a tensor-product grid.

    cells : ``edges``, a LIST with one increasing 1-D edge array per axis, or a TUPLE ``(lo, hi, shape)`` for a uniform box (scalars
            or one value per axis).  The M = prod(cells per axis) cells are numbered in C order over the axes.
    k     : points per axis; G = k ** dx must be a group size the fused tail serves (1, 2, 4, 8, 16), else ValueError.
    rule  : "gauss" (tensor-product Gauss-Legendre, exact for polynomials of degree 2 k - 1 per axis) or "midpoint" (k equal
            sub-intervals per axis).
    kind  : "cartesian" -- the plain mean; "sphere" -- cells in (phi, theta), colatitude theta second: the factors carry the area
            element sin(theta) and are normalised per cell, so that obs is the mean over the cell's AREA.
    Returns (x (M * G, dx), q (M * G,)): cell m owns rows m G .. m G + G - 1, and q sums to 1 over every cell."""
    edges = _edges(cells)
    dx = len(edges)
    G = int(k) ** dx
    if G not in GROUP_SIZES:
        raise ValueError(f"k = {k} on {dx} axes gives groups of {G} points; the fused tail serves {GROUP_SIZES}")
    if kind not in ("cartesian", "sphere"):
        raise ValueError(f"kind must be 'cartesian' or 'sphere', got {kind!r}")
    if kind == "sphere" and dx != 2:
        raise ValueError("kind='sphere' needs two axes, (phi, theta)")
    t, w = _rule_1d(int(k), rule)
    nodes, facs = [], []
    for e in edges:                                                     # per axis: (cells, k) nodes, (cells, k) factors
        mid, half = 0.5 * (e[1:] + e[:-1]), 0.5 * (e[1:] - e[:-1])
        nodes.append(mid[:, None] + half[:, None] * t[None, :])
        facs.append(np.broadcast_to(w[None, :], nodes[-1].shape).copy())
    if kind == "sphere":
        facs[1] = facs[1] * np.sin(nodes[1])
        facs[1] = facs[1] / facs[1].sum(axis=1, keepdims=True)
    counts = [n.shape[0] for n in nodes]
    # (cells per axis ..., k per axis ...) -> (M, G, dx)
    grids = np.meshgrid(*[np.arange(c) for c in counts], *[np.arange(int(k))] * dx, indexing="ij")
    x = np.stack([nodes[ax][grids[ax], grids[dx + ax]] for ax in range(dx)], axis=-1)
    q = np.ones(x.shape[:-1])
    for ax in range(dx):
        q = q * facs[ax][grids[ax], grids[dx + ax]]
    M = int(np.prod(counts))
    return (torch.tensor(x.reshape(M * G, dx), dtype=dtype, device=device), torch.tensor(q.reshape(M * G), dtype=dtype, device=device))


@torch.no_grad()
def decode_cell_averages(nef, params, x, q, group, p, a, window):
    """obs (B, M, O) = sum_k q[m G + k] out[b, m G + k] of a decode at the quadrature points: the decode (nef.apply) and the group sum
    in torch ops -- a convenience without a kernel of its own.  x (N, dx) or (B, N, dx); q (N,), (B, N) or None for 1 / group."""
    B = p.shape[0]
    xb, qb = _batched(x, q, B)
    out = nef.apply(params, xb, p, a, window)
    N, O = out.shape[1], out.shape[2]
    if N % int(group):
        raise ValueError(f"{N} query points are not a multiple of group = {group}")
    w = torch.full((B, N), 1.0 / int(group), device=out.device, dtype=out.dtype) if qb is None else qb.to(out.dtype)
    return (out * w[..., None]).reshape(B, N // int(group), int(group), O).sum(dim=2)


def draw_cell_samples(num_cells, sample, steps, generator=None):
    """(steps + 1, sample) long: for every step and for the final loss a fresh set of `sample` distinct observations out of
    `num_cells`, by index (shared by the signals).  Drawn where the generator lives (the CPU without one)."""
    if not 1 <= int(sample) <= int(num_cells):
        raise ValueError(f"sample must be in [1, {num_cells}], got {sample}")
    dev = generator.device if generator is not None else torch.device("cpu")
    return torch.stack([torch.randperm(int(num_cells), generator=generator, device=dev)[:int(sample)] for _ in range(int(steps) + 1)])


def _one_weight_kind(what, obs_weight, obs_channel_weight, shape):
    """Both weight kinds at once is a ValueError; the per-value weights are (B, M, O)."""
    if obs_channel_weight is None:
        return
    if obs_weight is not None:
        raise ValueError(f"{what}: pass one weight per observation or obs_channel_weight (one per value), not both")
    if tuple(obs_channel_weight.shape) != tuple(shape):
        raise ValueError(f"obs_channel_weight has shape {tuple(obs_channel_weight.shape)}, expected {tuple(shape)}")


def check_obs_weights(what, obs_weight, obs_channel_weight, shape, named="obs_weight has"):
    """The one check of a fit's weights on observations of any kind, ``shape`` = (B, M, O): per observation (B, M), or per value
    (B, M, O), not both.  Returns (the weights to fit with or None, whether they are per value).  ``named``: the caller's own argument."""
    if obs_weight is not None and tuple(obs_weight.shape) != tuple(shape[:2]):
        raise ValueError(f"{named} shape {tuple(obs_weight.shape)}, expected {tuple(shape[:2])}")
    _one_weight_kind(what, obs_weight, obs_channel_weight, shape)
    per_value = obs_channel_weight is not None
    return (obs_channel_weight if per_value else obs_weight), per_value


def fit_cell_averages(nef, params, latents0, lrs, x, q, group, targets, steps, obs_weight=None, sample=None, generator=None,
                      optimize_gaussian_window=False, per_signal_loss=False, obs_channel_weight=None):
    """Fit per-signal latents to cell averages with `steps` steps of the inner loop's meta-SGD rule (inner_loop: meta_sgd_update on the
    gradient of the batch-mean loss times B, so that the signals are independent).

    latents0 : {'p_pos', 'a', 'gaussian_window'[, 'p_ori']} with leading dimension 1, as for inner_loop;  lrs: the same keys
    x, q     : the quadrature points (N, dx) and factors (N,) of the M = N / group cells (cell_quadrature), shared by the signals;
               q None is the plain mean, 1 / group
    targets  : (B, M, O) observed cell averages;  obs_weight: None or (B, M), finite and >= 0 -- an observation of weight 0 does not
               exist and its target may be NaN;  obs_channel_weight: None or (B, M, O), one weight per observed value in its place (both:
               ValueError), the zero-weight rule per value
    sample   : None (every step sees all M observations), an int (every step and the final loss draw a fresh set of that many
               observations, draw_cell_samples with ``generator``), or the index tensor (steps + 1, M_s) itself.  The points,
               factors, targets and weights of all steps are gathered once, in torch ops.
    Each step is one nef.mse_value_and_cell_grads; the final loss is nef.eval_cell_loss at the fitted latents (no decode).
    Returns (loss on the last set, fitted latents dict with leading dimension B), with ``per_signal_loss`` followed by loss_b
    (steps + 1, B) -- what inner_loop returns."""
    G, S = int(group), int(steps)
    B, M, O = targets.shape
    check_cells((x, q, group), M, q_wrong=lambda q: f"q has shape {tuple(q.shape)}, expected {(M * G,)}",
                x_wrong=lambda x: (f"x must be (M * group, dx), got {tuple(x.shape)} with group = {G}" if x.dim() != 2 or x.shape[0] % G else
                                   f"x holds {x.shape[0] // G} cells, targets {M}"))
    w, per_value = check_obs_weights("fit_cell_averages", obs_weight, obs_channel_weight, (B, M, O))
    dev = targets.device
    tg = targets.float()
    if sample is None:                                                   # the caller's tensors themselves, a stride-0 batch: no gather
        given = (*_batched(x.to(dev), None if q is None else q.to(dev), B), tg, w)
        inputs = lambda s: given
    else:
        idx = sample if torch.is_tensor(sample) else draw_cell_samples(M, sample, S, generator)
        if idx.dim() != 2 or idx.shape[0] != S + 1:
            raise ValueError(f"sample indices have shape {tuple(idx.shape)}, expected ({S + 1}, M_s)")
        idx = idx.to(device=dev, dtype=torch.long)
        rows = (idx[..., None] * G + torch.arange(G, device=dev)).reshape(S + 1, -1)       # the groups' query rows, in order
        xs_all = x.to(dev)[rows]                                                            # (S + 1, M_s G, dx)
        qs_all = q.to(dev)[rows] if q is not None else None
        ys_all = tg[:, idx].transpose(0, 1).contiguous()                                    # (S + 1, B, M_s, O)
        ws_all = w.to(dev)[:, idx].transpose(0, 1).contiguous() if w is not None else None
        inputs = lambda s: (*_batched(xs_all[s], None if qs_all is None else qs_all[s], B), ys_all[s], None if ws_all is None else ws_all[s])
    return _fit_given(nef, params, Cells.given(rows=G), latents0, lrs, inputs, B, S, dev, per_value, optimize_gaussian_window, per_signal_loss)


def gather_cell_samples(x, q, group, obs, masks, obs_weight=None, obs_channel_weight=None):
    """What enf_fit_inputs_g gathers, in torch ops: x (M G, dx) quadrature points, q (M G,) factors or None, obs (B, M, O), masks long
    cell indices (Ms, S1) shared by the signals or (B, Ms, S1) per signal, obs_weight (B, M) or None
    -> xs (S1, Ms G, dx) | (S1, B, Ms G, dx), qs alike without the last axis (None without q), ys (S1, B, Ms, O), ws (S1, B, Ms).
    Row i G + k of a sampled set is row m G + k of cell m.  An index outside [0, M) gives cell 0's points and factors, zero targets and
    weight 0; ws is None on shared masks without ``obs_weight`` and 1 / 0 on per-signal masks without it.
    ``obs_channel_weight`` (B, M, O) in place of ``obs_weight`` (enf_fit_inputs_gc): ws is (S1, B, Ms, O), O zeros for an index outside."""
    G = int(group)
    B, M, O = obs.shape
    _one_weight_kind("gather_cell_samples", obs_weight, obs_channel_weight, (B, M, O))
    S1 = masks.shape[-1]
    per_signal = masks.dim() == 3
    idx = masks.permute(2, 0, 1) if per_signal else masks.t()                        # (S1, B, Ms) | (S1, Ms)
    ok = (idx >= 0) & (idx < M)
    ic = torch.where(ok, idx, torch.zeros_like(idx))
    rows = (ic[..., None] * G + torch.arange(G, device=ic.device)).reshape(*ic.shape[:-1], -1)
    xs = x[rows].contiguous()
    qs = q[rows].contiguous() if q is not None else None
    icb, okb = (ic, ok) if per_signal else (ic[:, None].expand(-1, B, -1), ok[:, None].expand(-1, B, -1))
    ys = torch.gather(obs[None].expand(S1, -1, -1, -1), 2, icb[..., None].expand(-1, -1, -1, O)).float()
    ys = torch.where(okb[..., None], ys, torch.zeros_like(ys)).contiguous()
    if obs_channel_weight is not None:
        w = torch.gather(obs_channel_weight[None].expand(S1, -1, -1, -1), 2, icb[..., None].expand(-1, -1, -1, O)).float()
        return xs, qs, ys, torch.where(okb[..., None], w, torch.zeros_like(w)).contiguous()
    if obs_weight is None and not per_signal:
        return xs, qs, ys, None
    w = torch.gather(obs_weight[None].expand(S1, -1, -1), 2, icb).float() if obs_weight is not None else \
        torch.ones(icb.shape, device=obs.device, dtype=torch.float32)
    return xs, qs, ys, torch.where(okb, w, torch.zeros_like(w)).contiguous()


def cell_mse_torch(out, target, group, qweight=None, obs_weight=None, obs_channel_weight=None):
    """The grouped loss in torch ops, differentiable by autograd -- the mirror of nef.cell_mse (enf_mse_value_grad_g):
    sum_{b,m} w[b,m] sum_o (obs - target)^2 / (B M O) with obs = sum_k q out over each group; w == 0 is a select, so that
    observation's target may be NaN and its share of the loss and of d out is zero.
    ``obs_channel_weight`` (B, M, O) in place of ``obs_weight`` (both: ValueError): one weight, and one select, per observed value."""
    G = int(group)
    B, N, O = out.shape
    M = N // G
    _one_weight_kind("cell_mse_torch", obs_weight, obs_channel_weight, (B, M, O))
    q = torch.full((B, N), 1.0 / G, device=out.device, dtype=out.dtype) if qweight is None else qweight.to(out.dtype)
    w = torch.ones((B, M), device=out.device, dtype=out.dtype) if obs_weight is None else obs_weight.to(out.dtype)
    obs = (q[..., None] * out).reshape(B, M, G, O).sum(2)
    w = w[..., None] if obs_channel_weight is None else obs_channel_weight.to(out.dtype)
    live = (w > 0).expand(B, M, O)
    dd = torch.where(live, obs - torch.where(live, target.to(out.dtype), torch.zeros_like(obs)), torch.zeros_like(obs))
    return (w * dd * dd).sum() / (B * M * O)


def _cell_inputs(latents0, x, q, group, obs, masks, obs_weight, per_value=False):
    """enf_fit_inputs_g (include/enf_hip.h): (lat, xs_all, qs_all, ys_all, losses, ws_all) of inner_loop_cells in one launch, or None
    where the arguments are not what the kernel takes (fp32, contiguous, on one GPU, long masks, at most four latent components of
    leading dimension 1).  ``per_value``: obs_weight is (B, M, O) and the launch is enf_fit_inputs_gc, ws_all (S1, B, Ms, O)."""
    ts = list(latents0.values()) + [x, obs] + [t for t in (q, obs_weight) if t is not None]
    if not (obs.is_cuda and masks.is_cuda and masks.dtype == torch.int64 and masks.dim() in (2, 3) and masks.is_contiguous() and x.dim() == 2
            and obs.dim() == 3 and 1 <= len(latents0) <= _lib.ENF_SGD_MAX_SEGMENTS and masks.shape[0] > 0
            and all(t.dtype == torch.float32 and t.is_contiguous() and t.device == obs.device for t in ts)
            and all(v.dim() == 3 and v.shape[0] == 1 for v in latents0.values())
            and len({v.shape[1] for v in latents0.values()}) == 1):
        return None
    G = int(group)
    B, M, O = obs.shape
    Ms, S1 = masks.shape[-2:]
    per_signal = masks.dim() == 3
    if per_signal and masks.shape[0] != B:
        return None
    Z = next(iter(latents0.values())).shape[1]
    dev, dx = obs.device, x.shape[1]
    lead = (S1, B, Ms * G) if per_signal else (S1, Ms * G)
    lat = {k: torch.empty((B, Z, v.shape[2]), device=dev, dtype=torch.float32) for k, v in latents0.items()}
    xs = torch.empty(lead + (dx,), device=dev, dtype=torch.float32)
    qs = torch.empty(lead, device=dev, dtype=torch.float32) if q is not None else None
    ys = torch.empty((S1, B, Ms, O), device=dev, dtype=torch.float32)
    ws = torch.empty((S1, B, Ms) + ((O,) if per_value else ()), device=dev, dtype=torch.float32) if obs_weight is not None or per_signal else None
    losses = torch.empty(S1, device=dev, dtype=torch.float32)
    comps = (_lib.EnfFitComponent * _lib.ENF_SGD_MAX_SEGMENTS)()
    keep = []
    for i, (k, v) in enumerate(latents0.items()):
        src = v.detach()
        keep.append(src)
        comps[i] = _lib.EnfFitComponent(src.data_ptr(), lat[k].data_ptr(), v.shape[2], 0)
    fn = _lib.load().enf_fit_inputs_gc if per_value else _lib.load().enf_fit_inputs_g
    _lib.launch(dev, fn, len(latents0), comps, B, Z, M, Ms, S1, G, dx, O, _lib.ptr(x), _lib.ptr(q), _lib.ptr(obs),
                _lib.ptr(masks), _lib.ptr(xs), _lib.ptr(qs), _lib.ptr(ys), _lib.ptr(losses), _lib.ptr(obs_weight), _lib.ptr(ws),
                1 if per_signal else 0, _lib.stream(dev))
    return lat, xs, qs, ys, losses, ws


class Cells(_Observed):
    """Averages of the field over ``num`` cells: quadrature points ``x`` (num * group, dx) and factors ``q`` (num * group,) or None for
    the plain mean, ``rows`` = group query rows per observation.  The constructor is where ``cells=`` is validated (check_cells).
    Where it differs from points: the loop's final loss is always nef.eval_cell_loss, never a decode; the shared-latent hint of step 0
    is given only without per-value weights; meta_gradients' forward sweep runs the grouped fit step instead of autograd."""
    WEIGHT_KW = ("obs_weight", "obs_channel_weight")
    STEP, EVAL, PRODUCT = "mse_value_and_cell_grads", "eval_cell_loss", "gn_cell_product"

    def __init__(self, x, q, group, num):
        self.x, self.q, self.rows = check_cells((x, q, group), num)
        self.num = num

    def _call(self, nef, name, params, xs, qs, p, a, window, *ys, **kw):
        return getattr(nef, name)(params, xs, p, a, window, *ys, self.rows, qweight=qs, **kw)

    def num_sampled(self, max_points):
        return max(1, max_points // self.rows)

    def hints(self, channel):
        return not channel

    def step_kw(self, lw):
        return {"cells": (self.x, self.q, self.rows), **({} if lw is None else {"cell_channel_weights" if lw.channel else "weights": lw.w})}

    def loop_args(self, img, masks, lw, decode_free=False):
        """What inner_loop_cells takes after the learning rates, and by keyword (its last loss never decodes)."""
        return (self.x, self.q, self.rows, img, masks), {} if lw is None else {"obs_channel_weight" if lw.channel else "obs_weights": lw.w}

    def gather(self, latents0, img, masks, w, channel, fused_launch):
        """One launch (enf_fit_inputs_g / _gc), or gather_cell_samples where the tensors are not what the kernel takes or without
        ``fused_launch``, the loop's reading of inner_loop.FUSED_FIT_INPUTS: one switch for points and cells."""
        fused = _cell_inputs(latents0, self.x, self.q, self.rows, img, masks, w, channel) if fused_launch else None
        if fused is not None:
            return fused
        dev = img.device
        lat, losses = _fresh(latents0, img.shape[0], masks.shape[-1], dev)
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


def inner_loop_cells(nef, nef_params, latents0, lrs, x, q, group, targets, masks, obs_weights=None, optimize_gaussian_window=False,
                     noise_pos=0.0, generator=None, normalize_weights=False, per_signal_loss=False, obs_channel_weight=None):
    """inner_loop on cell averages: fit per-signal latents with S steps of meta-SGD, every step against a sampled set of cells.

    x, q     : the quadrature points (M G, dx) and factors (M G,) of the M cells (cell_quadrature), shared by the signals; q None is
               the plain mean, 1 / group
    targets  : (B, M, O) observed cell averages;  obs_weights: None or (B, M), finite and >= 0, taken as they are
    masks    : long CELL indices, (Ms, S + 1) shared by the signals or (B, Ms, S + 1) per signal; with per-signal masks an index outside
               [0, M) -- a sampler's padding -- has weight 0 and does not exist
    The sampled points, factors, targets and weights of all steps, the signals' copies of the latent initialisation and the zeroed loss
    accumulators come from ONE launch (enf_fit_inputs_g), or from gather_cell_samples where the tensors are not what the kernel takes.
    Each step is one nef.mse_value_and_cell_grads -- step 0 with the shared-latent hint under the conditions of inner_loop (shared masks,
    no pose noise, not deterministic, a decoder that knows the keyword) -- and the final loss is nef.eval_cell_loss, without a decode.
    obs_channel_weight : None or (B, M, O), one weight per observed value in place of obs_weights (both: ValueError); the gather is
               enf_fit_inputs_gc, every step enf_fit_step_gc and runs unshared (no shared-latent hint at step 0)
    normalize_weights, noise_pos, optimize_gaussian_window, per_signal_loss and the return values are inner_loop's."""
    G = int(group)
    B, M, O = targets.shape
    check_cells((x, q, group), M, x_wrong=lambda x: f"x must be (M * group, dx) = ({M * G}, dx), got {tuple(x.shape)}",
                q_wrong=lambda q: f"q has shape {tuple(q.shape)}, expected {(M * G,)}")
    w, per_value = check_obs_weights("inner_loop_cells", obs_weights, obs_channel_weight, (B, M, O), named="obs_weights have")
    if masks.dim() not in (2, 3) or (masks.dim() == 3 and masks.shape[0] != B):
        raise ValueError(f"masks have shape {tuple(masks.shape)}, expected (Ms, S + 1) or ({B}, Ms, S + 1)")
    w = w.to(device=targets.device, dtype=torch.float32).contiguous() if w is not None else None
    return _fit_loop(nef, nef_params, Cells.given(x=x, q=q, rows=G, num=M), latents0, lrs, targets, masks, w, per_value,
                     optimize_gaussian_window, noise_pos, generator, normalize_weights, per_signal_loss)
