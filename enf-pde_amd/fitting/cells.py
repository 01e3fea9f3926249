"""Fits against cell averages (include/enf_hip.h, "Grouped observations"; no counterpart in the reference).

Data on a coarse grid are mostly not point values: a finite-volume solver gives cell means, a reanalysis box means, a satellite a
footprint's weighted mean.  Such an observation is a fixed linear functional of the decoded field,
    obs[m] = sum_k q[m G + k] u(x[m G + k]),
a quadrature rule over G points of cell m.  ``cell_quadrature`` builds the points and factors, ``decode_cell_averages`` applies the
functional to a decode in torch ops, and ``fit_cell_averages`` runs the inner loop's update rule on the fused grouped step
(nef.mse_value_and_cell_grads: the group sums are formed in the tail's registers, no decode exists in memory).
``inner_loop_cells`` is inner_loop on sampled cells -- the same loop (inner_loop.py: _fit_loop) given a ``Cells`` value
(fitting/observations.py): one gather launch (enf_fit_inputs_g), the shared-latent hint at step 0 -- and what the trainers run with
``cells=``; ``fit_cell_averages`` keeps its own sampling and takes the step body from that loop (_sgd_step).  ``gather_cell_samples`` and
``cell_mse_torch`` are the torch-op mirrors of the gather kernel and of the unfused grouped loss (nef.cell_mse)."""
import numpy as np
import torch

from .. import _lib
from .inner_loop import _fit_loop, _pose, _sgd_step, _shared_kw      # (_shared_kw: re-exported)

GROUP_SIZES = (1, 2, 4, 8, 16)


def check_cells(cells, num_cells):
    """What every step takes as ``cells=``: (x (M G, dx), q (M G,) or None, group) with group a size the fused tail serves and
    M = ``num_cells``, the cells the data hold.  Returns (x, q, int(group)); ValueError otherwise."""
    if int(cells[2]) not in GROUP_SIZES:
        raise ValueError(f"group must be one of {GROUP_SIZES}, got {cells[2]}")
    if cells[0].dim() != 2 or cells[0].shape[0] != num_cells * int(cells[2]):
        raise ValueError(f"cells hold {tuple(cells[0].shape)} quadrature points, img {num_cells} cells of {int(cells[2])}")
    if cells[1] is not None and tuple(cells[1].shape) != (cells[0].shape[0],):
        raise ValueError(f"cells hold {cells[0].shape[0]} quadrature points and factors of shape {tuple(cells[1].shape)}")
    return cells[0], cells[1], int(cells[2])


def cell_weight_kw(ws, channel):
    """The keyword nef.mse_value_and_cell_grads, nef.eval_cell_loss, nef.cell_mse and nef.cell_fit_loss take sampled weights by."""
    return {} if ws is None else {"obs_channel_weight" if channel else "obs_weight": ws}


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


def _batched(x, q, B):
    """x (N, dx) or (B, N, dx) -> a batch (stride 0 where shared); q None, (N,) or (B, N) -> None or (B, N)."""
    xb = x[None].expand(B, -1, -1) if x.dim() == 2 else x
    qb = None if q is None else (q[None].expand(B, -1) if q.dim() == 1 else q)
    return xb, qb


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
    if G not in GROUP_SIZES:
        raise ValueError(f"group must be one of {GROUP_SIZES}, got {group}")
    if x.dim() != 2 or x.shape[0] % G:
        raise ValueError(f"x must be (M * group, dx), got {tuple(x.shape)} with group = {G}")
    B, M, O = targets.shape
    if x.shape[0] != M * G:
        raise ValueError(f"x holds {x.shape[0] // G} cells, targets {M}")
    if q is not None and tuple(q.shape) != (M * G,):
        raise ValueError(f"q has shape {tuple(q.shape)}, expected {(M * G,)}")
    if obs_weight is not None and tuple(obs_weight.shape) != (B, M):
        raise ValueError(f"obs_weight has shape {tuple(obs_weight.shape)}, expected {(B, M)}")
    _one_weight_kind("fit_cell_averages", obs_weight, obs_channel_weight, (B, M, O))
    from .observations import Cells                  # (observations imports this module)
    obs, per_value = Cells(x, q, G, M), obs_channel_weight is not None
    if per_value:
        obs_weight = obs_channel_weight
    dev = targets.device
    tg = targets.float()
    if sample is None:
        pick = lambda s: (x, q, tg, obs_weight)
    else:
        idx = sample if torch.is_tensor(sample) else draw_cell_samples(M, sample, S, generator)
        if idx.dim() != 2 or idx.shape[0] != S + 1:
            raise ValueError(f"sample indices have shape {tuple(idx.shape)}, expected ({S + 1}, M_s)")
        idx = idx.to(device=dev, dtype=torch.long)
        rows = (idx[..., None] * G + torch.arange(G, device=dev)).reshape(S + 1, -1)       # the groups' query rows, in order
        xs_all = x.to(dev)[rows]                                                            # (S + 1, M_s G, dx)
        qs_all = q.to(dev)[rows] if q is not None else None
        ys_all = tg[:, idx].transpose(0, 1).contiguous()                                    # (S + 1, B, M_s, O)
        ws_all = obs_weight.to(dev)[:, idx].transpose(0, 1).contiguous() if obs_weight is not None else None
        pick = lambda s: (xs_all[s], None if qs_all is None else qs_all[s], ys_all[s], None if ws_all is None else ws_all[s])
    lat = {k: v.detach().repeat_interleave(B, dim=0) for k, v in latents0.items()}
    losses = torch.zeros(S + 1, device=dev, dtype=torch.float32)
    rows_b = [] if per_signal_loss else None
    for s in range(S + 1):                                               # S steps, then the loss on the last set
        xs, qs, ys, ws = pick(s)
        xb, qb = _batched(xs.to(dev), None if qs is None else qs.to(dev), B)
        if s < S:
            lat = _sgd_step(nef, params, obs, lat, lrs, xb, qb, ys, ws, per_value, optimize_gaussian_window, rows_b,
                            loss_out=losses[s:s + 1], return_errors=per_signal_loss)
    lb = obs.final_loss(nef, params, xb, qb, _pose(lat, nef.cross_attn_invariant.num_z_ori_dims), lat["a"], lat.get("gaussian_window"), ys, ws,
                        per_value, losses[S:], per_signal_loss)
    if per_signal_loss:
        return losses[S], lat, torch.stack(rows_b + [lb])
    return losses[S], lat


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
    if G not in GROUP_SIZES:
        raise ValueError(f"group must be one of {GROUP_SIZES}, got {group}")
    B, M, O = targets.shape
    if x.dim() != 2 or x.shape[0] != M * G:
        raise ValueError(f"x must be (M * group, dx) = ({M * G}, dx), got {tuple(x.shape)}")
    if q is not None and tuple(q.shape) != (M * G,):
        raise ValueError(f"q has shape {tuple(q.shape)}, expected {(M * G,)}")
    if obs_weights is not None and tuple(obs_weights.shape) != (B, M):
        raise ValueError(f"obs_weights have shape {tuple(obs_weights.shape)}, expected {(B, M)}")
    _one_weight_kind("inner_loop_cells", obs_weights, obs_channel_weight, (B, M, O))
    from .observations import Cells                  # (observations imports this module)
    if masks.dim() not in (2, 3) or (masks.dim() == 3 and masks.shape[0] != B):
        raise ValueError(f"masks have shape {tuple(masks.shape)}, expected (Ms, S + 1) or ({B}, Ms, S + 1)")
    per_value = obs_channel_weight is not None
    w = obs_channel_weight if per_value else obs_weights
    w = w.to(device=targets.device, dtype=torch.float32).contiguous() if w is not None else None
    return _fit_loop(nef, nef_params, Cells(x, q, G, M), latents0, lrs, targets, masks, w, per_value, optimize_gaussian_window, noise_pos,
                     generator, normalize_weights, per_signal_loss)
