"""Fits against cell averages (include/enf_hip.h, "Grouped observations"; no counterpart in the reference).

Data on a coarse grid are mostly not point values: a finite-volume solver gives cell means, a reanalysis box means, a satellite a
footprint's weighted mean.  Such an observation is a fixed linear functional of the decoded field,
    obs[m] = sum_k q[m G + k] u(x[m G + k]),
a quadrature rule over G points of cell m.  ``cell_quadrature`` builds the points and factors, ``decode_cell_averages`` applies the
functional to a decode in torch ops, and ``fit_cell_averages`` runs the inner loop's update rule on the fused grouped step
(nef.mse_value_and_cell_grads: the group sums are formed in the tail's registers, no decode exists in memory).
Nothing here is wired into ``inner_loop`` or the trainers."""
import numpy as np
import torch

from .inner_loop import _pose, meta_sgd_update

GROUP_SIZES = (1, 2, 4, 8, 16)


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


def fit_cell_averages(nef, params, latents0, lrs, x, q, group, targets, steps, obs_weight=None, sample=None, generator=None,
                      optimize_gaussian_window=False, per_signal_loss=False):
    """Fit per-signal latents to cell averages with `steps` steps of the inner loop's meta-SGD rule (inner_loop: meta_sgd_update on the
    gradient of the batch-mean loss times B, so that the signals are independent).

    latents0 : {'p_pos', 'a', 'gaussian_window'[, 'p_ori']} with leading dimension 1, as for inner_loop;  lrs: the same keys
    x, q     : the quadrature points (N, dx) and factors (N,) of the M = N / group cells (cell_quadrature), shared by the signals;
               q None is the plain mean, 1 / group
    targets  : (B, M, O) observed cell averages;  obs_weight: None or (B, M), finite and >= 0 -- an observation of weight 0 does not
               exist and its target may be NaN
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
    n_ori = nef.cross_attn_invariant.num_z_ori_dims
    lat = {k: v.detach().repeat_interleave(B, dim=0) for k, v in latents0.items()}
    losses = torch.zeros(S + 1, device=dev, dtype=torch.float32)
    n_pos = lat["p_pos"].shape[-1]
    rows_b = []
    for s in range(S + 1):
        xs, qs, ys, ws = pick(s)
        xb, qb = _batched(xs.to(dev), None if qs is None else qs.to(dev), B)
        args = (params, xb, _pose(lat, n_ori), lat["a"], lat.get("gaussian_window"), ys, G)
        if s == S:
            lb, _ = nef.eval_cell_loss(*args, qweight=qb, obs_weight=ws, loss_out=losses[S:], per_signal=per_signal_loss)
            rows_b.append(lb)
            break
        res = nef.mse_value_and_cell_grads(*args, qweight=qb, obs_weight=ws, loss_out=losses[s:s + 1], return_errors=per_signal_loss)
        _, dp, da, dsig = res[:4]
        if per_signal_loss:
            rows_b.append(res[5])
        grads = {"p_pos": dp[..., :n_pos], "a": da}
        if n_ori > 0:
            grads["p_ori"] = dp[..., n_pos:]
        if optimize_gaussian_window and dsig is not None:
            grads["gaussian_window"] = dsig
        lat = meta_sgd_update(lat, grads, lrs, B)
    if per_signal_loss:
        return losses[S], lat, torch.stack(rows_b)
    return losses[S], lat
