"""Per-point loss weights (include/enf_hip.h, "Weighted loss"): one value per signal and grid point, finite and >= 0,

    loss = 1 / (B N O) * sum_{b,n} w[b,n] * sum_o (out[b,n,o] - target[b,n,o])^2

A point of weight 0 does not exist: its target may be NaN or Inf and never enters the arithmetic.  The library does not
normalise; the trainers call ``normalize_point_weights`` once on the FULL grid, before any sampling, so that the loss on a
random subset of points is an unbiased estimate of the full-grid weighted mean and weights of all ones change nothing.
Where the subset is drawn per signal from its observed points only, ``observed_sampling_weights`` keeps that property.
Pure torch, no GPU needed.
"""
import torch

QUADRATURE_KINDS = ("latitude", "colatitude", "ball")


def normalize_point_weights(w):
    """``w`` (..., N) >= 0 -> the same weights with mean 1 over every signal's N points.  A signal whose weights are all zero
    stays zero (it then contributes nothing to a loss); weights of all ones come back as all ones exactly."""
    w = torch.as_tensor(w)
    if not w.is_floating_point():
        w = w.float()
    if bool((w < 0).any()) or not bool(torch.isfinite(w).all()):
        raise ValueError("point weights must be finite and >= 0")
    mean = w.mean(dim=-1, keepdim=True)
    return torch.where(mean > 0, w / torch.where(mean > 0, mean, torch.ones_like(mean)), torch.zeros_like(w))


def quadrature_weights(coords, column, kind, radius_column=None):
    """Area (volume) weights of a regular grid in angles, (N,), not normalised: the surface element of the sphere is
    cos(latitude) d lat d lon = sin(colatitude) d colat d lon, the volume element of the ball r^2 sin(colatitude) dr d colat d lon.

    coords : (N, dx) grid;  column : the column of ``coords`` that holds the polar angle, in radians
    kind   : "latitude" (angle in [-pi/2, pi/2], weight cos), "colatitude" (angle in [0, pi], weight sin) or
             "ball" (colatitude, times the square of the radius in ``radius_column``)
    The convention is the caller's to state: it is not guessed from an invariant's name.  Values an angle beyond the pole
    would make negative are clamped to 0."""
    if kind not in QUADRATURE_KINDS:
        raise ValueError(f"kind must be one of {QUADRATURE_KINDS}, got {kind!r}")
    angle = coords[..., column]
    w = torch.cos(angle) if kind == "latitude" else torch.sin(angle)
    if kind == "ball":
        if radius_column is None:
            raise ValueError('kind="ball" needs radius_column')
        w = w * coords[..., radius_column] ** 2
    elif radius_column is not None:
        raise ValueError(f'radius_column only goes with kind="ball", not {kind!r}')
    return w.clamp_min(0)


def valid_weights(field):
    """``field`` (..., O) -> (...) float: 1 where every channel is finite, 0 where any is NaN or Inf."""
    return torch.isfinite(field).all(dim=-1).to(torch.float32)


def prepare_point_weights(weights, B, N, normalize=True, device=None):
    """What a trainer does with its ``weights`` argument: None stays None; (N,) or (B, N) becomes float32 (B, N), with
    mean 1 per signal unless ``normalize`` is False."""
    if weights is None:
        return None
    w = torch.as_tensor(weights, dtype=torch.float32)
    if w.dim() == 1:
        w = w[None].expand(B, -1)
    if tuple(w.shape) != (B, N):
        raise ValueError(f"weights have shape {tuple(w.shape)}, expected {(B, N)} or {(N,)}")
    if normalize:
        w = normalize_point_weights(w)
    return w.to(device).contiguous() if device is not None else w.contiguous()


def gather_point_weights(weights, masks):
    """weights (B, N), masks (N_s, S1) long -> (S1, B, N_s): ws[s, b, i] = weights[b, masks[i, s]] (what enf_fit_inputs_w gathers)."""
    return weights[:, masks.t()].transpose(0, 1).contiguous()


def observed_sampling_weights(weights, num_sampled):
    """Full-grid weights (B, N) -> the weights to fit with when every signal's points are drawn uniformly from its OWN observed set
    {weights > 0} (inner_loop.make_signal_masks) instead of from the whole grid.  Such a draw meets only observed points, so the
    sampled loss 1 / N_s * sum_i w_i d_i^2 estimates the mean of w d^2 over the n_b observed points, which is N / n_b times the
    full-grid weighted mean 1 / N * sum_n w_n d_n^2 that a draw from the whole grid estimates.  Signal b's weights are therefore
    multiplied by n_b / N, and where n_b < N_s -- the rows the sampler pads: all n_b points are met once, the divisor stays N_s
    -- by N_s / n_b as well:

        c_b = n_b / N * N_s / min(N_s, n_b)

    With these weights the sampled loss is an unbiased estimate of the same full-grid weighted mean as with shared masks (exact
    where n_b <= N_s), so loss values and step lengths keep their scale; 0/1 weights normalised to mean 1 on the grid (1 / f
    on the observed points) come out as 1 on the observed points.  A signal that observes nothing stays zero."""
    w = torch.as_tensor(weights)
    N = w.shape[-1]
    n = (w > 0).sum(dim=-1, keepdim=True).to(w.dtype)
    c = n / N * (float(num_sampled) / n.clamp(min=1.0).clamp(max=float(num_sampled)))
    return w * c


def weighted_mse(out, target, weights=None):
    """The loss above in torch (differentiable): ``out`` / ``target`` (..., N, O), ``weights`` (..., N) or None (the plain
    mean).  Where the weight is 0 the target is not used: NaN there reaches neither the value nor a gradient."""
    if weights is None:
        return ((out - target) ** 2).mean()
    w = weights[..., None].to(out.dtype)
    d = torch.where(w > 0, out - target, torch.zeros_like(out))
    return (w * d * d).mean()
