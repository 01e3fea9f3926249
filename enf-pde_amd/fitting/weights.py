"""Per-point loss weights (include/enf_hip.h, "Weighted loss"): one value per signal and grid point, finite and >= 0,

    loss = 1 / (B N O) * sum_{b,n} w[b,n] * sum_o (out[b,n,o] - target[b,n,o])^2

A point of weight 0 does not exist: its target may be NaN or Inf and never enters the arithmetic.  The library does not
normalise; the trainers call ``normalize_point_weights`` once on the FULL grid, before any sampling, so that the loss on a
random subset of points is an unbiased estimate of the full-grid weighted mean and weights of all ones change nothing.
Where the subset is drawn per signal from its observed points only, ``observed_sampling_weights`` keeps that property.

Per-channel weights (the same section of the header): one value per signal, grid point AND output channel, (B, N, O), for
variables that are observed separately,

    loss = 1 / (B N O) * sum_{b,n,o} cw[b,n,o] * (out[b,n,o] - target[b,n,o])^2

with the same rule per value.  ``valid_channel_weights``, ``prepare_channel_weights``, ``point_support`` and
``observed_channel_sampling_weights`` are the counterparts of the per-point helpers; ``weighted_mse`` and
``gather_point_weights`` take either kind.
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


def valid_channel_weights(field):
    """``field`` (..., N, O) -> (..., N, O) float: 1 where the value is finite, 0 where it is NaN or Inf -- per value, not per point."""
    return torch.isfinite(field).to(torch.float32)


def normalize_channel_weights(cw):
    """``cw`` (..., N, O) >= 0 -> the same weights with mean 1 over every signal's N * O values.  A signal whose weights are all zero
    stays zero; weights of all ones come back as all ones exactly."""
    cw = torch.as_tensor(cw)
    if not cw.is_floating_point():
        cw = cw.float()
    if cw.dim() < 2:
        raise ValueError(f"channel weights must be (..., N, O), got {tuple(cw.shape)}")
    return normalize_point_weights(cw.reshape(*cw.shape[:-2], -1)).reshape(cw.shape)


def prepare_channel_weights(weights, B, N, O, normalize=True, device=None):
    """What a trainer does with its ``channel_weights`` argument: None stays None; (N, O) or (B, N, O) becomes float32 (B, N, O),
    finite and >= 0 (ValueError otherwise), with mean 1 over each signal's N * O values unless ``normalize`` is False."""
    if weights is None:
        return None
    w = torch.as_tensor(weights, dtype=torch.float32)
    if w.dim() == 2:
        w = w[None].expand(B, -1, -1)
    if tuple(w.shape) != (B, N, O):
        raise ValueError(f"channel weights have shape {tuple(w.shape)}, expected {(B, N, O)} or {(N, O)}")
    if normalize:
        w = normalize_channel_weights(w)
    elif bool((w < 0).any()) or not bool(torch.isfinite(w).all()):
        raise ValueError("channel weights must be finite and >= 0")
    return w.to(device).contiguous() if device is not None else w.contiguous()


def point_support(cweights):
    """Channel weights (..., N, O) -> point weights (..., N), > 0 exactly where at least one channel of the point is observed (the
    sum over the channels).  What make_signal_masks takes, so that per-signal sampling draws from the points that carry a value."""
    cw = torch.as_tensor(cweights)
    if cw.dim() < 2:
        raise ValueError(f"channel weights must be (..., N, O), got {tuple(cw.shape)}")
    return cw.clamp_min(0).sum(dim=-1)


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
    """weights (B, N), masks (N_s, S1) long -> (S1, B, N_s): ws[s, b, i] = weights[b, masks[i, s]] (what enf_fit_inputs_w gathers).
    Channel weights (B, N, O) give (S1, B, N_s, O) the same way (enf_fit_inputs_cw)."""
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


def observed_channel_sampling_weights(cweights, num_sampled):
    """observed_sampling_weights for channel weights (B, N, O): a point is observed where any of its channels is (point_support),
    n_b counts those points, and the same factor c_b multiplies all channels of signal b's points."""
    cw = torch.as_tensor(cweights)
    N = cw.shape[-2]
    n = (point_support(cw) > 0).sum(dim=-1, keepdim=True).to(cw.dtype)
    c = n / N * (float(num_sampled) / n.clamp(min=1.0).clamp(max=float(num_sampled)))
    return cw * c[..., None]


def weighted_mse(out, target, weights=None):
    """The loss above in torch (differentiable): ``out`` / ``target`` (..., N, O), ``weights`` (..., N), per-channel (..., N, O)
    -- told apart by their rank -- or None (the plain mean).  Where the weight is 0 the target is not used: NaN there reaches
    neither the value nor a gradient."""
    if weights is None:
        return ((out - target) ** 2).mean()
    if weights.dim() == out.dim():
        if tuple(weights.shape) != tuple(out.shape):
            raise ValueError(f"channel weights have shape {tuple(weights.shape)}, expected {tuple(out.shape)}")
        w = weights.to(out.dtype)
    else:
        w = weights[..., None].to(out.dtype)
    d = torch.where(w > 0, out - target, torch.zeros_like(out))
    return (w * d * d).mean()
