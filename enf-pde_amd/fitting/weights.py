"""Per-point loss weights (include/enf_hip.h, "Weighted loss"): one value per signal and grid point, finite and >= 0,

    loss = 1 / (B N O) * sum_{b,n} w[b,n] * sum_o (out[b,n,o] - target[b,n,o])^2

A point of weight 0 does not exist: its target may be NaN or Inf and never enters the arithmetic.  The library does not
normalise; the trainers call ``normalize_point_weights`` once on the FULL grid, before any sampling, so that the loss on a
random subset of points is an unbiased estimate of the full-grid weighted mean and weights of all ones change nothing.
Where the subset is drawn per signal from its observed points only, ``observed_sampling_weights`` keeps that property.

Per-channel weights (the same section of the header): one value per signal, grid point AND output channel, (B, N, O), for
variables that are observed separately,

    loss = 1 / (B N O) * sum_{b,n,o} cw[b,n,o] * (out[b,n,o] - target[b,n,o])^2

with the same rule per value; ``point_support`` says where a point carries any value.  ``weighted_mse`` and
``gather_point_weights`` take either kind and tell them apart by rank.  (B, T, N) point weights and (B, N, O) channel weights have
the same rank, so the trainers carry a ``LossWeights``: the prepared tensor and its kind, with the frames, subsets, support and
rescaling a step needs; the prepare_* / frame_* / observed_* functions are the same code, one kind at a time.
Pure torch, no GPU needed.
"""
from dataclasses import dataclass

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


def point_support(cweights):
    """Channel weights (..., N, O) -> point weights (..., N), > 0 exactly where at least one channel of the point is observed (the
    sum over the channels).  What make_signal_masks takes, so that per-signal sampling draws from the points that carry a value."""
    cw = torch.as_tensor(cweights)
    if cw.dim() < 2:
        raise ValueError(f"channel weights must be (..., N, O), got {tuple(cw.shape)}")
    return cw.clamp_min(0).sum(dim=-1)


def cut_frames(weights, frames, channel=False):
    """A caller's weights with a frame axis -- (B, T, N), per-channel (B, T, N, O) -- cut to ``weights[:, frames]`` (an index or a
    slice); weights without one, and None, come back as they are."""
    if weights is None:
        return None
    w = torch.as_tensor(weights)
    return w[:, frames] if w.dim() == (4 if channel else 3) else w


def _prepare(weights, B, N, O, T, channel, normalize, device):
    """The one preparation behind prepare_* (``T`` None) and frame_*: float32, broadcast over the batch (and over T frames), mean 1
    per signal(-frame) unless ``normalize`` is False, on ``device``.  Channel weights are checked finite and >= 0 where they are not
    normalised and wherever they come with a frame axis; point weights only by normalize_point_weights (every check is a host
    synchronisation, so none is added)."""
    if weights is None:
        return None
    w = torch.as_tensor(weights, dtype=torch.float32)
    name, grid = ("channel weights", (N, O)) if channel else ("weights", (N,))
    framed = T is not None and w.dim() == len(grid) + 2
    if framed:
        if tuple(w.shape) != (B, T) + grid:
            raise ValueError(f"{name} have shape {tuple(w.shape)}, expected {(B, T) + grid}, {(B,) + grid} or {grid}")
    else:
        if w.dim() == len(grid):
            w = w[None].expand(B, *w.shape)
        if tuple(w.shape) != (B,) + grid:
            raise ValueError(f"{name} have shape {tuple(w.shape)}, expected {(B,) + grid} or {grid}")
    if channel and (framed or not normalize) and (bool((w < 0).any()) or not bool(torch.isfinite(w).all())):
        raise ValueError("channel weights must be finite and >= 0")
    if normalize:
        w = normalize_channel_weights(w) if channel else normalize_point_weights(w)
    w = w.to(device) if device is not None else w
    if framed:
        return w
    return w.contiguous() if T is None else w.contiguous()[:, None].expand(B, T, *grid)


def prepare_point_weights(weights, B, N, normalize=True, device=None):
    """What a trainer does with its ``weights`` argument: None stays None; (N,) or (B, N) becomes float32 (B, N), with
    mean 1 per signal unless ``normalize`` is False."""
    return _prepare(weights, B, N, None, None, False, normalize, device)


def prepare_channel_weights(weights, B, N, O, normalize=True, device=None):
    """What a trainer does with its ``channel_weights`` argument: None stays None; (N, O) or (B, N, O) becomes float32 (B, N, O),
    finite and >= 0 (ValueError otherwise), with mean 1 over each signal's N * O values unless ``normalize`` is False."""
    return _prepare(weights, B, N, O, None, True, normalize, device)


def frame_weights(weights, B, T, N, normalize=True, device=None):
    """``weights`` (N,), (B, N) or (B, T, N) -> float32 (B, T, N), every signal-frame's weights of mean 1 over the full grid
    unless ``normalize`` is False; None stays None."""
    return _prepare(weights, B, N, None, T, False, normalize, device)


def frame_channel_weights(weights, B, T, N, O, normalize=True, device=None):
    """Per-channel ``weights`` (N, O), (B, N, O) or (B, T, N, O) -> float32 (B, T, N, O), every signal-frame's weights of mean 1 over
    its N * O values unless ``normalize`` is False; None stays None."""
    return _prepare(weights, B, N, O, T, True, normalize, device)


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
    return w * _observed_factor(w, num_sampled)


def _observed_factor(support, num_sampled):
    """c_b of observed_sampling_weights, (..., 1), from point weights (..., N) that are > 0 on signal b's n_b observed points."""
    N = support.shape[-1]
    n = (support > 0).sum(dim=-1, keepdim=True).to(support.dtype)
    return n / N * (float(num_sampled) / n.clamp(min=1.0).clamp(max=float(num_sampled)))


def observed_channel_sampling_weights(cweights, num_sampled):
    """observed_sampling_weights for channel weights (B, N, O): a point is observed where any of its channels is (point_support),
    n_b counts those points, and the same factor c_b multiplies all channels of signal b's points."""
    cw = torch.as_tensor(cweights)
    return cw * _observed_factor(point_support(cw), num_sampled)[..., None]


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


@dataclass(frozen=True, eq=False)
class LossWeights:
    """The loss weights of one step, prepared: ``w`` float32 and whether it is per point -- (B, N), with frames (B, T, N) -- or per
    channel -- (B, N, O), (B, T, N, O).  Rank alone cannot tell (B, T, N) from (B, N, O); this value can, so a trainer carries one
    variable whatever its caller passed.  "No weights" is None, never an instance: ``build`` returns None for it, and ``loop_kw`` /
    ``nef_kw`` / ``loss_tensor`` below take None and hand on nothing, so an unweighted step runs not one operation more.

    What the trainers rely on:
      - ``build`` is the only place that tells ``weights=`` from ``channel_weights=``; it raises for both, for a wrong shape, and for
        values that are not finite and >= 0 exactly where the prepare_* / frame_* helpers do (_prepare), and costs their host
        synchronisations, no more.
      - The weights of the fit (``frames=0``) and those of the errors over all frames (``T=``) are prepared from the caller's weights
        separately: frame 0 is normalised on its own, not cut from the normalised frames.
      - Nothing here draws random numbers.  A step draws its masks from ``support()`` and only then calls ``drawn_on(masks)``; under
        point drop-out it draws the keep-mask first, then the masks, then ``keep`` / ``renormalized`` / ``observed_draw``.
      - ``observed_draw`` rescales the weights a FIT on per-signal masks takes; errors on the full grid (fit_errors, val_step) take the
        value as built."""
    w: torch.Tensor
    channel: bool = False

    @classmethod
    def build(cls, weights, channel_weights, B, N, O, T=None, normalize=True, device=None, frames=None):
        """From a step's ``weights`` ((N,), (B, N), (B, T', N)) and ``channel_weights`` ((N, O), (B, N, O), (B, T', N, O)): None for
        neither, ValueError for both.  ``frames``: an index or slice of the frame axis, where the input has one (cut_frames), taken
        first.  ``T`` None gives (B, N[, O]); otherwise (B, T, N[, O]), input without a frame axis repeated over the T frames."""
        if channel_weights is not None and weights is not None:
            raise ValueError("pass weights= or channel_weights=, not both")
        channel = channel_weights is not None
        raw = channel_weights if channel else weights
        if frames is not None:
            raw = cut_frames(raw, frames, channel)
        w = _prepare(raw, B, N, O, T, channel, normalize, device)
        return None if w is None else cls(w, channel)

    def _like(self, w):
        return LossWeights(w, self.channel)

    def _per_point(self, t):
        """``t`` (..., N), one value per point, shaped to multiply ``w``."""
        return t[..., None] if self.channel else t

    def frame_range(self, start, stop):
        return self._like(self.w[:, start:stop])

    def support(self):
        """(..., N), > 0 exactly where the point is observed: what make_signal_masks takes."""
        return point_support(self.w) if self.channel else self.w

    def points(self, index):
        """The weights of a subset of the grid points, ``[:, index]`` along N."""
        return self._like(self.w[:, index])

    def keep(self, mask):
        """Times a (B, N) keep-mask: a point that is not kept is not observed."""
        return self._like(self.w * self._per_point(mask))

    def renormalized(self):
        return self._like(normalize_channel_weights(self.w) if self.channel else normalize_point_weights(self.w))

    def observed_draw(self, num_sampled):
        """Rescaled for a fit on ``num_sampled`` points per signal drawn from its observed set (observed_sampling_weights)."""
        return self._like(self.w * self._per_point(_observed_factor(self.support(), num_sampled)))

    def drawn_on(self, masks):
        """The weights of a fit on ``masks`` the step drew itself: rescaled where they are per signal (B, N_s, S+1), else as they are."""
        return self.observed_draw(masks.shape[1]) if masks.dim() == 3 else self


def loop_kw(lw):
    """The keyword inner_loop and meta_gradients take a LossWeights (or None) by."""
    return {} if lw is None else {"channel_weights" if lw.channel else "weights": lw.w}


def nef_kw(lw):
    """The keyword nef.mse_value_and_latent_grads and nef.eval_loss take it by."""
    return {} if lw is None else {"channel_weight" if lw.channel else "weight": lw.w}


def loss_tensor(lw):
    """What weighted_mse, gather_signal_points and sample_frames take: the tensor (they tell the kinds apart by its rank) or None."""
    return None if lw is None else lw.w
