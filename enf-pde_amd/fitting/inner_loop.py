"""MAML inner loop and decode on the HIP path (trainers/pde_trainer.py:122-235, 389-405).

Every meta-SGD fit of the package ends in ONE body, ``_fit_body``: S times ``_sgd_step``, the loss on the last set, the return values.
``inner_loop`` (point values) and fitting/cells.py: ``inner_loop_cells`` (cell averages) reach it through ``_fit_loop``, which gathers the
sampled inputs of all steps once and jitters the poses; fitting/cells.py: ``fit_cell_averages`` and fitting/operators.py:
``fit_linear_observations`` through ``_fit_given``, on inputs they choose themselves.  What differs between the kinds of observation --
the gather, the decoder's calls, the form of the last loss, when step 0 may share its forward -- the body asks of the observation
value it is given: ``_Observed`` is what the kinds share, ``Points`` the kind of this module (``Cells``: fitting/cells.py,
``LinearObservations``: fitting/operators.py).  The loop and the body look up ``meta_sgd_update``, ``_shared_kw`` and
``FUSED_FIT_INPUTS`` in this module when they run -- the switch is handed to the kind's gather -- so that one patch of any of them
reaches every fit, on points and on cells.  This module imports no other module of the fitting layer but weights.py; cells.py,
operators.py, observations.py (the parser ``observed``), gauss_newton.py and the trainers import it, in that order."""
import functools
import inspect

import torch

from .. import _lib
from .weights import LossWeights, gather_point_weights, loop_kw


def default_meta_sgd_lrs(latent_dim, lr_p=1.0, lr_a=5.0, lr_window=0.0, with_ori=False, device="cuda"):
    """Initial inner learning rates (pde_trainer.py:83-97): scalar for poses/window, (C,) for a."""
    lrs = {"p_pos": torch.full((1,), lr_p, device=device), "a": torch.full((latent_dim,), lr_a, device=device),
           "gaussian_window": torch.full((1,), lr_window, device=device)}
    if with_ori:
        lrs["p_ori"] = torch.full((1,), lr_p, device=device)
    return lrs


def make_masks(num_coords, num_sampled, num_inner_steps, generator=None, device="cuda"):
    """(N_s, S+1) independent column permutations truncated to N_s rows (pde_trainer.py:148-154).
    jax.random.permutation cannot be reproduced; parity tests pass masks explicitly."""
    cols = [torch.randperm(num_coords, generator=generator)[:num_sampled] for _ in range(num_inner_steps + 1)]
    return torch.stack(cols, dim=1).to(device)


def make_signal_masks(weights_or_valid, num_sampled, num_inner_steps, generator=None, device="cuda"):
    """(B, N_s, S+1) long: for every signal and step, N_s distinct indices drawn uniformly from that signal's observed set
    {weights_or_valid[b] > 0} -- the per-signal counterpart of make_masks for fields observed at different places (sensor drop-out,
    land masks, cloud gaps; fitting/weights.py: valid_weights).  A signal with fewer than N_s observed points gets them all, in random
    order, followed by -1: enf_fit_inputs_b gives such a row weight 0, so it does not exist (include/enf_hip.h).
    A draw from the observed set meets no zero-weight point, so full-grid weights of mean 1 no longer make the sampled loss an
    estimate of the full-grid weighted mean: fit with fitting/weights.py: observed_sampling_weights(weights, N_s) to keep its scale.
    Random fp64 keys, the unobserved points keyed to +inf, and the N_s smallest keys of every row; the keys are drawn where the
    generator lives (the CPU without one), so a seed fixes the masks."""
    valid = torch.as_tensor(weights_or_valid)
    if valid.dim() != 2:
        raise ValueError(f"weights_or_valid must be (B, N), got {tuple(valid.shape)}")
    gdev = generator.device if generator is not None else torch.device("cpu")
    observed = (valid > 0).to(gdev)
    B, N = observed.shape
    S1 = num_inner_steps + 1
    keys = torch.rand((S1, B, N), generator=generator, dtype=torch.float64, device=gdev)
    keys = keys.masked_fill(~observed[None], float("inf"))
    k = min(int(num_sampled), N)
    vals, idx = torch.topk(keys, k, dim=-1, largest=False, sorted=True)          # ascending: the +inf keys come last
    idx = idx.masked_fill(torch.isinf(vals), -1)
    if k < num_sampled:
        idx = torch.cat((idx, idx.new_full((S1, B, int(num_sampled) - k), -1)), dim=-1)
    return idx.permute(1, 2, 0).contiguous().to(device)


def gather_signal_points(coords, img, masks, weights=None):
    """What enf_fit_inputs_b gathers, in torch ops: coords (N, dx), img (B, N, O), masks (B, N_s, S1) long, weights (B, N) or None
    -> xs (S1, B, N_s, dx), ys (S1, B, N_s, O), ws (S1, B, N_s).  An index outside [0, N) gives coords[0], zero targets and weight 0;
    without ``weights`` ws is 1 for an index in range.  Channel weights (B, N, O) give ws (S1, B, N_s, O), a row of O zeros for an
    index outside (enf_fit_inputs_cw)."""
    B, N, O = img.shape
    S1 = masks.shape[2]
    idx = masks.permute(2, 0, 1)
    ok = (idx >= 0) & (idx < N)
    ic = torch.where(ok, idx, torch.zeros_like(idx))
    xs = coords[ic]
    ys = torch.gather(img[None].expand(S1, -1, -1, -1), 2, ic[..., None].expand(-1, -1, -1, O))
    ys = torch.where(ok[..., None], ys, torch.zeros_like(ys))
    if weights is not None and weights.dim() == 3:
        w = torch.gather(weights[None].expand(S1, -1, -1, -1), 2, ic[..., None].expand(-1, -1, -1, O)).float()
        return xs.contiguous(), ys.float().contiguous(), torch.where(ok[..., None], w, torch.zeros_like(w)).contiguous()
    w = torch.gather(weights[None].expand(S1, -1, -1), 2, ic) if weights is not None else torch.ones(ic.shape, device=img.device)
    ws = torch.where(ok, w.float(), torch.zeros_like(w, dtype=torch.float32))
    return xs.contiguous(), ys.float().contiguous(), ws.contiguous()


def normalize_sampled_weights(ws, channel=False):
    """ws (..., N_s) >= 0 -> the same with mean 1 over every signal's N_s samples; a signal whose samples sum to zero stays zero.
    ``channel``: ws is (..., N_s, O) and the mean is over every signal's N_s * O sampled values."""
    if channel:
        return normalize_sampled_weights(ws.reshape(*ws.shape[:-2], -1)).reshape(ws.shape)
    total = ws.sum(dim=-1, keepdim=True)
    return torch.where(total > 0, ws * (ws.shape[-1] / torch.where(total > 0, total, torch.ones_like(total))), torch.zeros_like(ws))


FUSED_FIT_INPUTS = __import__("os").environ.get("ENF_FIT_INPUTS") != "0"


def _fit_inputs(latents0, coords, img, masks, weights=None, channel=False):
    """enf_fit_inputs[_w] (include/enf_hip.h): (lat, xs_all, ys_all, losses) of inner_loop in one launch, or None where the
    arguments are not what the kernel takes (fp32, contiguous, on one GPU, at most four latent components of leading dimension 1).
    With ``weights`` (B, N) a fifth value, their gather ws_all (S1, B, Ns).  Per-signal ``masks`` (B, Ns, S1) go to enf_fit_inputs_b:
    xs_all is then (S1, B, Ns, dx) and ws_all is always returned.  ``channel``: ``weights`` are per-channel, (B, N, O); both mask
    layouts go to enf_fit_inputs_cw and ws_all is (S1, B, Ns, O)."""
    ts = list(latents0.values()) + [coords, img] + ([weights] if weights is not None else [])
    per_signal = masks.dim() == 3          # masks (B, Ns, S1): enf_fit_inputs_b, xs (S1, B, Ns, dx) and ws always (1 / 0 without weights)
    if not (img.is_cuda and masks.is_cuda and masks.dtype == torch.int64 and masks.dim() in (2, 3) and masks.is_contiguous() and coords.dim() == 2
            and img.dim() == 3 and 1 <= len(latents0) <= _lib.ENF_SGD_MAX_SEGMENTS and masks.shape[0] > 0
            and all(t.dtype == torch.float32 and t.is_contiguous() and t.device == img.device for t in ts)
            and all(v.dim() == 3 and v.shape[0] == 1 for v in latents0.values())
            and len({v.shape[1] for v in latents0.values()}) == 1):
        return None
    B, N, O = img.shape
    Ns, S1 = masks.shape[-2:]
    if per_signal and masks.shape[0] != B:
        return None
    Z = next(iter(latents0.values())).shape[1]
    dev = img.device
    lat = {k: torch.empty((B, Z, v.shape[2]), device=dev, dtype=torch.float32) for k, v in latents0.items()}
    xs = torch.empty((S1, B, Ns, coords.shape[1]) if per_signal else (S1, Ns, coords.shape[1]), device=dev, dtype=torch.float32)
    ys = torch.empty((S1, B, Ns, O), device=dev, dtype=torch.float32)
    losses = torch.empty(S1, device=dev, dtype=torch.float32)
    comps = (_lib.EnfFitComponent * _lib.ENF_SGD_MAX_SEGMENTS)()
    keep = []
    for i, (k, v) in enumerate(latents0.items()):
        src = v.detach()
        keep.append(src)
        comps[i] = _lib.EnfFitComponent(src.data_ptr(), lat[k].data_ptr(), v.shape[2], 0)
    st = _lib.stream(dev)
    if channel:
        ws = torch.empty((S1, B, Ns, O), device=dev, dtype=torch.float32)
        _lib.launch(dev, _lib.load().enf_fit_inputs_cw, len(latents0), comps, B, Z, N, Ns, S1, coords.shape[1], O, coords.data_ptr(),
                    img.data_ptr(), masks.data_ptr(), xs.data_ptr(), ys.data_ptr(), losses.data_ptr(), weights.data_ptr(), ws.data_ptr(),
                    1 if per_signal else 0, st)
        return lat, xs, ys, losses, ws
    ws = torch.empty((S1, B, Ns), device=dev, dtype=torch.float32) if weights is not None or per_signal else None
    if per_signal:
        _lib.launch(dev, _lib.load().enf_fit_inputs_b, len(latents0), comps, B, Z, N, Ns, S1, coords.shape[1], O, coords.data_ptr(),
                    img.data_ptr(), masks.data_ptr(), xs.data_ptr(), ys.data_ptr(), losses.data_ptr(),
                    weights.data_ptr() if weights is not None else None, ws.data_ptr(), st)
        return lat, xs, ys, losses, ws
    _lib.launch(dev, _lib.load().enf_fit_inputs_w, len(latents0), comps, B, Z, N, Ns, S1, coords.shape[1], O, coords.data_ptr(), img.data_ptr(),
                masks.data_ptr(), xs.data_ptr(), ys.data_ptr(), losses.data_ptr(), weights.data_ptr() if weights is not None else None,
                ws.data_ptr() if ws is not None else None, st)
    return (lat, xs, ys, losses) if weights is None else (lat, xs, ys, losses, ws)


def _full_grid_weights(img, weights, channel_weights):
    """The loss weights of a fit on the full grid, float32 and contiguous next to ``img``: ``channel_weights`` (B, N, O), or ``weights``
    (B, N), or None."""
    if channel_weights is not None:
        if weights is not None:
            raise ValueError("pass weights= (B, N) or channel_weights= (B, N, O), not both")
        if tuple(channel_weights.shape) != tuple(img.shape):
            raise ValueError(f"channel_weights have shape {tuple(channel_weights.shape)}, expected {tuple(img.shape)}")
        return channel_weights.to(device=img.device, dtype=torch.float32).contiguous()
    if weights is None:
        return None
    if tuple(weights.shape) != tuple(img.shape[:2]):
        raise ValueError(f"weights have shape {tuple(weights.shape)}, expected {tuple(img.shape[:2])}")
    return weights.to(device=img.device, dtype=torch.float32).contiguous()


def _fresh(latents0, B, S1, dev):
    """What every fit starts from: the signals' own copies of the latent initialisation (pde_trainer.py:157-159; fresh tensors) and one
    zeroed loss accumulator per step and for the last loss."""
    return {k: v.detach().repeat_interleave(B, dim=0) for k, v in latents0.items()}, torch.zeros(S1, device=dev, dtype=torch.float32)


def _batched(x, q, B):
    """The one place that broadcasts shared query rows to a batch: x (N, dx) or (B, N, dx) -> a batch (stride 0 where shared);
    q None, (N,) or (B, N) -> None or (B, N)."""
    xb = x[None].expand(B, -1, -1) if x.dim() == 2 else x
    qb = None if q is None else (q[None].expand(B, -1) if q.dim() == 1 else q)
    return xb, qb


def _gather_inputs(latents0, coords, img, masks, weights, channel, fused_launch):
    """What inner_loop prepares before its first step, for every weight form and both mask layouts: the signals' copies of the latent
    initialisation (pde_trainer.py:157-159), the coordinates and targets of all S+1 steps gathered once (:193-197), one zeroed loss
    accumulator per step and the gathered weights -- (lat, xs_all, ys_all, losses, ws_all), ws_all None without weights on shared
    masks.  ONE launch (_fit_inputs) instead of eight framework kernels, or -- where the launch declines, or without ``fused_launch``, the
    loop's reading of FUSED_FIT_INPUTS -- the same in torch ops."""
    fused = _fit_inputs(latents0, coords, img, masks, weights, channel=channel) if fused_launch else None
    if fused is not None:
        return fused if len(fused) == 5 else (*fused, None)
    lat, losses = _fresh(latents0, img.shape[0], masks.shape[-1], img.device)
    if masks.dim() == 3:                                                 # (S+1, B, N_s, .): enf_fit_inputs_b / _cw in torch ops
        xs_all, ys_all, ws_all = gather_signal_points(coords, img, masks, weights)
        return lat, xs_all, ys_all, losses, ws_all
    masks_t = masks.t().contiguous()                                     # (a gather inherits the strides of a transposed index)
    xs_all = coords[masks_t]                                             # (S+1, N_s, dx)
    ys_all = img[:, masks_t].transpose(0, 1).float().contiguous()        # (S+1, B, N_s, O)
    ws_all = gather_point_weights(weights, masks) if weights is not None else None      # (S+1, B, N_s[, O])
    return lat, xs_all, ys_all, losses, ws_all


def _pose(lat, num_ori_dims):
    return torch.cat((lat["p_pos"], lat["p_ori"]), dim=-1) if num_ori_dims > 0 else lat["p_pos"]


def meta_sgd_update(lat, grads, lrs, scale):
    """One meta-SGD update of every latent component in a single HIP launch (pde_trainer.py:206-219):
    ``lat[k] - lrs[k] * (scale * grads[k])`` for the keys of ``grads``; the other entries of ``lat`` are passed through.
    A gradient may be a column slice of a wider (..., P) array (the pose gradient split into p_pos / p_ori)."""
    lib = _lib.load()
    new = dict(lat)
    segs = (_lib.EnfSgdSegment * _lib.ENF_SGD_MAX_SEGMENTS)()
    keep = []
    for i, (k, g) in enumerate(grads.items()):
        x = lat[k].float().contiguous()
        w = x.shape[-1]
        if g.dtype != torch.float32 or g.shape != x.shape or g.stride(-1) != 1 or \
                any(g.stride(d) != g.stride(d + 1) * g.shape[d + 1] for d in range(g.dim() - 2)):
            g = g.float().contiguous()
        lr = lrs[k].detach().float().contiguous()
        out = torch.empty_like(x)
        keep += [x, g, lr]
        segs[i] = _lib.EnfSgdSegment(x.data_ptr(), g.data_ptr(), lr.data_ptr(), out.data_ptr(), x.numel(), w,
                                     g.stride(-2) if g.dim() > 1 else w, lr.numel(), 0)
        new[k] = out
    _lib.launch(out.device, lib.enf_meta_sgd_update, len(grads), segs, float(scale), _lib.stream(out.device))
    return new


@functools.lru_cache(maxsize=64)
def _takes_shared_hint(fn):
    """Whether a decoder's step names the ``shared_latents`` keyword.  inner_loop is duck-typed over ``nef`` and the hint is new, so it
    looks at its callee's signature once per function instead of breaking every decoder -- the stand-ins of the older tests among them --
    whose step was written before the keyword existed."""
    try:
        params = inspect.signature(fn).parameters.values()      # (by name only: a **kwargs wrapper may record what it is given)
    except (TypeError, ValueError):
        return False
    return any(q.name == "shared_latents" for q in params)


def _shared_kw(nef, s, per_signal, noise_pos, step="mse_value_and_latent_grads"):
    """The keyword of step ``s``'s mse_value_and_latent_grads (or of ``step``, the grouped step of inner_loop_cells): at step 0 every
    signal still holds the one latent initialisation, and with
    shared masks the same points (a stride-0 batch) -- unless the poses were jittered per signal -- so the step may run its forward pair
    kernel once for all signals (include/enf_hip.h: ENF_FIT_SHARED_LATENTS).  A decoder whose step does not know the hint is not given it,
    and neither is one in deterministic mode: the one forward adds a query's partial sums in another fp32 order, and that mode keeps a
    fit on shared masks equal, bit for bit, to the same fit on per-signal masks that repeat them."""
    if s != 0 or per_signal or noise_pos:
        return {}
    det = getattr(nef, "is_deterministic", None)
    if det is not None and det():
        return {}
    fn = getattr(nef, step)
    return {"shared_latents": True} if _takes_shared_hint(getattr(fn, "__func__", fn)) else {}


class _Observed:
    """What the kinds of observation share.  A kind has two halves.  The CALLS half says which calls of the decoder are the kind's fit
    step, evaluation and Gauss-Newton product (STEP / EVAL / PRODUCT), what they take beside the query rows (``_call``: nothing, the
    group size and the factors, the operator) and which keywords carry sampled weights (WEIGHT_KW, chosen here and nowhere else); it
    needs no grid.  The constructor adds the other half, the shared grid the loops sample from, and validates it.  ``Kind.given(...)``
    builds a kind from parts that its caller has checked in its own words: both halves, or the calls half alone for a caller that
    brings batched inputs of its own (gauss_newton._lm_loop, fit_cell_averages, fit_linear_observations)."""

    @classmethod
    def given(cls, **owns):
        obs = object.__new__(cls)
        obs.__dict__.update(owns)
        return obs

    def _weight_kw(self, ws, channel, always=False):
        return {self.WEIGHT_KW[bool(channel)]: ws} if ws is not None or always else {}

    def weights_kw(self, *ws):
        """A front end's own weight arguments, in the order of WEIGHT_KW (per observation, then per value), by the decoder's keywords."""
        return dict(zip(self.WEIGHT_KW, ws))

    def reserve_kw(self):
        """What nef.gn_reserve takes beside the sizes."""
        return {}

    def fit_step(self, nef, params, xs, qs, p, a, window, ys, ws, channel, always=False, **kw):
        return self._call(nef, self.STEP, params, xs, qs, p, a, window, ys, **kw, **self._weight_kw(ws, channel, always))

    def gn_product(self, nef, params, xs, qs, p, a, window, **kw):
        return self._call(nef, self.PRODUCT, params, xs, qs, p, a, window, **kw)

    def loss_b(self, nef, params, xs, qs, p, a, window, ys, **kw):
        """Every signal's loss from the kind's evaluation, without a decode."""
        return self._call(nef, self.EVAL, params, xs, qs, p, a, window, ys, **kw)[0]

    def final_loss(self, nef, params, xs, qs, p, a, window, ys, ws, channel, loss_out, per_signal_loss):
        """The loop's loss on the last set, added to ``loss_out``; returns loss_b with ``per_signal_loss``."""
        return self.loss_b(nef, params, xs, qs, p, a, window, ys, loss_out=loss_out, per_signal=per_signal_loss,
                           **self._weight_kw(ws, channel, True))

    def decode_loss(self, nef, params, img, masks, s, lat, weights, mse):
        xs, qs, ys, ws = self.sampled(img, masks, s, weights)                      # pde_trainer.py:193-197
        out = nef.apply(params, xs, _pose(lat, nef.cross_attn_invariant.num_z_ori_dims), lat["a"], lat.get("gaussian_window"))
        return self.loss_of_decode(nef, out, ys, qs, ws, mse)


class Points(_Observed):
    """Values of the field at the N grid points ``coords`` (N, dx): one query row per observation."""
    rows, WEIGHT_KW = 1, ("weight", "channel_weight")
    STEP, EVAL, PRODUCT = "mse_value_and_latent_grads", "eval_loss", "gn_product"

    def __init__(self, coords):
        self.x, self.num = coords, coords.shape[0]

    def _call(self, nef, name, params, xs, qs, p, a, window, *ys, **kw):
        return getattr(nef, name)(params, xs, p, a, window, *ys, **kw)

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

    def gather(self, latents0, img, masks, w, channel, fused_launch):
        lat, xs_all, ys_all, losses, ws_all = _gather_inputs(latents0, self.x, img, masks, w, channel, fused_launch)
        return lat, xs_all, None, ys_all, losses, ws_all

    def step_inputs(self, xs_all, qs_all, ws_all, s, B, per_signal):
        return xs_all[s] if per_signal else _batched(xs_all[s], None, B)[0], None, None if ws_all is None else ws_all[s]

    def sampled(self, img, masks, s, weights, copies=1):
        """The points of step ``s``: (xs (copies * B, N_s, dx), None, ys (B, N_s, O), weights (B, N_s) or None).  Shared masks (N_s, S+1)
        give the reference's gather (pde_trainer.py:193-197) with a stride-0 batch; per-signal masks (B, N_s, S+1) give every signal its
        own points and always weights (0 where the sampler padded with -1; gather_signal_points).  Per-channel ``weights`` (B, N, O) come
        back as (B, N_s, O); weighted_mse tells the two apart by their rank."""
        if masks.dim() == 2:
            m = masks[:, s]
            return _batched(self.x[m], None, copies * img.shape[0])[0], None, img[:, m], (None if weights is None else weights[:, m])
        xs, ys, ws = gather_signal_points(self.x, img, masks[:, :, s:s + 1], weights)
        return (xs[0] if copies == 1 else xs[0].repeat(copies, 1, 1)), None, ys[0].to(img.dtype), ws[0]

    def eval(self, nef, params, part, n, p, a, window, ys, ws, channel):
        """(loss_b or None, err (n, |part|)) of ``n`` signals on the slice ``part`` of the grid, without a decode (nef.eval_loss)."""
        return nef.eval_loss(params, _batched(self.x[part], None, n)[0], p, a, window, ys, per_signal=False, **self._weight_kw(ws, channel))

    def loss_of_decode(self, nef, out, ys, qs, ws, mse):
        """``mse``: the calling module's weighted_mse (fitting/weights.py), formed only where there are weights."""
        return ((out - ys) ** 2).mean() if ws is None else mse(out, ys, ws)         # pde_trainer.py:185

    def final_loss(self, nef, params, xs, qs, p, a, window, ys, ws, channel, loss_out, per_signal_loss):
        """The loop's loss on the last mask, added to ``loss_out``: enf_eval_loss with ``per_signal_loss`` (returns loss_b), else the
        reference's decode (pde_trainer.py:225-235) and the loss kernel of the weight form (returns None)."""
        if per_signal_loss:
            return self.loss_b(nef, params, xs, qs, p, a, window, ys, loss_out=loss_out, **self._weight_kw(ws, channel, True))
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
        return img, _batched(coords, None, img.shape[0])[0], None, lw

    def sample_frames(self, traj, point_masks=None, weights=None):
        """Queries and targets of the B T signal-frames: ``traj`` (B, T, N, O), ``point_masks`` (T, n_s) long or None for the full grid.
        Returns xs (B T, n, dx), None, ys (B T, n, O), signal-major like the flattened roll-out, and the gather of ``weights`` (B, T, N)
        -> ws (B T, n), per-channel (B, T, N, O) -> (B T, n, O), or None."""
        B, T, N, O = traj.shape
        if point_masks is None:
            return (_batched(self.x, None, B * T)[0], None, traj.reshape(B * T, N, O),
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


def inner_loop(nef, nef_params, latents0, lrs, coords, img, masks, optimize_gaussian_window=False,
               noise_pos=0.0, generator=None, weights=None, normalize_weights=False, channel_weights=None, per_signal_loss=False):
    """Fit per-signal latents with S steps of meta-SGD (pde_trainer.py:156-235).

    latents0 : {'p_pos','a','gaussian_window'[,'p_ori']} with leading dim 1 (the meta-init)
    lrs      : inner learning rates, same keys
    coords   : (N, dx) grid;  img: (B, N, O) targets;  masks: (N_s, S+1) long, one index set per step shared by the signals, or
               (B, N_s, S+1) long, one per signal and step (make_signal_masks; enf_fit_inputs_b): every signal is then fitted on
               its own points, x (B, N_s, dx) with a real batch stride.  There an index outside [0, N) -- the sampler's -1 padding
               of a signal with fewer than N_s observed points -- has weight 0 and does not exist.
    Each step is one HIP forward, the fused loss/d-out kernel and one HIP backward-to-latents
    (nef.mse_value_and_latent_grads: no autograd graph); the gradient of the batch-mean loss is multiplied by B
    (pde_trainer.py:207) so signals are independent.
    weights  : None, or (B, N) loss weights on the full grid, finite and >= 0 (fitting/weights.py; taken as they are -- the trainers
               normalise them to mean 1 per signal first).  They are gathered with the targets and weigh every step's loss and
               the final one; a point of weight 0 does not exist, its target may be NaN.
    normalize_weights : rescale every signal's sampled weights ws[s, b, :] to mean 1 over its N_s samples before each step (a zero
               sum stays zero), so that a signal with few valid samples takes a step as long as a fully sampled one.  Off by
               default: the loss is the library's un-normalised 1 / (B N_s O) sum, as with ``weights`` alone.  Needs sampled
               weights (``weights``, ``channel_weights`` or per-signal masks).
    channel_weights : None, or (B, N, O) loss weights per value on the full grid, finite and >= 0 (fitting/weights.py:
               prepare_channel_weights), for fields whose variables are observed separately; not together with ``weights``.  They are
               gathered with the targets in the same launch (enf_fit_inputs_cw, either mask layout) and every step runs
               enf_fit_step_cw; a value of weight 0 does not exist, its target may be NaN.  ``normalize_weights`` then rescales to
               mean 1 over every signal's N_s * O sampled values.
    per_signal_loss : also return loss_b (S + 1, B), every signal's own loss at each step and on the last mask (include/enf_hip.h,
               "Per-signal and per-point errors": loss_b[s].mean() is step s's loss up to rounding).  The steps then run enf_fit_step_e
               -- the kernels of the plain steps with one store added, so the fitted latents are the same -- and the final loss comes
               from enf_eval_loss, without a decode, instead of enf_forward + enf_mse_value_grad*: the same sum in another order.
               Every weight form and both mask layouts.
    Returns (loss on the last mask, fitted latents dict with leading dim B), with ``per_signal_loss`` followed by loss_b.
    """
    B = img.shape[0]
    if masks.dim() == 3 and masks.shape[0] != B:
        raise ValueError(f"per-signal masks have shape {tuple(masks.shape)}, expected ({B}, N_s, S + 1)")
    return _fit_loop(nef, nef_params, Points(coords), latents0, lrs, img, masks, _full_grid_weights(img, weights, channel_weights),
                     channel_weights is not None, optimize_gaussian_window, noise_pos, generator, normalize_weights, per_signal_loss)


def split_latent_grads(dp, da, dsig, n_pos, ori=True):
    """A fit step's (dp, da, dsig) by the latents' names: the pose gradient split into ``p_pos`` and, with ``ori``, ``p_ori`` (column
    slices of dp), ``a``, and ``gaussian_window`` where dsig is not None."""
    grads = {"p_pos": dp[..., :n_pos], "a": da}
    if ori:
        grads["p_ori"] = dp[..., n_pos:]
    if dsig is not None:
        grads["gaussian_window"] = dsig
    return grads


def _sgd_step(nef, nef_params, obs, lat, lrs, xs, qs, ys, ws, channel, optimize_gaussian_window, rows, **kw):
    """One inner step: obs.fit_step at ``lat``, then the meta-SGD update with the gradient of the batch-mean loss times B
    (pde_trainer.py:206), scaled by the learned rates (:215-219); sigma only moves when asked to (:209-212).  ``rows``: None, or the
    list that takes the step's loss_b."""
    n_ori = nef.cross_attn_invariant.num_z_ori_dims
    res = obs.fit_step(nef, nef_params, xs, qs, _pose(lat, n_ori), lat["a"], lat.get("gaussian_window"), ys, ws, channel, True, **kw)
    if rows is not None:
        rows.append(res[5])
    grads = split_latent_grads(res[1], res[2], res[3] if optimize_gaussian_window else None, lat["p_pos"].shape[-1], n_ori > 0)
    return meta_sgd_update(lat, grads, lrs, ys.shape[0])


def _fit_loop(nef, nef_params, obs, latents0, lrs, data, masks, w, channel, optimize_gaussian_window, noise_pos, generator,
              normalize_weights, per_signal_loss):
    """The loop behind inner_loop and inner_loop_cells (``obs`` says which): gather once, jitter once, then the body on step s's share
    of the gather, with the shared-latent hint where step 0 may take it.  ``w``: the full weights next to ``data``, float32 and
    contiguous, or None; ``channel``: they are per value."""
    B, S, per_signal = data.shape[0], masks.shape[-1] - 1, masks.dim() == 3
    lat, xs_all, qs_all, ys_all, losses, ws_all = obs.gather(latents0, data, masks, w, channel, FUSED_FIT_INPUTS)
    if normalize_weights:
        if ws_all is None:
            raise ValueError("normalize_weights needs sampled weights: pass weights or per-signal masks")
        ws_all = normalize_sampled_weights(ws_all, channel=channel)
    if noise_pos:                                                                             # pde_trainer.py:162-167
        lat["p_pos"] = lat["p_pos"] + torch.randn(lat["p_pos"].shape, generator=generator,
                                                  device="cpu").to(lat["p_pos"].device) * noise_pos
    more = {"return_errors": True} if per_signal_loss else {}

    def inputs(s):
        xs, qs, ws = obs.step_inputs(xs_all, qs_all, ws_all, s, B, per_signal)
        return xs, qs, ys_all[s], ws
    return _fit_body(nef, nef_params, obs, lat, lrs, inputs, S, losses, channel, optimize_gaussian_window, per_signal_loss,
                     lambda s: {**more, **(_shared_kw(nef, s, per_signal, noise_pos, step=obs.STEP) if obs.hints(channel) else {})})


def _fit_given(nef, nef_params, obs, latents0, lrs, inputs, B, S, dev, channel, optimize_gaussian_window, per_signal_loss):
    """The fit of fit_cell_averages and fit_linear_observations: the body on inputs the caller chose -- ``inputs(s)`` -> step s's (xs, qs,
    ys, ws), already a batch -- from the latent initialisation, never with the shared-latent hint."""
    lat, losses = _fresh(latents0, B, S + 1, dev)
    return _fit_body(nef, nef_params, obs, lat, lrs, inputs, S, losses, channel, optimize_gaussian_window, per_signal_loss,
                     lambda s: {"return_errors": per_signal_loss})


def _fit_body(nef, nef_params, obs, lat, lrs, inputs, S, losses, channel, optimize_gaussian_window, per_signal_loss, step_kw):
    """What every meta-SGD fit runs, whatever it observes and however it chose its inputs: S steps from the signals' latents ``lat``,
    step s on ``inputs(s)`` = (xs, qs, ys, ws) with the keywords ``step_kw(s)`` and its loss in ``losses[s]``; then the loss on
    ``inputs(S)`` at the fitted latents in ``losses[S]``.  Returns (that loss, the latents), with ``per_signal_loss`` followed by
    loss_b (S + 1, B)."""
    rows = [] if per_signal_loss else None                              # loss_b, with per_signal_loss
    for s in range(S):                                                  # pde_trainer.py:191
        xs, qs, ys, ws = inputs(s)
        lat = _sgd_step(nef, nef_params, obs, lat, lrs, xs, qs, ys, ws, channel, optimize_gaussian_window, rows, loss_out=losses[s:s + 1],
                        **step_kw(s))
    xs, qs, ys, ws = inputs(S)
    lb = obs.final_loss(nef, nef_params, xs, qs, _pose(lat, nef.cross_attn_invariant.num_z_ori_dims), lat["a"], lat.get("gaussian_window"),
                        ys, ws, channel, losses[S:], per_signal_loss)
    if per_signal_loss:
        rows.append(lb)
        return losses[S], lat, torch.stack(rows)
    return losses[S], lat


@torch.no_grad()
def decode(nef, nef_params, coords, p, a, window, chunk=None):
    """Reconstruct (B, N, O) on the full grid (pde_trainer.py:393-402).  The fused kernel tiles over
    queries itself, so ``chunk`` is optional (the reference chunks by max_num_sampled_points)."""
    x = _batched(coords, None, p.shape[0])[0]
    if chunk is None:
        return nef.apply(nef_params, x, p, a, window)
    outs = [nef.apply(nef_params, x[:, i:i + chunk], p, a, window) for i in range(0, x.shape[1], chunk)]
    return torch.cat(outs, dim=1)
