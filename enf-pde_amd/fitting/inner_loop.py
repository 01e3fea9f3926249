"""MAML inner loop and decode on the HIP path (trainers/pde_trainer.py:122-235, 389-405).

``inner_loop`` (point values) and fitting/cells.py: ``inner_loop_cells`` (cell averages) are one loop, ``_fit_loop``: what differs between
the two kinds of observation -- the gather, the decoder's calls, the form of the last loss, when step 0 may share its forward -- it asks
of the observation value it is given (fitting/observations.py)."""
import functools
import inspect

import torch

from .. import _lib
from .weights import gather_point_weights


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


def _gather_inputs(latents0, coords, img, masks, weights, channel):
    """What inner_loop prepares before its first step, for every weight form and both mask layouts: the signals' copies of the latent
    initialisation (pde_trainer.py:157-159), the coordinates and targets of all S+1 steps gathered once (:193-197), one zeroed loss
    accumulator per step and the gathered weights -- (lat, xs_all, ys_all, losses, ws_all), ws_all None without weights on shared
    masks.  ONE launch (_fit_inputs) instead of eight framework kernels, or the same in torch ops."""
    fused = _fit_inputs(latents0, coords, img, masks, weights, channel=channel) if FUSED_FIT_INPUTS else None
    if fused is not None:
        return fused if len(fused) == 5 else (*fused, None)
    B = img.shape[0]
    lat = {k: v.detach().repeat_interleave(B, dim=0) for k, v in latents0.items()}       # (a fresh tensor)
    losses = torch.zeros(masks.shape[-1], device=img.device, dtype=torch.float32)        # zeroed in one fill
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
    from .observations import Points                 # (observations imports this module)
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
    """The loop behind inner_loop and inner_loop_cells (fitting/observations.py: ``obs`` says which): gather once, jitter once, S steps,
    the loss on the last mask.  ``w``: the full weights next to ``data``, float32 and contiguous, or None; ``channel``: they are per value."""
    B, S, per_signal = data.shape[0], masks.shape[-1] - 1, masks.dim() == 3
    lat, xs_all, qs_all, ys_all, losses, ws_all = obs.gather(latents0, data, masks, w, channel)
    if normalize_weights:
        if ws_all is None:
            raise ValueError("normalize_weights needs sampled weights: pass weights or per-signal masks")
        ws_all = normalize_sampled_weights(ws_all, channel=channel)
    if noise_pos:                                                                             # pde_trainer.py:162-167
        lat["p_pos"] = lat["p_pos"] + torch.randn(lat["p_pos"].shape, generator=generator,
                                                  device="cpu").to(lat["p_pos"].device) * noise_pos
    rows = [] if per_signal_loss else None                              # loss_b, with per_signal_loss
    more = {"return_errors": True} if per_signal_loss else {}
    for s in range(S):                                                  # pde_trainer.py:191
        xs, qs, ws = obs.step_inputs(xs_all, qs_all, ws_all, s, B, per_signal)
        lat = _sgd_step(nef, nef_params, obs, lat, lrs, xs, qs, ys_all[s], ws, channel, optimize_gaussian_window, rows,
                        loss_out=losses[s:s + 1], **more, **(_shared_kw(nef, s, per_signal, noise_pos, step=obs.STEP) if obs.hints(channel) else {}))
    xs, qs, ws = obs.step_inputs(xs_all, qs_all, ws_all, S, B, per_signal)
    lb = obs.final_loss(nef, nef_params, xs, qs, _pose(lat, nef.cross_attn_invariant.num_z_ori_dims), lat["a"], lat.get("gaussian_window"),
                        ys_all[S], ws, channel, losses[S:], per_signal_loss)
    if per_signal_loss:
        rows.append(lb)
        return losses[S], lat, torch.stack(rows)
    return losses[S], lat


@torch.no_grad()
def decode(nef, nef_params, coords, p, a, window, chunk=None):
    """Reconstruct (B, N, O) on the full grid (pde_trainer.py:393-402).  The fused kernel tiles over
    queries itself, so ``chunk`` is optional (the reference chunks by max_num_sampled_points)."""
    B = p.shape[0]
    x = coords[None].expand(B, -1, -1) if coords.dim() == 2 else coords
    if chunk is None:
        return nef.apply(nef_params, x, p, a, window)
    outs = [nef.apply(nef_params, x[:, i:i + chunk], p, a, window) for i in range(0, x.shape[1], chunk)]
    return torch.cat(outs, dim=1)
