"""The latent-ODE arithmetic both trainers share: roll the latents of frame 0 out with the latent ODE, decode every frame
at (a random subset of) the grid points and compare with the trajectory (pde_trainer.py:429-481 from the fitted latents on;
nonmaml_pde_trainer.py:257-307 from the table's latents on -- the same lines).  The MAML trainer gets its frame-0 latents
from the inner loop, the auto-decoder trainer from its latent table; from there on there is one copy, here.
Whether the trajectory holds point values or cell means is asked of the observation value (fitting/observations.py: ``observed`` parses
the step's four keywords): ``rollout_loss`` has one body for both, ``_errors`` is the one decode-free evaluation in chunks, and
``sample_frames`` / ``sample_cell_frames`` are the two kinds' frame samplers by their old names.

``LatentODEMixin`` expects ``self.config`` (node.dt, node.method, training.max_num_sampled_points), ``self.nef``,
``self.ode_model``, ``self.coords`` and ``self.graph_ode_training``.
"""
import torch

from ..inner_loop import _pose
from ..observations import Cells, Points, cell_loss_weights, observed      # (cell_loss_weights: re-exported)
from ..weights import loss_tensor, weighted_mse
from .trainer_utils.solvers import solve_latent_ode


def _leaves(tree):
    """Leaves of a nested parameter dict in a fixed (sorted-key) order."""
    out = []
    for k in sorted(tree):
        out += _leaves(tree[k]) if isinstance(tree[k], dict) else [tree[k]]
    return out


def _unflatten(tree, leaves):
    it = iter(leaves)

    def build(t):
        return {k: (build(t[k]) if isinstance(t[k], dict) else next(it)) for k in sorted(t)}
    return build(tree)


def draw_point_masks(num_points, num_sampled, num_frames, generator=None, device=None):
    """(num_frames, num_sampled) long: every frame draws its own permutation of the grid points and keeps the first
    ``num_sampled``; the signals of a batch share them (pde_trainer.py:446-453, nonmaml_pde_trainer.py:273-283)."""
    masks = torch.stack([torch.randperm(num_points, generator=generator)[:num_sampled] for _ in range(num_frames)])
    return masks if device is None else masks.to(device)


def sample_frames(coords, traj, point_masks=None, weights=None):
    """Queries and targets of the B T signal-frames: ``coords`` (N, dx), ``traj`` (B, T, N, O), ``point_masks`` (T, n_s) long or
    None for the full grid.  Returns xs (B T, n, dx) and ys (B T, n, O), signal-major like the flattened roll-out; with
    ``weights`` (B, T, N) also their gather ws (B T, n); per-channel weights (B, T, N, O) give ws (B T, n, O).
    (fitting/observations.py: Points.sample_frames)"""
    xs, _, ys, ws = Points(coords).sample_frames(traj, point_masks, weights)
    return (xs, ys) if weights is None else (xs, ys, ws)


def sample_cell_frames(cells, traj, cell_masks=None, weights=None):
    """sample_frames on cell averages: ``cells`` = (x (M G, dx), q (M G,) or None, group), ``traj`` (B, T, M, O) cell means,
    ``cell_masks`` (T, m_s) long CELL indices or None for all M.  Returns (xs, qs, ys, ws) of Cells.sample_frames."""
    return Cells(*cells, traj.shape[2]).sample_frames(traj, cell_masks, weights)


class LatentODEMixin:
    def rollout(self, ode_params, lat, num_frames, graph=False):
        """Latents of ``num_frames`` frames from those of frame 0: (B, T, Z, .) each (pde_trainer.py:432-441).  ``lat``: the
        latent dict of the inner loop, or the (p, a, window) tuple of an auto-decoder.
        graph=True (inference): every derivative evaluation replays one captured hipGraph (PonitaODEGen.graphed)."""
        cfg = self.config
        if isinstance(lat, dict):
            lat = (_pose(lat, self.nef.cross_attn_invariant.num_z_ori_dims), lat["a"], lat.get("gaussian_window"))
        z0 = tuple(lat)
        if graph and hasattr(self.ode_model, "graphed") and not torch.is_grad_enabled():
            # one capture per (parameter tensors, latent shapes): validation sweeps many batches with the same parameters
            leaves = _leaves(ode_params)
            key = (tuple(id(t) for t in leaves), tuple(None if v is None else tuple(v.shape) for v in z0))
            hit = getattr(self, "_ode_graph", None)
            if hit is None or hit[0] != key:
                hit = (key, self.ode_model.graphed(ode_params, z0), leaves)      # (leaves kept alive: ids stay unique)
                self._ode_graph = hit
            f = hit[1]
            return solve_latent_ode(lambda z, t: f(z), z0, 0, num_frames - 1, cfg.node.dt, method=cfg.node.method)
        if graph and torch.is_grad_enabled() and hasattr(self.ode_model, "graphed_train") and z0[1].is_cuda:
            # training: one captured (forward, backward) pair per derivative evaluation of the roll-out; ``ode_params`` must
            # be the persistent leaves of _ode_static_leaves (the graphs keep their addresses)
            leaves = _leaves(ode_params)
            n_eval = (num_frames - 1) * (4 if cfg.node.method == "rk4" else 1)
            key = (tuple(id(t) for t in leaves), tuple(None if v is None else tuple(v.shape) for v in z0), n_eval)
            cache = self.__dict__.setdefault("_ode_train_graphs", {})
            if key not in cache:
                if len(cache) >= 4:
                    cache.clear()
                cache[key] = (self.ode_model.graphed_train(ode_params, z0, n_eval), leaves)
            calls = iter(cache[key][0])
            return solve_latent_ode(lambda z, t: next(calls)(z), z0, 0, num_frames - 1, cfg.node.dt, method=cfg.node.method)
        return solve_latent_ode(lambda z, t: self.ode_model.apply(ode_params, z), z0, 0, num_frames - 1, cfg.node.dt,
                                method=cfg.node.method)

    def _ode_static_leaves(self, ode_params):
        """The ODE parameters as PERSISTENT leaf tensors that require grad, holding the current values: captured training
        evaluations read their parameters by address, the optimiser hands out new tensors every step."""
        cur = _leaves(ode_params)
        st = getattr(self, "_ode_static", None)
        if st is None or len(st) != len(cur) or any(a.shape != b.shape or a.device != b.device for a, b in zip(st, cur)):
            st = [t.detach().clone().requires_grad_(True) for t in cur]
            self._ode_static = st
            self.__dict__.pop("_ode_train_graphs", None)
        else:
            with torch.no_grad():
                torch._foreach_copy_(st, [t.detach() for t in cur])
        return st

    def _ode_train_leaves(self, ode_params):
        if self.graph_ode_training and _leaves(ode_params)[0].is_cuda:
            return self._ode_static_leaves(ode_params), True
        return [t.detach().requires_grad_(True) for t in _leaves(ode_params)], False

    def rollout_loss(self, nef_params, ode_params, lat, trajectory, point_masks=None, generator=None, graph=False, weights=None,
                     normalize=True, channel_weights=None, cells=None, cell_channel_weights=None, fused=False):
        """Roll ``lat`` out over the frames of ``trajectory`` (B, T, *grid, O), decode every frame in ONE nef.apply over the
        B T signal-frames (at ``max_num_sampled_points`` random grid points per frame when the grid is larger) and return the
        mean squared error.  ``point_masks`` (T, n_s) long, or None to draw them from ``generator``.
        ``weights``: None, or (N,) / (B, N) / (B, T, N) loss weights on the full grid (fitting/weights.py), normalised to mean 1
        per signal-frame before the points are sampled unless ``normalize`` is False; they are gathered with the point masks.
        ``channel_weights``: None, or per-channel (N, O) / (B, N, O) / (B, T, N, O) weights, treated alike; not with ``weights``.
        ``cells``: None, or (x (M G, dx), q (M G,) or None, group): ``trajectory`` holds (B, T, M, O) CELL MEANS, ``point_masks`` (T, m_s)
        index cells -- max(1, max_num_sampled_points // group) of them per frame when there are more --, the B T signal-frames are
        decoded at the sampled cells' quadrature rows and the loss is the grouped one (nef.cell_mse).  ``weights`` are then per
        observation, (M,) / (B, M) / (B, T, M); ``cell_channel_weights`` (M, O) / (B, M, O) / (B, T, M, O) weigh every observed value
        (not together with ``weights``); ``channel_weights`` with ``cells`` is a ValueError.
        ``fused`` (cells only): the loss does not decode -- nef.cell_fit_loss, ONE grouped fit step over the B T signal-frames whose
        latent gradients the backward scales; the nef weights get no gradient (ode_train_step: they are frozen there)."""
        if fused and cells is None:
            raise ValueError("fused= goes with cells=")
        B, T = trajectory.shape[:2]
        traj = trajectory.reshape(B, T, -1, trajectory.shape[-1])
        obs, fw = observed(self.coords, weights, channel_weights, cells, cell_channel_weights, B, traj.shape[2], traj.shape[3], T=T,
                           normalize=normalize, device=traj.device, nef=self.nef)
        n_s = obs.num_sampled(self.config.training.max_num_sampled_points)
        if n_s >= obs.num:                                                        # pde_trainer.py:446-471
            point_masks = None
        elif point_masks is None:
            point_masks = draw_point_masks(obs.num, n_s, T, generator, traj.device)
        sol = self.rollout(ode_params, lat, T, graph=graph)
        p_fl, a_fl, w_fl = (None if v is None else v.reshape(B * T, *v.shape[2:]) for v in sol)
        xs, qs, ys, ws = obs.sample_frames(traj, point_masks, loss_tensor(fw))
        if fused:
            return obs.fused_loss(self.nef, nef_params, xs, qs, p_fl, a_fl, w_fl, ys, ws)
        return obs.loss_of_decode(self.nef, self.nef.apply(nef_params, xs, p_fl, a_fl, w_fl), ys, qs, ws, weighted_mse)

    @torch.no_grad()
    def _errors(self, nef_params, obs, p, a, window, targets, lw=None, chunk=None):
        """err (n, num) of ``n`` signals with latents (p, a, window) against ALL ``num`` observations ``targets`` (n, num, O), without a
        decode: obs.eval (nef.eval_loss / nef.eval_cell_loss) in chunks of ``chunk`` observations (None: one call), every chunk's errors
        written into the one tensor, so that nef.signal_losses sums them once, in a fixed order -- the same bits for every chunking.
        ``lw``: a LossWeights or None, its tensor read as (n, num[, O])."""
        n, num = targets.shape[:2]
        w = None if lw is None else lw.w.reshape(n, num, *lw.w.shape[lw.w.dim() - lw.channel:])
        err = torch.empty((n, num), device=targets.device, dtype=torch.float32)
        step = num if chunk is None else max(1, int(chunk))
        for i in range(0, num, step):
            part = slice(i, min(i + step, num))
            _, e = obs.eval(self.nef, nef_params, part, n, p, a, window, targets[:, part], None if w is None else w[:, part],
                            lw is not None and lw.channel)
            err[:, part] = e
        return err

    @torch.no_grad()
    def _val_cells(self, nef_params, ode_params, lat, trajectory, num_in, obs, fw=None, return_frames=False, chunk=None):
        """The validation roll-out on cell means ``trajectory`` (B, T, M, O) from frame-0 latents ``lat``: roll out, evaluate all M cells
        of all B T signal-frames without a decode (_errors; ``chunk`` cells per call, default max_num_sampled_points // group) and
        return (mean of loss_b over the first ``num_in`` frames, mean beyond them -- zero where there are none), with ``return_frames``
        followed by loss_b (B, T)."""
        B, T, M, O = trajectory.shape
        if isinstance(lat, dict):
            lat = {k: v.detach() for k, v in lat.items()}
        else:
            lat = tuple(None if v is None else v.detach() for v in lat)
        sol = self.rollout(ode_params, lat, T, graph=T > 4)
        p_fl, a_fl, w_fl = (None if v is None else v.reshape(B * T, *v.shape[2:]) for v in sol)
        if chunk is None:
            chunk = obs.num_sampled(self.config.training.max_num_sampled_points)
        loss_b = self.nef.signal_losses(self._errors(nef_params, obs, p_fl, a_fl, w_fl, trajectory.reshape(B * T, M, O), fw, chunk)).reshape(B, T)
        e_in = loss_b[:, :num_in].mean()
        e_out = loss_b[:, num_in:].mean() if T > num_in else loss_b.new_zeros(())
        return (e_in, e_out, loss_b) if return_frames else (e_in, e_out)

    def _horizon_errors(self, recon, trajectory, num_in, fw=None):
        """(mean squared error of ``recon`` over the first ``num_in`` frames of ``trajectory`` (B, T, *grid, O), the same beyond them, zero
        where there are none); with ``fw``, a LossWeights over the (B, T, N) signal-frame points, the two weighted_mse."""
        T = trajectory.shape[1]
        if fw is None:
            err = (recon - trajectory) ** 2
            return err[:, :num_in].mean(), (err[:, num_in:].mean() if T > num_in else err.new_zeros(()))
        rec, tgt = (v.reshape(*fw.w.shape[:3], -1) for v in (recon, trajectory))
        return weighted_mse(rec[:, :num_in], tgt[:, :num_in], fw.frame_range(0, num_in).w), \
            (weighted_mse(rec[:, num_in:], tgt[:, num_in:], fw.frame_range(num_in, T).w) if T > num_in else recon.new_zeros(()))
