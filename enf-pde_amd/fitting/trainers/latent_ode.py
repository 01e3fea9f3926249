"""The latent-ODE arithmetic both trainers share: roll the latents of frame 0 out with the latent ODE, decode every frame
at (a random subset of) the grid points and compare with the trajectory (pde_trainer.py:429-481 from the fitted latents on;
nonmaml_pde_trainer.py:257-307 from the table's latents on -- the same lines).  The MAML trainer gets its frame-0 latents
from the inner loop, the auto-decoder trainer from its latent table; from there on there is one copy, here.

``LatentODEMixin`` expects ``self.config`` (node.dt, node.method, training.max_num_sampled_points), ``self.nef``,
``self.ode_model``, ``self.coords`` and ``self.graph_ode_training``.
"""
import torch

from ..inner_loop import _pose
from ..weights import LossWeights, loss_tensor, weighted_mse
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
    ``weights`` (B, T, N) also their gather ws (B T, n); per-channel weights (B, T, N, O) give ws (B T, n, O)."""
    B, T, N, O = traj.shape
    if point_masks is None:
        xs, ys = coords[None].expand(B * T, -1, -1), traj.reshape(B * T, N, O)
        return (xs, ys) if weights is None else (xs, ys, weights.reshape(B * T, N, *weights.shape[3:]))
    n_s = point_masks.shape[1]
    xs = coords[point_masks][None].expand(B, -1, -1, -1).reshape(B * T, n_s, -1)
    ys = torch.gather(traj, 2, point_masks[None, :, :, None].expand(B, -1, -1, O)).reshape(B * T, n_s, O)
    if weights is None:
        return xs, ys
    if weights.dim() == 4:
        return xs, ys, torch.gather(weights, 2, point_masks[None, :, :, None].expand(B, -1, -1, O)).reshape(B * T, n_s, O)
    return xs, ys, torch.gather(weights, 2, point_masks[None].expand(B, -1, -1)).reshape(B * T, n_s)


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
                     normalize=True, channel_weights=None):
        """Roll ``lat`` out over the frames of ``trajectory`` (B, T, *grid, O), decode every frame in ONE nef.apply over the
        B T signal-frames (at ``max_num_sampled_points`` random grid points per frame when the grid is larger) and return the
        mean squared error.  ``point_masks`` (T, n_s) long, or None to draw them from ``generator``.
        ``weights``: None, or (N,) / (B, N) / (B, T, N) loss weights on the full grid (fitting/weights.py), normalised to mean 1
        per signal-frame before the points are sampled unless ``normalize`` is False; they are gathered with the point masks.
        ``channel_weights``: None, or per-channel (N, O) / (B, N, O) / (B, T, N, O) weights, treated alike; not with ``weights``."""
        B, T = trajectory.shape[:2]
        N, n_s = self.coords.shape[0], self.config.training.max_num_sampled_points
        fw = LossWeights.build(weights, channel_weights, B, N, trajectory.shape[-1], T=T, normalize=normalize, device=trajectory.device)
        sol = self.rollout(ode_params, lat, T, graph=graph)
        p_fl, a_fl, w_fl = (None if v is None else v.reshape(B * T, *v.shape[2:]) for v in sol)
        traj = trajectory.reshape(B, T, -1, trajectory.shape[-1])
        if n_s < N:                                                               # pde_trainer.py:446-471
            if point_masks is None:
                point_masks = draw_point_masks(N, n_s, T, generator, self.coords.device)
        else:
            point_masks = None
        xs, ys, *ws = sample_frames(self.coords, traj, point_masks, loss_tensor(fw))
        recon = self.nef.apply(nef_params, xs, p_fl, a_fl, w_fl)
        return weighted_mse(recon, ys, ws[0]) if ws else ((recon - ys) ** 2).mean()

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
