"""Auto-decoder (non-meta) ENF trainer, mirroring experiments/fitting/trainers/nonmaml_pde_trainer.py: the nef phase, the
latent-ODE phase, the validation roll-out and the validation protocol (validate_epoch, with its latent-only fit step).

Every training signal owns a row of latents in a PositionOrientationFeatureAutodecoder (:37-45); one nef step is

    recon_loss, grads = jax.value_and_grad(self.enf_loss)(params, state, autodecoder_fn, trajectory, mask, traj_idx)   (:118)
    nef:          clip_by_global_norm(1.0) -> adamw(lr_enf)                                                        (:63-66,121-122)
    autodecoder:  adam(lr_codes) over the WHOLE latent table (rows outside the batch move by momentum only)          (:67,125-126)

with enf_loss = mean((nef.apply(params['nef'], coords[mask], *autodecoder(params['autodecoder'], traj_idx)) - state)^2)
(:309-341).  The gradient is first order, so it is exactly what the training path of the decoder provides (weight
gradients through the HIP pair kernels' activation store, latent gradients through the latent table).

The ODE phase (:173-199, 244-307) trains the latent ODE on the STORED latents: the rows of ``traj_idx`` are rolled out over
the first 10 frames (t0 = 0, tf = 9, node.dt, node.method), all B x 10 signal-frames are decoded in one nef.apply at
``max_num_sampled_points`` random grid points per frame and compared with the trajectory;

    ode:          clip_by_global_norm(1.0) -> adamw(lr_enf)       (:68-69 -- learning_rate_enf, not learning_rate_ode)

The reference differentiates the loss w.r.t. every parameter group and keeps the ODE's (:182-187); here only the ODE
parameters are differentiated: nef weights and table rows enter as constants, so the decoder's backward is its latent
backward alone (HIP pair kernels) -> solver -> ODE model.  From the latents on this is the arithmetic of the MAML trainer's
ode_loss / rollout; both trainers take it from latent_ode.LatentODEMixin.  ``val_step`` (:201-241) rolls the same rows out
over 20 frames, decodes the full grid in chunks of ``max_num_sampled_points`` and returns the errors of frames 0..9 and 10..19.
"""
from dataclasses import dataclass, field

import torch

from ..optim import Adam, AdamW, clip_by_global_norm, global_norm, scatter_rows, table_adam_update
from ..parallel import allreduce_mean_
from ..inner_loop import decode, split_latent_grads
from ..weights import cut_frames, loss_tensor, weighted_mse
from ..observations import observed
from .latent_ode import LatentODEMixin, _leaves, _unflatten
from .pde_trainer import _tree_from_tensors

TRAIN_FRAMES, VAL_FRAMES = 10, 20            # fixed in the reference (:206,241,252), not read from the dataset config


@dataclass
class NonMetaTrainState:
    params: dict
    nef_opt_state: dict
    autodecoder_opt_state: dict
    ode_opt_state: dict = None
    step: int = 0
    rng: torch.Generator = field(default_factory=lambda: torch.Generator().manual_seed(0))


class NonMetaPDETrainer(LatentODEMixin):
    """``config`` fields used: optimizer.learning_rate_enf, optimizer.learning_rate_codes,
    training.max_num_sampled_points; with an ``ode_model`` also node.dt, node.method and, for the phase schedule,
    training.nef / training.ode .train_from_epoch / .train_until_epoch.
    ``autodecoder``: enf_pde_amd.enf.latents.autodecoder.PositionOrientationFeatureAutodecoder sized for the training set.
    ``ode_model`` (keyword only): PonitaODEGen / MLPODE, the second value of get_model_pde(cfg).  Without one the train state
    has no ODE entries and ode_train_step / val_step raise ValueError.

    ``training.graph_ode_training`` is honoured as in the MAML trainer (ode_train_step replays captured derivative
    evaluations; off by default).  Validation signals need no second shell here: a shell only indexes the table it is given,
    so val_step takes the shell as an argument and reads ``state.params['autodecoder']`` through it (:209-210), which the
    caller has replaced by the validation table as validate_epoch does (:437-444).

    ``sample_observed`` (keyword only): a nef step that is given ``weights`` draws its point subset per signal from that signal's
    observed points ({weight > 0}; make_signal_masks, from the state's generator) instead of one subset shared by the batch, with
    the weights rescaled by fitting/weights.py: observed_sampling_weights so that the loss still estimates the full-grid weighted
    mean (without it signal b's loss would be N / n_b times the shared subset's).  Off by default.  (val_step fits nothing here -- it reads stored latents -- so it has no drop-out variant.)"""

    def __init__(self, config, nef, autodecoder, coords, seed=42, *, ode_model=None, sample_observed=False):
        self.sample_observed = bool(sample_observed)
        self.config, self.nef, self.autodecoder, self.coords, self.seed = config, nef, autodecoder, coords, seed
        self.ode_model = ode_model
        self.graph_ode_training = bool(getattr(getattr(config, "training", None), "graph_ode_training", False))
        self.nef_opt = AdamW(config.optimizer.learning_rate_enf)                # after clip_by_global_norm(1.0)
        self.autodecoder_opt = Adam(config.optimizer.learning_rate_codes)
        self.ode_opt = AdamW(config.optimizer.learning_rate_enf) if ode_model is not None else None    # after clip (:68-69)

    def init_train_state(self, nef_params=None, ode_params=None):
        dev = self.coords.device
        g = torch.Generator().manual_seed(self.seed)
        ad = self.autodecoder.init(g, device=dev)
        if nef_params is None:
            nef_params = self.nef.init(g, device=dev)
        params = {"nef": nef_params, "autodecoder": ad}
        ode_opt_state = None
        if self.ode_model is not None:                                           # :80-81,89: shapes from row 0 of the table
            if ode_params is None:
                ode_params = self.ode_model.init(self.seed + 1, self.autodecoder.apply(ad, torch.tensor([0])), device=dev)
            params["ode_params"] = ode_params
            ode_opt_state = self.ode_opt.init(_leaves(ode_params))
        return NonMetaTrainState(params=params,
                                 nef_opt_state=self.nef_opt.init(self.nef.param_tensors(nef_params)),
                                 autodecoder_opt_state=self.autodecoder_opt.init(list(ad["params"].values())),
                                 ode_opt_state=ode_opt_state, step=0, rng=g)

    def save_checkpoint(self, state, path, epoch=0):
        """_base_pde_trainer.py:192-202: the whole train state (parameters, every optimiser's count / mu / nu, step, rng)
        and the config, in one .npz (enf_pde_amd/checkpoint.py: save_train_state)."""
        from ...checkpoint import save_train_state
        save_train_state(path, state, config=self.config, epoch=epoch)

    def load_checkpoint(self, path, **init_kwargs):
        """_base_pde_trainer.py:204-237: restore into a freshly initialised state of this trainer.  Returns (state, epoch)."""
        from ...checkpoint import load_train_state
        state, epoch, _ = load_train_state(path, self.init_train_state(**init_kwargs))
        return state, epoch

    def _fit(self, state, initial_state, mask, weights, normalize, channel_weights, cells, cell_channel_weights):
        """What a nef step fits: (obs, targets (B, n, O), xs (B, n G, dx), qs (B, n G) or None, ws (B, n[, O]) or None, whether ws is per
        value) -- the four keywords parsed (fitting/observations.py: observed) and the subset drawn by obs.subset, the one place where a
        nef step draws from ``state.rng``: loss_and_grads and fit_latents_step both call it, so the two consume the generator alike."""
        img = initial_state.reshape(initial_state.shape[0], -1, initial_state.shape[-1])
        obs, lw = observed(self.coords, weights, channel_weights, cells, cell_channel_weights, *img.shape, normalize=normalize, device=img.device)
        img, xs, qs, lw = obs.subset(img, mask, lw, self.config.training.max_num_sampled_points, state.rng, self.sample_observed)
        return obs, img, xs, qs, loss_tensor(lw), lw is not None and lw.channel

    def loss_and_grads(self, state, initial_state, traj_idx, mask=None, weights=None, normalize=True, channel_weights=None, cells=None,
                       cell_channel_weights=None):
        """(recon_loss, grads['nef'] as 46 tensors, grads['autodecoder'] as dense tensors like the latent table).
        ``weights``: None, or (N,) / (B, N) loss weights on the full grid (fitting/weights.py), normalised to mean 1 per signal
        before ``mask`` and the point sampling unless ``normalize`` is False.
        ``channel_weights``: None, or (N, O) / (B, N, O) weights per value (mean 1 over each signal's N * O values unless
        ``normalize`` is False), for fields whose variables are observed separately; not together with ``weights``.
        ``cells``: None, or (x (M G, dx), q (M G,) or None, group): ``initial_state`` holds (B, M, O) cell means, ``mask`` and
        ``weights`` are per observation (Cells.subset), and the loss is the grouped one (nef.cell_mse) of the decode at the sampled
        cells' quadrature points.  ``channel_weights`` with ``cells`` is a ValueError; ``cell_channel_weights`` (M, O) / (B, M, O) are
        the weights per observed value of the cells (not together with ``weights``)."""
        obs, img, xs, qs, ws, channel = self._fit(state, initial_state, mask, weights, normalize, channel_weights, cells, cell_channel_weights)
        P = state.params["autodecoder"]["params"]
        names = list(P.keys())
        leaves = {k: P[k].detach().requires_grad_(True) for k in names}
        w = [t.detach().requires_grad_(True) for t in self.nef.param_tensors(state.params["nef"])]
        p, a, window = self.autodecoder.apply({"params": leaves}, traj_idx)               # :338
        loss = obs.loss_of_decode(self.nef, self.nef.apply(_tree_from_tensors(w, self.nef), xs, p, a, window), img, qs, ws, weighted_mse)      # :341
        g = torch.autograd.grad(loss, w + [leaves[k] for k in names], allow_unused=True)
        gw = [torch.zeros_like(t) if gi is None else gi for t, gi in zip(w, g[:len(w)])]
        ga = [torch.zeros_like(leaves[k]) if gi is None else gi for k, gi in zip(names, g[len(w):])]
        return loss.detach(), gw, dict(zip(names, ga))

    def _step(self, state, batch, mask, update_nef, weights=None, normalize=True, channel_weights=None, cells=None, cell_channel_weights=None):
        initial_state, traj_idx = batch
        loss, gw, ga = self.loss_and_grads(state, initial_state, traj_idx, mask, weights, normalize, channel_weights, cells, cell_channel_weights)
        names = list(ga.keys())
        flat = gw + [ga[k] for k in names] + [loss.reshape(1)]
        allreduce_mean_(flat, weight=initial_state.shape[0])
        loss = flat[-1][0]
        nef_params, nef_opt_state = state.params["nef"], state.nef_opt_state
        if update_nef:
            new_w, nef_opt_state = self.nef_opt.update(clip_by_global_norm(gw, 1.0), state.nef_opt_state,
                                                       self.nef.param_tensors(state.params["nef"]))
            nef_params = _tree_from_tensors(new_w, self.nef)
        P = state.params["autodecoder"]["params"]
        new_p, ad_state = self.autodecoder_opt.update([ga[k] for k in names], state.autodecoder_opt_state, [P[k] for k in names])
        params = dict(state.params, nef=nef_params, autodecoder={"params": dict(zip(names, new_p))})    # ode_params carried over
        return loss, NonMetaTrainState(params=params, nef_opt_state=nef_opt_state, autodecoder_opt_state=ad_state,
                                       ode_opt_state=state.ode_opt_state, step=state.step + 1, rng=state.rng)

    def nef_train_step(self, state, batch, mask=None, weights=None, normalize=True, channel_weights=None, cells=None,
                       cell_channel_weights=None):
        """batch = (initial states (B, ..., O), trajectory indices (B,) long)   (:101-137); ``weights`` / ``channel_weights`` /
        ``cells`` / ``cell_channel_weights`` as in loss_and_grads"""
        return self._step(state, batch, mask, True, weights, normalize, channel_weights, cells, cell_channel_weights)

    def nef_train_step_autodec_only(self, state, batch, mask=None, weights=None, normalize=True, channel_weights=None, cells=None,
                                    cell_channel_weights=None):
        """Only the latents move (:139-171)."""
        return self._step(state, batch, mask, False, weights, normalize, channel_weights, cells, cell_channel_weights)

    @torch.no_grad()
    def fit_latents_step(self, state, batch, mask=None, weights=None, normalize=True, channel_weights=None, per_signal_loss=False,
                         cells=None, cell_channel_weights=None):
        """nef_train_step_autodec_only (:139-171) on the native latent-only path: same arguments, same (loss, new_state), same draw
        from ``state.rng`` (_fit), but nothing that only the weights need is computed.  The rows ``traj_idx`` of the table
        are read under no_grad, ONE nef.mse_value_and_latent_grads (enf_fit_step_w: forward, fused weighted loss, backward to the
        latents; neither ``out`` nor an autograd graph nor a weight gradient exists) returns the loss and the gradient w.r.t.
        those rows, and ONE enf_table_adam_update (optim.table_adam_update) applies optax adam to the whole table from them: rows
        outside the batch move by their momentum only, as in _step.  A shared point subset is passed as a stride-0 ``x``.
        The nef parameters, ``nef_opt_state`` and ``ode_opt_state`` are handed on untouched.  In a multi-rank run the gathered
        gradients are scattered to dense tensors, averaged with the loss by the flat all-reduce of _step, and the kernel runs in
        its dense form (idx = None).  This is the step validate_epoch repeats; nef_train_step_autodec_only stays as it is.
        ``channel_weights`` (N, O) / (B, N, O): the one fit call is enf_fit_step_cw; still one fit call and one table update.
        ``per_signal_loss``: the one fit call is enf_fit_step_e and a third value is returned, loss_b (B,): every signal's own loss
        (this rank's signals; loss_b.mean() is the loss before the all-reduce, up to rounding).  Same draw from ``state.rng``, same
        new state.
        ``cells``: None, or (x (M G, dx), q (M G,) or None, group): the batch holds (B, M, O) cell means (loss_and_grads) and the one
        fit call is the grouped step, enf_fit_step_g (nef.mse_value_and_cell_grads); the table update is the same.
        ``cell_channel_weights`` (M, O) / (B, M, O), with ``cells``: weights per observed value, the one fit call is enf_fit_step_gc."""
        initial_state, traj_idx = batch
        obs, img, xs, qs, ws, channel = self._fit(state, initial_state, mask, weights, normalize, channel_weights, cells, cell_channel_weights)
        P = state.params["autodecoder"]["params"]
        names = list(P.keys())
        tables = [P[k].detach() for k in names]
        p, a, window = self.autodecoder.apply({"params": dict(zip(names, tables))}, traj_idx)
        loss, dp, da, dwin, *errs = obs.fit_step(self.nef, state.params["nef"], xs, qs, p, a, window, img, ws, channel,
                                                 **({"return_errors": True} if per_signal_loss else {}))
        loss = loss.reshape(())
        by_name = split_latent_grads(dp, da, dwin, P["p_pos"].shape[-1])
        grads = [by_name.get(k) for k in names]
        grads = [torch.zeros((dp.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) if g is None else g
                 for g, t in zip(grads, tables)]                                             # e.g. a decoder without a window
        idx = traj_idx
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            grads = scatter_rows([g.float() for g in grads], traj_idx, tables[0].shape[0])
            flat = grads + [loss.reshape(1).clone()]
            allreduce_mean_(flat, weight=initial_state.shape[0])
            loss, idx = flat[-1][0], None
        new_tables, ad_state = table_adam_update(self.autodecoder_opt, state.autodecoder_opt_state, tables, grads, idx=idx)
        params = dict(state.params, autodecoder={"params": dict(zip(names, new_tables))})    # nef, ode_params carried over
        new_state = NonMetaTrainState(params=params, nef_opt_state=state.nef_opt_state, autodecoder_opt_state=ad_state,
                                      ode_opt_state=state.ode_opt_state, step=state.step + 1, rng=state.rng)
        return (loss, new_state, errs[1]) if per_signal_loss else (loss, new_state)

    # ------------------------------------------------------------------ latent-ODE phase (:173-307)
    def _need_ode(self, what):
        if self.ode_model is None:
            raise ValueError(f"NonMetaPDETrainer.{what} needs a latent ODE: build the trainer with ode_model=... "
                             "(the second value of get_model_pde(cfg))")

    def ode_loss(self, params, trajectory, traj_idx, point_masks=None, generator=None, graph=False, weights=None, normalize=True,
                 cells=None, cell_channel_weights=None, fused=False):
        """:244-307.  The first 10 frames of ``trajectory`` (B, T, *grid, O) against the roll-out of the table rows ``traj_idx``
        (B,) long, decoded at ``point_masks`` (frames, n_s) long -- one permutation of the grid per frame, shared by the signals of
        the batch; drawn from ``generator`` when None and max_num_sampled_points is smaller than the grid.
        ``cells`` / ``cell_channel_weights`` / ``fused``: the trajectory holds cell means (LatentODEMixin.rollout_loss)."""
        self._need_ode("ode_loss")
        trajectory = trajectory[:, :TRAIN_FRAMES]                                # :252
        weights = cut_frames(weights, slice(TRAIN_FRAMES))                       # (B, T, N): the frames the loss sees
        cell_channel_weights = cut_frames(cell_channel_weights, slice(TRAIN_FRAMES), channel=True)
        z0 = self.autodecoder.apply(params["autodecoder"], traj_idx)             # :255
        return self.rollout_loss(params["nef"], params["ode_params"], z0, trajectory, point_masks, generator, graph=graph,
                                 weights=weights, normalize=normalize, cells=cells, cell_channel_weights=cell_channel_weights, fused=fused)

    def ode_train_step(self, state, batch, point_masks=None, weights=None, normalize=True, cells=None, cell_channel_weights=None):
        """:173-199: one clip_by_global_norm(1) + AdamW step on the ODE parameters only.  ``batch`` = (trajectory (B, T, *grid, O),
        trajectory indices (B,) long) or the reference's (trajectory, _, traj_idx): the trajectory is ``batch[0]`` and the indices
        are ``batch[-1]``, whatever lies between is ignored.  nef weights, the latent table and their optimiser states are handed
        on untouched; the gradient runs decoder -> (HIP latent backward) -> solver -> ODE model.  In a multi-rank run every rank
        passes its shard; gradients and loss are averaged by one flat all-reduce.
        ``point_masks`` (10, n_s) long, or None to draw them from ``state.rng``.  The reference splits ``state.rng`` every step
        (:175); here the generator advances only when masks are drawn (ten permutations), so a step with given masks, or on a grid
        no larger than max_num_sampled_points, leaves it where it was.
        A loss or gradient that is not finite raises FloatingPointError BEFORE anything is updated (on every rank alike: the test
        is on the all-reduced values), so it reaches neither the parameters nor the AdamW moments.  The known way there is a
        table still at its initial value: with features exactly 1 the ODE model sees a - 1 = 0, every LayerNorm(eps 1e-6) in it
        normalises a constant vector with gain 1000, and the Jacobian of da/dt w.r.t. a (~1e5 for three layers) compounds over
        the nine steps of the roll-out beyond the fp32 range.
        ``cells``: None, or (x (M G, dx), q (M G,) or None, group): the trajectory holds (B, T, M, O) cell means, ``point_masks`` index
        cells, ``weights`` are per observation and ``cell_channel_weights`` (M, O) / (B, M, O) / (B, T, M, O) per observed value (not
        both).  The nef weights are frozen, so the loss does not decode: nef.cell_fit_loss, one grouped fit step over the B T
        signal-frames (rollout_loss(cells=, fused=True))."""
        self._need_ode("ode_train_step")
        trajectory, traj_idx = batch[0], batch[-1]
        leaves, graph = self._ode_train_leaves(state.params["ode_params"])
        P = state.params["autodecoder"]["params"]
        params = {"nef": state.params["nef"], "autodecoder": {"params": {k: v.detach() for k, v in P.items()}},
                  "ode_params": _unflatten(state.params["ode_params"], leaves)}
        loss = self.ode_loss(params, trajectory, traj_idx, point_masks, state.rng, graph=graph, weights=weights, normalize=normalize,
                             cells=cells, cell_channel_weights=cell_channel_weights, fused=cells is not None)
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
        grads = [torch.zeros_like(t) if g is None else g for t, g in zip(leaves, grads)]
        flat = grads + [loss.detach().reshape(1)]
        allreduce_mean_(flat, weight=trajectory.shape[0])
        if not bool(torch.isfinite(torch.stack([global_norm(grads), flat[-1][0]])).all()):
            raise FloatingPointError(f"NonMetaPDETrainer.ode_train_step: loss {float(flat[-1][0])}, ODE gradient norm "
                                     f"{float(global_norm(grads))} at step {state.step}; nothing was updated.  (A latent table still "
                                     "at its initial value, features exactly 1, does this through the 10-frame roll-out.)")
        new_leaves, ode_opt_state = self.ode_opt.update(clip_by_global_norm(grads, 1.0), state.ode_opt_state,
                                                        [t.detach() for t in leaves])
        params = dict(state.params, ode_params=_unflatten(state.params["ode_params"], new_leaves))
        return flat[-1][0], NonMetaTrainState(params=params, nef_opt_state=state.nef_opt_state,
                                              autodecoder_opt_state=state.autodecoder_opt_state, ode_opt_state=ode_opt_state,
                                              step=state.step + 1, rng=state.rng)

    @torch.no_grad()
    def val_step(self, state, batch, autodecoder=None, weights=None, normalize=True, channel_weights=None, cells=None,
                 cell_channel_weights=None, return_frames=False, chunk=None):
        """:201-241: ``batch`` = (trajectory, traj_idx) or (trajectory, _, traj_idx), read as ``batch[0]`` and ``batch[-1]`` like
        ode_train_step's.  The first 20 frames against the roll-out of the rows ``traj_idx`` of ``state.params['autodecoder']``, read
        through ``autodecoder`` (a shell for validation signals; default: the trainer's own), decoded on the full grid in chunks of
        max_num_sampled_points.  Returns (mse over frames 0..9, mse over frames 10..19); a trajectory of at most 10 frames gives
        zero for the second.  Roll-outs of more than 4 frames replay one captured hipGraph per derivative evaluation.
        ``channel_weights``: None, or (N, O) / (B, N, O) / (B, T, N, O) weights per value; the two errors are then weighted per value
        (a NaN under a zero weight does not count); not together with ``weights``.
        ``cells``: None, or (x (M G, dx), q (M G,) or None, group): the trajectory holds (B, T, M, O) cell means; all M cells of all
        B T signal-frames of the roll-out are evaluated with nef.eval_cell_loss in chunks of ``chunk`` cells (default
        max_num_sampled_points // group) -- no decode.  Returns the two means of loss_b over the horizons, with ``return_frames``
        followed by loss_b (B, T).  ``weights`` per observation or ``cell_channel_weights`` per observed value; ``channel_weights``
        with ``cells`` is a ValueError."""
        self._need_ode("val_step")
        trajectory, traj_idx = batch[0], batch[-1]
        trajectory = trajectory[:, :VAL_FRAMES]                                  # :206
        B, T = trajectory.shape[:2]
        if return_frames and cells is None:
            raise ValueError("return_frames= goes with cells=")
        traj = trajectory.reshape(B, T, -1, trajectory.shape[-1])
        # weights with or without a frame axis, per point / observation or per value: the pair is then the two weighted errors
        obs, fw = observed(self.coords, weights, channel_weights, cells, cell_channel_weights, B, traj.shape[2], traj.shape[3], T=T,
                           normalize=normalize, device=traj.device, frames=slice(T), nef=self.nef)
        z0 = (autodecoder or self.autodecoder).apply(state.params["autodecoder"], traj_idx)     # :209-210
        if cells is not None:      # no decode: all cells of all signal-frames evaluated by nef.eval_cell_loss
            return self._val_cells(state.params["nef"], state.params["ode_params"], z0, traj, TRAIN_FRAMES, obs, fw, return_frames, chunk)
        sol = self.rollout(state.params["ode_params"], tuple(None if v is None else v.detach() for v in z0), T, graph=T > 4)
        p_fl, a_fl, w_fl = (None if v is None else v.reshape(B * T, *v.shape[2:]) for v in sol)
        recon = decode(self.nef, state.params["nef"], self.coords, p_fl, a_fl, w_fl,
                       chunk=self.config.training.max_num_sampled_points).reshape(trajectory.shape)    # :228-238
        return self._horizon_errors(recon, trajectory, TRAIN_FRAMES, fw)

    def validate_epoch(self, state, train_loader, val_loader, val_autodecoder, *, drop_rates=(0.0, 0.05, 0.1, 0.5), epochs=None,
                       fit_train=True, channel_weights=None):
        """:399-548, without its logging and plots.  Validating an auto-decoder means fitting a FRESH latent table to the signals
        with the decoder frozen, then rolling the fitted rows out.  Returns (metrics, the last validation state):

            train_mse_{in,out}_t_sc                     val_step over ``train_loader`` on the STORED table of ``state`` (:419-431)
            val_mse_{in,out}_t[_dpR]   per drop rate R  a table from ``val_autodecoder.init`` and a fresh Adam state (:436-444),
                                                        ``epochs`` passes of fit_latents_step over ``val_loader`` on frame 0
                                                        (:460-474), then val_step over ``val_loader``, averaged (:477-496)
            train_mse_{in,out}_t[_dpR] (``fit_train``)  the same with ``self.autodecoder.init`` over ``train_loader`` (:501-536)

        (the keys of rate 0.0 carry no suffix; the others end in ``_dp0.05`` etc., the reference's f-string.)  Loaders are
        re-iterable and yield (trajectory (B, T, *grid, O), _, traj_idx) or (trajectory, traj_idx); ``val_autodecoder`` is the
        shell sized for the validation set.  Tables are initialised on the device of ``self.coords`` with ``state.rng`` as key,
        and the fits draw their point subsets from it (the reference splits the key per rate, :436; here the one generator runs
        on).  The nef and ODE parameters and the stored table of ``state`` are only read.  Two points are the reference's verbatim:
          - epochs: ``range(1, total_val_epochs)`` with total_val_epochs = training.nef.train_until_epoch (:447,460), so the
            default is train_until_epoch - 1 passes;
          - drop-out: the mask of rate R is ``permutation(N)[:int(N * R)]`` (:452-455), and nef_loss indexes WITH it
            (``initial_state[:, mask]``, :321), so it KEEPS int(N * R) points: R = 0.05 fits on 5 % of the grid.  It is drawn once
            per rate and shared by the validation and the training fit; rate 0 has no mask.
        ``channel_weights``: None, or a function ``batch -> (B, T, N, O) or (B, N, O) or (N, O)`` weights per value for that batch
        (e.g. ``lambda b: valid_channel_weights(b[0].flatten(2, -2))``), or such a tensor for every batch: the fits run
        fit_latents_step(channel_weights=) on frame 0's weights and the errors are val_step(channel_weights=)'s."""
        self._need_ode("validate_epoch")

        def cw_of(batch, frame0):      # the extra keyword of the two steps; nothing without channel weights
            if channel_weights is None:
                return {}
            cw = torch.as_tensor(channel_weights(batch) if callable(channel_weights) else channel_weights)
            return {"channel_weights": cw[:, 0] if frame0 and cw.dim() == 4 else cw}
        if epochs is None:
            epochs = self.config.training.nef.train_until_epoch - 1
        dev, N = self.coords.device, self.coords.shape[0]

        def rollout_errors(st, loader, shell):
            tot_in, tot_out, n = 0.0, 0.0, 0
            for batch in loader:
                e_in, e_out = self.val_step(st, batch, autodecoder=shell, **cw_of(batch, False))
                tot_in, tot_out, n = tot_in + e_in, tot_out + e_out, n + 1
            return float(tot_in) / max(n, 1), float(tot_out) / max(n, 1)

        def fit(shell, loader, dp_mask):
            table = shell.init(state.rng, device=dev)
            st = NonMetaTrainState(params=dict(state.params, autodecoder=table), nef_opt_state=state.nef_opt_state,
                                   autodecoder_opt_state=self.autodecoder_opt.init(list(table["params"].values())),
                                   ode_opt_state=state.ode_opt_state, step=state.step, rng=state.rng)
            for _ in range(epochs):
                for batch in loader:
                    _, st = self.fit_latents_step(st, (batch[0][:, 0], batch[-1]), mask=dp_mask, **cw_of(batch, True))
            return st

        metrics = {}
        metrics["train_mse_in_t_sc"], metrics["train_mse_out_t_sc"] = rollout_errors(state, train_loader, self.autodecoder)
        val_state = None
        for dp in drop_rates:
            dp_mask = torch.randperm(N, generator=state.rng)[:int(N * dp)].to(dev) if dp > 0 else None
            suffix = f"_dp{dp}" if dp > 0 else ""
            val_state = fit(val_autodecoder, val_loader, dp_mask)
            metrics["val_mse_in_t" + suffix], metrics["val_mse_out_t" + suffix] = rollout_errors(val_state, val_loader, val_autodecoder)
            if fit_train:
                train_state = fit(self.autodecoder, train_loader, dp_mask)
                metrics["train_mse_in_t" + suffix], metrics["train_mse_out_t" + suffix] = \
                    rollout_errors(train_state, train_loader, self.autodecoder)
        return metrics, val_state

    def select_train_step(self, epoch):
        """The step of ``epoch`` by the windows of _base_pde_trainer.py:280-289: nef while training.nef.train_from_epoch < epoch
        <= train_until_epoch, ode likewise.  Where the two windows OVERLAP the nef step runs: this trainer has no dual step, and
        its own train_epoch in the reference tests the nef window first (nonmaml_pde_trainer.py:380-383).  An epoch in neither
        window raises ValueError (as :298-299), and so does an ODE epoch on a trainer built without an ODE model.  Every
        returned step takes (state, batch) with batch = (trajectory (B, T, *grid, O), traj_idx) or (trajectory, _, traj_idx);
        the nef step fits frame 0 (:311)."""
        t = self.config.training
        if t.nef.train_from_epoch < epoch <= t.nef.train_until_epoch:
            return lambda state, batch, **kw: self.nef_train_step(state, (batch[0][:, 0], batch[-1]), **kw)
        if t.ode.train_from_epoch < epoch <= t.ode.train_until_epoch:
            self._need_ode("select_train_step (epoch %d lies in the ode window)" % epoch)
            return self.ode_train_step
        raise ValueError("No training step set")

    def train_epoch(self, state, loader, epoch):
        """One pass over ``loader`` (an iterable of the batches select_train_step describes) with the step the schedule
        selects; returns (mean loss, state)."""
        step = self.select_train_step(epoch)
        total, n = 0.0, 0
        for batch in loader:
            loss, state = step(state, batch)
            total, n = total + float(loss), n + 1
        return total / max(n, 1), state
