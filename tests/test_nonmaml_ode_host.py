"""Host logic of the auto-decoder trainer's latent-ODE phase (nonmaml_pde_trainer.py:14-99, 173-307; _base_pde_trainer.py:280-299):
state layout with and without an ODE model, the phase schedule, checkpoints, the per-frame point masks, and -- with a small
differentiable stand-in for the decoder, which has no CPU path -- the bookkeeping of ode_train_step / val_step."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import optim_ref_np as OP
from enf_pde_amd import checkpoint as ck
from enf_pde_amd.enf.latents.autodecoder import PositionOrientationFeatureAutodecoder
from enf_pde_amd.fitting import get_model_pde
from enf_pde_amd.fitting.ode_models import MLPODE, PonitaODEGen
from enf_pde_amd.fitting.trainers import NonMetaPDETrainer, NonMetaTrainState, draw_point_masks, sample_frames
from enf_pde_amd.fitting.trainers.latent_ode import _leaves


def _cfg(n_s=2048, nef=(0, 600), ode=(600, 2000), method="euler"):
    """config_navier_stokes_nonmaml.yaml's nef / node / training / optimizer blocks."""
    return NS(nef=NS(num_in=2, num_out=1, num_layers=0, num_hidden=128, num_heads=2, condition_value_transform=True,
                     latent_dim=16, num_latents=4, use_gaussian_window=True, embedding_type="rff",
                     embedding_freq_multiplier_invariant=0.05, embedding_freq_multiplier_value=0.2, invariant_type="rel_pos_periodic"),
              node=NS(name="ponita", num_layers=3, num_hidden=128, widening_factor=2, kernel_size="global", degree=3, basis_dim=64,
                      dt=1, method=method),
              training=NS(max_num_sampled_points=n_s, nef=NS(train_from_epoch=nef[0], train_until_epoch=nef[1]),
                          ode=NS(train_from_epoch=ode[0], train_until_epoch=ode[1])),
              optimizer=NS(learning_rate_enf=1e-4, learning_rate_codes=1e-3, learning_rate_ode=1e-3))


def _trainer(with_ode=True, ode_model=None, signals=6, grid=8, **kw):
    cfg = _cfg(**kw)
    nef, ode = get_model_pde(cfg)
    ad = PositionOrientationFeatureAutodecoder(signals, 4, 16, 2, 0, gaussian_window_size=-1)
    lin = torch.linspace(-1, 1, grid)
    coords = torch.stack(torch.meshgrid(lin, lin, indexing="xy"), -1).reshape(-1, 2)
    if not with_ode:
        return cfg, NonMetaPDETrainer(cfg, nef, ad, coords, seed=0)
    return cfg, NonMetaPDETrainer(cfg, nef, ad, coords, seed=0, ode_model=ode_model or ode)


def test_node_block_of_the_nonmaml_config_builds():
    nef, ode = get_model_pde(_cfg())
    assert isinstance(ode, PonitaODEGen) and ode.ponita.num_layers == 3 and ode.ponita.num_hidden == 128 and ode.ponita.basis_dim == 64
    assert ode.scalar_num_out == 16 and nef.cross_attn_invariant.num_z_ori_dims == 0


def test_without_an_ode_model_the_state_is_todays_and_the_ode_steps_raise():
    cfg, tr = _trainer(with_ode=False)
    assert tr.ode_model is None and tr.ode_opt is None
    st = tr.init_train_state()
    assert set(st.params) == {"nef", "autodecoder"} and st.ode_opt_state is None
    assert set(vars(st)) == {"params", "nef_opt_state", "autodecoder_opt_state", "ode_opt_state", "step", "rng"}
    # the positional form of the constructor and of the state (existing callers)
    old = NonMetaTrainState(params=st.params, nef_opt_state=st.nef_opt_state, autodecoder_opt_state=st.autodecoder_opt_state)
    assert old.ode_opt_state is None and old.step == 0
    batch = (torch.zeros(2, 12, 8, 8, 1), torch.tensor([0, 1]))
    for call in (lambda: tr.ode_train_step(st, batch), lambda: tr.val_step(st, batch),
                 lambda: tr.ode_loss(st.params, batch[0], batch[1])):
        with pytest.raises(ValueError, match="ode_model"):
            call()
    with pytest.raises(ValueError, match="ode_model"):
        tr.select_train_step(601)                                          # an ODE epoch without an ODE model
    assert callable(tr.select_train_step(600))


def test_init_train_state_holds_ode_params_and_an_adamw_state():
    cfg, tr = _trainer()
    st = tr.init_train_state()
    assert set(st.params) == {"nef", "autodecoder", "ode_params"}
    leaves = _leaves(st.params["ode_params"])
    # the shapes of an initialisation from a (1, Z, .) sample of the table (:80-89)
    p, a, w = tr.autodecoder.apply(st.params["autodecoder"], torch.tensor([0]))
    assert p.shape == (1, 4, 2) and a.shape == (1, 4, 16) and w.shape == (1, 4, 1)
    want = _leaves(tr.ode_model.init(123, (p, a, w)))
    assert [tuple(t.shape) for t in leaves] == [tuple(t.shape) for t in want] and len(leaves) > 10
    s = st.ode_opt_state
    assert s["count"] == 0 and len(s["mu"]) == len(s["nu"]) == len(leaves)
    for t, m, v in zip(leaves, s["mu"], s["nu"]):
        assert m.shape == v.shape == t.shape and not m.any() and not v.any()
    # clip_by_global_norm(1.0) -> adamw(learning_rate_enf): the rule of :68-69, not the MAML trainer's adam(learning_rate_ode)
    assert tr.ode_opt.lr == cfg.optimizer.learning_rate_enf and tr.ode_opt.wd == 1e-4
    given = tr.ode_model.init(5, (p, a, w))
    assert tr.init_train_state(ode_params=given).params["ode_params"] is given


def test_phase_schedule():
    cfg, tr = _trainer()
    calls = []
    tr.nef_train_step = lambda state, batch, **kw: calls.append(("nef", tuple(batch[0].shape), batch[1])) or (0.0, state)
    tr.ode_train_step = lambda state, batch, **kw: calls.append(("ode", tuple(batch[0].shape), batch[-1])) or (0.0, state)
    idx = torch.tensor([3, 1])
    batch = (torch.zeros(2, 12, 8, 8, 1), None, idx)                       # the reference's (trajectory, _, traj_idx)
    for epoch, want in ((1, "nef"), (600, "nef"), (601, "ode"), (2000, "ode")):
        tr.select_train_step(epoch)(None, batch)
        assert calls[-1][0] == want, epoch
    assert calls[0][1] == (2, 8, 8, 1) and calls[0][2] is idx             # the nef step fits frame 0 (:311)
    assert calls[-1][1] == (2, 12, 8, 8, 1) and calls[-1][2] is idx
    for epoch in (0, 2001):
        with pytest.raises(ValueError, match="No training step set"):
            tr.select_train_step(epoch)
    # overlapping windows: the nef step, as the docstring says (the reference's own train_epoch tests the nef window first)
    cfg, tr = _trainer(nef=(0, 700), ode=(600, 2000))
    tr.nef_train_step = lambda state, batch, **kw: calls.append(("nef",)) or (1.0, state)
    tr.ode_train_step = lambda state, batch, **kw: calls.append(("ode",)) or (3.0, state)
    tr.select_train_step(650)(None, batch)
    assert calls[-1] == ("nef",)
    tr.select_train_step(701)(None, batch)
    assert calls[-1] == ("ode",)
    n = len(calls)
    loss, state = tr.train_epoch("state", [batch, batch, batch], 800)
    assert loss == 3.0 and state == "state" and calls[n:] == [("ode",)] * 3


@pytest.mark.parametrize("kind", ["mlp", "ponita"])
def test_checkpoint_round_trip_with_ode_state(tmp_path, kind):
    ode = MLPODE(num_hidden=32, num_layers=3, scalar_num_out=16, vec_num_out=1) if kind == "mlp" else None
    cfg, tr = _trainer(ode_model=ode)
    st = tr.init_train_state()
    g = torch.Generator().manual_seed(3)
    leaves = _leaves(st.params["ode_params"])
    st.ode_opt_state = {"count": 7, "mu": [torch.randn(t.shape, generator=g) for t in leaves],
                        "nu": [torch.randn(t.shape, generator=g).abs() for t in leaves]}
    st.step = 9
    path = str(tmp_path / "ckpt.npz")
    tr.save_checkpoint(st, path, epoch=601)
    cfg2, tr2 = _trainer(ode_model=ode)
    tr2.seed = 1                                                           # another initialisation to be overwritten
    new, epoch = tr2.load_checkpoint(path)
    assert epoch == 601 and new.step == 9 and new.ode_opt_state["count"] == 7 and type(new.ode_opt_state["count"]) is int
    for a, b in zip(_leaves(new.params["ode_params"]), leaves):
        assert a.dtype == b.dtype and torch.equal(a, b)
    for part in ("mu", "nu"):
        assert all(torch.equal(a, b) for a, b in zip(new.ode_opt_state[part], st.ode_opt_state[part]))
    flat_a, flat_b = ck.flatten_tree(new.params), ck.flatten_tree(st.params)
    assert set(flat_a) == set(flat_b) and all(torch.equal(flat_a[k], flat_b[k]) for k in flat_b)
    with np.load(path) as z:
        assert z["ode_opt_state/count"].dtype == np.int64 and "ode_opt_state/nu/0" in z.files


def test_a_checkpoint_without_ode_entries(tmp_path):
    """What the trainer wrote before it had an ODE phase: no params/ode_params, no ode_opt_state."""
    cfg, tr = _trainer(with_ode=False)
    st = tr.init_train_state()
    st.params["autodecoder"]["params"]["a"] += 0.25
    path = str(tmp_path / "old.npz")
    tr.save_checkpoint(st, path, epoch=3)
    with np.load(path) as z:
        assert not [k for k in z.files if k.startswith(("params/ode_params", "ode_opt_state"))]
    cfg, fresh = _trainer(with_ode=False)
    new, epoch = fresh.load_checkpoint(path)
    assert epoch == 3 and new.ode_opt_state is None and set(new.params) == {"nef", "autodecoder"}
    assert torch.equal(new.params["autodecoder"]["params"]["a"], st.params["autodecoder"]["params"]["a"])
    cfg, with_ode = _trainer()
    with pytest.raises(ValueError, match="no latent-ODE state"):
        with_ode.load_checkpoint(path)
    # and the other way round
    st2 = with_ode.init_train_state()
    path2 = str(tmp_path / "new.npz")
    with_ode.save_checkpoint(st2, path2)
    with pytest.raises(ValueError):
        fresh.load_checkpoint(path2)


def test_point_masks_are_independent_per_frame_and_shared_over_the_batch():
    N, n_s, T, B = 64, 24, 10, 3
    pm = draw_point_masks(N, n_s, T, torch.Generator().manual_seed(4))
    assert pm.shape == (T, n_s) and pm.dtype == torch.int64
    assert torch.equal(pm, draw_point_masks(N, n_s, T, torch.Generator().manual_seed(4)))
    rows = [tuple(r.tolist()) for r in pm]
    assert all(len(set(r)) == n_s and 0 <= min(r) and max(r) < N for r in rows)          # a truncated permutation per frame
    assert len(set(rows)) == T                                                           # every frame its own
    # the generator is consumed frame by frame: frame k of a longer draw is frame k of a shorter one
    assert torch.equal(draw_point_masks(N, n_s, 4, torch.Generator().manual_seed(4)), pm[:4])
    g = torch.Generator().manual_seed(0)
    coords, traj = torch.randn(N, 2, generator=g), torch.randn(B, T, N, 1, generator=g)
    xs, ys = sample_frames(coords, traj, pm)
    assert xs.shape == (B * T, n_s, 2) and ys.shape == (B * T, n_s, 1)
    for b in range(B):
        for t in range(T):
            assert torch.equal(xs[b * T + t], coords[pm[t]]) and torch.equal(ys[b * T + t], traj[b, t, pm[t]])
    xs, ys = sample_frames(coords, traj, None)
    assert xs.shape == (B * T, N, 2) and torch.equal(ys.reshape(B, T, N, 1), traj) and torch.equal(xs[7], coords)


# ---------------------------------------------------------------------------------------------------------------------
class _ToyDecoder:
    """A differentiable stand-in with the decoder's calling convention (the HIP decoder raises on host tensors): gaussian
    bumps at the latent positions weighted by a projection of ``a``.  Only for the host bookkeeping tests below."""

    def __init__(self, nef):
        self.cross_attn_invariant, self._nef = nef.cross_attn_invariant, nef
        self.w = torch.linspace(-1, 1, 16, dtype=torch.float64)
        self.calls = []

    def param_tensors(self, params):
        return self._nef.param_tensors(params)

    def apply(self, params, x, p, a, window):
        self.calls.append(tuple(x.shape))
        d2 = ((x[:, :, None, :] - p[:, None, :, :]) ** 2).sum(-1)                       # (B, N, Z)
        return ((torch.exp(-d2 / window[:, None, :, 0] ** 2) * (a @ self.w.to(a.dtype))[:, None, :]).sum(-1, keepdim=True))


def _toy(method="euler", n_s=24, grid=8):
    ode = MLPODE(num_hidden=16, num_layers=3, scalar_num_out=16, vec_num_out=1)
    cfg, tr = _trainer(ode_model=ode, n_s=n_s, grid=grid, method=method)
    st = tr.init_train_state()
    tr.nef = _ToyDecoder(tr.nef)
    g = torch.Generator().manual_seed(8)
    P = st.params["autodecoder"]["params"]
    P["a"] = P["a"] + 0.2 * torch.randn(P["a"].shape, generator=g)
    traj = torch.randn(3, 22, grid, grid, 1, generator=g)
    idx = torch.tensor([4, 0, 5])
    return cfg, tr, st, traj, idx


@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_ode_train_step_bookkeeping_on_the_host(method):
    """One step = clip_by_global_norm(1) + AdamW(learning_rate_enf) on the ODE leaves from the gradient of the 10-frame loss;
    everything else is handed on; the loss is the fp64 evaluation of the same composition."""
    cfg, tr, st, traj, idx = _toy(method)
    pm = draw_point_masks(64, 24, 10, torch.Generator().manual_seed(1))
    rng_before = st.rng.get_state().clone()
    loss, new = tr.ode_train_step(st, (traj, idx), point_masks=pm)
    assert tr.nef.calls == [(30, 24, 2)]                                                # ONE decode of B x 10 signal-frames
    assert torch.equal(st.rng.get_state(), rng_before)                                  # given masks: nothing drawn
    # fp64 restatement
    from enf_pde_amd.fitting.trainers.trainer_utils import solve_latent_ode
    from enf_pde_amd.fitting.trainers.latent_ode import _unflatten
    dl = [t.detach().double().requires_grad_(True) for t in _leaves(st.params["ode_params"])]
    dp = _unflatten(st.params["ode_params"], dl)
    z0 = tuple(v.double() for v in tr.autodecoder.apply(st.params["autodecoder"], idx))
    sol = solve_latent_ode(lambda z, t: tr.ode_model.apply(dp, z), z0, 0, 9, 1, method=method)
    xs, ys = sample_frames(tr.coords.double(), traj[:, :10].reshape(3, 10, 64, 1).double(), pm)
    ref = ((tr.nef.apply(None, xs, *(v.reshape(30, *v.shape[2:]) for v in sol)) - ys) ** 2).mean()
    g = torch.autograd.grad(ref, dl)
    ref = ref.detach()
    assert abs(float(loss) - float(ref)) < 1e-5 * float(ref)
    want, wstate = OP.adam_step([t.detach().numpy() for t in dl], OP.clip_by_global_norm([x.numpy() for x in g], 1.0),
                                OP.init_state([x.numpy() for x in g]), lr=1e-4, weight_decay=1e-4)
    got = _leaves(new.params["ode_params"])
    assert new.ode_opt_state["count"] == 1
    # The first AdamW step from zero moments is lr g / (|g| + eps): it does not change when g is rescaled, so the parameters
    # alone would not show a missing clip.  The moments do: mu = 0.1 clip(g), nu = 0.001 clip(g)^2, and the clip acts here.
    gnorm = float(np.sqrt(sum((x.numpy() ** 2).sum() for x in g)))
    print("gradient norm", gnorm)
    assert gnorm > 1.5
    for part, tol in (("mu", 2e-4), ("nu", 4e-4)):                     # fp32 gradient against fp64; nu squares it
        for a, b in zip(new.ode_opt_state[part], wstate[part]):
            assert np.abs(a.numpy() - b).max() <= tol * np.abs(b).max(), part
    for a, b, old in zip(got, want, dl):
        np.testing.assert_allclose(a.numpy(), b, rtol=2e-4, atol=2e-6)
    assert any(not torch.equal(a, b.float()) for a, b in zip(got, dl))
    assert new.params["nef"] is st.params["nef"] and new.params["autodecoder"] is st.params["autodecoder"]
    assert new.nef_opt_state is st.nef_opt_state and new.autodecoder_opt_state is st.autodecoder_opt_state
    assert new.step == st.step + 1 and new.rng is st.rng
    # without masks they come from state.rng: 10 permutations
    ref_gen = torch.Generator()
    ref_gen.set_state(rng_before)
    loss2, _ = tr.ode_train_step(st, (traj, idx))
    loss3, _ = tr.ode_train_step(st, (traj, idx), point_masks=draw_point_masks(64, 24, 10, ref_gen))
    assert float(loss2) == float(loss3) and torch.equal(st.rng.get_state(), ref_gen.get_state())


def test_val_step_on_the_host():
    cfg, tr, st, traj, idx = _toy(n_s=24)
    from enf_pde_amd.fitting.trainers.trainer_utils import solve_latent_ode
    mse_in, mse_out = tr.val_step(st, (traj, None, idx))
    assert tr.nef.calls == [(60, 24, 2), (60, 24, 2), (60, 16, 2)]                      # 20 frames, 64 points in chunks of 24
    z0 = tr.autodecoder.apply(st.params["autodecoder"], idx)
    sol = solve_latent_ode(lambda z, t: tr.ode_model.apply(st.params["ode_params"], z), z0, 0, 19, 1, method="euler")
    rec = tr.nef.apply(None, tr.coords[None].expand(60, -1, -1), *(v.reshape(60, *v.shape[2:]) for v in sol)).reshape(3, 20, 8, 8, 1)
    err = (rec - traj[:, :20]) ** 2
    assert abs(float(mse_in) - float(err[:, :10].mean())) < 1e-5 * float(err[:, :10].mean())
    assert abs(float(mse_out) - float(err[:, 10:].mean())) < 1e-5 * float(err[:, 10:].mean())
    a, b = tr.val_step(st, (traj[:, :12], idx))
    assert abs(float(a) - float(mse_in)) < 1e-5 * float(mse_in) and abs(float(b) - float(err[:, 10:12].mean())) < 1e-5 * float(b)
    a, b = tr.val_step(st, (traj[:, :10], idx))
    assert float(b) == 0.0 and np.isfinite(float(a))
    # the lookup goes through the given shell, into the table of the state
    other = PositionOrientationFeatureAutodecoder(2, 4, 16, 2, 0, gaussian_window_size=-1)
    vt = other.init(device="cpu")
    vt["params"]["a"] = st.params["autodecoder"]["params"]["a"][[5, 4]].clone()
    vstate = NonMetaTrainState(params=dict(st.params, autodecoder=vt), nef_opt_state=None, autodecoder_opt_state=None,
                               ode_opt_state=st.ode_opt_state)
    c, d = tr.val_step(vstate, (traj[:1], torch.tensor([1])), autodecoder=other)        # row 1 of the validation table = row 4
    e, f = tr.val_step(st, (traj[:1], torch.tensor([4])))
    assert float(c) == float(e) and float(d) == float(f)


def test_a_non_finite_gradient_raises_and_updates_nothing():
    cfg, tr, st, traj, idx = _toy()
    pm = draw_point_masks(64, 24, 10, torch.Generator().manual_seed(1))
    leaves = _leaves(st.params["ode_params"])
    before = [t.clone() for t in leaves]
    mom = [[t.clone() for t in st.ode_opt_state[part]] for part in ("mu", "nu")]
    with pytest.raises(FloatingPointError, match="nothing was updated"):
        tr.ode_train_step(st, (traj * float("inf"), idx), point_masks=pm)            # an infinite target: loss inf, gradient nan
    assert st.ode_opt_state["count"] == 0 and st.step == 0
    assert all(torch.equal(a, b) for a, b in zip(_leaves(st.params["ode_params"]), before))
    assert all(torch.equal(a, b) for part, old in zip(("mu", "nu"), mom) for a, b in zip(st.ode_opt_state[part], old))
    loss, new = tr.ode_train_step(st, (traj, idx), point_masks=pm)                   # the same state still steps
    assert np.isfinite(float(loss)) and new.ode_opt_state["count"] == 1
