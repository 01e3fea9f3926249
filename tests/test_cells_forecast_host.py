"""Per-value weights on grouped observations and the forecast steps on cell averages, without a GPU: the four new symbols in the header,
the library and the binding; the torch-op mirror against the fp64 yardstick (tests/cells_cw_ref.py); the refusals of the Python layer
and of the C-ABI (every native call here fails its checks, so nothing is launched)."""
import ctypes
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import cells_cw_ref as CW
from tests.helpers import build_nef, make_cfg
from enf_pde_amd import _lib
from enf_pde_amd.fitting import cell_mse_torch, fit_cell_averages, gather_cell_samples, inner_loop_cells
from enf_pde_amd.fitting.trainers import MetaSGDPDETrainer, NonMetaPDETrainer, meta_gradients
from enf_pde_amd.fitting.trainers.latent_ode import sample_cell_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("enf_fit_step_gc", "enf_eval_loss_gc", "enf_mse_value_grad_gc", "enf_fit_inputs_gc")


def test_the_four_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "enf_hip.h")).read()
    lib = _lib.load()
    assert lib.enf_abi_version() == 2 and re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", header)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == getattr(lib, name[:-1]).argtypes, name       # the _g call's arguments
    assert header.index("enf_fit_step_gc(") > header.index("enf_mse_value_grad_g(")         # appended behind the existing calls


def test_c_abi_refusals():
    """cweight_g is required; ENF_FIT_SHARED_LATENTS on enf_fit_step_gc is ENF_EUNSUPPORTED, behind the descriptor's errors; the
    refusals of the _g calls hold"""
    lib = _lib.load()
    nef = build_nef(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32")
    desc = nef._desc(2, 16, 4)
    nbytes = int(lib.enf_workspace_bytes(ctypes.byref(desc)))
    one = ctypes.c_void_p(16)            # never dereferenced: every call below is refused before any launch
    fit = lambda G, cw, flags=0, d=desc: lib.enf_fit_step_gc(ctypes.byref(d), one, 0, one, one, one, one, one, G, None, cw, 1.0, one, one, one, one,
                                                             None, None, one, nbytes, flags, None)
    ev = lambda G, cw: lib.enf_eval_loss_gc(ctypes.byref(desc), one, 0, one, one, one, one, one, G, None, cw, one, None, None, one, nbytes, 0, None)
    EINVAL, EUNSUPPORTED = -1, -3
    assert lib.enf_strerror(EUNSUPPORTED) and fit(4, None) == EINVAL and ev(4, None) == EINVAL
    assert fit(3, one) == EINVAL and fit(32, one) == EINVAL and ev(3, one) == EINVAL
    assert fit(4, one, _lib.ENF_FIT_SHARED_LATENTS) == EUNSUPPORTED
    bad = nef._desc(2, 16, 4)
    bad.H = 7
    assert fit(4, one, _lib.ENF_FIT_SHARED_LATENTS, bad) == lib.enf_check_desc(ctypes.byref(bad)) != 0
    mse = lambda cw, G=4: lib.enf_mse_value_grad_gc(one, one, 2, 16, 2, G, None, cw, 1.0, None, one, None, None, 0, 0, None)
    assert mse(None) == EINVAL and mse(one, 3) == EINVAL
    comps = (_lib.EnfFitComponent * _lib.ENF_SGD_MAX_SEGMENTS)()
    comps[0] = _lib.EnfFitComponent(16, 16, 2, 0)
    gat = lambda cw, ws, per: lib.enf_fit_inputs_gc(1, comps, 2, 4, 8, 3, 2, 4, 2, 2, one, None, one, one, one, None, one, one, cw, ws, per, None)
    assert gat(None, one, 0) == EINVAL and gat(one, None, 0) == EINVAL and gat(None, None, 0) == EINVAL and gat(None, one, 1) == EINVAL


@pytest.mark.parametrize("G,N,O", [(4, 80, 2), (16, 48, 17), (2, 50, 17), (1, 33, 2)])
def test_cell_mse_torch_with_channel_weights_is_the_yardstick(G, N, O):
    """fp64: value and gradient w.r.t. the decode within 1e-12, NaN / Inf targets under the zero weights"""
    rng = np.random.default_rng(G + O)
    Bn, M = 3, N // G
    out = torch.tensor(rng.standard_normal((Bn, N, O)), requires_grad=True)
    q = rng.uniform(0.2, 2.0, (Bn, N)) / G
    y = rng.standard_normal((Bn, M, O))
    cw = CW.weights(rng, Bn, M, O)
    c = NS(y=y, cw=cw)
    y_bad = CW.poisoned(c)
    assert np.isnan(y_bad).any() and np.isinf(y_bad).any()
    ref = CW.group_loss(out, y, G, q, cw)
    (g_ref,) = torch.autograd.grad(ref.loss, out)
    got = cell_mse_torch(out, torch.tensor(y_bad), G, torch.tensor(q), obs_channel_weight=torch.tensor(cw))
    (g_got,) = torch.autograd.grad(got, out)
    got, same_as = got.detach(), ref.loss.detach()
    assert abs(float(got) - float(same_as)) <= 1e-12 * float(same_as)
    assert bool(torch.isfinite(g_got).all()) and float((g_got - g_ref).abs().max()) <= 1e-12 * float(g_ref.abs().max())
    assert float((g_got - ref.dout).abs().max()) <= 1e-12 * float(g_ref.abs().max())           # the closed form of the header
    dead = torch.tensor(cw == 0)[:, :, None, :].expand(Bn, M, G, O)
    assert bool((g_got.reshape(Bn, M, G, O)[dead] == 0).all())
    # one weight per observation is the per-value form with equal channels
    w = cw[..., 0]
    same = cell_mse_torch(out, torch.tensor(y), G, torch.tensor(q), obs_channel_weight=torch.tensor(np.repeat(w[..., None], O, -1)))
    assert abs(float(same.detach()) - float(cell_mse_torch(out, torch.tensor(y), G, torch.tensor(q), torch.tensor(w)).detach())) <= 1e-12 * float(same.detach())


def test_gather_of_channel_weights_is_plain_indexing():
    rng = np.random.default_rng(0)
    Bn, M, O, G, Ms, S1 = 2, 9, 3, 2, 4, 3
    x, q, obs, cw = (torch.tensor(rng.standard_normal(s)) for s in ((M * G, 2), (M * G,), (Bn, M, O), (Bn, M, O)))
    masks = torch.tensor(np.stack([np.stack([rng.permutation(M)[:Ms] for _ in range(S1)], 1) for _ in range(Bn)]))
    masks[1, 2, :] = -1
    xs, qs, ys, ws = gather_cell_samples(x, q, G, obs, masks, obs_channel_weight=cw.float())
    assert ws.shape == (S1, Bn, Ms, O) and float(ws[:, 1, 2].abs().max()) == 0.0
    for s in range(S1):
        for b in range(Bn):
            for i in range(Ms):
                if masks[b, i, s] >= 0:
                    assert torch.equal(ws[s, b, i], cw[b, masks[b, i, s]].float())
    shared = gather_cell_samples(x, q, G, obs, masks[0], obs_channel_weight=cw.float())[3]
    assert torch.equal(shared[1, 1], cw[1, masks[0][:, 1]].float())


def _frames_problem():
    rng = np.random.default_rng(1)
    x, q = torch.tensor(rng.standard_normal((6 * 4, 2))), torch.tensor(rng.uniform(0.1, 1, 6 * 4))
    traj = torch.tensor(rng.standard_normal((2, 3, 6, 2)))
    return x, q, traj, rng


def test_sample_cell_frames_is_plain_indexing():
    x, q, traj, rng = _frames_problem()
    pm = torch.tensor(np.stack([rng.permutation(6)[:4] for _ in range(3)]))
    w, cw = torch.tensor(rng.uniform(0, 1, (2, 3, 6))), torch.tensor(rng.uniform(0, 1, (2, 3, 6, 2)))
    xs, qs, ys, ws = sample_cell_frames((x, q, 4), traj, pm, w)
    assert xs.shape == (6, 16, 2) and qs.shape == (6, 16) and ys.shape == (6, 4, 2) and ws.shape == (6, 4)
    for b in range(2):
        for k in range(3):
            for i in range(4):
                c = int(pm[k, i])
                assert torch.equal(xs[b * 3 + k, 4 * i:4 * i + 4], x[4 * c:4 * c + 4]) and torch.equal(qs[b * 3 + k, 4 * i:4 * i + 4], q[4 * c:4 * c + 4])
                assert torch.equal(ys[b * 3 + k, i], traj[b, k, c]) and ws[b * 3 + k, i] == w[b, k, c]
    assert torch.equal(sample_cell_frames((x, q, 4), traj, pm, cw)[3].reshape(2, 3, 4, 2)[1, 2, 3], cw[1, 2, pm[2, 3]])
    full = sample_cell_frames((x, None, 4), traj, None, cw)
    assert full[0].shape == (6, 24, 2) and full[1] is None and torch.equal(full[2], traj.reshape(6, 6, 2)) and torch.equal(full[3], cw.reshape(6, 6, 2))


# ---- the refusals of the Python layer
def _nef():
    return build_nef(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32")


def test_both_weight_kinds_at_once_are_refused():
    nef = _nef()
    x, p, a, s = torch.zeros(2, 16, 2), torch.zeros(2, 4, 2), torch.zeros(2, 4, 8), torch.ones(2, 4, 1)
    y, w, cw = torch.zeros(2, 4, 2), torch.ones(2, 4), torch.ones(2, 4, 2)
    for call in (lambda: nef.mse_value_and_cell_grads(None, x, p, a, s, y, 4, obs_weight=w, obs_channel_weight=cw),
                 lambda: nef.eval_cell_loss(None, x, p, a, s, y, 4, obs_weight=w, obs_channel_weight=cw),
                 lambda: nef.cell_fit_loss(None, x, p, a, s, y, 4, obs_weight=w, obs_channel_weight=cw),
                 lambda: nef.cell_mse(torch.zeros(2, 16, 2), y, 4, obs_weight=w, obs_channel_weight=cw),
                 lambda: cell_mse_torch(torch.zeros(2, 16, 2), y, 4, obs_weight=w, obs_channel_weight=cw),
                 lambda: gather_cell_samples(x[0], None, 4, y, torch.zeros(2, 3, dtype=torch.long), w, cw),
                 lambda: inner_loop_cells(nef, None, {}, {}, x[0], None, 4, y, torch.zeros(2, 3, dtype=torch.long), obs_weights=w, obs_channel_weight=cw),
                 lambda: fit_cell_averages(nef, None, {}, {}, x[0], None, 4, y, 2, obs_weight=w, obs_channel_weight=cw)):
        with pytest.raises(ValueError, match="not both"):
            call()
    with pytest.raises(ValueError, match="obs_channel_weight has shape"):
        nef.mse_value_and_cell_grads(None, x, p, a, s, y, 4, obs_channel_weight=w)
    with pytest.raises(ValueError, match="obs_channel_weight has shape"):
        nef.cell_mse(torch.zeros(2, 16, 2), y, 4, obs_channel_weight=torch.ones(2, 4, 3))
    with pytest.raises(ValueError, match="obs_channel_weight has shape"):
        inner_loop_cells(nef, None, {}, {}, x[0], None, 4, y, torch.zeros(2, 3, dtype=torch.long), obs_channel_weight=w)


def test_shared_latents_with_channel_weights_is_not_implemented():
    nef = _nef()
    x, p, a, s = torch.zeros(2, 16, 2), torch.zeros(2, 4, 2), torch.zeros(2, 4, 8), torch.ones(2, 4, 1)
    with pytest.raises(NotImplementedError, match="shared_latents"):
        nef.mse_value_and_cell_grads(None, x, p, a, s, torch.zeros(2, 4, 2), 4, obs_channel_weight=torch.ones(2, 4, 2), shared_latents=True)


def _meta_trainer(n_s=8):
    conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=0.0, learning_rate_ode=1e-3),
              meta=NS(learning_rate_meta_sgd=1e-2, num_inner_steps=2, inner_learning_rate_p=0.5, inner_learning_rate_a=2.0,
                      inner_learning_rate_window=0.0, noise_pos_inner_loop=0.0),
              nef=NS(optimize_gaussian_window=False), training=NS(max_num_sampled_points=n_s),
              node=NS(dt=1, method="euler"), dataset=NS(traj_len_train=3, traj_len_out_horizon=2))
    return MetaSGDPDETrainer(conf, _nef(), None, torch.zeros(16, 2), ode_model=None)


STATE = NS(params={"nef": None, "ode_params": {"w": torch.zeros(1)}, "meta_sgd_lrs": {}, "autodecoder": {"params": {}}}, rng=None)


def test_trainer_steps_refuse_what_cells_do_not_serve():
    """channel_weights + cells still raises and names channel_weights; drop_rate + cells; both cell weight kinds; wrong (B, T, M, O)
    shapes; cell_channel_weights without cells -- all before anything touches a device"""
    tr = _meta_trainer()
    x = torch.zeros(16, 2)
    cells = (x, None, 4)
    traj = torch.zeros(2, 5, 4, 2)
    with pytest.raises(ValueError, match="channel_weights"):
        meta_gradients(None, None, {}, {}, None, traj[:, 0], torch.zeros(2, 3, dtype=torch.long), channel_weights=torch.ones(4, 2), cells=cells)
    for step in (tr.ode_train_step, tr.val_step, tr.fit_errors):
        with pytest.raises(ValueError, match="cell_channel_weights"):
            step(STATE, traj, cell_channel_weights=torch.ones(4, 2))                        # without cells=
    for call in (lambda: tr.dual_train_step(STATE, traj, channel_weights=torch.ones(4, 2), cells=cells),
                 lambda: tr.val_step(STATE, traj, channel_weights=torch.ones(4, 2), cells=cells),
                 lambda: tr.fit_errors(STATE, traj[:, 0], channel_weights=torch.ones(4, 2), cells=cells),
                 lambda: tr.nef_train_step(STATE, traj[:, 0], channel_weights=torch.ones(4, 2), cells=cells),
                 lambda: tr.rollout_loss(None, None, None, traj, channel_weights=torch.ones(4, 2), cells=cells)):
        with pytest.raises(ValueError, match="channel_weights"):
            call()
    with pytest.raises(ValueError, match="drop_rate"):
        tr.val_step(STATE, traj, drop_rate=0.1, cells=cells)
    both = dict(weights=torch.ones(4), cell_channel_weights=torch.ones(4, 2), cells=cells)
    for call in (lambda: tr.ode_train_step(STATE, traj, **both), lambda: tr.dual_train_step(STATE, traj, **both),
                 lambda: tr.rollout_loss(None, None, None, traj, **both), lambda: tr.fit_errors(STATE, traj[:, 0], **both),
                 lambda: meta_gradients(None, None, {}, {}, None, traj[:, 0], torch.zeros(2, 3, dtype=torch.long), **both)):
        with pytest.raises(ValueError, match="not both"):
            call()
    for bad in (torch.ones(2, 5, 4, 3), torch.ones(2, 4, 4, 2), torch.ones(3, 5, 4, 2), torch.ones(5, 2)):
        with pytest.raises(ValueError, match="channel weights have shape"):
            tr.rollout_loss(None, None, None, traj, cells=cells, cell_channel_weights=bad)
    with pytest.raises(ValueError, match="weights have shape"):
        tr.rollout_loss(None, None, None, traj, cells=cells, weights=torch.ones(2, 5, 5))
    with pytest.raises(ValueError, match="channel weights have shape"):
        tr.ode_train_step(STATE, traj, cells=cells, cell_channel_weights=torch.ones(2, 5, 4, 3))


def test_the_steps_validate_cells_as_meta_gradients_does():
    tr = _meta_trainer()
    x = torch.zeros(16, 2)
    traj = torch.zeros(2, 5, 4, 2)
    calls = {"rollout_loss": lambda c: tr.rollout_loss(None, None, None, traj, cells=c),
             "val_step": lambda c: tr.val_step(STATE, traj, cells=c),
             "fit_errors": lambda c: tr.fit_errors(STATE, traj[:, 0], cells=c),
             "ode_train_step": lambda c: tr.ode_train_step(STATE, traj, cells=c),
             "dual_train_step": lambda c: tr.dual_train_step(STATE, traj, cells=c),
             "meta_gradients": lambda c: meta_gradients(None, None, {}, {}, None, traj[:, 0], torch.zeros(2, 3, dtype=torch.long), cells=c)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match="group"):
            call((x, None, 3))
        with pytest.raises(ValueError, match="cells hold"):
            call((x, None, 2))
    tr.nef.num_layers = 1
    with pytest.raises(NotImplementedError, match="num_layers"):
        tr.rollout_loss(None, None, None, traj, cells=(x, None, 4))


def test_autodecoder_trainer_refusals():
    conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=1e-2, learning_rate_ode=1e-1),
              nef=NS(optimize_gaussian_window=False), training=NS(max_num_sampled_points=8), node=NS(dt=1, method="euler"))
    tr = NonMetaPDETrainer(conf, _nef(), None, torch.zeros(16, 2), ode_model=object())
    x = torch.zeros(16, 2)
    traj = torch.zeros(2, 12, 4, 2)
    idx = torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError, match="channel_weights"):
        tr.val_step(STATE, (traj, idx), channel_weights=torch.ones(4, 2), cells=(x, None, 4))
    with pytest.raises(ValueError, match="group"):
        tr.val_step(STATE, (traj, idx), cells=(x, None, 3))
    with pytest.raises(ValueError, match="cell_channel_weights"):
        tr.val_step(STATE, (traj, idx), cell_channel_weights=torch.ones(4, 2))
    with pytest.raises(ValueError, match="channel_weights"):
        tr.fit_latents_step(STATE, (traj[:, 0], idx), channel_weights=torch.ones(4, 2), cells=(x, None, 4))
    with pytest.raises(ValueError, match="cell_channel_weights"):
        tr.fit_latents_step(STATE, (traj[:, 0], idx), cell_channel_weights=torch.ones(4, 2))
