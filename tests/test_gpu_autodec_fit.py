"""The auto-decoder trainer's latent-only step and validation protocol on the GPU (nonmaml_pde_trainer.py:139-171, 399-548):
fit_latents_step -- enf_fit_step_w + enf_table_adam_update -- against float64 autograd of the oracle decoder's mean squared error
w.r.t. the gathered table rows followed by float64 adam, against the existing autograd step, and validate_epoch end to end.
f32 precision unless said otherwise; num_hidden 64, 2 heads, latent_dim 8, 2 outputs; a table of 5 signals x 5 latents, an 8 x 8
grid, 37 sampled points, the batch [4, 0, 2]."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from oracle import optim_ref_np as OP
from tests import table_adam_ref as TA
from tests.helpers import make_cfg, make_inputs, build_nef
from tests.test_gpu_forward import TOL as FIELD_TOL            # max |err| / max |ref| of a field, per precision
from tests.test_gpu_backward import TOL as GRAD_TOL            # relative L2 error of a latent gradient, per precision
from enf_pde_amd.enf.latents.autodecoder import PositionOrientationFeatureAutodecoder
from enf_pde_amd.fitting.inner_loop import make_signal_masks, gather_signal_points, decode
from enf_pde_amd.fitting.ode_models import MLPODE
from enf_pde_amd.fitting.trainers import NonMetaPDETrainer, NonMetaTrainState
from enf_pde_amd.fitting.weights import valid_weights, normalize_point_weights, observed_sampling_weights

pytestmark = pytest.mark.gpu

S, Z, C, O, SIDE, N_S, IDX, LR, SEED = 5, 5, 8, 2, 8, 37, [4, 0, 2], 1e-2, 7
ROWS_OUT = [1, 3]


def _problem(invariant):
    cfg = make_cfg(invariant, D=64, H=2, C=C, O=O)
    prm = R.init_params(3, cfg, jitter=0.1)
    _, p, a, s = make_inputs(cfg, S, 1, Z, 4)
    names = ("p_pos", "p_ori", "a", "gaussian_window") if invariant == "ponita" else ("p_pos", "a", "gaussian_window")
    table = {"p_pos": p[..., :2], "p_ori": p[..., 2:], "a": a, "gaussian_window": s}
    table = {k: table[k].astype(np.float32) for k in names}
    lin = np.linspace(-1, 1, SIDE)
    coords = np.stack(np.meshgrid(lin, lin), -1).reshape(-1, 2).astype(np.float32)
    img = np.random.default_rng(5).standard_normal((3, SIDE, SIDE, O)).astype(np.float32)
    return NS(cfg=cfg, prm=prm, table=table, names=names, coords=coords, img=img, invariant=invariant)


def _trainer(cuda, pb, precision="f32", sample_observed=False, ode_model=None, shell=None):
    conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=LR), training=NS(max_num_sampled_points=N_S, nef=NS(train_until_epoch=4)),
              node=NS(dt=1, method="euler"))
    nef = build_nef(pb.cfg, precision)
    ad = shell or PositionOrientationFeatureAutodecoder(S, Z, C, 2, 1 if pb.invariant == "ponita" else 0, gaussian_window_size=-1)
    tr = NonMetaPDETrainer(conf, nef, ad, torch.tensor(pb.coords, device=cuda), seed=0, sample_observed=sample_observed, ode_model=ode_model)
    return tr, nef.load_params(pb.prm, device=cuda)


def _state(cuda, tr, nef_params, pb):
    table = {k: torch.tensor(v, device=cuda) for k, v in pb.table.items()}
    return NonMetaTrainState(params={"nef": nef_params, "autodecoder": {"params": table}}, nef_opt_state="nef-opt",
                             autodecoder_opt_state=tr.autodecoder_opt.init(list(table.values())), ode_opt_state="ode-opt", step=0,
                             rng=torch.Generator().manual_seed(SEED))


def _points(pb, case):
    """The points a step from a generator seeded with SEED fits on, restated on the host: (xs (B, n, 2), ys (B, n, O), ws (B, n) or
    None, the field handed to the trainer, the trainer's keyword arguments)."""
    g = torch.Generator().manual_seed(SEED)
    coords, img = torch.tensor(pb.coords), torch.tensor(pb.img).reshape(3, -1, O).clone()
    if case == "plain":
        sub = torch.randperm(64, generator=g)[:N_S]
        return coords[sub][None].expand(3, -1, -1), img[:, sub], None, img, {}
    holes = torch.rand(3, 64, generator=torch.Generator().manual_seed(11)) < 0.3
    img[holes] = float("nan")
    w = valid_weights(img)
    pw = normalize_point_weights(w)
    if case == "weights+mask":
        mask = torch.randperm(64, generator=torch.Generator().manual_seed(12))[:50]
        sub = torch.randperm(50, generator=g)[:N_S]
        pick = mask[sub]
        return coords[pick][None].expand(3, -1, -1), img[:, pick], pw[:, pick], img, {"weights": w, "mask": mask}
    assert case == "weights+sample_observed"
    m = make_signal_masks(pw, N_S, 0, generator=g, device="cpu")
    xs, ys, ws = (t[0] for t in gather_signal_points(coords, img, m, observed_sampling_weights(pw, N_S)))
    return xs, ys, ws, img, {"weights": w}


_ORACLE = {}


def _oracle(pb, case):
    """float64: loss and its gradient w.r.t. the gathered rows (pose, a, window), once per (invariant, case)."""
    key = (pb.invariant, case)
    if key not in _ORACLE:
        xs, ys, ws, _, _ = _points(pb, case)
        pose = np.concatenate([pb.table[k] for k in pb.names if k.startswith("p_")], -1)
        rows = [torch.tensor(v[IDX].astype(np.float64), requires_grad=True) for v in (pose, pb.table["a"], pb.table["gaussian_window"])]
        out = T.nef_apply(T.to_torch(pb.prm, torch.float64), pb.cfg, xs.double(), *rows)
        if ws is None:
            loss = ((out - ys.double()) ** 2).mean()
        else:
            wd = ws.double()[..., None]
            d = torch.where(wd > 0, out - ys.double(), torch.zeros_like(out))
            loss = (wd * d * d).mean()
        g = torch.autograd.grad(loss, rows)
        _ORACLE[key] = (float(loss.detach()), [x.numpy() for x in g])
    return _ORACLE[key]


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _own_gradient(new, pb):
    """The gradient the step took, read back from its first moments: mu' = (1 - b1) g from a zero state."""
    return {k: m.cpu().numpy().astype(np.float64) / (1 - TA.B1) for k, m in zip(pb.names, new.autodecoder_opt_state["mu"])}


def _check_step(cuda, pb, case, precision, sample_observed=False):
    tr, nef_params = _trainer(cuda, pb, precision, sample_observed)
    state = _state(cuda, tr, nef_params, pb)
    _, _, _, field, kw = _points(pb, case)
    kw = {k: v.to(cuda) for k, v in kw.items()}
    loss, new = tr.fit_latents_step(state, (field.reshape(3, SIDE, SIDE, O).to(cuda), torch.tensor(IDX, device=cuda)), **kw)
    torch.cuda.synchronize()
    ref_loss, (rp, ra, rs) = _oracle(pb, case)
    el = abs(float(loss) - ref_loss) / ref_loss
    g = _own_gradient(new, pb)
    gp = np.concatenate([g[k] for k in pb.names if k.startswith("p_")], -1)
    errs = {"p": _rel(gp[IDX], rp), "a": _rel(g["a"][IDX], ra), "sigma": _rel(g["gaussian_window"][IDX], rs)}
    print(f"{pb.invariant} {case} {precision}: loss rel err {el:.2e}, gradient rel errs {errs}")
    assert el < FIELD_TOL[precision], el
    for k, e in errs.items():
        assert np.isfinite(e) and e < GRAD_TOL[precision], (k, e, errs)
    # rows outside the batch: zero gradient and zero moments, so they are where they were, bit for bit
    P0, P1 = state.params["autodecoder"]["params"], new.params["autodecoder"]["params"]
    for k, mu, nu in zip(pb.names, new.autodecoder_opt_state["mu"], new.autodecoder_opt_state["nu"]):
        assert torch.equal(P1[k][ROWS_OUT], P0[k][ROWS_OUT]) and not mu[ROWS_OUT].any() and not nu[ROWS_OUT].any()
        assert P1[k] is not P0[k] and P1[k].shape == P0[k].shape
    # the parameters: float64 adam on the step's OWN gradient (the first step, lr g / (|g| + eps), is ill-conditioned in g where
    # |g| is near eps: against the oracle's gradient this would test noise; the gradient check above is the parity check)
    x0 = [pb.table[k].astype(np.float64) for k in pb.names]
    want, st = OP.adam_step(x0, [g[k] for k in pb.names], OP.init_state(x0), lr=LR, b1=TA.B1, b2=TA.B2, eps=TA.EPS)
    for k, w, v, nu in zip(pb.names, want, st["nu"], new.autodecoder_opt_state["nu"]):
        err = np.abs(P1[k].cpu().numpy() - w)
        assert (err <= 1e-5 * LR + 1e-6 * np.abs(w)).all(), (k, err.max())
        assert np.abs(nu.cpu().numpy() - v).max() <= 1e-5 * np.abs(v).max(), k            # nu' = (1 - b2) g^2 of the same g
    assert float(np.median(np.abs(P1["a"].cpu().numpy() - x0[pb.names.index("a")])[IDX])) > 0.5 * LR   # the batch rows did move
    assert new.autodecoder_opt_state["count"] == 1 and new.step == 1 and new.rng is state.rng
    assert new.params["nef"] is nef_params and new.nef_opt_state == "nef-opt" and new.ode_opt_state == "ode-opt"
    assert torch.equal(state.rng.get_state(), _after_draw(pb, case))


def _after_draw(pb, case):
    g = torch.Generator().manual_seed(SEED)
    if case == "weights+sample_observed":
        make_signal_masks(torch.ones(3, 64), N_S, 0, generator=g, device="cpu")
    else:
        torch.randperm(50 if case == "weights+mask" else 64, generator=g)
    return g.get_state()


@pytest.mark.parametrize("invariant", ["rel_pos_periodic", "ponita"])
def test_one_step_from_a_zero_adam_state(cuda, invariant):
    _check_step(cuda, _problem(invariant), "plain", "f32")


@pytest.mark.parametrize("case", ["weights+sample_observed", "weights+mask"])
@pytest.mark.parametrize("invariant", ["rel_pos_periodic", "ponita"])
def test_one_step_with_weights_of_a_field_with_holes(cuda, invariant, case):
    """valid_weights of a field with NaN in it (the NaN stay in the targets): once drawn per signal from its observed points
    (sample_observed: x with a real batch stride), once with ``mask=`` and the subset shared by the batch."""
    _check_step(cuda, _problem(invariant), case, "f32", sample_observed=case == "weights+sample_observed")


@pytest.mark.parametrize("invariant", ["rel_pos_periodic", "ponita"])
def test_one_step_in_bf16(cuda, invariant):
    _check_step(cuda, _problem(invariant), "plain", "bf16")


@pytest.mark.parametrize("case", ["plain", "weights+sample_observed"])
@pytest.mark.parametrize("invariant", ["rel_pos_periodic", "ponita"])
def test_agrees_with_the_autograd_step(cuda, invariant, case):
    """fit_latents_step and nef_train_step_autodec_only from the same state and generator seed draw the same subset: losses to the
    f32 field tolerance, first-step moments to the latent-gradient tolerance.  Both are HIP paths: this guards the plumbing."""
    pb = _problem(invariant)
    tr, nef_params = _trainer(cuda, pb, "f32", sample_observed=case != "plain")
    _, _, _, field, kw = _points(pb, case)
    kw = {k: v.to(cuda) for k, v in kw.items()}
    batch = (field.reshape(3, SIDE, SIDE, O).to(cuda), torch.tensor(IDX, device=cuda))
    s_old, s_new = _state(cuda, tr, nef_params, pb), _state(cuda, tr, nef_params, pb)
    loss_old, old = tr.nef_train_step_autodec_only(s_old, batch, **kw)
    loss_new, new = tr.fit_latents_step(s_new, batch, **kw)
    assert torch.equal(s_old.rng.get_state(), s_new.rng.get_state())
    el = abs(float(loss_new) - float(loss_old)) / float(loss_old)
    errs = {k: _rel(a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64))
            for k, a, b in zip(pb.names, new.autodecoder_opt_state["mu"], old.autodecoder_opt_state["mu"])}
    print(f"{invariant} {case}: loss rel diff {el:.2e}, moment rel diffs {errs}")
    assert el < FIELD_TOL["f32"]
    assert all(e < GRAD_TOL["f32"] for e in errs.values()), errs


class _FiveLatents(PositionOrientationFeatureAutodecoder):
    """A shell for 5 latents per signal (the reference's grid initialiser wants a square number): the four cell centres and the
    middle of the domain."""

    def init(self, key=None, device="cuda"):
        n = self.num_signals
        pos = torch.tensor([[-0.5, -0.5], [-0.5, 0.5], [0.5, -0.5], [0.5, 0.5], [0.0, 0.0]])
        P = {"p_pos": pos[None].repeat(n, 1, 1), "a": torch.ones(n, 5, self.latent_dim), "gaussian_window": torch.full((n, 5, 1), 1.0)}
        return {"params": {k: v.to(device=device, dtype=torch.float32) for k, v in P.items()}}


def test_validate_epoch(cuda):
    pb = _problem("rel_pos_periodic")
    ode = MLPODE(num_hidden=16, num_layers=3, scalar_num_out=C, vec_num_out=1)
    tr, nef_params = _trainer(cuda, pb, "f32", ode_model=ode, shell=_FiveLatents(S, 5, C, 2, 0, gaussian_window_size=-1))
    val_shell = _FiveLatents(4, 5, C, 2, 0, gaussian_window_size=-1)
    state = tr.init_train_state(nef_params)
    state.params["autodecoder"]["params"] = {k: torch.tensor(v, device=cuda) for k, v in pb.table.items()}
    # smooth fields with an offset, 4 frames each (roll-outs of at most 4 frames run without graph capture)
    xy = torch.tensor(pb.coords, device=cuda)

    def fields(n, seed):
        g = torch.Generator().manual_seed(seed)
        amp, ph = torch.rand(n, 1, 1, O, generator=g).to(cuda), (6.28 * torch.rand(n, 4, 1, O, generator=g)).to(cuda)
        f = 0.6 + 0.4 * amp * torch.sin(2.0 * xy[None, None, :, :1] + 1.5 * xy[None, None, :, 1:] + ph)
        return f.reshape(n, 4, SIDE, SIDE, O)

    t = lambda i: torch.tensor(i, device=cuda)
    train = [(fields(3, 1), None, t([4, 0, 2])), (fields(2, 2), None, t([1, 3]))]
    val = [(fields(2, 3), t([0, 1])), (fields(2, 4), t([3, 2]))]
    keep = [w.clone() for w in tr.nef.param_tensors(state.params["nef"])] + [v.clone() for v in state.params["autodecoder"]["params"].values()]
    metrics, last = tr.validate_epoch(state, train, val, val_shell, epochs=3, drop_rates=(0.0, 0.5))
    torch.cuda.synchronize()
    assert set(metrics) == {"train_mse_in_t_sc", "train_mse_out_t_sc"} | {f"{s}_mse_{io}_t{d}" for s in ("val", "train")
                                                                          for io in ("in", "out") for d in ("", "_dp0.5")}
    assert all(type(v) is float and np.isfinite(v) for v in metrics.values()), metrics
    now = tr.nef.param_tensors(state.params["nef"]) + list(state.params["autodecoder"]["params"].values())
    assert all(torch.equal(a, b) for a, b in zip(now, keep))                                # the state was only read
    assert last.autodecoder_opt_state["count"] == 3 * 2 and last.params["autodecoder"]["params"]["a"].shape == (4, 5, C)

    def frame0_error(table):
        err = 0.0
        for traj, idx in val:
            rec = decode(tr.nef, state.params["nef"], tr.coords, *val_shell.apply(table, idx))
            err += float(((rec - traj[:, 0].reshape(2, -1, O)) ** 2).mean())
        return err / len(val)

    e0, e1 = frame0_error(val_shell.init(device=cuda)), frame0_error(last.params["autodecoder"])
    print(f"frame-0 error of the validation table: {e0:.4f} at initialisation, {e1:.4f} after 3 epochs; metrics {metrics}")
    assert e1 < e0
