"""Per-value weights on grouped observations and the forecast steps on cell averages, on the GPU (include/enf_hip.h, "Grouped
observations": enf_fit_step_gc, enf_eval_loss_gc, enf_mse_value_grad_gc, enf_fit_inputs_gc; rollout_loss / ode_train_step /
dual_train_step / val_step / fit_errors with cells=).

Kernels: the shapes of tests/test_gpu_cells.py (B = 3, Z = 7, D = 64, H = 2; PAIRS reaches whole tiles, group = tile, a clamped last
tile and a tile holding two signals) at O = 2 and O = 17 (channel 16 sits in the second accumulator of lane quad 0), against
tests/cells_cw_ref.py in fp64.  About a third of the weights are exact zeros, one observation has one live and one dead channel, one
has every channel dead, NaN / Inf targets lie under the dead values.
Trainers: the problem of tests/test_gpu_ode_trainer.py (2 trajectories, 8 x 8 cells, T = 3 + 2, Z = 9, ODE hidden 16) with
cell_quadrature(k = 2): G = 4, 256 quadrature rows."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from oracle import ode_ref_torch as OT
from tests import cells_cw_ref as CW
from tests import cells_ref as CR
from tests.cells_ref import B, Z, f32, rel
from tests.helpers import build_nef
from tests.test_gpu_cells import LOSS_TOL, PAIRS, TOL
from tests.test_gpu_forward import TOL as TAU
from tests.test_gpu_ode import _flat
from tests.test_gpu_ode_trainer import _setup
from tests.test_gpu_nonmaml_ode import IDX, make_trainer
from enf_pde_amd import _lib
from enf_pde_amd.fitting import cell_mse_torch, cell_quadrature, gather_cell_samples
from enf_pde_amd.fitting import cells as CELLS
from enf_pde_amd.fitting.trainers.latent_ode import _unflatten

pytestmark = pytest.mark.gpu

GUARD = 16
U = 2.0 ** -24
DET = _lib.ENF_FIT_DETERMINISTIC
INVS = ["rel_pos_periodic", "latitude_periodic"]
NAMES = ("loss", "dp", "da", "ds", "err", "loss_b")


def _t(cuda):
    return lambda v: torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda)


def _ptr(v):
    return ctypes.c_void_p(v.data_ptr()) if v is not None else None


def _stream(cuda):
    return ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)


def _guarded(n, cuda):
    """n floats of NaN with GUARD floats of NaN in front and behind: (the whole buffer, the view the kernel gets)"""
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=cuda)
    return buf, buf[GUARD:GUARD + n]


def _untouched(buf, n):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())


def _run(cuda, nef, params, c, kind, wt, y, flags=0, poison=255):
    """One raw C-ABI call on a workspace filled with ``poison``: kind "fit_gc" / "eval_gc" with wt = cweight_g (B, M, O), "fit_g" /
    "eval_g" with wt = oweight (B, M).  err_g and loss_b sit in NaN-filled buffers with GUARD floats in front and behind."""
    lib = _lib.load()
    t = _t(cuda)
    x, p, a, s, q = t(c.x), t(c.p), t(c.a), t(c.s), t(c.q)
    desc = nef._desc(B, c.N, Z)
    nbytes = int(lib.enf_workspace_bytes_ex(ctypes.byref(desc), flags))
    ws = torch.full((nbytes,), poison, device=cuda, dtype=torch.uint8)
    packed = nef.pack(params)
    loss = torch.zeros(1, device=cuda)
    ebuf, err = _guarded(B * c.M, cuda)
    lbuf, loss_b = _guarded(B, cuda)
    dp, da, ds = torch.full_like(p, float("nan")), torch.full_like(a, float("nan")), torch.full_like(s, float("nan"))
    head = (ctypes.byref(desc), _ptr(x), c.N * x.shape[-1], _ptr(p), _ptr(a), _ptr(s), _ptr(packed), _ptr(y))
    if kind.startswith("fit"):
        _lib.launch(cuda, getattr(lib, "enf_fit_step_" + kind[4:]), *head, c.G, _ptr(q), _ptr(wt), c.gs, _ptr(loss), _ptr(dp), _ptr(da), _ptr(ds),
                    _ptr(err), _ptr(loss_b), _ptr(ws), nbytes, flags, _stream(cuda))
    else:
        _lib.launch(cuda, getattr(lib, "enf_eval_loss_" + kind[5:]), *head, c.G, _ptr(q), _ptr(wt), _ptr(loss), _ptr(err), _ptr(loss_b), _ptr(ws),
                    nbytes, flags, _stream(cuda))
    torch.cuda.synchronize()
    assert _untouched(ebuf, B * c.M) and _untouched(lbuf, B), ("guard", kind)
    return NS(loss=loss, dp=dp, da=da, ds=ds, err=err.view(B, c.M), loss_b=loss_b)


def _mse_gc(cuda, out, y, G, q, cw, gscale, flags=0):
    lib = _lib.load()
    Bn, N, O = out.shape
    M = N // G
    nb = int(lib.enf_mse_scratch_bytes(Bn * M * O, flags))
    scr = torch.full((max(nb, 1),), 255, device=cuda, dtype=torch.uint8)
    dbuf, dout = _guarded(Bn * N * O, cuda)
    ebuf, err = _guarded(Bn * M, cuda)
    loss = torch.zeros(1, device=cuda)
    _lib.launch(cuda, lib.enf_mse_value_grad_gc, _ptr(out), _ptr(y), Bn, N, O, G, _ptr(q), _ptr(cw), float(gscale), _ptr(dout), _ptr(loss),
                _ptr(err), _ptr(scr) if nb else None, nb, flags, _stream(cuda))
    torch.cuda.synchronize()
    assert _untouched(dbuf, Bn * N * O) and _untouched(ebuf, Bn * M), "guard"
    return NS(loss=loss, dout=dout.view(Bn, N, O), err=err.view(Bn, M))


def _same_bits(u, v, names=NAMES):
    return [n for n in names if not torch.equal(getattr(u, n), getattr(v, n))]


# ---- 1. the three calls against the yardstick
@pytest.mark.parametrize("O", [2, 17])
@pytest.mark.parametrize("gn", PAIRS)
@pytest.mark.parametrize("inv", INVS)
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_per_value_weights_match_the_yardstick(cuda, precision, inv, gn, O):
    """enf_fit_step_gc and enf_eval_loss_gc: loss, d(p, a, sigma) at tests/test_gpu_cells.py's TOL; err_g and loss_b at that file's
    bound with the weight per value -- an output within eps0 = tau max|out_ref| moves obs by at most eps = eps0 sum_k |q| and a squared
    residual by at most 2 |dd| eps + eps^2.  enf_mse_value_grad_gc on the reference's decode rounded to fp32: d out and err_g at the
    bounds of tests/test_gpu_cells_train.py::test_grouped_loss_kernel, (G + 4) u S on the residual -- the weight per value changes no
    rounding count -- plus (O + 1) u err_g for the O products and the O - 1 additions of the sum over the channels, which that file
    folds into the residual's slack at O = 2 and which O = 17 needs spelled out.  Every output is finite, d out of a dead value is
    exactly 0.0f, clean and poisoned targets give the same bits, guard bands in front of and behind err_g, loss_b and d out stay NaN."""
    c = CW.case(inv, *gn, O=O)
    nef = build_nef(c.cfg, precision)
    params = nef.load_params(c.prm, device=cuda)
    t = _t(cuda)
    cw, y_bad, y_clean = t(c.cw), t(CW.poisoned(c)), t(c.y)
    assert bool(torch.isnan(y_bad).any()) and bool(torch.isinf(y_bad).any())
    assert c.cw[0, 1, 0] > 0 and c.cw[0, 1, 1] == 0 and not c.cw[1, 0].any()
    tol_l, tol_g = TOL[precision]
    fit = _run(cuda, nef, params, c, "fit_gc", cw, y_bad, DET)
    ev = _run(cuda, nef, params, c, "eval_gc", cw, y_bad, DET)
    plain = _run(cuda, nef, params, c, "fit_gc", cw, y_bad)
    e_loss = abs(float(fit.loss) - c.ref.loss) / c.ref.loss
    e_g = [rel(g.cpu().numpy(), r) for g, r in zip((fit.dp, fit.da, fit.ds), c.ref.g)]
    e_gp = [rel(g.cpu().numpy(), r) for g, r in zip((plain.dp, plain.da, plain.ds), c.ref.g)]
    eps = TAU[precision] * c.ref.out_max * np.abs(c.q).reshape(B, c.M, c.G).sum(-1)
    ebound = (c.cw * (2 * np.abs(c.ref.dd) * eps[..., None] + (eps * eps)[..., None])).sum(-1)
    lbound = ebound.sum(1) / (c.M * O)
    d_err, d_lb = np.abs(fit.err.double().cpu().numpy() - c.ref.err_g), np.abs(fit.loss_b.double().cpu().numpy() - c.ref.loss_b)
    print(f"cells per value {precision} {inv} G={c.G} N={c.N} O={O}: loss {e_loss:.2e} dp {e_g[0]:.2e} da {e_g[1]:.2e} dsigma {e_g[2]:.2e} "
          f"err_g / bound {float((d_err / np.maximum(ebound, 1e-300))[ebound > 0].max()):.2e} "
          f"loss_b / bound {float((d_lb / np.maximum(lbound, 1e-300)).max()):.2e} eval loss {abs(float(ev.loss) - c.ref.loss) / c.ref.loss:.2e}")
    assert e_loss <= tol_l and abs(float(ev.loss) - c.ref.loss) <= tol_l * c.ref.loss and abs(float(plain.loss) - c.ref.loss) <= tol_l * c.ref.loss
    assert all(e <= tol_g for e in e_g + e_gp), (e_g, e_gp)
    assert (d_err <= ebound).all() and (d_lb <= lbound).all()
    dead_obs = torch.tensor((c.cw == 0).all(-1))
    for r in (fit, ev, plain):
        assert all(bool(torch.isfinite(getattr(r, n)).all()) for n in ("loss", "err", "loss_b"))
        assert bool((r.err[dead_obs] == 0).all()) and bool((r.err[~dead_obs] > 0).all())
        assert abs(float(r.loss_b.double().mean()) - float(r.loss)) <= 1e-5 * float(r.loss)
    assert all(bool(torch.isfinite(g).all()) for g in (fit.dp, fit.da, fit.ds, plain.dp, plain.da, plain.ds))
    # the evaluation's err_g and loss_b are the fit step's bits, in both modes; clean targets change no bit
    assert _same_bits(fit, ev, ("err", "loss_b")) == [] and _same_bits(fit, plain, ("err", "loss_b")) == []
    assert _same_bits(fit, _run(cuda, nef, params, c, "fit_gc", cw, y_clean, DET, poison=0x5A)) == []
    assert _same_bits(ev, _run(cuda, nef, params, c, "eval_gc", cw, y_clean, DET, poison=0), ("loss", "err", "loss_b")) == []
    if precision == "bf16":
        return
    # the unfused loss on a decode that exists: the reference's, rounded to fp32
    G, M, N, gsc = c.G, c.M, c.N, 3.0
    out64 = f32(c.ref.out)
    ref = CW.group_loss(torch.tensor(out64), c.y, G, c.q, c.cw)
    v = c.q[..., None] * out64
    S = np.abs(v).reshape(B, M, G, O).sum(2) + np.abs(c.y)
    live = c.cw > 0
    dd = ref.dd.numpy()
    inv_n = np.float32(1.0) / (np.float32(B) * np.float32(M) * np.float32(O))
    gs = float(np.float32(2.0) * inv_n * np.float32(gsc))
    fac = c.q.reshape(B, M, G, 1) * (c.cw[:, :, None, :] * gs)                                    # (B, M, G, O): q cw gs
    ref_dout = (fac * dd[:, :, None, :]).reshape(B, N, O)
    bound_dout = (np.abs(fac) * ((G + 4) * U * np.where(live, S, 0.0))[:, :, None, :]).reshape(B, N, O)
    ref_err = ref.err_g.numpy()
    e1 = (G + 4) * U * S
    bound_err = (c.cw * (2 * np.abs(dd) * e1 + e1 * e1)).sum(-1) + (O + 1) * U * ref_err
    runs = [_mse_gc(cuda, t(out64), yy, G, t(c.q), cw, gsc, flags) for yy, flags in ((y_bad, 0), (y_bad, DET), (y_clean, DET))]
    for r in runs:
        d_dout, d_e = np.abs(r.dout.double().cpu().numpy() - ref_dout), np.abs(r.err.double().cpu().numpy() - ref_err)
        el = abs(float(r.loss) - float(ref.loss)) / float(ref.loss)
        print(f"  unfused: d out / bound {float((d_dout / np.maximum(bound_dout, 1e-300))[bound_dout > 0].max()):.2e} "
              f"err_g / bound {float((d_e / np.maximum(bound_err, 1e-300))[bound_err > 0].max()):.2e} loss {el:.2e}")
        assert (d_dout <= bound_dout).all() and (d_e <= bound_err).all() and el < 1e-5
        assert bool(torch.isfinite(r.dout).all()) and bool(torch.isfinite(r.err).all())
        gone = torch.tensor(~live, device=cuda)[:, :, None, :].expand(B, M, G, O)
        assert bool((r.dout.view(B, M, G, O)[gone] == 0).all()) and bool((r.err[dead_obs.to(cuda)] == 0).all())
    assert torch.equal(runs[0].dout, runs[1].dout) and torch.equal(runs[0].err, runs[1].err)
    assert _same_bits(runs[1], runs[2], ("loss", "dout", "err")) == []


# ---- 2. the bitwise link to the per-observation form
@pytest.mark.parametrize("O", [2, 17])
@pytest.mark.parametrize("gn", PAIRS)
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_equal_channel_weights_give_the_bits_of_the_per_observation_form(cuda, precision, gn, O):
    """ENF_FIT_DETERMINISTIC: enf_fit_step_gc with cw[b, m, :] = w[b, m] returns enf_fit_step_g(oweight = w)'s loss, dp, da, dsigma,
    err_g and loss_b, bit for bit, and enf_eval_loss_gc's err_g is the fit step's; so does the unfused kernel."""
    c = CR.case("rel_pos_periodic", *gn, O=O)
    nef = build_nef(c.cfg, precision)
    params = nef.load_params(c.prm, device=cuda)
    t = _t(cuda)
    w, y = t(c.w), t(CR.poisoned(c))
    cw = w[..., None].expand(B, c.M, O).contiguous()
    old = _run(cuda, nef, params, c, "fit_g", w, y, DET)
    new = _run(cuda, nef, params, c, "fit_gc", cw, y, DET, poison=0x5A)
    assert _same_bits(old, new) == [] and all(bool(torch.isfinite(getattr(new, n)).all()) for n in NAMES)
    ev = _run(cuda, nef, params, c, "eval_gc", cw, y, DET)
    assert _same_bits(new, ev, ("err", "loss_b")) == [] and _same_bits(_run(cuda, nef, params, c, "eval_g", w, y, DET), ev, ("loss", "err", "loss_b")) == []
    out = t(np.random.default_rng(O).standard_normal((B, c.N, O)))
    nef.deterministic = True
    lo, ln = [], []
    for kw, acc in (({"obs_weight": w}, lo), ({"obs_channel_weight": cw}, ln)):
        o = out.clone().requires_grad_(True)
        loss = nef.cell_mse(o, y, c.G, t(c.q), **kw)
        loss.backward()
        acc += [loss.detach(), o.grad]
    assert torch.equal(lo[0], ln[0]) and torch.equal(lo[1], ln[1])


# ---- 3. the gather
@pytest.mark.parametrize("per_signal", [False, True])
@pytest.mark.parametrize("dx", [2, 3])
@pytest.mark.parametrize("G", [1, 4, 16])
def test_gather_of_sampled_cells_with_per_value_weights(cuda, G, dx, per_signal, O=17, M=30, Ms=11, S1=3, Zl=5):
    """enf_fit_inputs_gc against torch indexing (gather_cell_samples): every output bit for bit, O = 17, per-signal masks holding -1, M
    and M + 7 (their ws rows are O zeros); NaN guard bands in front of and behind every output; Ms G is no multiple of 16"""
    rng = np.random.default_rng(100 * G + 10 * dx + per_signal)
    t = _t(cuda)
    x, q, obs = t(rng.standard_normal((M * G, dx))), t(rng.uniform(0.1, 1.0, M * G)), t(rng.standard_normal((B, M, O)))
    cw = t(rng.uniform(0, 2, (B, M, O)))
    cols = lambda: np.stack([rng.permutation(M)[:Ms] for _ in range(S1)], 1)
    masks = np.stack([cols() for _ in range(B)]) if per_signal else cols()
    if per_signal:
        masks[1, Ms - 4:, :] = -1
        masks[2, 0, 1], masks[0, 3, 2] = M, M + 7
    masks = torch.tensor(masks, device=cuda)
    lat0 = {"p_pos": t(rng.standard_normal((1, Zl, 2))), "a": t(rng.standard_normal((1, Zl, 6))), "gaussian_window": t(rng.uniform(0.5, 1, (1, Zl, 1)))}
    lead = (S1, B, Ms * G) if per_signal else (S1, Ms * G)
    shapes = {"xs": lead + (dx,), "qs": lead, "ys": (S1, B, Ms, O), "ws": (S1, B, Ms, O), "losses": (S1,), "p_pos": (B, Zl, 2), "a": (B, Zl, 6),
              "gaussian_window": (B, Zl, 1)}
    bufs = {k: _guarded(int(np.prod(s)), cuda) for k, s in shapes.items()}
    comps = (_lib.EnfFitComponent * _lib.ENF_SGD_MAX_SEGMENTS)()
    for i, k in enumerate(lat0):
        comps[i] = _lib.EnfFitComponent(lat0[k].data_ptr(), bufs[k][1].data_ptr(), lat0[k].shape[2], 0)
    _lib.launch(cuda, _lib.load().enf_fit_inputs_gc, 3, comps, B, Zl, M, Ms, S1, G, dx, O, _ptr(x), _ptr(q), _ptr(obs), _ptr(masks), _ptr(bufs["xs"][1]),
                _ptr(bufs["qs"][1]), _ptr(bufs["ys"][1]), _ptr(bufs["losses"][1]), _ptr(cw), _ptr(bufs["ws"][1]), int(per_signal), _stream(cuda))
    torch.cuda.synchronize()
    xs, qs, ys, ws = gather_cell_samples(x, q, G, obs, masks, obs_channel_weight=cw)
    idx = masks.permute(2, 0, 1) if per_signal else masks.t()[:, None].expand(-1, B, -1)             # (S1, B, Ms): plain indexing again
    ok = (idx >= 0) & (idx < M)
    bi = torch.arange(B, device=cuda)[None, :, None].expand_as(idx)
    assert torch.equal(ws, torch.where(ok[..., None], cw[bi, idx.clamp(0, M - 1)], torch.zeros((), device=cuda)))
    want = {"xs": xs, "qs": qs, "ys": ys, "ws": ws, "losses": torch.zeros(S1, device=cuda), **{k: v.expand(B, -1, -1) for k, v in lat0.items()}}
    for k, s in shapes.items():
        assert torch.equal(bufs[k][1].view(s), want[k]), (k, G, dx, per_signal)
        assert _untouched(bufs[k][0], int(np.prod(s))), ("guard", k)
    if per_signal:
        assert float(ws[:, 1, Ms - 4:].abs().max()) == 0.0 and float(ws[1, 2, 0].abs().max()) == 0.0
    fused = CELLS._cell_inputs(lat0, x, q, G, obs, masks, cw, per_value=True)               # the package's own route takes the launch
    assert fused is not None
    torch.cuda.synchronize()
    for got, k in zip(fused[1:], ("xs", "qs", "ys", "losses", "ws")):
        assert torch.equal(got, want[k]), k


# ---- the trainers
def _cells(t, k=2):
    x, q = cell_quadrature((-1.0, 1.0, (8, 8)), k)
    return (t(x.numpy()), t(q.numpy()), k * k), f32(x.numpy()), f32(q.numpy())


def _masks(cuda, n, cols, seed, frames=None):
    """(n, cols) long fit masks over 64 cells, or with ``frames`` (frames, n) per-frame masks"""
    g = torch.Generator().manual_seed(seed)
    if frames is None:
        return torch.stack([torch.randperm(64, generator=g)[:n] for _ in range(cols)], 1).to(cuda)
    return torch.stack([torch.randperm(64, generator=g)[:n] for _ in range(frames)]).to(cuda)


def _frame_weights(rng, shape):
    w = f32(rng.uniform(0.5, 1.5, shape))
    w[rng.uniform(size=shape) < 0.3] = 0.0
    return w


# ---- 5. the roll-out loss against the oracle
@pytest.mark.parametrize("kind", ["weights", "cell_channel_weights"])
def test_rollout_loss_on_cells_and_its_gradients_match_the_oracle(cuda, kind):
    """decoder + solver + the yardstick's grouped loss in fp64: loss 1e-4 relative, gradients w.r.t. the ODE parameters and the latents
    5e-3 (tests/test_gpu_ode_trainer.py::test_ode_loss_and_gradient_match_oracle); 8 sampled cells per frame, (B, T, M[, O]) weights
    with zeros and NaN targets under them, normalised to mean 1 per signal-frame on all 64 cells before the sampling"""
    cfg, prm, ocfg, oprm, coords, traj, conf, tr, state, t = _setup(cuda)
    cells, x64, q64 = _cells(t)
    G, Tn, Ms = 4, 3, 8
    rng = np.random.default_rng(5)
    lat = {"p_pos": R.init_positions_grid(2, 9, 2) + 0.05 * rng.standard_normal((2, 9, 2)),
           "a": 1 + 0.2 * rng.standard_normal((2, 9, 8)), "gaussian_window": np.full((2, 9, 1), 2.0 / 3)}
    pm = np.stack([rng.permutation(64)[:Ms] for _ in range(Tn)])
    tj = f32(traj[:, :Tn]).reshape(2, Tn, 64, 1)
    w = _frame_weights(rng, (2, Tn, 64) + ((1,) if kind == "cell_channel_weights" else ()))
    w[0, 1, pm[1, 0]] = 0.0
    wn = w / w.reshape(2, Tn, -1).mean(-1).reshape((2, Tn) + (1,) * (w.ndim - 2))
    # oracle
    rp = T.to_torch(oprm, torch.float64, requires_grad=True)
    tl = {k: torch.tensor(v, requires_grad=True) for k, v in lat.items()}
    sol = OT.solve_latent_ode(lambda z, _: OT.ponita_ode(rp, ocfg, z), (tl["p_pos"], tl["a"], tl["gaussian_window"]), 0, Tn - 1, 1, "euler")
    p_fl, a_fl, w_fl = (v.reshape(2 * Tn, *v.shape[2:]) for v in sol)
    rows = (pm[..., None] * G + np.arange(G)).reshape(Tn, Ms * G)
    xs = torch.tensor(x64[rows])[None].expand(2, -1, -1, -1).reshape(2 * Tn, Ms * G, 2)
    qs = np.broadcast_to(q64[rows][None], (2, Tn, Ms * G)).reshape(2 * Tn, Ms * G)
    ys = np.stack([np.stack([tj[b, k, pm[k]] for k in range(Tn)]) for b in range(2)]).reshape(2 * Tn, Ms, 1)
    wsel = np.stack([np.stack([wn[b, k, pm[k]] for k in range(Tn)]) for b in range(2)]).reshape(2 * Tn, Ms, -1)
    cw = np.broadcast_to(wsel, (2 * Tn, Ms, 1))
    ref = CW.group_loss(T.nef_apply(T.to_torch(prm, torch.float64), cfg, xs, p_fl, a_fl, w_fl), ys, G, qs, cw).loss
    ref.backward()
    # product: NaN where the weight is zero
    tj_bad = tj.copy()
    tj_bad[(w == 0).reshape(2, Tn, 64, -1).all(-1)] = np.nan
    leaves = dict(_flat(state.params["ode_params"]))
    for v in leaves.values():
        v.requires_grad_(True)
    dl = {k: t(v).requires_grad_(True) for k, v in lat.items()}
    loss = tr.rollout_loss(state.params["nef"], state.params["ode_params"], dl, t(tj_bad), torch.tensor(pm, device=cuda), cells=cells, **{kind: t(w)})
    loss.backward()
    ref_leaves = dict(_flat(rp))
    errs = {k: rel(v.grad.cpu().double().numpy(), ref_leaves[k].grad.numpy()) for k, v in leaves.items()}
    e_lat = {k: rel(dl[k].grad.cpu().double().numpy(), tl[k].grad.numpy()) for k in ("p_pos", "a")}
    print(f"rollout_loss(cells=, {kind}): loss {float(loss.detach()):.6f} oracle {float(ref.detach()):.6f} worst ODE gradient {max(errs.values()):.2e} latents {e_lat}")
    assert abs(float(loss.detach()) - float(ref.detach())) < 1e-4 * float(ref.detach())
    assert all(e < 5e-3 for e in errs.values()), errs
    assert all(e < 5e-3 for e in e_lat.values()), e_lat


# ---- 6. ode_train_step(cells=): the fused loss against the composed route
@pytest.mark.parametrize("kind", ["weights", "cell_channel_weights"])
def test_ode_train_step_on_cells_fused_loss_against_the_composed_route(cuda, kind):
    """nef.cell_fit_loss (one grouped fit step over the B T signal-frames, no decode) against apply + nef.cell_mse at the same fitted
    latents: the loss within LOSS_TOL["f32"], the ODE gradients within 5e-3; the step's loss is the fused one and only the ODE
    parameters move"""
    cfg, prm, ocfg, oprm, coords, traj, conf, tr, state, t = _setup(cuda)
    cells, _, _ = _cells(t)
    batch = t(traj).reshape(2, 5, 64, 1)
    mk, pm = _masks(cuda, 8, 3, 1), _masks(cuda, 8, None, 2, frames=3)
    w = _frame_weights(np.random.default_rng(3), (2, 5, 64) + ((1,) if kind == "cell_channel_weights" else ()))
    kw = {kind: t(w)}
    batch[t(w).reshape(2, 5, 64, -1).sum(-1) == 0] = float("nan")
    w0 = [v.clone() for v in tr.nef.param_tensors(state.params["nef"])]
    before = {k: v.clone() for k, v in _flat(state.params["ode_params"])}
    loss, new = tr.ode_train_step(state, batch, masks=mk, point_masks=pm, cells=cells, **kw)
    from enf_pde_amd.fitting.trainers.latent_ode import cell_loss_weights
    w3 = {kind: t(w)[:, :3]}
    lw0 = cell_loss_weights(w3.get("weights"), w3.get("cell_channel_weights"), 2, 64, 1, device=cuda, frames=0)
    lat = tr._fitted_cells(state, batch[:, 0], mk, lw0, cells)
    got = {}
    for fused in (True, False):
        leaves = [v.detach().clone().requires_grad_(True) for _, v in _flat(state.params["ode_params"])]
        l2 = tr.rollout_loss(state.params["nef"], _unflatten(state.params["ode_params"], leaves), lat, batch[:, :3], pm, cells=cells, fused=fused,
                             **w3)
        got[fused] = (float(l2.detach()), [g.cpu().double().numpy() for g in torch.autograd.grad(l2, leaves)])
    e_loss = abs(got[True][0] - got[False][0]) / got[False][0]
    errs = [rel(a, b) for a, b in zip(got[True][1], got[False][1])]
    print(f"ode_train_step(cells=, {kind}): step loss {float(loss):.6f} fused {got[True][0]:.6f} composed {got[False][0]:.6f} worst ODE gradient {max(errs):.2e}")
    assert np.isfinite(got[True][0]) and e_loss <= LOSS_TOL["f32"] and all(e < 5e-3 for e in errs), (e_loss, errs)
    assert abs(float(loss) - got[True][0]) <= 1e-6 * max(1.0, got[True][0])
    after = dict(_flat(new.params["ode_params"]))
    assert any(not torch.equal(after[k], before[k]) for k in before) and all(bool(torch.isfinite(v).all()) for v in after.values())
    assert all(torch.equal(a, b) for a, b in zip(tr.nef.param_tensors(new.params["nef"]), w0))
    assert new.params["meta_sgd_lrs"] is state.params["meta_sgd_lrs"] and new.params["autodecoder"] is state.params["autodecoder"]


# ---- 7. cells of one point are the point steps
def _rel_t(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def test_cells_of_one_point_reproduce_the_point_steps(cuda):
    """G = 1, q = None, the grid as cells, the same masks and point masks: ode_train_step, dual_train_step and val_step give the point
    steps' loss within 1e-5 relative and every updated parameter tensor within 1e-5 relative
    (tests/test_gpu_cells_train.py::test_meta_gradient_on_cells_of_one_point_is_the_point_meta_gradient)"""
    cfg, prm, ocfg, oprm, coords, traj, conf, tr, state, t = _setup(cuda)
    batch = t(traj)
    cells = (t(coords), None, 1)
    mk = torch.stack([torch.randperm(64, generator=torch.Generator().manual_seed(1))[:32] for _ in range(3)], 1).to(cuda)
    pm = torch.stack([torch.randperm(64, generator=torch.Generator().manual_seed(2))[:32] for _ in range(3)]).to(cuda)
    for step in ("ode_train_step", "dual_train_step"):
        lp, sp = getattr(tr, step)(state, batch, masks=mk, point_masks=pm)
        lc, sc = getattr(tr, step)(state, batch, masks=mk, point_masks=pm, cells=cells)
        errs = {"ode/" + k: _rel_t(v, dict(_flat(sp.params["ode_params"]))[k]) for k, v in _flat(sc.params["ode_params"])}
        errs.update({f"nef/{i}": _rel_t(a, b) for i, (a, b) in enumerate(zip(tr.nef.param_tensors(sc.params["nef"]), tr.nef.param_tensors(sp.params["nef"])))
                     if a is not None})
        errs.update({"lr/" + k: _rel_t(v, sp.params["meta_sgd_lrs"][k]) for k, v in sc.params["meta_sgd_lrs"].items()})
        worst = max(errs, key=errs.get)
        print(f"{step} on cells of one point: loss {float(lc):.7f} points {float(lp):.7f} worst updated tensor {worst} {errs[worst]:.2e}")
        assert abs(float(lc) - float(lp)) <= 1e-5 * abs(float(lp))
        assert all(e <= 1e-5 for e in errs.values()), {k: e for k, e in errs.items() if e > 1e-5}
    vp = tr.val_step(state, batch, masks=mk)
    vc = tr.val_step(state, batch, masks=mk, cells=cells)
    print("val_step on cells of one point:", [float(v) for v in vc], "points", [float(v) for v in vp])
    assert all(abs(float(a) - float(b)) <= 1e-5 * float(b) for a, b in zip(vc, vp))


# ---- 8. val_step(cells=, return_frames=True)
@pytest.mark.parametrize("kind", [None, "weights", "cell_channel_weights"])
def test_val_step_on_cells_returns_the_per_frame_errors_of_the_rollout(cuda, kind):
    """loss_b (B, T) against cell_mse_torch per signal-frame on a decode of the rolled-out latents (LOSS_TOL["f32"]); the two numbers
    are its means over the two horizons; chunked (8, 24 cells) and unchunked evaluation give equal bits"""
    cfg, prm, ocfg, oprm, coords, traj, conf, tr, state, t = _setup(cuda)
    cells, _, _ = _cells(t)
    batch = t(traj).reshape(2, 5, 64, 1)
    mk = _masks(cuda, 8, 3, 1)
    kw, wn = {}, None
    if kind is not None:
        w = t(_frame_weights(np.random.default_rng(4), (2, 5, 64) + ((1,) if kind == "cell_channel_weights" else ())))
        kw = {kind: w}
        batch[w.reshape(2, 5, 64, -1).sum(-1) == 0] = float("nan")
        wn = w / w.reshape(2, 5, -1).mean(-1).reshape((2, 5) + (1,) * (w.dim() - 2))
    e_in, e_out, loss_b = tr.val_step(state, batch, masks=mk, cells=cells, return_frames=True, **kw)
    assert loss_b.shape == (2, 5) and bool(torch.isfinite(loss_b).all())
    assert abs(float(e_in) - float(loss_b[:, :3].mean())) <= 1e-6 * float(e_in) and abs(float(e_out) - float(loss_b[:, 3:].mean())) <= 1e-6 * float(e_out)
    for chunk in (8, 24, 64):
        again = tr.val_step(state, batch, masks=mk, cells=cells, return_frames=True, chunk=chunk, **kw)
        assert torch.equal(again[2], loss_b) and torch.equal(again[0], e_in) and torch.equal(again[1], e_out), chunk
    from enf_pde_amd.fitting.trainers.latent_ode import cell_loss_weights
    lw0 = cell_loss_weights(kw.get("weights"), kw.get("cell_channel_weights"), 2, 64, 1, device=cuda, frames=0)
    lat = tr._fitted_cells(state, batch[:, 0], mk, lw0, cells, noise=False)
    with torch.no_grad():
        sol = tr.rollout(state.params["ode_params"], lat, 5)
        p_fl, a_fl, w_fl = (v.reshape(10, *v.shape[2:]) for v in sol)
        out = tr.nef.apply(state.params["nef"], cells[0][None].expand(10, -1, -1), p_fl, a_fl, w_fl).double()
        tgt = batch.reshape(10, 64, 1).double()
        wn10 = None if wn is None else wn.reshape(10, 64, *wn.shape[3:]).double()
        key = "obs_channel_weight" if kind == "cell_channel_weights" else "obs_weight"
        wkw = [{} if wn10 is None else {key: wn10[i:i + 1]} for i in range(10)]
        want = torch.stack([cell_mse_torch(out[i:i + 1], tgt[i:i + 1], 4, cells[1][None].double(), **wkw[i]) for i in range(10)]).reshape(2, 5)
    err = ((loss_b.double() - want).abs() / want).max()
    print(f"val_step(cells=, {kind}): loss_b {loss_b.tolist()} worst relative difference {float(err):.2e}")
    assert float(err) <= LOSS_TOL["f32"]


# ---- 9. fit_errors(cells=)
def test_fit_errors_on_cells_match_the_yardstick(cuda):
    """err_g (B, M) and loss_b of fit_errors(cells=, cell_channel_weights=) against tests/cells_cw_ref.py in fp64 at the fitted latents,
    at the err_g bound of the kernel test; chunked evaluation gives the same bits; NaN targets under the zero weights"""
    cfg, prm, ocfg, oprm, coords, traj, conf, tr, state, t = _setup(cuda)
    cells, x64, q64 = _cells(t)
    rng = np.random.default_rng(9)
    img = f32(traj[:, 0]).reshape(2, 64, 1)
    cw = _frame_weights(rng, (2, 64, 1))
    bad = img.copy()
    bad[cw == 0] = np.nan
    mk = _masks(cuda, 8, 3, 1)
    loss_b, err = tr.fit_errors(state, t(bad), masks=mk, cells=cells, cell_channel_weights=t(cw))
    lb2, err2 = tr.fit_errors(state, t(bad), masks=mk, cells=cells, cell_channel_weights=t(cw), chunk=24)
    assert err.shape == (2, 64) and torch.equal(err, err2) and torch.equal(loss_b, lb2)
    from enf_pde_amd.fitting.trainers.latent_ode import cell_loss_weights
    lw = cell_loss_weights(None, t(cw), 2, 64, 1, device=cuda)
    lat = tr._fitted_cells(state, t(bad), mk, lw, cells)
    n = lambda v: f32(v.cpu().numpy())
    cwn = n(lw.w)
    ref = CW.cell_loss(cfg, prm, np.broadcast_to(x64[None], (2, 256, 2)), n(lat["p_pos"]), n(lat["a"]), n(lat["gaussian_window"]), img, 4,
                       np.broadcast_to(q64[None], (2, 256)), cwn, grads=False)
    eps = TAU["f32"] * ref.out_max * np.abs(q64).reshape(64, 4).sum(-1)[None]
    ebound = (cwn * (2 * np.abs(ref.dd) * eps[..., None] + (eps * eps)[..., None])).sum(-1)
    d_err = np.abs(err.double().cpu().numpy() - ref.err_g)
    print(f"fit_errors(cells=): err_g / bound {float((d_err / np.maximum(ebound, 1e-300))[ebound > 0].max()):.2e} loss_b {loss_b.tolist()} reference {ref.loss_b.tolist()}")
    assert (d_err <= ebound).all() and bool((err[t(cw)[..., 0] == 0] == 0).all())
    assert np.all(np.abs(loss_b.double().cpu().numpy() - ref.loss_b) <= ebound.sum(1) / 64)


# ---- 10. the auto-decoder trainer
def test_autodecoder_trainer_steps_on_cells_against_the_composed_route(cuda):
    """NonMetaPDETrainer: one ode_train_step(cells=) -- its loss is the fused roll-out loss, which agrees with apply + nef.cell_mse within
    LOSS_TOL["f32"] and 5e-3 on the ODE gradients; only the ODE parameters move -- and one val_step(cells=, return_frames=True) against
    cell_mse_torch on a decode of the rolled-out latents"""
    pb, tr, state, t = make_trainer(cuda)
    cells, _, _ = _cells(t)
    traj = t(pb.traj).reshape(2, -1, 64, 1)
    idx = torch.tensor(IDX, device=cuda)
    pm = _masks(cuda, 8, None, 5, frames=10)
    cw = t(_frame_weights(np.random.default_rng(6), (2, 64, 1)))
    got = {}
    for fused in (True, False):
        leaves = [v.detach().clone().requires_grad_(True) for _, v in _flat(state.params["ode_params"])]
        params = dict(state.params, ode_params=_unflatten(state.params["ode_params"], leaves))
        l2 = tr.ode_loss(params, traj, idx, pm, cells=cells, cell_channel_weights=cw, fused=fused)
        got[fused] = (float(l2.detach()), [g.cpu().double().numpy() for g in torch.autograd.grad(l2, leaves)])
    errs = [rel(a, b) for a, b in zip(got[True][1], got[False][1])]
    before = {k: v.clone() for k, v in _flat(state.params["ode_params"])}
    w0 = [v.clone() for v in tr.nef.param_tensors(state.params["nef"])]
    loss, new = tr.ode_train_step(state, (traj, idx), point_masks=pm, cells=cells, cell_channel_weights=cw)
    print(f"auto-decoder ode_train_step(cells=): loss {float(loss):.6f} fused {got[True][0]:.6f} composed {got[False][0]:.6f} worst ODE gradient {max(errs):.2e}")
    assert abs(got[True][0] - got[False][0]) <= LOSS_TOL["f32"] * got[False][0] and all(e < 5e-3 for e in errs), errs
    assert abs(float(loss) - got[True][0]) <= 1e-6 * got[True][0]
    after = dict(_flat(new.params["ode_params"]))
    assert any(not torch.equal(after[k], before[k]) for k in before)
    assert all(torch.equal(a, b) for a, b in zip(tr.nef.param_tensors(new.params["nef"]), w0)) and new.params["autodecoder"] is state.params["autodecoder"]
    e_in, e_out, loss_b = tr.val_step(state, (traj, idx), cells=cells, return_frames=True)
    with torch.no_grad():
        z0 = tr.autodecoder.apply(state.params["autodecoder"], idx)
        sol = tr.rollout(state.params["ode_params"], z0, 20)
        p_fl, a_fl, w_fl = (v.reshape(40, *v.shape[2:]) for v in sol)
        out = tr.nef.apply(state.params["nef"], cells[0][None].expand(40, -1, -1), p_fl, a_fl, w_fl).double()
        tgt = traj[:, :20].reshape(40, 64, 1).double()
        want = torch.stack([cell_mse_torch(out[i:i + 1], tgt[i:i + 1], 4, cells[1][None].double()) for i in range(40)]).reshape(2, 20)
    err = float(((loss_b.double() - want).abs() / want).max())
    print(f"auto-decoder val_step(cells=): in {float(e_in):.5f} out {float(e_out):.5f} worst per-frame difference {err:.2e}")
    assert loss_b.shape == (2, 20) and err <= LOSS_TOL["f32"]
    assert abs(float(e_in) - float(loss_b[:, :10].mean())) <= 1e-6 * float(e_in) and abs(float(e_out) - float(loss_b[:, 10:].mean())) <= 1e-6 * float(e_out)
    assert torch.equal(tr.val_step(state, (traj, idx), cells=cells, return_frames=True, chunk=24)[2], loss_b)
