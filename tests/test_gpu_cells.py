"""Grouped observations on the GPU (include/enf_hip.h, "Grouped observations": enf_fit_step_g, enf_eval_loss_g):

    obs[b,m,o] = sum_{k<G} q[b, mG+k] out[b, mG+k, o]        loss = 1/(B M O) sum w[b,m] sum_o (obs - target)^2

B = 3, Z = 7, O = 2.  A wave's tile is 16 consecutive rows of the flattened (B N) axis, so the (G, N) pairs are: (4, 80) whole tiles;
(16, 48) a group IS a tile; (2, 50) B N = 150 is no multiple of 16 -- the last tile holds three valid groups and clamped lanes;
(8, 24) signal 1 starts in the middle of tile 1, so one tile holds groups of two signals.  x is per signal.  q > 0 random, w with about
a third exact zeros, NaN / Inf targets under them.

Bounds.  Against tests/cells_ref.py (fp64): the project's contract for the fit step -- f32: loss 1e-5 relative, gradients 2e-4
relative L2; bf16: loss 3e-2, gradients 7e-2.  Targets are random, so residuals are O(1) and averaging does not shrink them below
bf16 noise.  Against the composed route on the GPU (apply, the group sum and d out in torch, backward), which shares no tail-loss code
with the fused form: 1e-5 relative L2 in f32, the bound the Gauss-Newton product holds against its composed route."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from tests.cells_ref import B, Z, case, f32, fit_loop, poisoned, rel
from tests.helpers import build_nef, make_cfg
from tests.test_gpu_forward import TOL as TAU
from enf_pde_amd import _lib
from enf_pde_amd.fitting import cell_quadrature, decode_cell_averages, draw_cell_samples, fit_cell_averages

pytestmark = pytest.mark.gpu

GUARD = 16
PAIRS = [(4, 80), (16, 48), (2, 50), (8, 24)]
INVS = ["rel_pos_periodic", "latitude_periodic"]
#        D    H  precision  invariant           (G, N)
CASES = [(64, 2, prec, inv, gn) for prec in ("f32", "bf16") for inv in INVS for gn in PAIRS] + [(128, 2, "bf16", "rel_pos_periodic", (4, 80))]
TOL = {"f32": (1e-5, 2e-4), "bf16": (3e-2, 7e-2)}                   # (loss, gradients)
LOSS_TOL = {"f32": 5e-4, "bf16": 5e-2}                              # tests/test_gpu_signal_masks.py
DET = _lib.ENF_FIT_DETERMINISTIC


def _t(cuda):
    return lambda v: torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda)


def _run(cuda, nef, params, c, kind, flags=0, target=None, q="given", w="given", poison=255, want=("loss", "err", "loss_b")):
    """One raw C-ABI call on a workspace filled with `poison`: kind "fit" = enf_fit_step_g, "eval" = enf_eval_loss_g, "w" =
    enf_fit_step_w with weight `w` (G = 1 only).  err_g and loss_b sit in NaN-filled buffers with GUARD floats behind them."""
    lib = _lib.load()
    t = _t(cuda)
    x, p, a, s = t(c.x), t(c.p), t(c.a), t(c.s)
    y = t(poisoned(c)) if target is None else target
    qt = t(c.q) if isinstance(q, str) else q
    wt = t(c.w) if isinstance(w, str) else w
    desc = nef._desc(B, c.N, Z)
    nbytes = int(lib.enf_workspace_bytes_ex(ctypes.byref(desc), flags))
    ws = torch.full((nbytes,), poison, device=cuda, dtype=torch.uint8)
    packed = nef.pack(params)
    ptr = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    loss = torch.zeros(1, device=cuda)
    ebuf = torch.full((B * c.M + GUARD,), float("nan"), device=cuda)
    lbuf = torch.full((B + GUARD,), float("nan"), device=cuda)
    dp, da, ds = torch.full_like(p, float("nan")), torch.full_like(a, float("nan")), torch.full_like(s, float("nan"))
    head = (ctypes.byref(desc), ptr(x), c.N * x.shape[-1], ptr(p), ptr(a), ptr(s), ptr(packed), ptr(y))
    if kind == "fit":
        _lib.launch(cuda, lib.enf_fit_step_g, *head, c.G, ptr(qt), ptr(wt), c.gs, ptr(loss), ptr(dp), ptr(da), ptr(ds),
                    ptr(ebuf) if "err" in want else None, ptr(lbuf) if "loss_b" in want else None, ptr(ws), nbytes, flags, st)
    elif kind == "eval":
        _lib.launch(cuda, lib.enf_eval_loss_g, *head, c.G, ptr(qt), ptr(wt), ptr(loss) if "loss" in want else None,
                    ptr(ebuf) if "err" in want else None, ptr(lbuf) if "loss_b" in want else None, ptr(ws), nbytes, flags, st)
    else:
        assert c.G == 1
        _lib.launch(cuda, lib.enf_fit_step_w, *head, c.gs, ptr(loss), ptr(dp), ptr(da), ptr(ds), ptr(ws), nbytes, ptr(wt), flags, st)
    torch.cuda.synchronize()
    return NS(loss=loss, dp=dp, da=da, ds=ds, err=ebuf[:B * c.M].view(B, c.M), loss_b=lbuf[:B], err_guard=ebuf[B * c.M:], loss_b_guard=lbuf[B:])


def _model(cuda, c, precision):
    nef = build_nef(c.cfg, precision)
    return nef, nef.load_params(c.prm, device=cuda)


def _same_bits(u, v, names=("loss", "dp", "da", "ds", "err", "loss_b")):
    return [n for n in names if not torch.equal(getattr(u, n), getattr(v, n))]


def check_fit_step_and_evaluation(cuda, c, precision, what):
    """One case of tests/cells_ref.py (any num_out: c.O) through enf_fit_step_g and enf_eval_loss_g: loss, d(p, a, sigma), err_g and
    loss_b against the fp64 reference, NaN / Inf targets under every zero weight; the evaluation call gives the fit step's err_g and
    loss_b, bit for bit; loss_b.mean() is the loss; nothing behind the outputs.  (tests/test_gpu_wide_out.py runs it at num_out 5, 32.)"""
    O = c.O
    nef, params = _model(cuda, c, precision)
    tol_l, tol_g = TOL[precision]
    fit = _run(cuda, nef, params, c, "fit")
    ev = _run(cuda, nef, params, c, "eval")
    e_loss = abs(float(fit.loss) - c.ref.loss) / c.ref.loss
    e_g = [rel(g.cpu().numpy(), r) for g, r in zip((fit.dp, fit.da, fit.ds), c.ref.g)]
    # err_g and loss_b: the bound of tests/test_gpu_fit_errors.py carried through the group sum -- an output within eps0 = tau max|out_ref|
    # of the reference (tau: the project's forward tolerance) moves obs by at most eps = eps0 sum_k |q|, and a squared residual by at
    # most 2 |dd| eps + eps^2
    eps = TAU[precision] * c.ref.out_max * np.abs(c.q).reshape(B, c.M, c.G).sum(-1)
    ebound = c.w * (2 * np.abs(c.ref.dd) * eps[..., None] + (eps * eps)[..., None]).sum(-1)
    lbound = ebound.sum(1) / (c.M * O)
    d_err, d_lb = np.abs(fit.err.double().cpu().numpy() - c.ref.err_g), np.abs(fit.loss_b.double().cpu().numpy() - c.ref.loss_b)
    e_err, e_lb = float((d_err / np.maximum(ebound, 1e-300))[ebound > 0].max()), float((d_lb / np.maximum(lbound, 1e-300)).max())
    print(f"cells {what} {precision}: loss {e_loss:.2e} dp {e_g[0]:.2e} da {e_g[1]:.2e} dsigma {e_g[2]:.2e} "
          f"err_g / bound {e_err:.2e} loss_b / bound {e_lb:.2e} eval loss {abs(float(ev.loss) - c.ref.loss) / c.ref.loss:.2e}")
    assert e_loss <= tol_l and abs(float(ev.loss) - c.ref.loss) <= tol_l * c.ref.loss
    assert all(e <= tol_g for e in e_g), e_g
    assert (d_err <= ebound).all() and (d_lb <= lbound).all(), (e_err, e_lb)
    for r in (fit, ev):
        assert bool(torch.isfinite(r.err).all()) and bool(torch.isfinite(r.loss_b).all())
        assert bool(torch.isnan(r.err_guard).all()) and bool(torch.isnan(r.loss_b_guard).all())
        assert bool((r.err[torch.tensor(c.w == 0)] == 0).all()) and bool((r.err[torch.tensor(c.w > 0)] > 0).all())
        assert abs(float(r.loss_b.double().mean()) - float(r.loss)) <= 1e-5 * float(r.loss)
    assert all(bool(torch.isfinite(g).all()) for g in (fit.dp, fit.da, fit.ds))
    assert torch.equal(ev.err, fit.err) and torch.equal(ev.loss_b, fit.loss_b)


@pytest.mark.parametrize("D,H,precision,inv,gn", CASES)
def test_fit_step_and_evaluation_match_the_reference(cuda, D, H, precision, inv, gn):
    """loss, d(p, a, sigma), err_g and loss_b against tests/cells_ref.py in fp64, NaN / Inf targets under every zero weight; the
    evaluation call gives the fit step's err_g and loss_b, bit for bit; loss_b.mean() is the loss; nothing behind the outputs."""
    check_fit_step_and_evaluation(cuda, case(inv, *gn, D=D, H=H), precision, f"{D}x{H} {inv} G={gn[0]} N={gn[1]}")


@pytest.mark.parametrize("inv", INVS)
@pytest.mark.parametrize("gn", PAIRS)
def test_fit_step_matches_the_composed_route(cuda, inv, gn):
    """f32: apply, the group sum and d out in torch ops, backward through apply -- 1e-5 relative L2 on every gradient and the loss"""
    c = case(inv, *gn)
    nef, params = _model(cuda, c, "f32")
    t = _t(cuda)
    fit = _run(cuda, nef, params, c, "fit", target=t(c.y))
    G, M, O = c.G, c.M, c.O
    leaves = [t(v).requires_grad_(True) for v in (c.p, c.a, c.s)]
    out = nef.apply(params, t(c.x), *leaves)
    with torch.no_grad():
        q, w, y = t(c.q), t(c.w), t(c.y)
        obs = (q[..., None] * out).reshape(B, M, G, O).sum(2)
        dd = torch.where((w > 0)[..., None], obs - y, torch.zeros_like(obs))
        loss = (w[..., None] * dd * dd).sum() / (B * M * O)
        dobs = 2.0 * w[..., None] * dd / (B * M * O) * c.gs
        dout = q[..., None] * dobs.repeat_interleave(G, dim=1)
        ref_obs = decode_cell_averages(nef, params, t(c.x), q, G, leaves[0].detach(), leaves[1].detach(), leaves[2].detach())
    out.backward(dout)
    torch.cuda.synchronize()
    assert torch.allclose(ref_obs, obs, rtol=1e-6, atol=1e-7)
    errs = [rel(g.cpu().numpy(), l.grad.cpu().numpy()) for g, l in zip((fit.dp, fit.da, fit.ds), leaves)]
    e_loss = abs(float(fit.loss) - float(loss)) / float(loss)
    print(f"composed route {inv} G={G} N={c.N}: loss {e_loss:.2e} dp {errs[0]:.2e} da {errs[1]:.2e} dsigma {errs[2]:.2e}")
    assert e_loss <= 1e-5 and all(e <= 1e-5 for e in errs), (e_loss, errs)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("gn", PAIRS)
def test_same_bits(cuda, precision, gn):
    """ENF_FIT_DETERMINISTIC: two runs on differently poisoned workspaces are equal in every bit.  err_g and loss_b are the same bits
    in the fit step and the evaluation, in the default and the deterministic mode, and with any subset of the evaluation's outputs
    (loss_b without err_g goes through the workspace)."""
    c = case("rel_pos_periodic", *gn)
    nef, params = _model(cuda, c, precision)
    one = _run(cuda, nef, params, c, "fit", flags=DET, poison=255)
    two = _run(cuda, nef, params, c, "fit", flags=DET, poison=0x5A)
    assert _same_bits(one, two) == [] and all(bool(torch.isfinite(getattr(one, n)).all()) for n in ("loss", "dp", "da", "ds"))
    plain = _run(cuda, nef, params, c, "fit")
    assert _same_bits(one, plain, ("err", "loss_b")) == []
    ev_det = _run(cuda, nef, params, c, "eval", flags=DET, poison=0)
    ev = _run(cuda, nef, params, c, "eval", poison=0x5A)
    assert _same_bits(one, ev_det, ("err", "loss_b")) == [] and _same_bits(one, ev, ("err", "loss_b")) == []
    assert torch.equal(ev_det.loss, _run(cuda, nef, params, c, "eval", flags=DET).loss)
    only_b = _run(cuda, nef, params, c, "eval", want=("loss_b",))
    assert torch.equal(only_b.loss_b, one.loss_b) and bool(torch.isnan(only_b.err).all()) and float(only_b.loss) == 0.0
    only_e = _run(cuda, nef, params, c, "eval", want=("err",))
    assert torch.equal(only_e.err, one.err) and bool(torch.isnan(only_e.loss_b).all())
    only_l = _run(cuda, nef, params, c, "eval", flags=DET, want=("loss",))
    assert torch.equal(only_l.loss, ev_det.loss) and bool(torch.isnan(only_l.err).all())
    nofit = _run(cuda, nef, params, c, "fit", flags=DET, want=())                       # the fit step without err_g and loss_b
    assert _same_bits(one, nofit, ("loss", "dp", "da", "ds")) == [] and bool(torch.isnan(nofit.err).all())


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("gn", PAIRS)
def test_inf_targets_under_zero_weights_change_no_bit(cuda, precision, gn):
    c = case("latitude_periodic", *gn)
    nef, params = _model(cuda, c, precision)
    t = _t(cuda)
    clean = _run(cuda, nef, params, c, "fit", flags=DET, target=t(c.y))
    inf = _run(cuda, nef, params, c, "fit", flags=DET, target=t(poisoned(c, "inf")))
    assert bool(torch.isinf(t(poisoned(c, "inf"))).any()) and _same_bits(clean, inf) == []
    ev_clean = _run(cuda, nef, params, c, "eval", flags=DET, target=t(c.y))
    ev_inf = _run(cuda, nef, params, c, "eval", flags=DET, target=t(poisoned(c, "inf")))
    assert _same_bits(ev_clean, ev_inf, ("loss", "err", "loss_b")) == []


@pytest.mark.parametrize("N", [50, 33])
def test_group_of_one_is_the_per_point_step(cuda, N):
    """G = 1 with unit factors (given, or NULL = 1 / G) against enf_fit_step_w(weight = q w = w): 1e-6 relative in f32, deterministic
    mode -- another instantiation, the same arithmetic.  (With q != 1 the residual is q out - target, another loss.)"""
    c = case("rel_pos_periodic", 1, N)
    nef, params = _model(cuda, c, "f32")
    t = _t(cuda)
    old = _run(cuda, nef, params, c, "w", flags=DET)
    for q in (torch.ones(B, N, device=cuda), None):
        new = _run(cuda, nef, params, c, "fit", flags=DET, q=q)
        errs = {n: rel(getattr(new, n).cpu().numpy(), getattr(old, n).cpu().numpy()) for n in ("loss", "dp", "da", "ds")}
        print("G = 1 against enf_fit_step_w", N, errs)
        assert all(e <= 1e-6 for e in errs.values()), errs
    r = _run(cuda, nef, params, c, "fit", flags=DET, q=None, w=None, target=t(c.y))     # no weights at all: the plain step
    plain = _run(cuda, nef, params, c, "w", flags=DET, w=None, target=t(c.y))
    assert all(rel(getattr(r, n).cpu().numpy(), getattr(plain, n).cpu().numpy()) <= 1e-6 for n in ("loss", "dp", "da", "ds"))


# ---- fitting/cells.py
def _fit_problem(cuda, precision):
    C, Zl = 8, 4
    cfg = make_cfg("rel_pos_periodic", D=64, H=2, C=C, O=2)
    prm = R.init_params(7, cfg, jitter=0.1)
    rng = np.random.default_rng(8)
    x, q = cell_quadrature((-1.0, 1.0, (6, 5)), 2)                       # 30 cells of 4 Gauss points: B N = 360, no multiple of 128
    x64, q64 = f32(x.numpy()), f32(q.numpy())
    cx = x64.reshape(30, 4, 2).mean(1)
    y = np.stack([np.stack([np.sin(2.0 * cx[:, 0] + b) * np.cos(1.5 * cx[:, 1]), 0.5 * cx[:, 0] * cx[:, 1] + 0.1 * b], -1) for b in range(B)])
    y = f32(y + 0.05 * rng.standard_normal(y.shape))
    w = f32(rng.uniform(0.5, 1.5, (B, 30)))
    w[rng.uniform(size=(B, 30)) < 0.2] = 0.0
    lat0 = (f32(R.init_positions_grid(1, Zl, 2) + 0.02 * rng.standard_normal((1, Zl, 2))), f32(1 + 0.1 * rng.standard_normal((1, Zl, C))),
            f32(np.full((1, Zl, 1), 2.0 / 3)))
    lr_p, lr_a = 2.0, np.full((C,), 30.0)              # (the reference loop's loss falls by about 13 % per step: well above bf16 noise)
    t = _t(cuda)
    nef = build_nef(cfg, precision)
    nef.deterministic = True
    lat0_t = {"p_pos": t(lat0[0]), "a": t(lat0[1]), "gaussian_window": t(lat0[2])}
    lrs = {"p_pos": t([lr_p]), "a": t(lr_a), "gaussian_window": t([0.0])}
    return NS(cfg=cfg, prm=prm, x=x64, q=q64, y=y, w=w, lat0=lat0, lr=(lr_p, lr_a), nef=nef, params=nef.load_params(prm, device=cuda),
              lat0_t=lat0_t, lrs=lrs, xt=t(x64), qt=t(q64), yt=t(y), wt=t(w))


_FIT_REF = {}


def _fit_reference(pb):
    if "ref" not in _FIT_REF:
        _FIT_REF["ref"] = fit_loop(pb.cfg, pb.prm, pb.x, pb.q, 4, pb.y, pb.w, pb.lat0, pb.lr, 3)
    return _FIT_REF["ref"]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_fit_cell_averages_follows_the_reference_loop(cuda, precision):
    """three steps against the same loop on tests/cells_ref.py in fp64: every step's loss and the final one within LOSS_TOL; the loss
    falls; loss_b rows are the steps' per-signal losses; NaN targets under the zero weights"""
    pb = _fit_problem(cuda, precision)
    ref_losses, _ = _fit_reference(pb)
    y = pb.yt.clone()
    y[pb.wt == 0] = float("nan")
    loss, lat, loss_b = fit_cell_averages(pb.nef, pb.params, pb.lat0_t, pb.lrs, pb.xt, pb.qt, 4, y, 3, obs_weight=pb.wt, per_signal_loss=True)
    loss2, lat2 = fit_cell_averages(pb.nef, pb.params, pb.lat0_t, pb.lrs, pb.xt, pb.qt, 4, y, 3, obs_weight=pb.wt)
    torch.cuda.synchronize()
    got = loss_b.double().mean(1).cpu().numpy()
    print("fit_cell_averages", precision, "losses", got.tolist(), "reference", ref_losses.tolist())
    assert loss_b.shape == (4, B) and lat["a"].shape[0] == B
    assert np.all(np.abs(got - ref_losses) <= LOSS_TOL[precision] * ref_losses), (got, ref_losses)
    assert abs(float(loss) - ref_losses[3]) <= LOSS_TOL[precision] * ref_losses[3]
    assert ref_losses[3] < ref_losses[0] and float(loss) < got[0] and np.all(np.diff(got) < 0)
    assert torch.equal(loss, loss2) and all(torch.equal(lat[k], lat2[k]) for k in lat)


def test_sampled_fit_equals_the_fit_on_the_gathered_subset(cuda):
    """deterministic mode: with `sample` (the same subset at every step) the result is the unsampled call on the gathered points,
    factors, targets and weights, bit for bit; an int draws the index sets of draw_cell_samples with the same generator"""
    pb = _fit_problem(cuda, "f32")
    S, Ms, G = 2, 12, 4
    sub = torch.randperm(30, generator=torch.Generator().manual_seed(2))[:Ms].to(cuda)
    rows = (sub[:, None] * G + torch.arange(G, device=cuda)).reshape(-1)
    idx = sub[None].expand(S + 1, -1).contiguous()
    a_loss, a_lat, a_lb = fit_cell_averages(pb.nef, pb.params, pb.lat0_t, pb.lrs, pb.xt, pb.qt, G, pb.yt, S, obs_weight=pb.wt, sample=idx,
                                            per_signal_loss=True)
    b_loss, b_lat, b_lb = fit_cell_averages(pb.nef, pb.params, pb.lat0_t, pb.lrs, pb.xt[rows], pb.qt[rows], G, pb.yt[:, sub].contiguous(), S,
                                            obs_weight=pb.wt[:, sub].contiguous(), per_signal_loss=True)
    torch.cuda.synchronize()
    assert torch.equal(a_loss, b_loss) and torch.equal(a_lb, b_lb) and all(torch.equal(a_lat[k], b_lat[k]) for k in a_lat)
    assert bool(torch.isfinite(a_lb).all()) and float(a_loss) > 0
    drawn = draw_cell_samples(30, Ms, S, generator=torch.Generator().manual_seed(9))
    assert not torch.equal(drawn[0], drawn[1])                              # a fresh set per step
    c_loss, c_lat = fit_cell_averages(pb.nef, pb.params, pb.lat0_t, pb.lrs, pb.xt, pb.qt, G, pb.yt, S, obs_weight=pb.wt, sample=Ms,
                                      generator=torch.Generator().manual_seed(9))
    d_loss, d_lat = fit_cell_averages(pb.nef, pb.params, pb.lat0_t, pb.lrs, pb.xt, pb.qt, G, pb.yt, S, obs_weight=pb.wt, sample=drawn)
    assert torch.equal(c_loss, d_loss) and all(torch.equal(c_lat[k], d_lat[k]) for k in c_lat)
