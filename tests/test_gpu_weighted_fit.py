"""Per-point loss weights on the GPU path (include/enf_hip.h, "Weighted loss"):

    loss = 1 / (B N O) * sum_{b,n} w[b,n] * sum_o (out - target)^2,     d out = 2 w (out - target) / (B N O) * grad_scale

in the fused tail (enf_fit_step_w), enf_mse_value_grad_w, enf_fit_inputs_w, the inner loop, the outer step and the roll-out
loss / validation.  The oracle is oracle.enf_ref_torch.nef_apply in fp64; the weighted loss is formed here around it.
Shapes are the smallest that reach each place the kernel can go wrong: N = 70 is one partial 128-query tail workgroup with
clamped lanes, N = 130 with B = 2 puts 4 live queries into a third workgroup and exercises the flat index b N + n.

Tolerances: gradients tests/test_gpu_backward.TOL; a loss value against fp64 as in tests/test_gpu_golden.py's inner-loop trace
(5e-4 f32 / 5e-2 bf16 of max(1, loss)); fused against three calls as in test_gpu_backward's cross-check (1e-5 / 2e-2 on the
loss, ten times that on the gradients)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from tests.helpers import make_cfg, make_inputs, build_nef
from tests.test_gpu_backward import TOL, ref_grads, rel
from enf_pde_amd import _lib
from enf_pde_amd.fitting.weights import valid_weights, normalize_point_weights

pytestmark = pytest.mark.gpu

LOSS_TOL = {"f32": 5e-4, "bf16": 5e-2}          # tests/test_gpu_golden.py::test_inner_loop_matches_golden_trace


def _weights(rng, B, N):
    """random in [0, 2], about a quarter exactly 0"""
    w = rng.uniform(0, 2, (B, N))
    w[rng.uniform(size=(B, N)) < 0.25] = 0.0
    return w.astype(np.float32).astype(np.float64)


_REF = {}


def _case(invariant, D, H, O, N, seed=31, B=2, Z=9):
    """inputs and fp64 reference of one weighted fit step, computed once per session and left unchanged"""
    key = (invariant, D, H, O, N, seed, B, Z)
    if key not in _REF:
        cfg = make_cfg(invariant, D=D, H=H, C=12, O=O, freq=(0.3, 0.6))
        prm = R.init_params(seed, cfg, jitter=0.1)
        x, p, a, s = make_inputs(cfg, B, N, Z, seed + 1)
        rng = np.random.default_rng(seed + 2)
        y = rng.standard_normal((B, N, O))
        w = _weights(rng, B, N)
        out = T.nef_apply(T.to_torch(prm, torch.float64), cfg, *(torch.tensor(v) for v in (x, p, a, s))).numpy()
        loss = float((w[..., None] * (out - y) ** 2).sum() / (B * N * O))
        _, rp, ra, rs = ref_grads(prm, cfg, x, p, a, s, 2 * w[..., None] * (out - y) / (B * N * O))
        _REF[key] = (cfg, prm, (x, p, a, s, y, w), (loss, rp, ra, rs))
    return _REF[key]


def _t(cuda):
    return lambda v: torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda)


def _check_against(res, ref, precision, what):
    loss, rp, ra, rs = ref
    got = float(res[0])
    print(what, precision, "loss", got, "ref", loss)
    errs = {k: rel(g.cpu().numpy().astype(np.float64), r) for k, g, r in (("p", res[1], rp), ("a", res[2], ra), ("sigma", res[3], rs))}
    print(what, precision, "gradient errors", errs)
    assert np.isfinite(got) and abs(got - loss) < LOSS_TOL[precision] * max(1.0, loss), (what, got, loss)
    for k, e in errs.items():
        assert np.isfinite(e) and e < TOL[precision], (what, precision, k, e)


CASES = [("rel_pos_periodic", D, H, O, N) for (D, H) in ((128, 2), (64, 1)) for O in (1, 3) for N in (70, 130)] + \
        [("rel_pos_periodic", 32, 3, 3, 130), ("latitude_periodic", 128, 2, 3, 130)]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("invariant,D,H,O,N", CASES)
def test_weighted_fit_step_matches_oracle(cuda, bwd_variant, invariant, D, H, O, N, precision):
    cfg, prm, (x, p, a, s, y, w), ref = _case(invariant, D, H, O, N)
    nef = build_nef(cfg, precision)
    t = _t(cuda)
    res = nef.mse_value_and_latent_grads(nef.load_params(prm, device=cuda), t(x), t(p), t(a), t(s), t(y), weight=t(w))
    _check_against(res, ref, precision, (invariant, D, H, O, N))


def test_weight_of_the_wrong_shape_is_a_value_error(cuda):
    cfg, prm, (x, p, a, s, y, w), _ = _case("rel_pos_periodic", 64, 1, 1, 70)
    nef = build_nef(cfg, "f32")
    t = _t(cuda)
    with pytest.raises(ValueError):
        nef.mse_value_and_latent_grads(nef.load_params(prm, device=cuda), t(x), t(p), t(a), t(s), t(y), weight=t(w)[:, :-1])
    with pytest.raises(ValueError):
        nef.mse_value_and_latent_grads(nef.load_params(prm, device=cuda), t(x), t(p), t(a), t(s), t(y), weight=t(w)[..., None])


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("N", [70, 130])
def test_unit_weights_are_the_unweighted_call(cuda, N, precision):
    """deterministic mode: equal bits; default (atomic) mode: the oracle tolerances of the test above"""
    cfg, prm, (x, p, a, s, y, _), _ = _case("rel_pos_periodic", 128, 2, 3, N)
    t = _t(cuda)
    ones = torch.ones((2, N), device=cuda)
    det = build_nef(cfg, precision)
    det.deterministic = True
    assert det.is_deterministic()
    params = det.load_params(prm, device=cuda)
    plain = det.mse_value_and_latent_grads(params, t(x), t(p), t(a), t(s), t(y), grad_scale=2.0)
    unit = det.mse_value_and_latent_grads(params, t(x), t(p), t(a), t(s), t(y), grad_scale=2.0, weight=ones)
    for name, u, v in zip(("loss", "dp", "da", "dsigma"), unit, plain):
        assert torch.equal(u, v), (name, float((u - v).abs().max()))
    nef = build_nef(cfg, precision)
    params = nef.load_params(prm, device=cuda)
    plain = nef.mse_value_and_latent_grads(params, t(x), t(p), t(a), t(s), t(y))
    unit = nef.mse_value_and_latent_grads(params, t(x), t(p), t(a), t(s), t(y), weight=ones)
    assert abs(float(unit[0]) - float(plain[0])) < LOSS_TOL[precision] * max(1.0, float(plain[0]))
    for u, v in zip(unit[1:], plain[1:]):
        assert rel(u.cpu().numpy(), v.cpu().numpy()) < TOL[precision]


@pytest.mark.parametrize("N", [70, 130])
def test_zero_weight_removes_the_point(cuda, N, bwd_variant):
    """A 0/1 mask with NaN written into the masked-out targets: the weighted call on all N points is finite and equals the
    unweighted call on the compacted kept points times N_kept / N (same count per signal: the compacted call is rectangular).
    Queries 16..31 of the flat index (one 16-query tile) are all masked, queries 0..15 and 32..47 all kept."""
    cfg, prm, (x, p, a, s, y, _), _ = _case("rel_pos_periodic", 128, 2, 3, N)
    rng = np.random.default_rng(5)
    B = 2
    m = np.ones((B, N), bool)
    m[0, 16:32] = False                                     # a whole tile of signal 0
    m[0, 48:] = rng.uniform(size=N - 48) < 0.6
    k0 = int(m[0].sum())
    drop = rng.permutation(N)[:N - k0]                      # signal 1: the same count, elsewhere (its tiles hold both kinds)
    m[1, drop] = False
    assert m[0, :16].all() and m[0, 32:48].all() and not m[0, 16:32].any() and m[1].sum() == k0
    ynan = y.copy()
    ynan[~m] = np.nan
    t = _t(cuda)
    nef = build_nef(cfg, "f32")
    params = nef.load_params(prm, device=cuda)
    full = nef.mse_value_and_latent_grads(params, t(x), t(p), t(a), t(s), t(ynan), weight=t(m.astype(np.float64)))
    xk = np.stack([x[b][m[b]] for b in range(B)])
    yk = np.stack([y[b][m[b]] for b in range(B)])
    kept = nef.mse_value_and_latent_grads(params, t(xk), t(p), t(a), t(s), t(yk))
    f = k0 / N
    print("zero-weight", N, float(full[0]), float(kept[0]) * f)
    assert all(bool(torch.isfinite(v).all()) for v in full)
    assert abs(float(full[0]) - f * float(kept[0])) < LOSS_TOL["f32"] * max(1.0, f * float(kept[0]))
    for name, u, v in zip(("dp", "da", "dsigma"), full[1:], kept[1:]):
        e = rel(u.cpu().numpy().astype(np.float64), f * v.cpu().numpy().astype(np.float64))
        print("zero-weight", N, name, e)
        assert e < TOL["f32"], (name, e)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("deterministic", [False, True])
def test_fused_matches_the_three_calls(cuda, precision, deterministic, monkeypatch):
    from enf_pde_amd.enf import models as M
    cfg, prm, (x, p, a, s, y, w), _ = _case("latitude_periodic", 128, 2, 3, 130)
    nef = build_nef(cfg, precision)
    nef.deterministic = deterministic
    params = nef.load_params(prm, device=cuda)
    t = _t(cuda)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(M, "FUSED_FIT_STEP", fused)
        res[fused] = nef.mse_value_and_latent_grads(params, t(x), t(p), t(a), t(s), t(y), grad_scale=3.0, weight=t(w))
    tol = 1e-5 if precision == "f32" else 2e-2
    assert abs(float(res[True][0]) - float(res[False][0])) < tol * float(res[False][0])
    for g, r in zip(res[True][1:], res[False][1:]):
        assert rel(g.cpu().numpy(), r.cpu().numpy()) < 10 * tol


def test_mse_value_grad_w(cuda):
    """n = B N O with O = 3 and n / O = 2 * 333 = 666, no multiple of 256; fp64 torch is the reference.  fp32 bounds: every dout is
    three roundings from exact (2e-7 relative, asserted at 1e-6); the loss is a sum of 1998 non-negative terms (1e-5 relative)."""
    lib = _lib.load()
    rng = np.random.default_rng(3)
    B, N, O = 2, 333, 3
    out, y = rng.standard_normal((B, N, O)), rng.standard_normal((B, N, O))
    w = _weights(rng, B, N)
    y[w == 0] = np.nan
    t = _t(cuda)
    o_, y_, w_ = t(out), t(y), t(w)
    o64, y64, w64 = (v.double().cpu() for v in (o_, y_, w_))
    d = torch.where(w64[..., None] > 0, o64 - y64, torch.zeros_like(o64))
    ref_loss = float((w64[..., None] * d * d).sum() / (B * N * O))
    ref_dout = 2 * w64[..., None] * d / (B * N * O) * 1.5
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    n = B * N * O
    runs = []
    for flags in (0, _lib.ENF_MSE_DETERMINISTIC, _lib.ENF_MSE_DETERMINISTIC):
        nb = int(lib.enf_mse_scratch_bytes(n, flags))
        scr = torch.full((max(nb, 1),), 255, device=cuda, dtype=torch.uint8)
        dout, loss = torch.full_like(o_, 7.0), torch.zeros(1, device=cuda)
        _lib.launch(cuda, lib.enf_mse_value_grad_w, o_.data_ptr(), y_.data_ptr(), w_.data_ptr(), n, O, 1.5, dout.data_ptr(),
                    loss.data_ptr(), scr.data_ptr() if nb else None, nb, flags, st)
        torch.cuda.synchronize()
        runs.append((loss.clone(), dout.clone()))
        assert abs(float(loss) - ref_loss) < 1e-5 * ref_loss
        assert bool((dout[w_ == 0] == 0).all()) and bool(torch.isfinite(dout).all())
        assert float((dout.double().cpu() - ref_dout).abs().max()) < 1e-6 * float(ref_dout.abs().max())
    assert torch.equal(runs[1][0], runs[2][0]) and torch.equal(runs[1][1], runs[2][1])
    # NULL weight = the unweighted entry point, bit for bit (deterministic sums)
    yf = torch.nan_to_num(y_)
    got = []
    for fn, args in ((lib.enf_mse_value_grad_w, (None, n, O)), (lib.enf_mse_value_grad_ex, (n,))):
        nb = int(lib.enf_mse_scratch_bytes(n, 16))
        scr = torch.empty(nb, device=cuda, dtype=torch.uint8)
        dout, loss = torch.empty_like(o_), torch.zeros(1, device=cuda)
        head = (o_.data_ptr(), yf.data_ptr()) + args
        _lib.launch(cuda, fn, *head, 1.5, dout.data_ptr(), loss.data_ptr(), scr.data_ptr(), nb, 16, st)
        got.append((loss, dout))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


def test_fit_inputs_w(cuda):
    from enf_pde_amd.fitting.inner_loop import _fit_inputs
    rng = np.random.default_rng(11)
    B, N, Ns, S1, Z = 3, 50, 17, 4, 5
    t = _t(cuda)
    lat0 = {"p_pos": t(rng.standard_normal((1, Z, 2))), "a": t(rng.standard_normal((1, Z, 6))), "gaussian_window": t(np.ones((1, Z, 1)))}
    coords, img, w = t(rng.standard_normal((N, 2))), t(rng.standard_normal((B, N, 2))), t(_weights(rng, B, N))
    img[w == 0] = float("nan")
    masks = torch.tensor(np.stack([rng.permutation(N)[:Ns] for _ in range(S1)], 1), device=cuda)
    plain = _fit_inputs(lat0, coords, img, masks)
    lat, xs, ys, losses, ws = _fit_inputs(lat0, coords, img, masks, w)
    assert len(plain) == 4 and ws.shape == (S1, B, Ns)
    assert torch.equal(ws, w[:, masks.t()].transpose(0, 1))
    assert torch.equal(xs, plain[1]) and torch.equal(losses, plain[3]) and bool((losses == 0).all())
    assert torch.equal(torch.isnan(ys), torch.isnan(plain[2])) and torch.equal(torch.nan_to_num(ys), torch.nan_to_num(plain[2]))
    assert torch.equal(torch.nan_to_num(ys), torch.nan_to_num(img[:, masks.t()].transpose(0, 1)))
    for k in lat0:
        assert torch.equal(lat[k], plain[0][k]) and torch.equal(lat[k], lat0[k].expand(B, -1, -1))


# ---- inner loop and outer step: the oracle's inner loop (oracle/enf_ref_torch.py: inner_loop) with the weighted loss
def _oracle_inner_loop(params, cfg, lat0, lrs, coords, img, masks, w, create_graph=False):
    spec = T.invariant_spec(cfg["invariant"], cfg.get("num_in", 2))
    B, S = img.shape[0], masks.shape[1] - 1
    lat = {k: v.repeat_interleave(B, dim=0) for k, v in lat0.items()}
    if not create_graph:
        lat = {k: v.detach().clone().requires_grad_(True) for k, v in lat.items()}

    def loss_fn(lat, s):
        xs = coords[masks[:, s]][None].expand(B, -1, -1)
        ys, ws = img[:, masks[:, s]], w[:, masks[:, s]][..., None]
        out = T.nef_apply(params, cfg, xs, T.split_pose(lat, spec), lat["a"], lat["gaussian_window"])
        d = torch.where(ws > 0, out - ys, torch.zeros_like(out))
        return (ws * d * d).mean()

    for s in range(S):
        keys = list(lat.keys())
        g = torch.autograd.grad(loss_fn(lat, s), [lat[k] for k in keys], create_graph=create_graph, allow_unused=True)
        new = {}
        for k, gk in zip(keys, g):
            gk = torch.zeros_like(lat[k]) if (gk is None or k == "gaussian_window") else gk * B     # pde_trainer.py:206-212
            new[k] = lat[k] - lrs[k] * gk                                                            # pde_trainer.py:215-219
            if not create_graph:
                new[k] = new[k].detach().requires_grad_(True)
        lat = new
    return loss_fn(lat, S), lat


def _fit_problem(seed, B, side, Ns, Z, C=8, S=2):
    cfg = make_cfg("rel_pos_periodic", D=64, H=2, C=C, O=1)
    prm = R.init_params(seed, cfg, jitter=0.1)
    rng = np.random.default_rng(seed + 1)
    lin = np.linspace(-1, 1, side)
    coords = np.stack(np.meshgrid(lin, lin), -1).reshape(-1, 2)
    N = side * side
    img = rng.standard_normal((B, N, 1))
    lat0 = {"p_pos": R.init_positions_grid(1, Z, 2) + 0.02 * rng.standard_normal((1, Z, 2)),
            "a": 1 + 0.1 * rng.standard_normal((1, Z, C)), "gaussian_window": np.full((1, Z, 1), 2.0 / 3)}
    lrs = {"p_pos": np.array([0.5]), "a": np.full((C,), 2.0) * (1 + 0.1 * rng.standard_normal(C)), "gaussian_window": np.array([0.0])}
    masks = np.stack([rng.permutation(N)[:Ns] for _ in range(S + 1)], 1)
    return cfg, prm, coords, img, lat0, lrs, masks, rng


@pytest.mark.parametrize("holes", [False, True])
def test_inner_loop_with_weights_matches_fp64_trace(cuda, holes):
    """S = 2, explicit masks, B = 2, N = 64, Ns = 40, Z = 4, f32; tolerances of test_gpu_golden's inner-loop trace.
    holes: the weights are valid_weights of a field with NaN holes (the NaN stay in the targets handed to the product)."""
    from enf_pde_amd.fitting import inner_loop
    cfg, prm, coords, img, lat0, lrs, masks, rng = _fit_problem(7, B=2, side=8, Ns=40, Z=4)
    if holes:
        img[rng.uniform(size=img.shape) < 0.2] = np.nan
        w = valid_weights(torch.tensor(img)).numpy().astype(np.float64)
        assert 0 < w.mean() < 1
    else:
        w = _weights(rng, 2, 64)
    t64 = lambda v: torch.tensor(v, dtype=torch.float64)
    ref_loss, ref_fit = _oracle_inner_loop(T.to_torch(prm, torch.float64), cfg, {k: t64(v) for k, v in lat0.items()},
                                           {k: t64(v) for k, v in lrs.items()}, t64(coords), t64(img), torch.tensor(masks), t64(w))
    t = _t(cuda)
    nef = build_nef(cfg, "f32")
    loss, fit = inner_loop(nef, nef.load_params(prm, device=cuda), {k: t(v) for k, v in lat0.items()}, {k: t(v) for k, v in lrs.items()},
                           t(coords), t(img), torch.tensor(masks, device=cuda), weights=t(w))
    tol, ref_loss = 5e-4, ref_loss.detach()
    print("inner loop", holes, float(loss), float(ref_loss))
    assert abs(float(loss) - float(ref_loss)) < tol * max(1.0, float(ref_loss))
    for k, v in fit.items():
        ref, init = ref_fit[k].detach().numpy(), np.repeat(lat0[k], 2, 0)
        if np.abs(ref - init).max() == 0:
            assert np.abs(v.cpu().numpy() - init.astype(np.float32)).max() == 0, k      # gaussian_window frozen: its fp32 init, untouched
        else:
            e = rel(v.cpu().numpy().astype(np.float64) - init, ref - init)
            print("inner loop", holes, k, e)
            assert e < tol * 20, (k, e)


def test_meta_gradients_with_weights_match_exact_second_order(cuda):
    """tests/test_gpu_trainer.py's construction and tolerances, with the weighted objective (weights taken as they are)."""
    from enf_pde_amd.enf.models import TENSOR_PATHS
    from enf_pde_amd.fitting.trainers import meta_gradients
    from tests.test_gpu_trainer import _get
    cfg, prm, coords, img, lat0, lrs, masks, rng = _fit_problem(0, B=4, side=8, Ns=48, Z=9)
    w = _weights(rng, 4, 64)
    tp = T.to_torch(prm, torch.float64, requires_grad=True)
    tl = {k: torch.tensor(v, requires_grad=True) for k, v in lat0.items()}
    tr = {k: torch.tensor(v, requires_grad=True) for k, v in lrs.items()}
    loss_r, _ = _oracle_inner_loop(tp, cfg, tl, tr, torch.tensor(coords), torch.tensor(img), torch.tensor(masks), torch.tensor(w),
                                   create_graph=True)
    leaves = [_get(tp["params"], p) for p in TENSOR_PATHS]
    g_r = torch.autograd.grad(loss_r, leaves + list(tl.values()) + list(tr.values()), allow_unused=True)
    z = lambda gi, x: np.zeros(tuple(x.shape)) if gi is None else gi.numpy()
    gw_r = [z(a, b) for a, b in zip(g_r[:len(leaves)], leaves)]
    gl_r = {k: z(a, tl[k]) for k, a in zip(tl, g_r[len(leaves):len(leaves) + len(tl)])}
    gr_r = {k: z(a, tr[k]) for k, a in zip(tr, g_r[len(leaves) + len(tl):])}
    loss_r = float(loss_r.detach())
    nef = build_nef(cfg, "f32")
    t = _t(cuda)
    args = (nef, nef.load_params(prm, device=cuda), {k: t(v) for k, v in lat0.items()}, {k: t(v) for k, v in lrs.items()}, t(coords),
            t(img), torch.tensor(masks, device=cuda))
    loss, g = meta_gradients(*args, second_order="fd", weights=t(w), normalize=False)
    assert abs(float(loss) - loss_r) < 1e-5 * max(1.0, abs(loss_r))
    gmax = max(np.linalg.norm(x) for x in gw_r)
    bad = []
    for path, a, b in zip(TENSOR_PATHS, g["nef"], gw_r):
        nb = np.linalg.norm(b)
        e = np.linalg.norm(a.cpu().numpy() - b) / (nb if nb > 1e-3 * gmax else gmax)
        if not e < 2e-3:
            bad.append(("/".join(path[-3:]), e))
    assert not bad, bad
    for k, tol in (("a", 2e-3), ("p_pos", 5e-3)):
        e = np.linalg.norm(g["autodecoder"][k].cpu().numpy() - gl_r[k]) / max(np.linalg.norm(gl_r[k]), 1e-12)
        assert e < tol, (k, e)
    for k in ("p_pos", "a"):
        e = np.linalg.norm(g["meta_sgd_lrs"][k].cpu().numpy() - gr_r[k]) / max(np.linalg.norm(gr_r[k]), 1e-12)
        assert e < 2e-3, (k, e)
    # normalisation: weights of mean 1 per signal are what normalize=True makes of them
    loss_n, _ = meta_gradients(*args, second_order="none", weights=t(w))
    loss_m, _ = meta_gradients(*args, second_order="none", weights=normalize_point_weights(t(w)), normalize=False)
    assert torch.equal(loss_n, loss_m)


def test_nef_train_step_with_weights(cuda, monkeypatch):
    """finite loss, parameters move; weights=None takes the old code path (the weighted loss is never formed)"""
    from tests.test_gpu_ode_trainer import _setup
    from enf_pde_amd.fitting.trainers import pde_trainer as PT
    _, _, _, _, coords, traj, conf, tr, state, t = _setup(cuda)
    batch = t(traj[:, 0])
    w = t(_weights(np.random.default_rng(1), 2, 64))
    before = [x.clone() for x in tr.nef.param_tensors(state.params["nef"])]
    loss, new = tr.nef_train_step(state, batch, weights=w)
    assert np.isfinite(float(loss))
    assert any(not torch.equal(a, b) for a, b in zip(before, tr.nef.param_tensors(new.params["nef"])))

    # the ODE-phase steps take the same weights, per point or per frame and point
    tj = t(traj)
    for step, wt in ((tr.ode_train_step, w), (tr.dual_train_step, w[:, None].expand(2, 5, 64).contiguous())):
        loss, _ = step(state, tj, weights=wt)
        assert np.isfinite(float(loss))

    def never(*a, **k):
        raise AssertionError("the unweighted step formed a weighted loss")
    monkeypatch.setattr(PT, "weighted_mse", never)
    from enf_pde_amd.fitting.trainers import latent_ode as LO
    monkeypatch.setattr(LO, "weighted_mse", never)
    for step, arg in ((tr.nef_train_step, batch), (tr.ode_train_step, tj), (tr.dual_train_step, tj)):
        loss, _ = step(state, arg)
        assert np.isfinite(float(loss))


def test_rollout_loss_and_val_step_with_weights(cuda):
    """rollout_loss / val_step with weights against the same quantities formed here in fp64 from the product's own roll-out and
    decode.  rollout_loss: the decoded values are the same kernels' on the same inputs, so only the fp32 reduction over 6 x 32
    terms differs: 1e-5 relative.  val_step: the fit inside it and the one here differ by the order of the float atomics (1e-7
    relative per gradient), carried through two inner steps and a five-frame roll-out: 1e-4 relative."""
    from tests.test_gpu_ode_trainer import _setup
    from enf_pde_amd.fitting.inner_loop import decode, inner_loop
    _, _, _, _, coords, traj, conf, tr, state, t = _setup(cuda)
    rng = np.random.default_rng(9)
    B, T_in, T_all, N = 2, 3, 5, 64
    lat = {"p_pos": t(R.init_positions_grid(2, 9, 2) + 0.05 * rng.standard_normal((2, 9, 2))),
           "a": t(1 + 0.2 * rng.standard_normal((2, 9, 8))), "gaussian_window": t(np.full((2, 9, 1), 2.0 / 3))}
    pm = torch.tensor(np.stack([rng.permutation(N)[:32] for _ in range(T_in)]), device=cuda)
    trj = t(traj)

    def reference(lat, w_btn, frames, point_masks=None):
        with torch.no_grad():
            sol = tr.rollout(state.params["ode_params"], lat, frames)
            p_fl, a_fl, w_fl = (None if v is None else v.reshape(B * frames, *v.shape[2:]) for v in sol)
            rec = decode(tr.nef, state.params["nef"], tr.coords, p_fl, a_fl, w_fl).reshape(B, frames, N, 1).double()
        tgt, wn = trj[:, :frames].reshape(B, frames, N, 1).double(), normalize_point_weights(w_btn.double())
        if point_masks is not None:
            idx = point_masks[None].expand(B, -1, -1)
            rec, tgt, wn = torch.gather(rec, 2, idx[..., None]), torch.gather(tgt, 2, idx[..., None]), torch.gather(wn, 2, idx)
        d = torch.where(wn[..., None] > 0, rec - tgt, torch.zeros_like(rec))
        return wn[..., None] * d * d

    for w in (t(_weights(rng, B, N)), t(np.stack([_weights(rng, B, N) for _ in range(T_in)], 1))):
        w_btn = w if w.dim() == 3 else w[:, None].expand(B, T_in, N)
        ref = float(reference(lat, w_btn, T_in, pm).mean())
        got = float(tr.rollout_loss(state.params["nef"], state.params["ode_params"], lat, trj[:, :T_in], pm, weights=w))
        print("rollout_loss", got, ref)
        assert abs(got - ref) < 1e-5 * ref
    # validation: NaN holes in the trajectory, weights = valid_weights
    holes = traj.copy()
    holes[rng.uniform(size=holes.shape) < 0.15] = np.nan
    trj = t(holes)
    w = valid_weights(trj.reshape(B, T_all, N, 1))
    mk = torch.tensor(np.stack([rng.permutation(N)[:32] for _ in range(3)], 1), device=cuda)
    mse_in, mse_out = tr.val_step(state, trj, masks=mk, weights=w)
    _, fit = inner_loop(tr.nef, state.params["nef"], tr._latents0(state), state.params["meta_sgd_lrs"], tr.coords,
                        trj[:, 0].reshape(B, N, 1), mk, weights=normalize_point_weights(w[:, 0]))
    e = reference({k: v.detach() for k, v in fit.items()}, w, T_all)
    ref_in, ref_out = float(e[:, :T_in].mean()), float(e[:, T_in:].mean())
    print("val_step", float(mse_in), ref_in, float(mse_out), ref_out)
    assert np.isfinite(ref_in) and np.isfinite(ref_out)
    assert abs(float(mse_in) - ref_in) < 1e-4 * ref_in and abs(float(mse_out) - ref_out) < 1e-4 * ref_out
