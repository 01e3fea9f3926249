"""Deterministic mode on the GPU: with ``deterministic=True`` the decoder path's results are the same BITS run after run
(partial sums through scratch and fixed-order reductions, include/enf_hip.h "Deterministic mode"), still match the fp64 oracle
and the default (atomic) path within the tolerances of the existing backward tests.  Shapes are chosen so that the sums have
several terms: few latents, so the backward pair kernel splits the query tiles (nsplit = 8 at B = 1, Z = 5, N = 200)."""
import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from tests.helpers import make_cfg, make_inputs, build_nef
from tests.ffn_ref import ffn_net_np, ffn_net_torch, init_params_ffn, build_nef_ffn
from tests.test_gpu_backward import TOL, rel
from tests.test_gpu_weight_grads import TOL as TOL_W

pytestmark = pytest.mark.gpu

TOL_DX = {"f32": 5e-4, "bf16": 7e-2}       # tests/test_gpu_layers.py: test_gradient_wrt_query_coordinates
TOL_FIT = {"f32": 1e-5, "bf16": 2e-2}      # tests/test_gpu_backward.py: the fit step against its other forms (gradients: x 10)

#        name           invariant           D   H  C  O  B  Z  N    backward variant  embedding
CASES = {"split":      ("rel_pos_periodic", 128, 2, 16, 1, 1, 5, 200, "latent_split", "rff"),
         "zfold":      ("rel_pos_periodic", 128, 2, 16, 1, 1, 5, 200, "z_fold", "rff"),
         "ball":       ("ball", 32, 3, 8, 2, 3, 9, 50, "auto", "rff"),          # ext slots, 64-wide padded kernels, 3 -> 4 heads
         "ffn":        ("rel_pos_periodic", 64, 2, 8, 1, 1, 5, 200, "auto", "ffn")}
_REF = {}


def _t(cuda):
    return lambda v, g=False: torch.tensor(v, dtype=torch.float32, device=cuda, requires_grad=g)


def _case(name, monkeypatch):
    """cfg, parameters, inputs and the fp64 oracle's results (d/d latents of sum(out * w); loss and B * d loss / d latents of the
    fit step), computed once per case and shared by both precisions.  (The ffn case's oracle runs with its embedding replaced
    by ffn_net, as under tests/ffn_ref.py's ffn_oracle fixture.)"""
    if name in _REF:
        return _REF[name]
    inv, D, H, C, O, B, Z, N, _, emb = CASES[name]
    if emb == "ffn":
        monkeypatch.setattr(R, "rff_net", ffn_net_np)
        monkeypatch.setattr(T, "rff_net", ffn_net_torch)
    cfg = make_cfg(inv, D=D, H=H, C=C, O=O, freq=(0.3, 0.6))
    prm = (init_params_ffn if emb == "ffn" else R.init_params)(11, cfg, jitter=0.1)
    x, p, a, s = make_inputs(cfg, B, N, Z, 12)
    rng = np.random.default_rng(13)
    w, y = rng.standard_normal((B, N, O)), rng.standard_normal((B, N, O))
    tp = T.to_torch(prm, torch.float64)

    def grads(fn):
        lp, la, ls = (torch.tensor(v, requires_grad=True) for v in (p, a, s))
        val = fn(T.nef_apply(tp, cfg, torch.tensor(x), lp, la, ls))
        val.backward()
        return float(val.detach()), [np.zeros(v.shape) if v.grad is None else v.grad.numpy() for v in (lp, la, ls)]
    _, g_w = grads(lambda out: (out * torch.tensor(w)).sum())
    loss, g_fit = grads(lambda out: ((out - torch.tensor(y)) ** 2).mean())
    _REF[name] = (cfg, prm, (x, p, a, s, w, y), g_w, loss, [B * g for g in g_fit])
    return _REF[name]


def _nef(name, precision, deterministic):
    inv, D, H, C, O, B, Z, N, bwd, emb = CASES[name]
    cfg = _REF[name][0]
    nef = (build_nef_ffn if emb == "ffn" else build_nef)(cfg, precision)
    nef.deterministic = deterministic
    if bwd != "auto":
        nef.pair_variants = ("auto", bwd)
    return nef


def _churn(cuda, it):
    """Unrelated allocations between runs: other addresses, other contents of freed memory."""
    junk = [torch.randn(int(n), device=cuda) * 10 for n in np.random.default_rng(it).integers(1 << 10, 1 << 20, 6)]
    del junk


def _move_workspace(nef, cuda):
    """Replace every cached workspace of the model by a larger buffer at another offset: the next call runs on it."""
    for key, ws in list(nef._ws_cache.items()):
        big = torch.full((ws.numel() + 8192 + 256 * 3,), 0x5a, device=cuda, dtype=torch.uint8)
        nef._ws_cache[key] = big[256 * 3:]


def _grads_run(nef, params, t, x, p, a, s, w):
    lp, la, ls = t(p, True), t(a, True), t(s, True)
    out = nef.apply(params, t(x), lp, la, ls)
    (out * t(w)).sum().backward()
    return [out.detach(), lp.grad, la.grad, ls.grad]


def _check_against(got, ref, tol, what):
    scale = np.linalg.norm(ref[1])
    for k, g, r in zip(("p", "a", "sigma"), got, ref):
        g = g.double().cpu().numpy()
        e = rel(g, r) if np.linalg.norm(r) > 1e-9 * scale else np.linalg.norm(g) / scale
        print(f"{what} d{k}: relative error {e:.3e} (tolerance {tol:.1e})")
        assert np.isfinite(e) and e < tol, (what, k, e)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_latent_gradients_and_fit_step_are_bitwise_reproducible(cuda, name, precision, monkeypatch):
    cfg, prm, (x, p, a, s, w, y), g_w, loss_ref, g_fit = _case(name, monkeypatch)
    B = CASES[name][5]
    t = _t(cuda)
    nef = _nef(name, precision, True)
    assert nef.is_deterministic()
    params = nef.load_params(prm, device=cuda)
    # 1. five runs of forward + backward to the latents and of the one-call fit step, other allocations in between, one run on
    #    a workspace of another size at another offset: equal bits
    first_g = first_f = None
    for it in range(5):
        _churn(cuda, it)
        if it == 3:
            _move_workspace(nef, cuda)
        g = _grads_run(nef, params, t, x, p, a, s, w)
        f = list(nef.mse_value_and_latent_grads(params, t(x), t(p), t(a), t(s), t(y), grad_scale=float(B)))
        torch.cuda.synchronize()
        if first_g is None:
            first_g, first_f = g, f
            continue
        for k, u, v in zip(("out", "dp", "da", "dsigma"), first_g, g):
            assert torch.equal(u, v), (name, precision, "apply/backward", k, it, float((u - v).abs().max()))
        for k, u, v in zip(("loss", "dp", "da", "dsigma"), first_f, f):
            assert torch.equal(u, v), (name, precision, "fit step", k, it, float((u - v).abs().max()))
    # 2. against the fp64 oracle, tolerances of tests/test_gpu_backward.py
    _check_against(first_g[1:], g_w, TOL[precision], "backward vs oracle")
    _check_against(first_f[1:], g_fit, TOL[precision], "fit step vs oracle")
    e = abs(float(first_f[0]) - loss_ref) / abs(loss_ref)
    print(f"fit step loss: relative error {e:.3e}")
    assert e < TOL[precision]
    # 3. against the default path (float atomics), the same tolerances
    dflt = _nef(name, precision, False)
    assert not dflt.is_deterministic()
    dparams = dflt.load_params(prm, device=cuda)
    g0 = _grads_run(dflt, dparams, t, x, p, a, s, w)
    f0 = dflt.mse_value_and_latent_grads(dparams, t(x), t(p), t(a), t(s), t(y), grad_scale=float(B))
    assert torch.equal(g0[0], first_g[0])            # (the forward is the same kernels in both modes)
    _check_against(first_g[1:], [v.double().cpu().numpy() for v in g0[1:]], TOL[precision], "backward vs default path")
    _check_against(first_f[1:], [v.double().cpu().numpy() for v in f0[1:]], 10 * TOL_FIT[precision], "fit step vs default path")
    assert abs(float(first_f[0]) - float(f0[0])) < TOL_FIT[precision] * abs(float(f0[0]))


def test_three_call_fit_step_is_bitwise_reproducible(cuda, monkeypatch):
    """The same inner step as enf_forward_stages + enf_mse_value_grad_ex + enf_backward_latents_ex with the flag (the loss
    kernel of enf_loss.hip: one partial per block, N * O > 256 so that several blocks add up)."""
    from enf_pde_amd.enf import models as M
    name = "split"
    cfg, prm, (x, p, a, s, w, y), g_w, loss_ref, g_fit = _case(name, monkeypatch)
    t = _t(cuda)
    nef = _nef(name, "f32", True)
    params = nef.load_params(prm, device=cuda)
    x8, y8 = np.tile(x, (1, 8, 1)), np.tile(y, (1, 8, 1))          # 1600 outputs: seven blocks of the loss kernel
    monkeypatch.setattr(M, "FUSED_FIT_STEP", False)
    runs = []
    for it in range(3):
        _churn(cuda, it)
        runs.append(nef.mse_value_and_latent_grads(params, t(x8), t(p), t(a), t(s), t(y8), grad_scale=1.0))
    monkeypatch.setattr(M, "FUSED_FIT_STEP", True)
    fused = nef.mse_value_and_latent_grads(params, t(x8), t(p), t(a), t(s), t(y8), grad_scale=1.0)
    for r in runs[1:]:
        assert all(torch.equal(u, v) for u, v in zip(runs[0], r))
    assert abs(float(runs[0][0]) - float(fused[0])) < TOL_FIT["f32"] * float(fused[0])
    for u, v in zip(runs[0][1:], fused[1:]):
        assert rel(u.cpu().numpy(), v.cpu().numpy()) < 10 * TOL_FIT["f32"]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("inv", ["rel_pos", "ponita"])
def test_query_gradient_is_bitwise_reproducible(cuda, inv, precision, monkeypatch):
    """d out / d x through enf_backward_all with the flag: each latent's share goes to scratch and is summed over z in order.
    Equal bits over repeats, the oracle's autograd within the tolerance of the existing query-gradient test, and the destination
    is OVERWRITTEN: one repeat hands the call a buffer full of junk."""
    B, Z, N = 2, 12, 40
    cfg = make_cfg(inv, D=64, H=2, C=8, O=2, freq=(0.5, 1.0))
    prm = R.init_params(3, cfg, jitter=0.1)
    x, p, a, s = make_inputs(cfg, B, N, Z, 4)
    w = np.random.default_rng(2).standard_normal((B, N, 2))
    rx = torch.tensor(x, requires_grad=True)
    ref = T.nef_apply(T.to_torch(prm, torch.float64), cfg, rx, torch.tensor(p), torch.tensor(a), torch.tensor(s))
    (ref * torch.tensor(w)).sum().backward()
    nef = build_nef(cfg, precision)
    nef.deterministic = True
    P = nef.load_params(prm, device=cuda)
    t = _t(cuda)
    real_empty, junked = torch.empty, []

    def junk_empty(*args, **kw):                 # the (B, N, dx) float32 buffer the backward allocates for d x, pre-filled
        out = real_empty(*args, **kw)
        if out.dtype == torch.float32 and tuple(out.shape) == (B, N, x.shape[-1]) and out.is_cuda:
            out.fill_(1e30)
            junked.append(1)
        return out
    first = None
    for it in range(4):
        _churn(cuda, it)
        dx, dp = t(x, True), t(p, True)
        out = nef.apply(P, dx, dp, t(a), t(s))
        if it == 2:
            monkeypatch.setattr(torch, "empty", junk_empty)
        (out * t(w)).sum().backward()
        if it == 2:
            monkeypatch.setattr(torch, "empty", real_empty)
            assert junked, "the deterministic backward is expected to hand the library an uninitialised d x buffer"
        res = [dx.grad.clone(), dp.grad.clone()]
        if first is None:
            first = res
        else:
            assert torch.equal(first[0], res[0]) and torch.equal(first[1], res[1]), (inv, precision, it)
    e = rel(first[0].cpu().double().numpy(), rx.grad.numpy())
    print(f"d x vs oracle: {e:.3e}")
    assert e < TOL_DX[precision]


def test_backward_all_is_bitwise_reproducible(cuda):
    """enf_backward_all with the flag: all 46 weight gradients and the latent gradients, equal bits over three repeats, once
    more with the relu masks replayed (mask_mode = ENF_MASK_READ), and within the weight-gradient tolerance of the default path."""
    import contextlib
    from enf_pde_amd.fitting.trainers.pde_trainer import _tree_from_tensors
    B, Z, N = 2, 8, 100
    cfg = make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=1, freq=(0.5, 1.0))
    prm = R.init_params(5, cfg, jitter=0.1)
    x, p, a, s = make_inputs(cfg, B, N, Z, 6)
    t = _t(cuda)
    w = t(np.random.default_rng(7).standard_normal((B, N, 1)))

    def run(nef, P, masks=None):
        ws = [v.detach().clone().requires_grad_(True) for v in nef.param_tensors(P)]
        lp, la, ls = t(p, True), t(a, True), t(s, True)
        with (nef.relu_masks(masks, "read", B) if masks is not None else contextlib.nullcontext()):
            out = nef.apply(_tree_from_tensors(ws), t(x), lp, la, ls)
            g = torch.autograd.grad((out * w).sum(), ws + [lp, la, ls], allow_unused=True)
        return [out.detach()] + [gi for gi in g if gi is not None]
    nef = build_nef(cfg, "bf16")
    nef.deterministic = True
    P = nef.load_params(prm, device=cuda)
    runs = []
    for it in range(3):
        _churn(cuda, it)
        runs.append(run(nef, P))
    assert len(runs[0]) == 1 + 44 + 3            # 46 tensors less the two frozen coefficient matrices, and p, a, sigma
    for r in runs[1:]:
        assert all(torch.equal(u, v) for u, v in zip(runs[0], r))
    buf = nef.relu_mask_buffer(B, N, Z, cuda)
    buf.zero_()
    with torch.no_grad(), nef.relu_masks(buf, "write", B):
        nef.apply(P, t(x), t(p), t(a), t(s))
    m0, m1 = run(nef, P, buf), run(nef, P, buf)
    assert all(torch.equal(u, v) for u, v in zip(m0, m1))
    dflt = build_nef(cfg, "bf16")
    dflt.deterministic = False
    d0 = run(dflt, dflt.load_params(prm, device=cuda))
    gmax = max(float(v.norm()) for v in d0[1:45])
    for i, (u, v) in enumerate(zip(runs[0][1:], d0[1:])):
        nv = float(v.norm())
        e = float((u - v).norm()) / (nv if nv > 1e-6 * gmax else gmax)
        assert e < TOL_W["bf16"], (i, e)


def test_layers_path_is_bitwise_reproducible(cuda):
    """num_layers = 1: the self-attention block's pair backward (enf_pair_backward_ex2 / enf_backward_weights_ex with the flag,
    the query-side gradient included: its queries are the poses) -- apply() and its backward, equal bits over repeats."""
    from tests.test_gpu_layers import _nef as layered
    cfg = dict(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=1, freq=(0.5, 1.0)), num_layers=1)
    nef = layered(cfg, "f32")
    nef.deterministic = True
    prm = R.init_params(2, cfg, jitter=0.1)
    P = nef.load_params(prm, device=cuda)
    x, p, a, s = make_inputs(cfg, 2, 60, 6, 3)
    t = _t(cuda)
    w = t(np.random.default_rng(4).standard_normal((2, 60, 1)))
    for weights in (False, True):
        runs = []
        for it in range(3):
            _churn(cuda, it)
            ws = [v.detach().clone().requires_grad_(weights) for v in nef.param_tensors(P)]
            from enf_pde_amd.enf.models import tensor_paths, _set
            tree = {}
            for path, v in zip(tensor_paths(1), ws):
                _set(tree, path, v)
            lp, la, ls = t(p, True), t(a, True), t(s, True)
            out = nef.apply({"params": tree}, t(x), lp, la, ls)
            g = torch.autograd.grad((out * w).sum(), [lp, la, ls] + (ws if weights else []), allow_unused=True)
            runs.append([out.detach()] + [gi for gi in g if gi is not None])
        for r in runs[1:]:
            assert len(r) == len(runs[0]) and all(torch.equal(u, v) for u, v in zip(runs[0], r)), weights
