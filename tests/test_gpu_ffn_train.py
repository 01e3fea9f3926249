"""GPU parity of the 'ffn' embedding's training path against the patched fp64 oracle (tests/ffn_ref.py): every weight gradient
of enf_backward_all, the unused R?_W1 slots, d out / d x, and the outer (meta) step with finite-difference second order against
exact double-backward through the oracle's inner loop."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from tests.helpers import make_cfg, make_inputs
from tests.ffn_ref import ffn_oracle, init_params_ffn, build_nef_ffn  # noqa: F401  (fixture)
from enf_pde_amd.enf.models import FFN_TENSOR_PATHS

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("ffn_oracle")]


def _get(tree, path):
    for k in path:
        tree = tree[k]
    return tree


def _t(cuda):
    return lambda v, g=False: torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda, requires_grad=g)


def _rel(a, b, scale):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 1e-6 * scale else scale)


@pytest.mark.parametrize("precision,tol", [("f32", 5e-4), ("bf16", 2e-1)])
@pytest.mark.parametrize("invariant,D,H", [("rel_pos_periodic", 128, 2), ("ponita", 64, 2), ("latitude_periodic", 128, 1),
                                           ("rel_pos", 32, 3)])
def test_ffn_weight_gradients(cuda, invariant, D, H, precision, tol):
    """Every tensor of the ffn tree through enf_backward_all (first order) against fp64 autograd; Dense_0 included."""
    cfg = make_cfg(invariant, D=D, H=H, C=16, O=2, freq=(0.5, 1.0))
    prm = init_params_ffn(3, cfg, jitter=0.1)
    x, p, a, s = make_inputs(cfg, 2, 60, 9, 4)
    w = np.random.default_rng(5).standard_normal((2, 60, 2))
    tp = T.to_torch(prm, torch.float64, requires_grad=True)
    (T.nef_apply(tp, cfg, torch.tensor(x), torch.tensor(p), torch.tensor(a), torch.tensor(s)) * torch.tensor(w)).sum().backward()
    ref = [None if path is None else _get(tp["params"], path).grad.numpy() for path in FFN_TENSOR_PATHS]
    nef = build_nef_ffn(cfg, precision)
    params = nef.load_params(prm, device=cuda)
    ts = nef.param_tensors(params)
    for v in ts:
        v.requires_grad_(True)
    t = _t(cuda)
    (nef.apply(params, t(x), t(p), t(a), t(s)) * t(w)).sum().backward()
    torch.cuda.synchronize()
    scale = max(np.linalg.norm(r) for r in ref if r is not None)
    bad = []
    for path, v, r in zip(FFN_TENSOR_PATHS, ts, ref):
        if path is None:
            assert v.numel() == 0 and (v.grad is None or v.grad.numel() == 0)
            continue
        e = _rel(v.grad.cpu().numpy().astype(np.float64), r, scale)
        if not (np.isfinite(e) and e < tol):
            bad.append(("/".join(path[-3:]), e))
    assert not bad, (precision, bad)


def test_ffn_backward_all_writes_zeros_to_unused_slots(cuda):
    """enf_backward_all through the C-ABI with a buffer in each unused ENF_W_R?_W1 slot: exact zeros come back, and the other
    tensors' gradients equal the ones of a call with NULL there."""
    from enf_pde_amd import _lib
    cfg = make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=1)
    prm = init_params_ffn(7, cfg, jitter=0.1)
    x, p, a, s = make_inputs(cfg, 2, 40, 6, 8)
    nef = build_nef_ffn(cfg, "f32")
    params = nef.load_params(prm, device=cuda)
    lib, t = _lib.load(), _t(cuda)
    B, N, Z = 2, 40, 6
    desc = nef._desc(B, N, Z)
    ts = [v.contiguous() for v in nef.param_tensors(params)]
    ptr = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None and v.numel() else ctypes.c_void_p(0)
    blob = torch.empty(int(lib.enf_packed_weight_bytes(ctypes.byref(desc))), device=cuda, dtype=torch.uint8)
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    arrT = (ctypes.c_void_p * 46)(*[ptr(v) for v in ts])
    _lib.check(lib.enf_pack_weights(ctypes.byref(desc), arrT, ptr(blob), st))
    xt, pt, at, st_ = t(x), t(p), t(a), t(s)
    out = torch.empty((B, N, 1), device=cuda)
    ybar, lse = torch.empty((B, N, 128), device=cuda), torch.empty((B, N, 2), device=cuda)
    ws = torch.empty(int(lib.enf_workspace_bytes(ctypes.byref(desc))), device=cuda, dtype=torch.uint8)
    _lib.check(lib.enf_forward_stages(ctypes.byref(desc), ptr(xt), N * 2, ptr(pt), ptr(at), ptr(st_), ptr(blob), ptr(out), ptr(ybar),
                                      ptr(lse), ptr(ws), ws.numel(), 15 | 16, st))
    dout = torch.randn(B, N, 1, device=cuda)
    nscr = int(lib.enf_backward_all_scratch_bytes(ctypes.byref(desc), B))
    scratch = torch.empty(nscr, device=cuda, dtype=torch.uint8)
    results = []
    for unused_buffers in (False, True):
        grads = [torch.full((64, 64), 7.0, device=cuda) if v.numel() == 0 and unused_buffers else
                 (None if v.numel() == 0 else torch.empty_like(v)) for v in ts]
        dp, da, dsig = torch.empty_like(pt), torch.empty_like(at), torch.empty_like(st_)
        _lib.check(lib.enf_backward_all(ctypes.byref(desc), ptr(xt), N * 2, ptr(pt), ptr(at), ptr(st_), arrT, ptr(blob), ptr(ybar),
                                        ptr(lse), ptr(dout), ptr(dp), ptr(da), ptr(dsig), (ctypes.c_void_p * 46)(*[ptr(g) for g in grads]),
                                        ctypes.c_void_p(0), ptr(ws), ws.numel(), ptr(scratch), nscr, 0, st))   # (0: recompute
                                                                                                             # prologue and tail)
        torch.cuda.synchronize()
        results.append(grads)
    for i in (5, 10):
        assert torch.equal(results[1][i], torch.zeros(64, 64, device=cuda))
    for i, (g0, g1) in enumerate(zip(*results)):
        if i not in (5, 10):
            assert torch.equal(g0, g1), i
    assert float(results[0][4].abs().max()) > 0 and float(results[0][9].abs().max()) > 0      # d Dense_0.kernel, both branches


@pytest.mark.parametrize("invariant", ["rel_pos", "ponita"])
def test_ffn_query_gradient(cuda, invariant):
    """d out / d x (the query coordinates) against fp64 autograd, f32 (5e-4)."""
    cfg = make_cfg(invariant, D=64, H=2, C=8, O=2, freq=(0.5, 1.0))
    prm = init_params_ffn(9, cfg, jitter=0.1)
    x, p, a, s = make_inputs(cfg, 2, 50, 7, 10)
    w = np.random.default_rng(11).standard_normal((2, 50, 2))
    tx = torch.tensor(x, requires_grad=True)
    (T.nef_apply(T.to_torch(prm, torch.float64), cfg, tx, torch.tensor(p), torch.tensor(a), torch.tensor(s)) * torch.tensor(w)).sum().backward()
    nef = build_nef_ffn(cfg, "f32")
    t = _t(cuda)
    gx = t(x, True)
    (nef.apply(nef.load_params(prm, device=cuda), gx, t(p), t(a), t(s)) * t(w)).sum().backward()
    torch.cuda.synchronize()
    r = tx.grad.numpy()
    assert np.linalg.norm(gx.grad.cpu().numpy() - r) / np.linalg.norm(r) < 5e-4


def _problem(seed=0, D=64, H=2, C=8, Z=16, side=8, B=8, S=2, Ns=64):
    cfg = make_cfg("rel_pos_periodic", D=D, H=H, C=C, O=1)
    prm = init_params_ffn(seed, cfg, jitter=0.1)
    rng = np.random.default_rng(seed + 1)
    lin = np.linspace(-1, 1, side)
    coords = np.stack(np.meshgrid(lin, lin), -1).reshape(-1, 2)
    img = rng.standard_normal((B, side * side, 1))
    lat0 = {"p_pos": R.init_positions_grid(1, Z, 2) + 0.02 * rng.standard_normal((1, Z, 2)),
            "a": 1 + 0.1 * rng.standard_normal((1, Z, C)), "gaussian_window": np.full((1, Z, 1), 2.0 / 3)}
    lrs = {"p_pos": np.array([0.5]), "a": np.full((C,), 2.0) * (1 + 0.1 * rng.standard_normal(C)), "gaussian_window": np.array([0.0])}
    masks = np.stack([rng.permutation(side * side)[:Ns] for _ in range(S + 1)], 1)
    return cfg, prm, coords, img, lat0, lrs, masks


def test_ffn_meta_gradient_fd_matches_exact_second_order(cuda):
    from enf_pde_amd.fitting.trainers import meta_gradients
    cfg, prm, coords, img, lat0, lrs, masks = _problem()
    tp = T.to_torch(prm, torch.float64, requires_grad=True)
    tl = {k: torch.tensor(v, requires_grad=True) for k, v in lat0.items()}
    tr = {k: torch.tensor(v, requires_grad=True) for k, v in lrs.items()}
    loss_r, _ = T.inner_loop(tp, cfg, tl, tr, torch.tensor(coords), torch.tensor(img), torch.tensor(masks), create_graph=True)
    paths = [q for q in FFN_TENSOR_PATHS if q is not None]
    leaves = [_get(tp["params"], q) for q in paths]
    g = torch.autograd.grad(loss_r, leaves + list(tl.values()) + list(tr.values()), allow_unused=True)
    gw_r = [np.zeros(tuple(v.shape)) if gi is None else gi.numpy() for gi, v in zip(g, leaves)]
    gl_r = {k: gi.numpy() for k, gi in zip(tl, g[len(leaves):len(leaves) + len(tl)])}
    gr_r = {k: gi.numpy() for k, gi in zip(tr, g[len(leaves) + len(tl):])}
    nef = build_nef_ffn(cfg, "f32")
    params = nef.load_params(prm, device=cuda)
    t = _t(cuda)
    loss, gm = meta_gradients(nef, params, {k: t(v) for k, v in lat0.items()}, {k: t(v) for k, v in lrs.items()}, t(coords),
                              t(img), torch.tensor(masks, device=cuda), second_order="fd")
    assert abs(float(loss) - float(loss_r)) < 1e-5 * max(1.0, abs(float(loss_r)))
    own = [v for q, v in zip(FFN_TENSOR_PATHS, gm["nef"]) if q is not None]
    gmax = max(np.linalg.norm(v) for v in gw_r)
    bad = []
    for q, a_, b in zip(paths, own, gw_r):
        nb = np.linalg.norm(b)
        e = np.linalg.norm(a_.cpu().numpy() - b) / (nb if nb > 1e-3 * gmax else gmax)
        if not e < 1e-3:
            bad.append(("/".join(q[-3:]), e))
    assert not bad, bad
    for k in ("a", "p_pos"):
        e = np.linalg.norm(gm["autodecoder"][k].cpu().numpy() - gl_r[k]) / max(np.linalg.norm(gl_r[k]), 1e-12)
        assert e < 5e-3, (k, e)
        e = np.linalg.norm(gm["meta_sgd_lrs"][k].cpu().numpy() - gr_r[k]) / max(np.linalg.norm(gr_r[k]), 1e-12)
        assert e < 2e-3, (k, e)


def test_ffn_trainer_step(cuda):
    """MetaSGDPDETrainer with an ffn model: the train state builds, an outer step moves the parameters and the unused slots
    stay empty, and the loss goes down over steps."""
    from enf_pde_amd.fitting.trainers import MetaSGDPDETrainer
    from enf_pde_amd.enf.latents.autodecoder_meta import PositionOrientationFeatureAutodecoderMeta
    cfg, prm, coords, img, lat0, lrs, masks = _problem(seed=3, Z=9, B=3, Ns=32)
    nef = build_nef_ffn(cfg, "f32")
    conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=1e-3), meta=NS(learning_rate_meta_sgd=1e-2,
              num_inner_steps=2, inner_learning_rate_p=0.5, inner_learning_rate_a=2.0, inner_learning_rate_window=0.0,
              noise_pos_inner_loop=0.0), nef=NS(optimize_gaussian_window=False), training=NS(max_num_sampled_points=32))
    t = _t(cuda)
    ad = PositionOrientationFeatureAutodecoderMeta(1, 9, 8, 2, 0, gaussian_window_size=-1)
    tr = MetaSGDPDETrainer(conf, nef, ad, t(coords), seed=0, second_order="fd")
    state = tr.init_train_state(nef.load_params(prm, device=cuda))
    w0 = [v.clone() for v in nef.param_tensors(state.params["nef"])]
    batch = t(img).reshape(3, 8, 8, 1)
    mk = torch.tensor(masks, device=cuda)
    losses, st = [], state
    for _ in range(6):
        loss, st = tr.nef_train_step(st, batch, masks=mk)
        losses.append(float(loss))
    w1 = nef.param_tensors(st.params["nef"])
    assert w1[5].numel() == 0 and w1[10].numel() == 0
    assert not torch.equal(w1[4], w0[4]) and not torch.equal(w1[9], w0[9])           # Dense_0 trains
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
