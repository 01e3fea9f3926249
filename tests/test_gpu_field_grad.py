"""Derivative fields on the GPU (include/enf_hip.h, "Derivative fields"): EquivariantCrossAttentionNeF.jacobian / query_vjp and
fitting.decode_jacobian against fp64 autograd of the oracle, one backward per output channel.

Error measure: the relative Frobenius norm over the whole Jacobian (``rel`` of tests/test_gpu_backward.py).  Bounds: the project's
query-gradient contract (tests/test_gpu_layers.py, test_gradient_wrt_query_coordinates): 5e-4 in f32, 7e-2 in bf16.  ``out`` against
nef.apply under no_grad: the forward's tolerances on max|err| / max|ref| (tests/test_gpu_forward.py): 2e-5 in f32, 3e-2 in bf16."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from tests.helpers import make_cfg, make_inputs, build_nef
from tests.ffn_ref import ffn_net_np, ffn_net_torch, init_params_ffn, build_nef_ffn
from tests.test_gpu_backward import rel

pytestmark = pytest.mark.gpu

TOL = {"f32": 5e-4, "bf16": 7e-2}
TOL_OUT = {"f32": 2e-5, "bf16": 3e-2}
INVARIANTS = ["rel_pos_periodic", "latitude_periodic", "polar_periodic", "ponita", "abs_pos", "rel_pos", "norm_rel_pos", "ball", "ball_lat"]
_REF = {}


def _t(cuda):
    return lambda v: torch.tensor(v, dtype=torch.float32, device=cuda)


def _oracle(cfg, prm, x, p, a, s):
    """(out (B, N, O), jac (B, N, O, dx)) in fp64: one backward per output channel (out[b, n] depends on x[b, n] only)."""
    rx = torch.tensor(x, requires_grad=True)
    out = T.nef_apply(T.to_torch(prm, torch.float64), cfg, rx, torch.tensor(p), torch.tensor(a), torch.tensor(s))
    rows = [torch.autograd.grad(out[..., o].sum(), rx, retain_graph=True)[0] for o in range(out.shape[-1])]
    return out.detach().numpy(), torch.stack(rows, 2).numpy()


def _case(key, inv, D, H, C, O, B, N, Z, seed=3, ffn=False):
    """cfg, parameters, inputs and the oracle's decode and Jacobian: computed once per case, shared by the tests and precisions."""
    if key not in _REF:
        cfg = make_cfg(inv, D=D, H=H, C=C, O=O, freq=(0.5, 1.0))
        prm = (init_params_ffn if ffn else R.init_params)(seed, cfg, jitter=0.1)
        xpas = make_inputs(cfg, B, N, Z, seed + 1)
        _REF[key] = (cfg, prm, xpas) + _oracle(cfg, prm, *xpas)
    return _REF[key]


def _small(inv):
    """the shape of test_gradient_wrt_query_coordinates: N = 50 leaves a partial 16-query tile, 150 queries span two tail workgroups"""
    return _case(("small", inv), inv, 64, 2, 8, 2, 3, 50, 7)


def _jac_np(jac):
    return jac.double().cpu().numpy()


def _check_jac(jac, ref, tol, what):
    e = rel(_jac_np(jac), ref)
    print(f"{what}: relative Jacobian error {e:.3e} (bound {tol:.1e})")
    assert torch.isfinite(jac).all() and e < tol, (what, e)
    return e


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("inv", INVARIANTS)
def test_jacobian_matches_oracle_for_every_invariant(cuda, inv, precision):
    cfg, prm, (x, p, a, s), out_ref, jac_ref = _small(inv)
    nef = build_nef(cfg, precision)
    P = nef.load_params(prm, device=cuda)
    t = _t(cuda)
    out, jac = nef.jacobian(P, t(x), t(p), t(a), t(s))
    assert out.shape == out_ref.shape and jac.shape == jac_ref.shape
    assert jac.permute(2, 0, 1, 3).is_contiguous()                       # a view of the call's (O, B, N, dx) buffer
    _check_jac(jac, jac_ref, TOL[precision], f"{inv} {precision}")
    with torch.no_grad():
        plain = nef.apply(P, t(x), t(p), t(a), t(s))
    eo = float((out - plain).abs().max() / plain.abs().max())
    print(f"{inv} {precision}: out vs nef.apply {eo:.3e}")
    assert eo < TOL_OUT[precision]
    assert np.abs(out.double().cpu().numpy() - out_ref).max() / np.abs(out_ref).max() < TOL_OUT[precision]


@pytest.mark.parametrize("name,inv,D,H,O,B,N,Z", [("wide", "rel_pos_periodic", 128, 2, 3, 2, 130, 20),      # crosses a 128-query tile, three seeds
                                                   ("narrow", "rel_pos_periodic", 32, 3, 2, 2, 50, 7)])      # zero-padded to 64 wide, 3 -> 4 heads
def test_jacobian_other_widths(cuda, name, inv, D, H, O, B, N, Z):
    cfg, prm, (x, p, a, s), out_ref, jac_ref = _case(name, inv, D, H, 8, O, B, N, Z)
    nef = build_nef(cfg, "f32")
    t = _t(cuda)
    out, jac = nef.jacobian(nef.load_params(prm, device=cuda), t(x), t(p), t(a), t(s))
    _check_jac(jac, jac_ref, TOL["f32"], name)
    assert np.abs(out.double().cpu().numpy() - out_ref).max() / np.abs(out_ref).max() < TOL_OUT["f32"]


def test_jacobian_ffn_embedding(cuda, monkeypatch):
    monkeypatch.setattr(R, "rff_net", ffn_net_np)
    monkeypatch.setattr(T, "rff_net", ffn_net_torch)
    cfg, prm, (x, p, a, s), out_ref, jac_ref = _case("ffn", "rel_pos_periodic", 64, 2, 8, 2, 2, 50, 7, ffn=True)
    nef = build_nef_ffn(cfg, "f32")
    t = _t(cuda)
    out, jac = nef.jacobian(nef.load_params(prm, device=cuda), t(x), t(p), t(a), t(s))
    _check_jac(jac, jac_ref, TOL["f32"], "ffn")
    assert np.abs(out.double().cpu().numpy() - out_ref).max() / np.abs(out_ref).max() < TOL_OUT["f32"]


@pytest.mark.parametrize("variants", [("auto", "latent_split"), ("auto", "z_fold"), ("z_fold", "z_fold"), ("z_fold_zsplit", "latent_split")])
def test_jacobian_under_forced_pair_variants(cuda, variants):
    """The call picks no variant of its own: the descriptor's forward / backward choice runs (both backward kernels, the z-fold forwards)."""
    from enf_pde_amd import _lib
    cfg, prm, (x, p, a, s), out_ref, jac_ref = _small("rel_pos_periodic")
    nef = build_nef(cfg, "f32")
    nef.pair_variants = variants
    desc = nef._desc(*x.shape[:2], p.shape[1])
    lib = _lib.load()
    assert lib.enf_pair_variant(ctypes.byref(desc), 1) == _lib.VARIANT[variants[1]]
    if variants[0] != "auto":
        assert lib.enf_pair_variant(ctypes.byref(desc), 0) == _lib.VARIANT[variants[0]]
    t = _t(cuda)
    out, jac = nef.jacobian(nef.load_params(prm, device=cuda), t(x), t(p), t(a), t(s))
    _check_jac(jac, jac_ref, TOL["f32"], str(variants))
    assert np.abs(out.double().cpu().numpy() - out_ref).max() / np.abs(out_ref).max() < TOL_OUT["f32"]


def test_broadcast_grid_stays_per_signal(cuda):
    """x_bstride = 0: the Jacobian is per signal; its sum over the signals is the oracle's gradient w.r.t. the shared grid."""
    cfg, prm, (x, p, a, s), _, _ = _small("rel_pos")
    B = x.shape[0]
    xs = np.broadcast_to(x[:1], x.shape).copy()
    _, per_signal = _oracle(cfg, prm, xs, p, a, s)
    g1 = torch.tensor(x[0], requires_grad=True)
    ref = T.nef_apply(T.to_torch(prm, torch.float64), cfg, g1[None].expand(B, -1, -1), torch.tensor(p), torch.tensor(a), torch.tensor(s))
    shared = torch.stack([torch.autograd.grad(ref[..., o].sum(), g1, retain_graph=True)[0] for o in range(ref.shape[-1])], 1).numpy()   # (N, O, dx)
    nef = build_nef(cfg, "f32")
    t = _t(cuda)
    grid = t(x[0])[None].expand(B, -1, -1)
    assert grid.stride(0) == 0
    out, jac = nef.jacobian(nef.load_params(prm, device=cuda), grid, t(p), t(a), t(s))
    assert jac.shape == per_signal.shape
    _check_jac(jac, per_signal, TOL["f32"], "broadcast grid, per signal")
    e = rel(_jac_np(jac).sum(0), shared)
    print(f"broadcast grid, summed over signals: {e:.3e}")
    assert e < TOL["f32"]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_query_vjp_matches_oracle_and_the_contracted_jacobian(cuda, precision):
    cfg, prm, (x, p, a, s), _, jac_ref = _small("ponita")
    w = np.random.default_rng(2).standard_normal(jac_ref.shape[:3])
    want = np.einsum("bnoi,bno->bni", jac_ref, w)                        # the oracle's VJP: its Jacobian is exact per (b, n)
    rx = torch.tensor(x, requires_grad=True)
    ref = T.nef_apply(T.to_torch(prm, torch.float64), cfg, rx, torch.tensor(p), torch.tensor(a), torch.tensor(s))
    (ref * torch.tensor(w)).sum().backward()
    assert rel(want, rx.grad.numpy()) < 1e-12
    nef = build_nef(cfg, precision)
    P = nef.load_params(prm, device=cuda)
    t = _t(cuda)
    dx = nef.query_vjp(P, t(x), t(p), t(a), t(s), t(w))
    e = rel(dx.double().cpu().numpy(), rx.grad.numpy())
    print(f"query_vjp {precision} vs oracle: {e:.3e}")
    assert dx.shape == x.shape and e < TOL[precision]
    _, jac = nef.jacobian(P, t(x), t(p), t(a), t(s), return_out=False)
    contracted = torch.einsum("bnoi,bno->bni", jac.double(), t(w).double()).cpu().numpy()
    ec = rel(contracted, dx.double().cpu().numpy())
    print(f"query_vjp {precision} vs contracted Jacobian: {ec:.3e}")
    assert ec < TOL[precision]
    assert rel(contracted, rx.grad.numpy()) < TOL[precision]


def _poison_workspace(nef, cuda, byte, pad):
    """Replace every cached workspace of the model by a fresh, larger buffer full of `byte` at another offset."""
    for key, ws in list(nef._ws_cache.items()):
        big = torch.full((ws.numel() + 8192 + 256 * pad,), byte, device=cuda, dtype=torch.uint8)
        nef._ws_cache[key] = big[256 * pad:]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("bwd", ["latent_split", "z_fold"])
def test_deterministic_mode_is_bitwise_reproducible(cuda, bwd, precision):
    """ENF_BWD_DETERMINISTIC: two calls on fresh, differently poisoned workspaces (0x5a bytes; 0xff bytes = NaN) give equal bits, the
    result meets the oracle bound, and leaving out `out` changes no bit of the Jacobian."""
    cfg, prm, (x, p, a, s), out_ref, jac_ref = _small("rel_pos_periodic")
    nef = build_nef(cfg, precision)
    nef.deterministic = True
    nef.pair_variants = ("auto", bwd)
    P = nef.load_params(prm, device=cuda)
    t = _t(cuda)
    nef.jacobian(P, t(x), t(p), t(a), t(s))                              # (creates the cached workspace)
    runs = []
    for byte, pad in ((0x5a, 3), (0xff, 7)):
        _poison_workspace(nef, cuda, byte, pad)
        runs.append(nef.jacobian(P, t(x), t(p), t(a), t(s)))
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][0], runs[1][0])
    _check_jac(runs[0][1], jac_ref, TOL[precision], f"deterministic {bwd} {precision}")
    none, jac = nef.jacobian(P, t(x), t(p), t(a), t(s), return_out=False)
    assert none is None and torch.equal(jac, runs[0][1])
    dx0 = nef.query_vjp(P, t(x), t(p), t(a), t(s), torch.ones_like(runs[0][0]))
    _poison_workspace(nef, cuda, 0xff, 5)
    assert torch.equal(dx0, nef.query_vjp(P, t(x), t(p), t(a), t(s), torch.ones_like(runs[0][0])))


@pytest.mark.parametrize("deterministic", [False, True])
def test_overwrite_out_null_and_guard_bands(cuda, deterministic):
    """The C-ABI call on caller-owned buffers: `jac` pre-filled with NaN comes back finite (it is OVERWRITTEN, in both modes), the guard
    bands around `jac` and `out` stay untouched, and with out == NULL the Jacobian is the same to the bound."""
    from enf_pde_amd import _lib
    from enf_pde_amd.enf.models import _ptr
    cfg, prm, (x, p, a, s), out_ref, jac_ref = _small("polar_periodic")
    nef = build_nef(cfg, "f32")
    P = nef.load_params(prm, device=cuda)
    t = _t(cuda)
    lib = _lib.load()
    B, N, dx = x.shape
    Z, O, G = p.shape[1], out_ref.shape[-1], 64
    desc = nef._desc(B, N, Z)
    flags = _lib.ENF_BWD_DETERMINISTIC if deterministic else 0
    nbytes = int(lib.enf_field_grad_workspace_bytes(ctypes.byref(desc), flags))
    assert nbytes > 0
    packed = nef.pack(P)
    xs, ps, as_, ss = t(x), t(p), t(a), t(s)
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    results = []
    for with_out in (True, False):
        ws = torch.full((nbytes,), 0xff, device=cuda, dtype=torch.uint8)
        jbuf = torch.full((G + O * B * N * dx + G,), float("nan"), device=cuda)
        obuf = torch.full((G + B * N * O + G,), -7.0, device=cuda)
        jbuf[:G] = 11.0
        jbuf[-G:] = 13.0
        jac, out = jbuf[G:-G], obuf[G:-G]
        _lib.launch(cuda, lib.enf_field_grad, ctypes.byref(desc), _ptr(xs), N * dx, _ptr(ps), _ptr(as_), _ptr(ss), _ptr(packed),
                    _ptr(out) if with_out else None, _ptr(jac), _ptr(ws), nbytes, flags, st)
        torch.cuda.synchronize()
        assert bool((jbuf[:G] == 11.0).all()) and bool((jbuf[-G:] == 13.0).all())
        assert bool((obuf[:G] == -7.0).all()) and bool((obuf[-G:] == -7.0).all())
        if not with_out:
            assert bool((obuf == -7.0).all())                             # out == NULL: nothing outside jac and the workspace
        else:
            assert np.abs(out.reshape(B, N, O).double().cpu().numpy() - out_ref).max() / np.abs(out_ref).max() < TOL_OUT["f32"]
        j = jac.reshape(O, B, N, dx).permute(1, 2, 0, 3)
        _check_jac(j, jac_ref, TOL["f32"], f"raw call, det={deterministic}, out={with_out}")
        results.append(j.clone())
    if deterministic:
        assert torch.equal(results[0], results[1])


def test_curl_and_chunked_decode_jacobian(cuda):
    """A 2-channel field on 2 Cartesian coordinates (rel_pos): vorticity from decode_jacobian, chunked (16 + 16 + 16 + 2 points) and
    unchunked, on a grid shared by the batch.  Both meet the f32 bound; they need not agree bit for bit (the atomics' order differs)."""
    from enf_pde_amd.fitting import decode_jacobian, curl_2d, divergence, gradient_norm
    cfg, prm, (x, p, a, s), _, _ = _small("rel_pos")
    xs = np.broadcast_to(x[:1], x.shape).copy()
    out_ref, jac_ref = _oracle(cfg, prm, xs, p, a, s)
    curl_ref = jac_ref[..., 1, 0] - jac_ref[..., 0, 1]                   # dv/dx - du/dy
    nef = build_nef(cfg, "f32")
    P = nef.load_params(prm, device=cuda)
    t = _t(cuda)
    for chunk in (None, 16):
        out, jac = decode_jacobian(nef, P, t(x[0]), t(p), t(a), t(s), chunk=chunk)
        assert out.shape == out_ref.shape and jac.shape == jac_ref.shape
        _check_jac(jac, jac_ref, TOL["f32"], f"decode_jacobian chunk={chunk}")
        assert np.abs(out.double().cpu().numpy() - out_ref).max() / np.abs(out_ref).max() < TOL_OUT["f32"]
        ec = rel(curl_2d(jac).double().cpu().numpy(), curl_ref)
        print(f"curl_2d chunk={chunk}: {ec:.3e}")
        assert ec < TOL["f32"]
        assert rel(divergence(jac).double().cpu().numpy(), jac_ref[..., 0, 0] + jac_ref[..., 1, 1]) < TOL["f32"]
        assert rel(gradient_norm(jac).double().cpu().numpy(), np.sqrt((jac_ref ** 2).sum(-1))) < TOL["f32"]
