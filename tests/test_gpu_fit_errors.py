"""Per-signal and per-point errors on the GPU (include/enf_hip.h, "Per-signal and per-point errors": enf_fit_step_e, enf_eval_loss,
enf_signal_sum):

    err[b,n] = sum_o w[b,n,o] (out - target)^2        loss_b[b] = err[b].sum() / (N O)

Shapes are the smallest at which the indexing can go wrong (a wave = 16 consecutive queries of the flattened (B N) axis, a workgroup
= 128): (3, 50, 2) waves straddle two signals and the last wave is partly empty; (2, 130, 1) crosses a workgroup; (4, 5, 3) puts four
signals inside one wave; (2, 33, 2) at num_hidden 64 with 3 heads (run as 4) and the ponita invariant.  Z = 9; x is per signal
(x_bstride = N dx) except where said.

The oracle is oracle.enf_ref_np.nef_apply in fp64, err_ref formed in numpy.  The bound is derived from the project's forward
tolerance tau = 2e-5 (f32) / 3e-2 (bf16) of max|out_ref| (tests/test_gpu_forward.py: TOL): an output within
eps = tau max|out_ref| of the reference moves a squared residual by at most 2 |out_ref - t| eps + eps^2, so
    |err - err_ref| <= sum_o w (2 |out_ref - t| eps + eps^2)
per point, and the same summed over n and scaled by 1 / (N O) for loss_b.

Equality with the existing calls: enf_fit_step_e runs the SAME kernel instantiations as enf_fit_step_w / _cw (the store hangs on a
run-time pointer), so with ENF_FIT_DETERMINISTIC its loss, dp, da, dsigma are asserted bit-equal to theirs."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from tests.helpers import make_cfg, make_inputs, build_nef
from tests.test_gpu_forward import TOL as TAU
from enf_pde_amd import _lib
from enf_pde_amd.fitting.inner_loop import gather_signal_points, inner_loop, make_signal_masks
from enf_pde_amd.fitting.weights import valid_weights

pytestmark = pytest.mark.gpu

Z, GUARD = 9, 16
#        D   H  invariant            (B, N, O)
CASES = [(128, 2, "rel_pos_periodic", (3, 50, 2)),
         (128, 2, "rel_pos_periodic", (2, 130, 1)),
         (128, 2, "rel_pos_periodic", (4, 5, 3)),
         (64, 3, "ponita", (2, 33, 2))]
FORMS = ("none", "point", "channel")
_REF = {}


def _f32(v):
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def _case(D, H, inv, shape, seed=61):
    """inputs (rounded to fp32, so that the oracle sees the kernels' numbers) and the fp64 output, once per session.  Weights: about
    30 % exact zeros, the last signal all zero; per point w (B, N), per value cw (B, N, O)."""
    key = (D, H, inv, shape, seed)
    if key not in _REF:
        B, N, O = shape
        cfg = make_cfg(inv, D=D, H=H, C=12, O=O, freq=(0.3, 0.6))
        prm = R.init_params(seed, cfg, jitter=0.1)
        x, p, a, s = (_f32(v) for v in make_inputs(cfg, B, N, Z, seed + 1))
        rng = np.random.default_rng(seed + 2)
        y = _f32(rng.standard_normal((B, N, O)))
        w, cw = _f32(rng.uniform(0, 2, (B, N))), _f32(rng.uniform(0, 2, (B, N, O)))
        w[rng.uniform(size=(B, N)) < 0.3] = 0.0
        cw[rng.uniform(size=(B, N, O)) < 0.3] = 0.0
        w[B - 1], cw[B - 1] = 0.0, 0.0
        cw[0, 1] = 0.0                                       # a point all of whose values are missing
        out = R.nef_apply(prm, cfg, x, p, a, s)
        _REF[key] = NS(cfg=cfg, prm=prm, x=x, p=p, a=a, s=s, y=y, w=w, cw=cw, out=out, shape=shape)
    return _REF[key]


def _weights(c, form):
    """the (B, N, O) weights of a form, fp64"""
    B, N, O = c.shape
    return {"none": np.ones((B, N, O)), "point": np.repeat(c.w[..., None], O, -1), "channel": c.cw}[form]


def _reference(c, form, precision):
    """err_ref, its bound, loss_b_ref, its bound"""
    B, N, O = c.shape
    w3 = _weights(c, form)
    d = c.out - c.y
    eps = TAU[precision] * np.abs(c.out).max()
    err = (w3 * d * d).sum(-1)
    bound = (w3 * (2 * np.abs(d) * eps + eps * eps)).sum(-1)
    return err, bound, err.sum(1) / (N * O), bound.sum(1) / (N * O)


def _targets(c, form, cuda):
    """the targets with NaN / Inf wherever the form's weight is zero"""
    y = c.y.copy()
    gone = _weights(c, form) == 0
    y[gone] = np.array([np.nan, np.inf, -np.inf])[np.arange(int(gone.sum())) % 3]
    return torch.tensor(y, dtype=torch.float32, device=cuda)


def _t(cuda):
    return lambda v: torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda)


def _run(cuda, nef, params, c, form, kind, flags=0, target=None, shared_x=False, want=("loss", "err", "loss_b"), poison=255):
    """One raw C-ABI call on a workspace filled with `poison`: kind "fit" = enf_fit_step_e, "eval" = enf_eval_loss, "w" =
    enf_fit_step_w / _cw (the existing calls).  err and loss_b sit in NaN-filled buffers with GUARD floats behind them.  The latent
    count is the case's own (c.p): tests/test_gpu_wide_out.py runs its Z = 7 cases through here."""
    lib = _lib.load()
    t = _t(cuda)
    B, N, O = c.shape
    x, p, a, s = t(c.x[0] if shared_x else c.x), t(c.p), t(c.a), t(c.s)
    y = _targets(c, form, cuda) if target is None else target
    w = t(c.w) if form == "point" else None
    cw = t(c.cw) if form == "channel" else None
    desc = nef._desc(B, N, c.p.shape[1])
    nbytes = int(lib.enf_workspace_bytes_ex(ctypes.byref(desc), flags))
    ws = torch.full((nbytes,), poison, device=cuda, dtype=torch.uint8)
    packed = nef.pack(params)
    ptr = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    xstride = 0 if shared_x else N * x.shape[-1]
    loss = torch.zeros(1, device=cuda)
    ebuf = torch.full((B * N + GUARD,), float("nan"), device=cuda)
    lbuf = torch.full((B + GUARD,), float("nan"), device=cuda)
    dp, da, ds = torch.full_like(p, float("nan")), torch.full_like(a, float("nan")), torch.full_like(s, float("nan"))
    head = (ctypes.byref(desc), ptr(x), xstride, ptr(p), ptr(a), ptr(s), ptr(packed), ptr(y))
    if kind == "fit":
        _lib.launch(cuda, lib.enf_fit_step_e, *head, float(B), ptr(loss), ptr(dp), ptr(da), ptr(ds), ptr(ws), nbytes, ptr(w), ptr(cw),
                    ptr(ebuf), ptr(lbuf) if "loss_b" in want else None, flags, st)
    elif kind == "eval":
        _lib.launch(cuda, lib.enf_eval_loss, *head, ptr(w), ptr(cw), ptr(loss) if "loss" in want else None,
                    ptr(ebuf) if "err" in want else None, ptr(lbuf) if "loss_b" in want else None, ptr(ws), nbytes, flags, st)
    elif form == "channel":
        _lib.launch(cuda, lib.enf_fit_step_cw, *head, float(B), ptr(loss), ptr(dp), ptr(da), ptr(ds), ptr(ws), nbytes, ptr(cw), flags, st)
    else:
        _lib.launch(cuda, lib.enf_fit_step_w, *head, float(B), ptr(loss), ptr(dp), ptr(da), ptr(ds), ptr(ws), nbytes, ptr(w), flags, st)
    torch.cuda.synchronize()
    return NS(loss=loss, dp=dp, da=da, ds=ds, err=ebuf[:B * N].view(B, N), loss_b=lbuf[:B], err_guard=ebuf[B * N:], loss_b_guard=lbuf[B:])


def _check_against_oracle(c, form, precision, r, what, fit):
    B, N, O = c.shape
    err_ref, ebound, lb_ref, lbound = _reference(c, form, precision)
    err, lb = r.err.double().cpu().numpy(), r.loss_b.double().cpu().numpy()
    # poisoning: fully overwritten, nothing behind
    assert np.isfinite(err).all() and np.isfinite(lb).all(), what
    assert bool(torch.isnan(r.err_guard).all()) and bool(torch.isnan(r.loss_b_guard).all()), what
    worst = float(((np.abs(err - err_ref) - ebound) / np.maximum(ebound, 1e-300)).max()) if ebound.max() > 0 else 0.0
    print(what, "max |err - ref| / bound", float((np.abs(err - err_ref) / np.maximum(ebound, 1e-300))[ebound > 0].max()),
          "loss_b", lb, "ref", lb_ref, "bound", lbound, "loss", float(r.loss))
    assert (np.abs(err - err_ref) <= ebound).all(), (what, worst)
    assert (np.abs(lb - lb_ref) <= lbound).all(), (what, lb, lb_ref, lbound)
    # the zero-weight rule: exact zeros where all of a point's weights are zero; an all-zero signal
    dead = (_weights(c, form) == 0).all(-1)
    assert (err[dead] == 0).all(), what
    if form != "none":
        assert dead[B - 1].all() and float(r.loss_b[B - 1]) == 0.0, what
        if fit:
            for g in (r.dp, r.da, r.ds):
                assert bool((g[B - 1] == 0).all()), what
    # consistency: fp32 sums of at most a few hundred non-negative terms
    assert np.allclose(lb, err.sum(1) / (N * O), rtol=1e-6, atol=0), (what, lb, err.sum(1) / (N * O))
    assert abs(lb.mean() - float(r.loss)) <= 1e-5 * float(r.loss), (what, lb.mean(), float(r.loss))
    if fit:
        assert all(bool(torch.isfinite(g).all()) for g in (r.dp, r.da, r.ds)), what


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("D,H,inv,shape", CASES)
def test_errors_match_oracle(cuda, D, H, inv, shape, precision):
    """all three weight forms, enf_fit_step_e and enf_eval_loss, NaN / Inf targets under every zero weight, poisoned outputs"""
    c = _case(D, H, inv, shape)
    nef = build_nef(c.cfg, precision)
    params = nef.load_params(c.prm, device=cuda)
    for form in FORMS:
        fit = _run(cuda, nef, params, c, form, "fit")
        _check_against_oracle(c, form, precision, fit, (shape, precision, form, "fit"), True)
        ev = _run(cuda, nef, params, c, form, "eval")
        _check_against_oracle(c, form, precision, ev, (shape, precision, form, "eval"), False)
        # the evaluation is the fit step's forward: the same ybar, the same tail chain, the same epilogue
        assert torch.equal(ev.err, fit.err) and torch.equal(ev.loss_b, fit.loss_b), (shape, precision, form)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("D,H,inv,shape", CASES)
def test_fit_step_e_equals_the_existing_calls(cuda, D, H, inv, shape, precision):
    """ENF_FIT_DETERMINISTIC: loss, dp, da, dsigma of enf_fit_step_e against enf_fit_step_w / _cw, bit for bit (same instantiation)"""
    c = _case(D, H, inv, shape)
    nef = build_nef(c.cfg, precision)
    params = nef.load_params(c.prm, device=cuda)
    for form in FORMS:
        new = _run(cuda, nef, params, c, form, "fit", flags=_lib.ENF_FIT_DETERMINISTIC)
        old = _run(cuda, nef, params, c, form, "w", flags=_lib.ENF_FIT_DETERMINISTIC)
        for name in ("loss", "dp", "da", "ds"):
            u, v = getattr(new, name), getattr(old, name)
            assert bool(torch.isfinite(v).all()) and torch.equal(u, v), (shape, precision, form, name, float((u - v).abs().max()))
        # err and loss_b do not depend on the mode
        assert torch.equal(new.err, _run(cuda, nef, params, c, form, "fit").err), (shape, precision, form)


@pytest.mark.parametrize("variant", ["z_fold", "z_fold_zsplit"])
def test_forced_zfold_forward_and_shared_x(cuda, variant):
    """the z-fold forward variants forced, and x shared by the signals (x_bstride = 0)"""
    c = _case(*CASES[0])
    for precision in ("f32", "bf16"):
        nef = build_nef(c.cfg, precision)
        nef.pair_variants = (variant, "auto")
        params = nef.load_params(c.prm, device=cuda)
        for kind in ("fit", "eval"):
            r = _run(cuda, nef, params, c, "channel", kind)
            _check_against_oracle(c, "channel", precision, r, (variant, precision, kind), kind == "fit")
    shared = NS(**vars(c))
    shared.x = np.repeat(c.x[:1], c.shape[0], 0)
    shared.out = R.nef_apply(c.prm, c.cfg, shared.x, c.p, c.a, c.s)
    nef = build_nef(c.cfg, "f32")
    params = nef.load_params(c.prm, device=cuda)
    for kind in ("fit", "eval"):
        r = _run(cuda, nef, params, shared, "point", kind, shared_x=True)
        _check_against_oracle(shared, "point", "f32", r, ("shared x", kind), kind == "fit")


def test_eval_loss_output_subsets(cuda):
    """every output of enf_eval_loss is optional: loss_b without err (through the workspace), err alone, loss alone -- same bits"""
    c = _case(*CASES[0])
    nef = build_nef(c.cfg, "f32")
    params = nef.load_params(c.prm, device=cuda)
    full = _run(cuda, nef, params, c, "point", "eval", flags=_lib.ENF_FIT_DETERMINISTIC)
    only_b = _run(cuda, nef, params, c, "point", "eval", want=("loss_b",))
    assert torch.equal(only_b.loss_b, full.loss_b) and bool(torch.isnan(only_b.err).all()) and float(only_b.loss) == 0.0
    only_e = _run(cuda, nef, params, c, "point", "eval", want=("err",))
    assert torch.equal(only_e.err, full.err) and bool(torch.isnan(only_e.loss_b).all()) and float(only_e.loss) == 0.0
    only_l = _run(cuda, nef, params, c, "point", "eval", flags=_lib.ENF_FIT_DETERMINISTIC, want=("loss",))
    assert torch.equal(only_l.loss, full.loss) and bool(torch.isnan(only_l.err).all()) and bool(torch.isnan(only_l.loss_b).all())
    nofit = _run(cuda, nef, params, c, "point", "fit", want=("err",))                 # enf_fit_step_e without loss_b
    assert torch.equal(nofit.err, full.err) and bool(torch.isnan(nofit.loss_b).all())


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_errors_are_reproducible_in_the_default_mode(cuda, precision):
    """err and loss_b are the same bits run after run in the DEFAULT mode too, with other kernels and other contents of freed memory
    in between (tests/test_gpu_backward.py::test_backward_is_reproducible)"""
    c = _case(*CASES[0])
    nef = build_nef(c.cfg, precision)
    params = nef.load_params(c.prm, device=cuda)
    for kind in ("fit", "eval"):
        first = _run(cuda, nef, params, c, "channel", kind)
        for it in range(3):
            junk = [torch.randn(int(n), device=cuda) * 10 for n in np.random.default_rng(it).integers(1 << 10, 1 << 21, 8)]
            del junk
            again = _run(cuda, nef, params, c, "channel", kind)
            assert torch.equal(again.err, first.err) and torch.equal(again.loss_b, first.loss_b), (precision, kind, it)


def test_signal_sum_sizes(cuda):
    """enf_signal_sum for N below the block size, no multiple of anything, and above it; neighbours untouched"""
    lib = _lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    g = torch.Generator().manual_seed(4)
    for B, N in ((1, 1), (3, 7), (2, 255), (2, 256), (3, 1031)):
        err = torch.rand((B, N), generator=g).to(cuda)
        out = torch.full((B + GUARD,), float("nan"), device=cuda)
        runs = []
        for _ in range(2):
            _lib.launch(cuda, lib.enf_signal_sum, err.data_ptr(), B, N, 0.25, out.data_ptr(), st)
            torch.cuda.synchronize()
            runs.append(out.clone())
        ref = err.double().sum(1) * 0.25
        assert torch.allclose(out[:B].double(), ref, rtol=1e-6, atol=0), (B, N)
        assert bool(torch.isnan(out[B:]).all()) and torch.equal(runs[0][:B], runs[1][:B])


# ---- the Python mirror
def _fit_problem(cuda, per_signal, form):
    C, B, side, Ns, Zl, S = 8, 3, 8, 40, 4, 2
    cfg = make_cfg("rel_pos_periodic", D=64, H=2, C=C, O=2)
    prm = R.init_params(7, cfg, jitter=0.1)
    rng = np.random.default_rng(8)
    lin = np.linspace(-1, 1, side)
    coords = np.stack(np.meshgrid(lin, lin), -1).reshape(-1, 2)
    Ng = side * side
    img = rng.standard_normal((B, Ng, 2))
    img[1, rng.permutation(Ng)[30:]] = np.nan               # signal 1 observes 30 points: per-signal rows are padded with -1
    img[0, rng.uniform(size=Ng) < 0.3] = np.nan
    t = _t(cuda)
    w = valid_weights(t(img))
    lat0 = {"p_pos": t(R.init_positions_grid(1, Zl, 2) + 0.02 * rng.standard_normal((1, Zl, 2))),
            "a": t(1 + 0.1 * rng.standard_normal((1, Zl, C))), "gaussian_window": t(np.full((1, Zl, 1), 2.0 / 3))}
    lrs = {"p_pos": t([0.5]), "a": t(np.full((C,), 2.0)), "gaussian_window": t([0.0])}
    if per_signal:
        masks = make_signal_masks(w.cpu(), Ns, S, generator=torch.Generator().manual_seed(3), device=cuda)
        assert bool((masks[1] == -1).any())
    else:
        masks = torch.tensor(np.stack([rng.permutation(Ng)[:Ns] for _ in range(S + 1)], 1), device=cuda)
    kw = {"none": {}, "point": {"weights": w}, "channel": {"channel_weights": w[..., None].expand(-1, -1, 2).contiguous()}}[form]
    if form == "none" and not per_signal:
        img = np.nan_to_num(img)
    nef = build_nef(cfg, "f32")
    nef.deterministic = True
    return nef, nef.load_params(prm, device=cuda), lat0, lrs, t(coords), t(img), masks, kw, S


@pytest.mark.parametrize("per_signal,form,normalize", [(False, "none", False), (False, "point", False), (True, "none", True),
                                                       (True, "point", False), (True, "channel", True), (False, "channel", False)])
def test_inner_loop_per_signal_loss(cuda, per_signal, form, normalize):
    """deterministic mode: the fitted latents are the bits of per_signal_loss=False (the steps run the same instantiations); the final
    loss comes from another kernel sequence (enf_eval_loss, not enf_forward + enf_mse_value_grad*): the same fp32 sum in another
    order, 1e-5 relative.  loss_b[S] is eval_loss on the fitted latents, bit for bit, and err is 0 at the -1 pads."""
    nef, params, lat0, lrs, coords, img, masks, kw, S = _fit_problem(cuda, per_signal, form)
    B = img.shape[0]
    if normalize:
        kw = dict(kw, normalize_weights=True)
    loss0, lat_ref = inner_loop(nef, params, lat0, lrs, coords, img, masks, **kw)
    seen = []
    real = nef.eval_loss
    nef.eval_loss = lambda *a, **k: (seen.append((a, k, real(*a, **k))), seen[-1][2])[1]
    loss, lat, loss_b = inner_loop(nef, params, lat0, lrs, coords, img, masks, per_signal_loss=True, **kw)
    nef.eval_loss = real
    torch.cuda.synchronize()
    assert loss_b.shape == (S + 1, B) and bool(torch.isfinite(loss_b).all())
    for k in lat_ref:
        assert torch.equal(lat[k], lat_ref[k]), k
    print("inner loop", per_signal, form, float(loss), float(loss0), loss_b.tolist())
    assert abs(float(loss) - float(loss0)) <= 1e-5 * float(loss0)
    assert abs(float(loss_b[S].double().mean()) - float(loss)) <= 1e-5 * float(loss)
    assert len(seen) == 1
    (a, k, (lb, err)) = seen[0]
    again_b, again_err = nef.eval_loss(*a, **{kk: v for kk, v in k.items() if kk != "loss_out"})
    assert torch.equal(again_b, loss_b[S]) and torch.equal(lb, loss_b[S]) and torch.equal(again_err, err)
    if per_signal:
        pads = masks[:, :, S] < 0
        assert bool(pads.any()) and bool((err[pads] == 0).all()) and bool(torch.isfinite(err).all())
        xs, ys, ws = gather_signal_points(coords, torch.nan_to_num(img), masks, kw.get("weights"))
        assert torch.equal(a[1], xs[S])                                    # evaluated on the last mask's own points


def test_fit_latents_step_per_signal_loss(cuda):
    from tests.test_gpu_autodec_fit import _problem, _trainer, _state, SIDE, O
    pb = _problem("rel_pos_periodic")
    results = []
    for per_signal_loss in (False, True):
        tr, nef_params = _trainer(cuda, pb, "f32")
        tr.nef.deterministic = True
        state = _state(cuda, tr, nef_params, pb)
        batch = (torch.tensor(pb.img, device=cuda).reshape(3, SIDE, SIDE, O), torch.tensor([4, 0, 2], device=cuda))
        results.append(tr.fit_latents_step(state, batch, per_signal_loss=per_signal_loss) + (state.rng.get_state(),))
    (loss0, new0, rng0), (loss1, new1, loss_b, rng1) = results
    assert torch.equal(loss0, loss1) and torch.equal(rng0, rng1) and new0.step == new1.step
    for k, v in new0.params["autodecoder"]["params"].items():
        assert torch.equal(v, new1.params["autodecoder"]["params"][k]), k
    for m0, m1 in zip(new0.autodecoder_opt_state["mu"], new1.autodecoder_opt_state["mu"]):
        assert torch.equal(m0, m1)
    assert loss_b.shape == (3,) and abs(float(loss_b.double().mean()) - float(loss1)) <= 1e-5 * float(loss1)


def _maml16(cuda):
    from enf_pde_amd.fitting.trainers import MetaSGDPDETrainer
    from enf_pde_amd.enf.latents.autodecoder_meta import PositionOrientationFeatureAutodecoderMeta
    cfg = make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2)
    prm = R.init_params(0, cfg, jitter=0.1)
    lin = np.linspace(-1, 1, 16)
    coords = np.stack(np.meshgrid(lin, lin), -1).reshape(-1, 2)
    conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=1e-3),
              meta=NS(learning_rate_meta_sgd=1e-2, num_inner_steps=2, inner_learning_rate_p=0.5, inner_learning_rate_a=2.0,
                      inner_learning_rate_window=0.0, noise_pos_inner_loop=0.0),
              nef=NS(optimize_gaussian_window=False), training=NS(max_num_sampled_points=64))
    nef = build_nef(cfg, "f32")
    nef.deterministic = True
    nef.pair_variants = ("latent_split", "auto")            # (the split z-fold orders its partial sums by the call's shape)
    ad = PositionOrientationFeatureAutodecoderMeta(1, 9, 8, 2, 0, gaussian_window_size=-1)
    tr = MetaSGDPDETrainer(conf, nef, ad, _t(cuda)(coords), seed=0, second_order="fd")
    return tr, nef.load_params(prm, device=cuda)


@pytest.mark.parametrize("form", ["none", "point", "channel"])
def test_fit_errors_in_chunks(cuda, form):
    """a 16 x 16 grid in two chunks equals one chunk, bit for bit; with missing values err is 0 exactly there"""
    rng = np.random.default_rng(31)
    B, N, O = 3, 256, 2
    field = rng.standard_normal((B, 16, 16, O)).astype(np.float32)
    if form != "none":
        flat = field.reshape(B, N, O)
        flat[rng.uniform(size=(B, N)) < 0.25] = np.nan
    batch = torch.tensor(field, device=cuda)
    w = valid_weights(batch.reshape(B, N, O))
    kw = {"none": {}, "point": {"weights": w}, "channel": {"channel_weights": w[..., None].expand(-1, -1, O).contiguous()}}[form]
    runs = []
    for chunk in (None, 128):
        tr, params = _maml16(cuda)
        state = tr.init_train_state(params)
        state.rng.manual_seed(5)
        calls = []
        real = tr.nef.eval_loss
        tr.nef.eval_loss = lambda *a, **k: (calls.append(a[1].shape[1]), real(*a, **k))[1]
        tr.nef.apply = None                                  # nothing is decoded
        runs.append(tr.fit_errors(state, batch, chunk=chunk, **kw))
        assert calls == [64] + {None: [256], 128: [128, 128]}[chunk]         # (the inner loop's own final loss on its 64 samples first)
    torch.cuda.synchronize()
    loss_b, err = runs[0]
    assert loss_b.shape == (B,) and err.shape == (B, N) and bool(torch.isfinite(err).all()) and bool((err >= 0).all())
    for other_b, other_err in runs[1:]:
        assert torch.equal(other_err, err) and torch.equal(other_b, loss_b)
    assert torch.allclose(loss_b.double(), err.double().sum(1) / (N * O), rtol=1e-6, atol=0)
    if form != "none":
        assert bool((w == 0).any()) and bool((err[w == 0] == 0).all()) and bool((err[w > 0] > 0).all())
    print("fit_errors", form, loss_b.tolist())
