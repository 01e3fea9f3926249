"""Shared pieces of the wide-output tests (tests/test_gpu_wide_out.py, tests/test_wide_out_host.py): num_out 4 .. 32.

In the tail kernels a wave holds the outputs of 16 queries in two accumulator tiles; output channel o sits at o = 16 t + 4 quad + i
(tile t, quad = lane >> 4, element i).  With num_out <= 3 only elements i < 3 of tile 0 in lanes 0..15 ever carry a number, so the
widths here are: 4 fills quad 0; 5 the first value in quad 1; 16 tile 0 full; 17 the first value in tile 1; 32 everything live, nothing
masked by o < O.  Shapes: B = 3 signals of N = 50 points (150 rows: nine full 16-query tiles and a ragged tenth, signals start in
mid-tile), Z = 7 latents, latent_dim 8, embedding frequencies (0.5, 1.0), weights jittered by 0.1.

The metric.  A quantity with a channel axis is compared channel by channel,

    max_n |got[..., o] - ref[..., o]| <= tol * max |ref|        for every o,

so that a dead, misplaced or half-reduced lane cannot hide behind the other channels; `tol` is the constant the quantity's own test
file uses.  Gradients with respect to latents have no channel axis: the relative L2 error of tests/test_gpu_backward.py.  The
per-point error err[b, n] = sum_o w (out - target)^2 is held to the bound of tests/test_gpu_fit_errors.py: an output within
eps = tau max|out_ref| of the reference moves it by at most sum_o w (2 |out_ref - target| eps + eps^2).

Every reference is the fp64 oracle, computed once per process and never modified."""
from types import SimpleNamespace as NS

import numpy as np

from oracle import enf_ref_np as R
from tests.helpers import make_cfg, make_inputs
from tests.test_gpu_backward import ref_grads, rel  # noqa: F401

B, N, Z, C, FREQ = 3, 50, 7, 8, (0.5, 1.0)
WIDTHS = (4, 5, 16, 17, 32)
_CASES, _GRADS, _FITS, _JACS = {}, {}, {}, {}


def f32(v):
    """rounded to fp32 and back: the oracle sees the numbers the kernels get"""
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def problem(O, D=64, H=2, inv="rel_pos_periodic", seed=91):
    """NS(cfg, prm, x, p, a, s, out): one decode problem of width O at the shapes above and the oracle's output (B, N, O)"""
    key = (O, D, H, inv, seed)
    if key not in _CASES:
        cfg = make_cfg(inv, D=D, H=H, C=C, O=O, freq=FREQ)
        prm = R.init_params(seed, cfg, jitter=0.1)
        x, p, a, s = (f32(v) for v in make_inputs(cfg, B, N, Z, seed + 1))
        _CASES[key] = NS(cfg=cfg, prm=prm, x=x, p=p, a=a, s=s, O=O, out=R.nef_apply(prm, cfg, x, p, a, s), key=key)
    return _CASES[key]


def cotangent(O, kind="dense", seed=93):
    """d out (B, N, O): "dense" N(0, 1); "only16" the same values on channel 16 and exact zeros elsewhere (the first element of the
    second accumulator tile); ("drop", k) dense with the channels >= k zeroed"""
    w = f32(np.random.default_rng(seed).standard_normal((B, N, O)))
    if kind == "only16":
        keep = np.zeros(O, dtype=bool)
        keep[16] = True
        w = w * keep
    elif kind != "dense":
        w = w * (np.arange(O) < kind[1])
    return w


def latent_grads(c, kind="dense"):
    """(dp, da, dsigma) of sum(out * cotangent) by fp64 autograd of the oracle (tests/test_gpu_backward.ref_grads)"""
    key = (c.key, kind)
    if key not in _GRADS:
        _GRADS[key] = ref_grads(c.prm, c.cfg, c.x, c.p, c.a, c.s, cotangent(c.O, kind))[1:]
    return _GRADS[key]


def loss_problem(c, form, seed=95):
    """NS(y, w3, w, cw): targets N(0, 1) (residuals are O(1)) and the weights of a loss form -- "none"; "point": w (B, N); "channel":
    cw (B, N, O) -- with about a third exact zeros.  w3 is the form's weight per value, (B, N, O).  Per-channel zeros also fall on the
    channels >= 4 of points whose other channels are live (forced at two points besides the random ones), and one point has none."""
    rng = np.random.default_rng(seed)
    O = c.O
    y = f32(rng.standard_normal((B, N, O)))
    w, cw = f32(rng.uniform(0.2, 2.0, (B, N))), f32(rng.uniform(0.2, 2.0, (B, N, O)))
    w[rng.uniform(size=(B, N)) < 0.33] = 0.0
    cw[rng.uniform(size=(B, N, O)) < 0.33] = 0.0
    w[1, 0], cw[0, 1] = 0.0, 0.0
    cw[0, 2, :4], cw[0, 2, 4:] = 1.0, 0.0
    cw[1, 17] = 0.75
    cw[1, 17, O - 1] = 0.0
    w3 = {"none": np.ones((B, N, O)), "point": np.repeat(w[..., None], O, -1), "channel": cw}[form]
    return NS(y=y, w3=w3, w=w if form == "point" else None, cw=cw if form == "channel" else None, form=form)


def poisoned(lp):
    """the targets with NaN under every zero weight"""
    y = lp.y.copy()
    y[lp.w3 == 0] = np.nan
    return y


def fit_reference(c, form, grad_scale):
    """NS(lp, loss_b, loss, g, err): the weighted mean squared error of a fit step by tests/gn_ref.oracle_loss_grad in fp64, its
    gradients times grad_scale, and err[b, n] = sum_o w (out - target)^2 from the oracle's output"""
    from tests.gn_ref import oracle_loss_grad
    key = (c.key, form, grad_scale)
    if key not in _FITS:
        lp = loss_problem(c, form)
        weight = None if form == "none" else (lp.w if form == "point" else lp.cw)
        loss_b, g = oracle_loss_grad(c.cfg, c.prm, c.x, c.p, c.a, c.s, lp.y, weight, grad_scale)
        _FITS[key] = NS(lp=lp, loss_b=loss_b, loss=float(loss_b.mean()), g=g, err=point_errors(c.out, lp.y, lp.w3))
    return _FITS[key]


def jacobian_x(c):
    """d out[b, n, o] / d x[b, n, :] of the oracle, (B, N, O, dx): tests/tangent_x_ref.oracle_jacobian_x, one backward per channel"""
    from tests.tangent_x_ref import oracle_jacobian_x
    if c.key not in _JACS:
        _JACS[c.key] = oracle_jacobian_x(c.cfg, c.prm, c.x, c.p, c.a, c.s)
    return _JACS[c.key]


# ---- the metric
def channel_errors(got, ref, axis=-1):
    """max_n |got[..., o] - ref[..., o]| / max |ref| for every channel o of `axis`: (O,) in fp64"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = np.moveaxis(np.abs(got - ref), axis, -1)
    return d.reshape(-1, d.shape[-1]).max(0) / np.abs(ref).max()


def check_channels(got, ref, tol, what, axis=-1):
    """the per-channel metric: prints the worst channel, asserts every channel (and that nothing is NaN / Inf)"""
    e = channel_errors(got, ref, axis)
    print(f"{what}: worst channel {int(np.argmax(e))} of {e.size} at {e.max():.3e} of max|ref| (bound {tol:.1e}); "
          f"channels >= 16: {e[16:].max() if e.size > 16 else 0.0:.3e}")
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), what
    bad = np.nonzero(~(e <= tol))[0]
    assert bad.size == 0, (what, "channels", bad.tolist(), e[bad].tolist())
    return e


def check_grads(got, ref, tol, what, names=("dp", "da", "dsigma")):
    """relative L2 error of each latent gradient (tests/test_gpu_backward.py)"""
    es = [float(rel(np.asarray(g, dtype=np.float64).reshape(r.shape), r)) for g, r in zip(got, ref)]
    print(f"{what}: " + ", ".join(f"{n} {e:.3e}" for n, e in zip(names, es)) + f" (bound {tol:.1e})")
    for n, e in zip(names, es):
        assert np.isfinite(e) and e <= tol, (what, n, e)
    return es


def point_errors(out, y, w3):
    """err[b, n] = sum_o w (out - target)^2 with w == 0 a select (the target under it may be anything)"""
    d = np.where(w3 > 0, out - np.where(w3 > 0, y, 0.0), 0.0)
    return (w3 * d * d).sum(-1)


def error_bounds(out_ref, y, w3, tau):
    """(bound on |err - err_ref| (B, N), bound on |loss_b - loss_b_ref| (B,)) for outputs within tau max|out_ref| of the reference:
    the construction of tests/test_gpu_fit_errors.py, carried through the square"""
    eps = tau * np.abs(out_ref).max()
    d = np.where(w3 > 0, np.abs(out_ref - np.where(w3 > 0, y, 0.0)), 0.0)
    bound = (w3 * (2 * d * eps + eps * eps)).sum(-1)
    return bound, bound.sum(1) / (out_ref.shape[1] * out_ref.shape[2])


def check_point_errors(err, loss_b, out_ref, y, w3, tau, what):
    """err (B, N) and loss_b (B,) against the reference formed from out_ref, within error_bounds; exact zeros where every weight of a
    point is zero"""
    err, loss_b = np.asarray(err, dtype=np.float64), np.asarray(loss_b, dtype=np.float64)
    ref = point_errors(out_ref, y, w3)
    ref_b = ref.sum(1) / (out_ref.shape[1] * out_ref.shape[2])
    ebound, lbound = error_bounds(out_ref, y, w3, tau)
    assert np.isfinite(err).all() and np.isfinite(loss_b).all(), what
    d_err, d_lb = np.abs(err - ref), np.abs(loss_b - ref_b)
    print(f"{what}: max |err - ref| / bound {float((d_err / np.maximum(ebound, 1e-300))[ebound > 0].max()):.3e}, "
          f"|loss_b - ref| / bound {float((d_lb / np.maximum(lbound, 1e-300)).max()):.3e}")
    assert (d_err <= ebound).all(), (what, float((d_err - ebound).max()))
    assert (d_lb <= lbound).all(), (what, loss_b, ref_b, lbound)
    dead = (w3 == 0).all(-1)
    assert (err[dead] == 0).all(), what
