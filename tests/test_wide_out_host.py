"""num_out 1 .. 32 without a GPU: the descriptor's range and what the layout says about it, and the proof that the per-channel
metric of tests/wide_out.py has teeth -- on the fp64 oracle alone it rejects, at the bf16 tolerances (the widest the GPU tests use),
every way a tail epilogue could lose, misplace or half-reduce an output lane, and accepts the reference rounded to float32."""
import ctypes

import numpy as np
import pytest

from enf_pde_amd import _lib
from tests import wide_out as WO
from tests.test_gpu_backward import TOL as TOL_GRAD
from tests.test_gpu_forward import TOL as TAU

ENF_OK, ENF_EINVAL, ENF_EUNSUPPORTED = 0, -1, -3


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- 1. the descriptor
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("D,H", [(64, 2), (128, 2), (64, 4)])
def test_num_out_range_and_sizes(lib, D, H, precision):
    """enf_check_desc takes num_out 1 .. 32 and refuses 33.  enf_layout.h: the last layer is packed in OB = ceil(O / 32) blocks of 32
    output columns (bO4: 32 OB floats; the ato4 / gto4 panels and p_o4: OP = 32 OB columns), so within 1 .. 32 the packed weights
    have ONE size; EnfWorkspace has no term in O at all (out and d out are the caller's), nor have the deterministic partials, the
    derivative calls' workspace or the Gauss-Newton product's."""
    sizes = set()
    for O in range(1, 33):
        d = _lib.make_desc(WO.B, WO.N, WO.Z, H, D, WO.C, O, 2, 0, 1, precision)
        assert lib.enf_check_desc(ctypes.byref(d)) == ENF_OK, O
        sizes.add((int(lib.enf_packed_weight_bytes(ctypes.byref(d))), int(lib.enf_workspace_bytes_ex(ctypes.byref(d), 0)),
                   int(lib.enf_workspace_bytes_ex(ctypes.byref(d), _lib.ENF_FIT_DETERMINISTIC)),
                   int(lib.enf_field_grad_workspace_bytes(ctypes.byref(d), 0)), int(lib.enf_gn_workspace_bytes(ctypes.byref(d), 0))))
    assert len(sizes) == 1 and all(v > 0 for v in next(iter(sizes))), sizes
    for O in (0, 33, 64):
        d = _lib.make_desc(WO.B, WO.N, WO.Z, H, D, WO.C, O, 2, 0, 1, precision)
        assert lib.enf_check_desc(ctypes.byref(d)) == (ENF_EUNSUPPORTED if O > 32 else ENF_EINVAL), O
        assert lib.enf_packed_weight_bytes(ctypes.byref(d)) == 0 and lib.enf_workspace_bytes_ex(ctypes.byref(d), 0) == 0


# ---- 2. the metric has teeth
def _rejected(check, *args, **kw):
    with pytest.raises(AssertionError):
        check(*args, **kw)
    return True


@pytest.mark.parametrize("O", WO.WIDTHS)
def test_every_channel_carries_weight(O):
    """what the bounds rest on: no channel of the reference is small against the tensor (each max|out_o| >= 0.2 max|out|), so a
    channel that is lost moves the per-channel error far beyond 3e-2"""
    out = WO.problem(O).out
    share = np.abs(out).reshape(-1, O).max(0) / np.abs(out).max()
    print(f"O = {O}: smallest max|out_o| / max|out| = {share.min():.3f}")
    assert share.min() >= 0.2


@pytest.mark.parametrize("O", WO.WIDTHS)
def test_metric_accepts_the_reference_in_float32(O):
    c = WO.problem(O)
    WO.check_channels(WO.f32(c.out), c.out, TAU["f32"], f"O = {O}: out rounded to fp32")
    if O in (5, 17, 32):
        g = WO.latent_grads(c)
        WO.check_grads([WO.f32(v) for v in g], g, TOL_GRAD["f32"], f"O = {O}: gradients rounded to fp32")
        for form in ("none", "point", "channel"):
            r = WO.fit_reference(c, form, float(WO.B))
            got = WO.point_errors(WO.f32(c.out), WO.poisoned(r.lp), r.lp.w3)
            WO.check_point_errors(WO.f32(got), WO.f32(got.sum(1) / (WO.N * O)), c.out, r.lp.y, r.lp.w3, TAU["f32"], f"O = {O} {form}: err in fp32")


@pytest.mark.parametrize("O", WO.WIDTHS)
def test_metric_rejects_swapped_and_dead_channels(O):
    c = WO.problem(O)
    tol = TAU["bf16"]
    pairs = [(0, O - 1), (O - 2, O - 1)] + ([(3, 4)] if O > 4 else []) + ([(15, 16), (0, 16)] if O > 16 else [])
    for i, j in pairs:
        bad = c.out.copy()
        bad[..., [i, j]] = bad[..., [j, i]]
        e = WO.channel_errors(bad, c.out)
        assert e[i] > 10 * tol and e[j] > 10 * tol, (i, j, e)
        assert _rejected(WO.check_channels, bad, c.out, tol, f"O = {O}: channels {i}, {j} swapped")
    for first in (4, 16):
        if O > first:
            bad = c.out.copy()
            bad[..., first:] = 0.0
            assert _rejected(WO.check_channels, bad, c.out, tol, f"O = {O}: channels >= {first} zeroed")
            assert (WO.channel_errors(bad, c.out)[first:] > 5 * tol).all()      # every one of them, not the worst alone
    one = c.out.copy()
    one[..., O - 1] = 0.0
    assert _rejected(WO.check_channels, one, c.out, tol, f"O = {O}: the last channel zeroed")


@pytest.mark.parametrize("O", [5, 17, 32])
def test_metric_rejects_gradients_of_a_truncated_cotangent(O):
    c = WO.problem(O)
    g = WO.latent_grads(c)
    for first in (3, 16):
        if O > first:
            bad = WO.latent_grads(c, ("drop", first))
            assert _rejected(WO.check_grads, bad, g, TOL_GRAD["bf16"], f"O = {O}: cotangent of channels >= {first} dropped")
    if O == 17:                 # the single-channel cotangent of the GPU test: losing it leaves exact zeros
        only = WO.latent_grads(c, "only16")
        assert all(np.abs(v).max() > 0 for v in only)
        assert _rejected(WO.check_grads, [np.zeros_like(v) for v in only], only, TOL_GRAD["bf16"], "channel 16 alone, lost")


@pytest.mark.parametrize("form", ["none", "point", "channel"])
@pytest.mark.parametrize("O", [5, 17, 32])
def test_metric_rejects_errors_that_miss_channels(O, form):
    """err without the contribution of the channels 4 .. (quads 1 .. 3 and tile 1 not folded in), of the channels 16 .. (tile 1), and
    with a fold step applied twice"""
    c = WO.problem(O)
    r = WO.fit_reference(c, form, float(WO.B))
    lp = r.lp
    for first in (4, 16):
        if O > first:
            w_cut = lp.w3 * (np.arange(O) < first)
            bad = WO.point_errors(c.out, lp.y, w_cut)
            assert _rejected(WO.check_point_errors, bad, bad.sum(1) / (WO.N * O), c.out, lp.y, lp.w3, TAU["bf16"],
                             f"O = {O} {form}: err without channels >= {first}")
    twice = r.err + WO.point_errors(c.out, lp.y, lp.w3 * (np.arange(O) >= 4))
    assert _rejected(WO.check_point_errors, twice, twice.sum(1) / (WO.N * O), c.out, lp.y, lp.w3, TAU["bf16"], f"O = {O} {form}: a fold twice")
    # and the scalar loss of the same truncation is outside the fit step's widest bound
    assert abs(WO.point_errors(c.out, lp.y, lp.w3 * (np.arange(O) < 4)).sum() / (WO.B * WO.N * O) - r.loss) > 3e-2 * r.loss


def test_frobenius_bound_rejects_a_lost_derivative_channel():
    """Three bf16 derivative cases of tests/test_gpu_wide_out.py hold a per-channel bound above 7e-2 (operand rounding, measured against
    the rounding build); they also keep the project's relative Frobenius bound, and that one rejects any single lost channel of the
    Jacobian and of both tangents at O = 17"""
    from tests import tangent_ref, tangent_x_ref
    from tests.test_gpu_tangent import TOL as TOL_TAN
    refs = {"jacobian": (WO.jacobian_x(WO.problem(17)), 2), "tangent": (tangent_ref.case("rel_pos_periodic", O=17, freq=WO.FREQ)[5], -1),
            "tangent with xdot": (tangent_x_ref.case("rel_pos_periodic", O=17, freq=WO.FREQ)[7], -1)}
    for name, (ref, axis) in refs.items():
        worst = 1.0
        for o in range(17):
            bad = np.moveaxis(ref.copy(), axis, -1)
            bad[..., o] = 0.0
            worst = min(worst, float(WO.rel(np.moveaxis(bad, -1, axis), ref)))
        print(f"{name}: the least a lost channel moves the relative Frobenius error: {worst:.3f} (bound {TOL_TAN['bf16']:.1e})")
        assert worst > 2 * TOL_TAN["bf16"]
