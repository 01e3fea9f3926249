"""dx 1 .. 3 and latent_dim 1 .. 130 without a GPU: what enf_check_desc accepts, that the size functions follow, that the fp64 oracle
itself obeys the lifting identity and the group invariances tests/test_gpu_coord_dims.py holds the kernels to, and that every case of
tests/coord_dims_ref.py has its windows where the 2-D suite has them."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest

from enf_pde_amd import _lib
from oracle import enf_ref_np as R
from tests import coord_dims_ref as CD

ENF_OK, ENF_EDIM = 0, -6
TWO_D = ("rel_pos_periodic", "latitude_periodic", "polar_periodic", "ponita")
THREE_D = ("ball", "ball_lat", "ponita_full")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _desc(inv, dx, C=8, D=64, H=2, precision=0, shape=CD.BASE):
    B, N, Z = shape
    return _lib.make_desc(B, N, Z, H, D, C, 2, dx, _lib.INVARIANT_IDS[inv], 1, precision)


def _accepted(inv, dx):
    """the rule of enf_check_desc (include/enf_hip.h): dx in 1 .. 3; the four 2-D invariants take dx = 2 only, ponita_full and the ball
    invariants dx = 3 only, the three translation invariants any of 1 .. 3"""
    if inv in TWO_D:
        return dx == 2
    if inv in THREE_D:
        return dx == 3
    return 1 <= dx <= 3


# ---- 1. the descriptor
@pytest.mark.parametrize("precision", [0, 1])
def test_descriptor_acceptance_matrix(lib, precision):
    assert sorted(_lib.INVARIANT_IDS.values()) == list(range(10))
    for inv in _lib.INVARIANT_IDS:
        for dx in range(5):
            rc = lib.enf_check_desc(ctypes.byref(_desc(inv, dx, precision=precision)))
            assert rc == (ENF_OK if _accepted(inv, dx) else ENF_EDIM), (inv, dx, rc)
    for inv in CD.INVS:
        assert [_accepted(inv, dx) for dx in range(5)] == [False, True, True, True, False]


@pytest.mark.parametrize("precision", [0, 1])
def test_size_functions_follow_the_descriptor(lib, precision):
    """non-zero for every accepted (invariant, dx) at both shapes of the GPU tests, zero for every refused one"""
    flags = _lib.ENF_BWD_DETERMINISTIC | _lib.ENF_BWD_QUERY_GRAD
    for inv in _lib.INVARIANT_IDS:
        for dx in range(5):
            for shape in (CD.BASE, CD.TILES):
                d = _desc(inv, dx, precision=precision, shape=shape)
                sizes = (int(lib.enf_workspace_bytes(ctypes.byref(d))), int(lib.enf_workspace_bytes_ex(ctypes.byref(d), flags)),
                         int(lib.enf_field_grad_workspace_bytes(ctypes.byref(d), 0)), int(lib.enf_packed_weight_bytes(ctypes.byref(d))))
                assert all(v > 0 for v in sizes) if _accepted(inv, dx) else all(v == 0 for v in sizes), (inv, dx, shape, sizes)


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("D,H", [(64, 2), (128, 2)])
def test_packed_weights_grow_by_the_stem_rows(lib, D, H, precision):
    """stem_w is latent_dim x D fp32 and nothing else in the blob depends on latent_dim: 4 (C' - C) D bytes between two widths"""
    size = lambda C: int(lib.enf_packed_weight_bytes(ctypes.byref(_desc("rel_pos_periodic", 2, C=C, D=D, H=H, precision=precision))))
    sizes = [size(C) for C in CD.C_LIST]
    assert all(v > 0 for v in sizes)
    for (c0, s0), (c1, s1) in zip(zip(CD.C_LIST, sizes), zip(CD.C_LIST[1:], sizes[1:])):
        assert s1 - s0 == 4 * (c1 - c0) * D, (c0, c1, s0, s1)
    for C in CD.C_LIST:                                  # no upper bound on latent_dim, and the workspaces exist at every width
        d = _desc("rel_pos_periodic", 2, C=C, D=D, H=H, precision=precision, shape=(2, 40, 37))
        assert lib.enf_check_desc(ctypes.byref(d)) == ENF_OK
        assert lib.enf_workspace_bytes_ex(ctypes.byref(d), _lib.ENF_BWD_DETERMINISTIC) > 0 and lib.enf_gn_workspace_bytes(ctypes.byref(d), 0) > 0


# ---- 2. the oracle's dimensions against the package's invariant classes
@pytest.mark.parametrize("num_in", [1, 2, 3])
@pytest.mark.parametrize("inv", CD.INVS)
def test_invariant_spec_dims(lib, inv, num_in):
    from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant
    spec = R.invariant_spec(inv, num_in)
    cls = get_ca_invariant(NS(invariant_type=inv, num_in=num_in))
    assert (spec["dim"], spec["dx"], spec["z_pos"]) == (cls.dim, cls.num_x_pos_dims, cls.num_z_pos_dims)
    assert spec["dx"] == spec["z_pos"] == num_in and spec["dim"] == (1 if inv == "norm_rel_pos" else num_in)
    iid = _lib.INVARIANT_IDS[inv]
    assert lib.enf_invariant_dim(iid, num_in) == spec["dim"] and lib.enf_invariant_pose_dim(iid, num_in) == spec["z_pos"]


# ---- 3. the sigma condition
def test_every_case_keeps_its_windows_where_the_2d_suite_has_them():
    n = 0
    for label, c in CD.all_cases():
        m = float(c.s.mean())
        assert 0.5 <= m <= 1.5, (label, m)
        assert c.s.min() > 0.9 * CD.SIGMA - 1e-6 and c.s.max() < 1.1 * CD.SIGMA + 1e-6, label
        n += 1
    assert n >= 40
    # what make_inputs gives unscaled, the reason for the scale
    assert CD.sigma_scale("rel_pos", 1, 7) == pytest.approx(CD.SIGMA * 7) and CD.sigma_scale("rel_pos", 3, 7) == pytest.approx(CD.SIGMA / 1.5)
    assert CD.sigma_scale("rel_pos", 2, 7) == pytest.approx(1.0) and CD.sigma_scale("rel_pos_periodic", 2, 37) == pytest.approx(2.0)


# ---- 4. the oracle obeys the identities the kernels are held to
def _max_rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("dx", [1, 2])
@pytest.mark.parametrize("inv", CD.INVS)
def test_oracle_lifting_identity(inv, dx):
    """dx -> dx + 1 with a zero coordinate: out, d a, d sigma, the first dx columns of d x and d p and the mean squared error agree to
    1e-12, and the gradient along the added coordinate is the only thing that is new"""
    c = CD.problem(inv, dx)
    up = CD.lift(c)
    assert up.x.shape[-1] == dx + 1 and np.all(up.x[..., dx] == 0) and np.all(up.p[..., dx] == 0)
    g, gu = CD.backward(c), CD.backward(up)
    y = CD.fit(c).y
    errs = {"out": _max_rel(up.out, c.out), "d a": _max_rel(gu.ga, g.ga), "d sigma": _max_rel(gu.gs, g.gs), "d x": _max_rel(gu.gx[..., :dx], g.gx),
            "loss": abs(((up.out - y) ** 2).mean() - ((c.out - y) ** 2).mean()) / ((c.out - y) ** 2).mean()}
    scale = max(np.abs(g.gp).max(), 1e-9 * np.abs(g.ga).max())           # abs_pos: d p comes from the window alone
    errs["d p"] = float(np.abs(gu.gp[..., :dx] - g.gp).max() / scale)
    print(f"lifting {inv} {dx} -> {dx + 1} in fp64: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= 1e-12 for v in errs.values()), errs


@pytest.mark.parametrize("dx", CD.DXS)
@pytest.mark.parametrize("inv", CD.INVS)
def test_oracle_translation(inv, dx):
    """x + t, p + t: rel_pos and norm_rel_pos do not move (1e-12); abs_pos does"""
    c = CD.problem(inv, dx)
    t = CD.translation(dx)
    e = _max_rel(R.nef_apply(c.prm, c.cfg, c.x + t, c.p + t, c.a, c.s), c.out)
    print(f"translation {inv} dx={dx} in fp64: {e:.2e}")
    assert e > 1e-3 if inv == "abs_pos" else e <= 1e-12


def test_oracle_rotation():
    """x R^T, p R^T in 3-D: norm_rel_pos does not move (1e-12); rel_pos does"""
    Rm = CD.rotation()
    for inv in ("norm_rel_pos", "rel_pos"):
        c = CD.problem(inv, 3)
        e = _max_rel(R.nef_apply(c.prm, c.cfg, c.x @ Rm.T, c.p @ Rm.T, c.a, c.s), c.out)
        print(f"rotation {inv} in fp64: {e:.2e}")
        assert e <= 1e-12 if inv == "norm_rel_pos" else e > 1e-3
