"""CPU tests of the separable convolution's C entry points at C = 256 (config_shallow_water.yaml's node: hidden 256,
basis 128): the shape check accepts the width for every basis width, the scratch size is what the partial layout implies,
and the widths outside the kernel set are still refused."""
import pytest

ENF_EINVAL, ENF_EUNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def lib():
    from enf_pde_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("J", [16, 32, 64, 128])
@pytest.mark.parametrize("B,Z", [(3, 8), (1, 33), (128, 16)])
def test_weight_gradient_scratch_at_256(lib, B, Z, J):
    """One (J, C) + C partial (d W, then d bias) per workgroup, min(B Z, 256) workgroups over the (b, r) rows: the channel
    groups of the grid's second dimension write columns of the same partials, so the size does not depend on them."""
    n = lib.enf_ode_conv_backward_weight_scratch_bytes(B, Z, J, 256)
    assert n > 0
    assert n == min(B * Z, 256) * (J * 256 + 256) * 4
    assert n == 2 * lib.enf_ode_conv_backward_weight_scratch_bytes(B, Z, J, 128)


def test_widths_outside_the_kernel_set_are_refused(lib):
    for B, Z, J, C in [(2, 8, 64, 24), (2, 8, 64, 512), (2, 8, 256, 256), (2, 8, 256, 128), (2, 8, 48, 256), (2, 8, 64, 192)]:
        assert lib.enf_ode_conv_backward_weight_scratch_bytes(B, Z, J, C) == 0, (J, C)
        assert lib.enf_ode_conv_forward(B, Z, J, C, None, None, Z * J, J, None, None, None, None) == ENF_EUNSUPPORTED, (J, C)
        assert lib.enf_ode_conv_backward_basis(B, Z, J, C, None, None, None, None, None) == ENF_EUNSUPPORTED, (J, C)
        assert lib.enf_ode_conv_backward_weight(B, Z, J, C, None, None, None, None, None, 0, None) == ENF_EUNSUPPORTED, (J, C)


@pytest.mark.parametrize("J", [16, 32, 64, 128])
def test_null_pointers_at_256_are_invalid_arguments(lib, J):
    """The shape passes the check, so the NULL pointers are what is wrong: invalid argument, not unsupported."""
    assert lib.enf_ode_conv_forward(2, 8, J, 256, None, None, 8 * J, J, None, None, None, None) == ENF_EINVAL
    assert lib.enf_ode_conv_backward_basis(2, 8, J, 256, None, None, None, None, None) == ENF_EINVAL
    assert lib.enf_ode_conv_backward_weight(2, 8, J, 256, None, None, None, None, None, 0, None) == ENF_EINVAL
