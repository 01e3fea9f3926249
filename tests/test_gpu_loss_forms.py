"""The small kernels of csrc/enf_loss.hip that exist once for several entry points: what their forms must agree on, bit for bit.
  1. enf_mse_value_grad, _w with all-ones weights and _cw with all-ones weights are the same numbers (one kernel template);
  2. enf_signal_sum adds in its documented order (tests/test_loss_forms_host.py emulates it; a plain sum gives other bits there);
  3. enf_fit_inputs_b and _cw, both mask layouts, gather what gather_signal_points / gather_point_weights gather (one row kernel);
  4. the four enf_fit_inputs* entry points answer the same bad argument with the same error code (one host function)."""
import ctypes

import numpy as np
import pytest
import torch

from enf_pde_amd import _lib
from enf_pde_amd.fitting.inner_loop import _fit_inputs, gather_signal_points
from enf_pde_amd.fitting.weights import gather_point_weights
from tests.test_loss_forms_host import SIGNAL_SUM_N, signal_sum_emulated, signal_sum_input

pytestmark = pytest.mark.gpu
P = _lib.ptr


def _mse(cuda, form, out, tgt, O, flags):
    lib, st, n = _lib.load(), _lib.stream(cuda), out.numel()
    dout, loss = torch.empty_like(out), torch.zeros(1, device=cuda)
    nb = int(lib.enf_mse_scratch_bytes(n, flags))
    scr = torch.empty(max(nb, 1), device=cuda, dtype=torch.uint8)
    ones = torch.ones(n // O, device=cuda)
    if form == "plain" and not flags:
        _lib.launch(cuda, lib.enf_mse_value_grad, P(out), P(tgt), n, 3.0, P(dout), P(loss), st)
    elif form == "plain":
        _lib.launch(cuda, lib.enf_mse_value_grad_ex, P(out), P(tgt), n, 3.0, P(dout), P(loss), P(scr), nb, flags, st)
    elif form == "w":
        _lib.launch(cuda, lib.enf_mse_value_grad_w, P(out), P(tgt), P(ones), n, O, 3.0, P(dout), P(loss), P(scr), nb, flags, st)
    else:
        _lib.launch(cuda, lib.enf_mse_value_grad_cw, P(out), P(tgt), P(ones), n, 3.0, P(dout), P(loss), P(scr), nb, flags, st)
    torch.cuda.synchronize()
    return loss, dout


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("n", [258, 262146])          # two blocks; 6 x 43691 = 1024 x 256 + 2: the grid-stride loop runs
def test_mse_forms_agree(cuda, n, det):
    """Unweighted, one weight of 1 per O values (O = 1, 2, 3) and one weight of 1 per value: identical loss and dout.  The atomic form
    adds one partial per block to the loss in the order the blocks finish: with more than two blocks that order shows in the bits of
    ANY two calls, so there the loss is compared on a second input whose blocks all hold the same partial (every order then adds the
    same numbers: d = +-0.5 in the first 1024 x 256 elements, 0 in the last two, which block 0 takes) and random data is held to dout."""
    g = torch.Generator().manual_seed(n)
    out, tgt = torch.randn(n, generator=g).to(cuda), torch.randn(n, generator=g).to(cuda)
    flat = torch.zeros(n)
    flat[:n // 256 * 256] = torch.randint(0, 2, (n // 256 * 256,), generator=g).float() - 0.5
    flags = _lib.ENF_MSE_DETERMINISTIC if det else 0
    order_free = det or n <= 512
    for o, t, with_loss in ((out, tgt, order_free), (flat.to(cuda), torch.zeros(n, device=cuda), True)):
        loss0, dout0 = _mse(cuda, "plain", o, t, 1, flags)
        assert float(loss0) > 0 and bool(torch.isfinite(dout0).all()) and bool((dout0 != 0).sum() >= n - 2)
        for form, O in (("w", 1), ("w", 2), ("w", 3), ("cw", 1)):
            loss, dout = _mse(cuda, form, o, t, O, flags)
            assert torch.equal(dout, dout0), (form, O)
            if with_loss:
                assert torch.equal(loss, loss0), (form, O, float(loss), float(loss0))


@pytest.mark.parametrize("N", SIGNAL_SUM_N)
def test_signal_sum_order(cuda, N):
    err = signal_sum_input(N)
    scale = 1.0 / (3.0 * N)
    loss_b = torch.empty(err.shape[0], device=cuda)
    e = torch.tensor(err, device=cuda)
    _lib.launch(cuda, _lib.load().enf_signal_sum, P(e), err.shape[0], N, scale, P(loss_b), _lib.stream(cuda))
    torch.cuda.synchronize()
    want = signal_sum_emulated(err, scale)
    assert np.array_equal(loss_b.cpu().numpy().view(np.uint32), want.view(np.uint32)), (loss_b.cpu().numpy(), want)


# ---- the gathers: B = 3, Z = 5, N = 40, Ns = 7, S1 = 3, dx = 2, two latent components
B, Z, N, NS, S1, DX = 3, 5, 40, 7, 3, 2


def _gather_case(cuda, O, per_signal, bad):
    rng = np.random.default_rng(100 + O)
    t = lambda v: torch.tensor(v, dtype=torch.float32, device=cuda)
    lat0 = {"p_pos": t(rng.standard_normal((1, Z, 2))), "a": t(rng.standard_normal((1, Z, 6)))}
    coords, img = t(rng.standard_normal((N, DX))), t(rng.standard_normal((B, N, O)))
    m = rng.integers(0, N, (B, NS, S1) if per_signal else (NS, S1))
    if bad:
        m[..., 0, 0], m[..., 3, 1], m[..., NS - 1, S1 - 1] = -1, N, N + 9
    return lat0, coords, img, torch.tensor(m, device=cuda)


def _check_common(lat0, lat, losses):
    assert losses.shape == (S1,) and bool((losses == 0).all())
    for k in lat0:
        assert torch.equal(lat[k], lat0[k].expand(B, -1, -1))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("O", [1, 3])
def test_fit_inputs_b_gathers_signal_points(cuda, O, weighted):
    lat0, coords, img, masks = _gather_case(cuda, O, True, True)
    w = torch.rand(B, N, generator=torch.Generator().manual_seed(O)).to(cuda) + 0.5 if weighted else None
    lat, xs, ys, losses, ws = _fit_inputs(lat0, coords, img, masks, w)
    torch.cuda.synchronize()
    ref = gather_signal_points(coords, img, masks, w)
    assert xs.shape == (S1, B, NS, DX) and ys.shape == (S1, B, NS, O) and ws.shape == (S1, B, NS)
    assert torch.equal(xs, ref[0]) and torch.equal(ys, ref[1]) and torch.equal(ws, ref[2])
    assert int((ws == 0).sum()) == 3 * B                                  # the three indices outside [0, N) of every signal
    _check_common(lat0, lat, losses)


@pytest.mark.parametrize("per_signal", [False, True])
@pytest.mark.parametrize("O", [1, 3])
def test_fit_inputs_cw_gathers_signal_points(cuda, O, per_signal):
    cw = torch.rand(B, N, O, generator=torch.Generator().manual_seed(10 + O)).to(cuda) + 0.5
    for bad in (True, False):
        lat0, coords, img, masks = _gather_case(cuda, O, per_signal, bad)
        lat, xs, ys, losses, ws = _fit_inputs(lat0, coords, img, masks, cw, channel=True)
        torch.cuda.synchronize()
        full = masks if per_signal else masks[None].expand(B, -1, -1).contiguous()
        ref = gather_signal_points(coords, img, full, cw)
        assert ws.shape == (S1, B, NS, O) and torch.equal(ys, ref[1]) and torch.equal(ws, ref[2])
        assert torch.equal(xs, ref[0] if per_signal else ref[0][:, 0])    # shared masks: one (S1, Ns, dx) set
        assert int((ws == 0).sum()) == (3 * B * O if bad else 0)
        if not per_signal and not bad:
            assert torch.equal(ws, gather_point_weights(cw, masks))
        _check_common(lat0, lat, losses)


def test_fit_inputs_entry_points_share_their_error_codes(cuda):
    """NULL comps and ncomp = 0 are ENF_EINVAL, B = 0 is ENF_EDIM, from all four entry points; nothing is launched."""
    lib = _lib.load()
    lat0, coords, img, masks = _gather_case(cuda, 1, True, False)
    dst = torch.empty(B, Z, 2, device=cuda)
    comps = (_lib.EnfFitComponent * _lib.ENF_SGD_MAX_SEGMENTS)()
    comps[0] = _lib.EnfFitComponent(lat0["p_pos"].data_ptr(), dst.data_ptr(), 2, 0)
    buf = torch.zeros(S1 * B * NS * DX, device=cuda)
    st = _lib.stream(cuda)

    def codes(ncomp, comps_, B_):
        head = (ncomp, comps_, B_, Z, N, NS, S1, DX, 1, P(coords), P(img), P(masks), P(buf), P(buf), P(buf))
        return (lib.enf_fit_inputs(*head, st), lib.enf_fit_inputs_w(*head, P(buf), P(buf), st), lib.enf_fit_inputs_b(*head, P(buf), P(buf), st),
                lib.enf_fit_inputs_cw(*head, P(buf), P(buf), 0, st), lib.enf_fit_inputs_cw(*head, P(buf), P(buf), 1, st))
    EINVAL, EDIM = -1, -6
    assert codes(1, None, B) == (EINVAL,) * 5
    assert codes(0, comps, B) == (EINVAL,) * 5
    assert codes(1, comps, 0) == (EDIM,) * 5
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
