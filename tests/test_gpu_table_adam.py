"""enf_table_adam_update alone: one optax adam step over the four components of a latent table in one launch, from gathered gradient
rows, against float64 adam on identical inputs (tests/table_adam_ref.py; nonmaml_pde_trainer.py:67,125-126,159-160)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import table_adam_ref as TA

pytestmark = pytest.mark.gpu

LR = 1e-2


def _c(count):
    return 1.0 - TA.B1 ** count, 1.0 - TA.B2 ** count


def _launch(cuda, tables, mu, nu, grads, idx, count, lr=LR, inplace=False):
    """The C-ABI call itself.  ``grads`` are passed as they are (column slices included); returns (x', mu', nu') on the GPU."""
    from enf_pde_amd import _lib
    lib = _lib.load()
    S, Z = tables[0].shape[:2]
    outs = (tables, mu, nu) if inplace else tuple([torch.empty_like(t) for t in ts] for ts in (tables, mu, nu))
    segs = (_lib.EnfAdamSegment * _lib.ENF_ADAM_MAX_SEGMENTS)()
    for k, g in enumerate(grads):
        assert g.stride(2) == 1 and g.stride(0) == Z * g.stride(1)
        segs[k] = _lib.EnfAdamSegment(tables[k].data_ptr(), mu[k].data_ptr(), nu[k].data_ptr(), g.data_ptr(), outs[0][k].data_ptr(),
                                      outs[1][k].data_ptr(), outs[2][k].data_ptr(), tables[k].shape[2], g.stride(1))
    it = None if idx is None else torch.tensor(idx, dtype=torch.int64, device=cuda)
    c1, c2 = _c(count)
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    _lib.launch(cuda, lib.enf_table_adam_update, len(grads), segs, S, Z, None if it is None else it.data_ptr(),
                S if idx is None else len(idx), lr, TA.B1, TA.B2, TA.EPS, c1, c2, st)
    torch.cuda.synchronize()
    return outs


def _to(cuda, tables, mu, nu, grads, widths):
    """The problem on the GPU, the pose gradients still column slices of one tensor."""
    d = lambda ts: [t.to(cuda) for t in ts]
    if len(widths) == 4:
        pose = torch.cat((grads[0], grads[1]), dim=-1).to(cuda)
        g = [pose[..., :widths[0]], pose[..., widths[0]:], grads[2].to(cuda), grads[3].to(cuda)]
        assert not g[0].is_contiguous() and g[0].stride(1) == widths[0] + widths[1]
    else:
        g = d(grads)
    return d(tables), d(mu), d(nu), g


@pytest.mark.parametrize("count", [1, 7])
@pytest.mark.parametrize("idx", [[4, 0, 2], [1, 1, 3], [2, -1, 9], None], ids=["batch", "duplicates", "out-of-range", "dense"])
def test_kernel_is_optax_adam(cuda, idx, count):
    """S = 5, Z = 5, nidx = 3, widths (2, 1, 8, 1): 300 elements, two workgroups, the second one partly idle (the float4 units of
    ``a`` and the scalar ones of the other components share the launch)."""
    cpu = TA.problem(idx, count)
    tables, mu, nu, grads = _to(cuda, *cpu, TA.WIDTHS)
    keep = [t.clone() for t in tables + mu + nu]
    x, m, v = _launch(cuda, tables, mu, nu, grads, idx, count)
    assert all(torch.equal(a, b) for a, b in zip(tables + mu + nu, keep))                   # out of place: inputs untouched
    ref = TA.reference(*cpu, idx, count, LR)
    TA.check(x, m, v, ref, LR, label=f"idx={idx} count={count}")
    if idx is not None:                                                                    # rows outside the batch: momentum only
        out = [s for s in range(5) if s not in idx]
        b1, b2 = torch.tensor(TA.B1, device=cuda), torch.tensor(TA.B2, device=cuda)
        for k in range(4):
            assert torch.equal(m[k][out], b1 * mu[k][out]) and torch.equal(v[k][out], b2 * nu[k][out])
            if count == 1:
                assert torch.equal(x[k][out], tables[k][out])                              # zero moments: the row stays
            else:                                                                          # x moves by what the decayed moments give
                want = ref[0][k][out]
                assert np.abs(x[k][out].cpu().numpy() - want).max() <= 1e-5 * LR + 1e-6 * np.abs(want).max()
                assert not torch.equal(x[k][out], tables[k][out])
    # same inputs, same bits
    x2, m2, v2 = _launch(cuda, tables, mu, nu, grads, idx, count)
    assert all(torch.equal(a, b) for a, b in zip(x + m + v, x2 + m2 + v2))
    # in place
    t3, m3, v3 = ([t.clone() for t in ts] for ts in (tables, mu, nu))
    _launch(cuda, t3, m3, v3, grads, idx, count, inplace=True)
    assert all(torch.equal(a, b) for a, b in zip(x + m + v, t3 + m3 + v3))


def test_duplicate_rows_equal_their_sum(cuda):
    cpu = TA.problem([1, 1, 3], 7)
    tables, mu, nu, grads = _to(cuda, *cpu, TA.WIDTHS)
    got = _launch(cuda, tables, mu, nu, grads, [1, 1, 3], 7)
    summed = [torch.stack((g[0] + g[1], g[2])).contiguous() for g in grads]
    want = _launch(cuda, tables, mu, nu, summed, [1, 3], 7)
    assert all(torch.equal(a, b) for ga, wa in zip(got, want) for a, b in zip(ga, wa))


@pytest.mark.parametrize("S,Z,widths,idx", [(7, 3, (3, 5), [6, 2, 6, 0]),        # 168 elements: no multiple of the block, scalar units only
                                            (67, 9, (2, 1, 16, 1), [66, 0, 13]),  # 12060 elements, float4 and scalar units, many workgroups
                                            (3, 2, (4,), None)])                  # one component, dense
def test_other_shapes_and_mixed_sign_moments(cuda, S, Z, widths, idx):
    """Sizes that are no multiple of the 256-thread block, more than one block, one to four components -- with moments whose signs
    are independent of the gradient's: mu' is then judged on the scale of its terms (tests/table_adam_ref.py: check)."""
    cpu = TA.problem(idx, 7, S=S, Z=Z, widths=widths, seed=3, mixed_signs=True)
    tables, mu, nu, grads = _to(cuda, *cpu, widths)
    x, m, v = _launch(cuda, tables, mu, nu, grads, idx, 7)
    TA.check(x, m, v, TA.reference(*cpu, idx, 7, LR), LR, label=f"S={S} Z={Z} widths={widths}", mu0=cpu[1])
    cpu = TA.problem(idx, 7, S=S, Z=Z, widths=widths, seed=4)
    tables, mu, nu, grads = _to(cuda, *cpu, widths)
    x, m, v = _launch(cuda, tables, mu, nu, grads, idx, 7)
    TA.check(x, m, v, TA.reference(*cpu, idx, 7, LR), LR, label=f"S={S} Z={Z} widths={widths} (signed)")


def test_misaligned_wide_component_takes_the_scalar_units(cuda):
    """A width-8 component whose gradient is a column slice at an odd offset (stride 9, base 4 bytes in): not float4 material."""
    cpu = TA.problem([4, 0, 2], 7, widths=(8,), seed=5)
    tables, mu, nu, grads = cpu
    wide = torch.zeros(3, 5, 9)
    wide[..., 1:] = grads[0]
    wide = wide.to(cuda)
    d = lambda ts: [t.to(cuda) for t in ts]
    x, m, v = _launch(cuda, d(tables), d(mu), d(nu), [wide[..., 1:]], [4, 0, 2], 7)
    TA.check(x, m, v, TA.reference(*cpu, [4, 0, 2], 7, LR), LR, label="misaligned")


def test_table_adam_update_on_gpu_tensors(cuda):
    """The Python entry: column slices go through as they are, the state's count advances, three steps follow Adam.update."""
    from enf_pde_amd.fitting.optim import Adam, scatter_rows, table_adam_update
    opt = Adam(3e-3)
    cpu = TA.problem([4, 0, 2], 1)
    tables = [t.to(cuda) for t in cpu[0]]
    s_old, s_new, x_old, x_new = opt.init(tables), opt.init(tables), tables, tables
    for step, idx in enumerate(([4, 0, 2], [1, 1, 3], [0, 3, 4])):
        _, _, _, grads = _to(cuda, *TA.problem(idx, 1, seed=step + 1), TA.WIDTHS)
        it = torch.tensor(idx, device=cuda)
        x_old, s_old = opt.update(scatter_rows(grads, it, 5), s_old, x_old)
        x_new, s_new = table_adam_update(opt, s_new, x_new, grads, idx=it)
    assert s_new["count"] == 3 and all(t.is_cuda for t in x_new)
    for a, b in zip(x_new + s_new["mu"] + s_new["nu"], x_old + s_old["mu"] + s_old["nu"]):
        torch.testing.assert_close(a, b, rtol=2e-5, atol=1e-7)
    dense = scatter_rows(grads, it, 5)
    x_d, s_d = table_adam_update(opt, s_old, x_old, dense, idx=None)                        # the multi-rank form
    x_g, s_g = table_adam_update(opt, s_old, x_old, grads, idx=it)
    assert all(torch.equal(a, b) for a, b in zip(x_d + s_d["mu"] + s_d["nu"], x_g + s_g["mu"] + s_g["nu"]))
