"""Sparse linear observations on the GPU (include/enf_hip.h, "Sparse linear observations": enf_obs_apply, enf_mse_value_grad_a,
enf_fit_step_a, enf_eval_loss_a) against tests/operators_ref.py in fp64.

    obs[b,m,o] = sum_e val[e] out[b, col[e], o]      loss = 1/(B M O) sum w (obs - target)^2      d out = gs A^T (w (obs - target))

Shapes.  The two kernels alone run on N = 200 columns with rows of 0, 1, 3, 9, 17, 27, 64, 65 and 200 entries -- both sides of the
threshold (65) between the one-lane sum and the whole-wave sum, a row longer than 64 + 64 -- and two more operators that move rows
between waves: the same lengths among forty short rows (mean length <= 16: full waves of one-lane rows with long rows among them) and
long rows only (one wave per row).  The last three columns are in no row; rows overlap; columns inside a row are unsorted; the row of 200
repeats columns.  O = 2 and 17 (one channel at a time) and 4 (the 16-byte path).  The fit step runs at B = 3, Z = 7, D = 64, H = 2.

Bounds.  The kernels alone: 1e-6 of the largest reference value (fp32 sums of at most 200 terms of size O(1 / sqrt(length))).  The fit
step against fp64: the contract of tests/test_gpu_cells.py for the same quantities -- f32 loss 1e-5, gradients 2e-4 relative L2; bf16
3e-2 and 7e-2.  Against enf_fit_step_g at equal groups: 1e-5 relative L2 (tests/test_gpu_gn_cells.py's bound for a composed route).
The loop: DESIGN.md section 2's inner-loop row -- f32 loss 5e-4, updates 1e-2; bf16 5e-2 and 1."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from tests.helpers import build_nef, make_cfg
from tests.operators_ref import B, Z, case, dense_loss, f32, fit_loop, poisoned, ragged_entries, rel
from enf_pde_amd import _lib
from enf_pde_amd.enf.models import TENSOR_PATHS
from enf_pde_amd.fitting import SparseObservations, cell_operator, decode_observations, fit_cell_averages, fit_linear_observations

pytestmark = pytest.mark.gpu

GUARD = 16
TOL = {"f32": (1e-5, 2e-4), "bf16": (3e-2, 7e-2)}                   # (loss, gradients): tests/test_gpu_cells.py
LOOP_TOL = {"f32": (5e-4, 1e-2), "bf16": (5e-2, 1.0)}               # (loss trajectory, updates): DESIGN.md section 2
LOSS_TOL = {"f32": 5e-4, "bf16": 5e-2}                              # per-signal losses: tests/test_gpu_cells.py
DET = _lib.ENF_FIT_DETERMINISTIC
ISSUE_LENGTHS = [0, 1, 3, 9, 17, 27, 64, 65, 200]
OPERATORS = {"nine rows": ISSUE_LENGTHS,                                                  # mean 42: four rows per wave
             "among short rows": ISSUE_LENGTHS + [1 + (i % 4) for i in range(40)],       # mean 10: 64 rows per wave, long rows among them
             "long rows": [130, 65, 64, 200, 128, 66]}                                    # mean 108: one wave per row
FIT_LENGTHS = [1, 27, 0, 5, 9, 13, 2, 20, 7, 3]
# One bf16 case is over the borrowed 7e-2 while its f32 twin sits at 2.4e-6: d p of the fit step with weights per value, 8.307e-2.  Decided
# with the rounding build libenf_hip_f32r.so (precision f32 with every operand rounded where bf16 rounds it): its error
# against the oracle on the same case is the same, d p 8.290e-2, and bf16 - f32r is 8.6e-4 of the reference's norm (d a 4.3e-4, d sigma
# 1.2e-3), as in the cases that keep 7e-2 (per observation: f32r 3.783e-2, bf16 - f32r 1.9e-4; latitude_periodic: 5.027e-2, 2.8e-4; 128x2:
# 3.063e-2, 3.0e-3).  The excess is operand rounding, and that component holds twice the f32r error.  The weights of this case zero about
# a third of the VALUES, so d p is a sum with fewer terms left to average the rounding.
BF16_OPERAND_ROUNDING = {"rel_pos_periodic weights per value bf16": {"dp": 2 * 8.290e-2}}


def _t(cuda):
    return lambda v: torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda)


def _ptr(v):
    return ctypes.c_void_p(v.data_ptr()) if v is not None else None


def _stream(cuda):
    return ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)


def _guarded(n, cuda):
    return torch.full((n + GUARD,), float("nan"), device=cuda)


# ---- 1. the two kernels alone
def _kernel_problem(name, O, seed=11):
    lengths, N = OPERATORS[name], 200
    rng = np.random.default_rng(seed)
    rows, cols, vals = ragged_entries(lengths, N, seed + 1, spare=3)
    M = len(lengths)
    A = np.zeros((M, N))
    np.add.at(A, (rows, cols), vals)
    out, y = f32(rng.standard_normal((B, N, O))), f32(rng.standard_normal((B, M, O)))
    w = f32(rng.uniform(0.2, 2.0, (B, M)))
    w[rng.uniform(size=(B, M)) < 0.3] = 0.0
    w[0, -1] = 0.0
    cw = f32(rng.uniform(0.2, 2.0, (B, M, O)))
    cw[rng.uniform(size=(B, M, O)) < 0.3] = 0.0
    cw[1, -1, 0] = 0.0
    return NS(rows=rows, cols=cols, vals=vals, A=A, out=out, y=y, w=w, cw=cw, M=M, N=N, O=O, gs=float(B))


def _mse_a(cuda, pb, op, y, w=None, cw=None, flags=0, poison=0, want_dout=True):
    """one enf_mse_value_grad_a call on poisoned scratch; dout, err_a in NaN-guarded buffers; r is read back from the scratch"""
    lib, t = _lib.load(), _t(cuda)
    out = t(pb.out)
    nscr = int(lib.enf_mse_a_scratch_bytes(B, pb.M, pb.O, 1 if want_dout else 0, flags))
    scr = torch.full((max(nscr, 4),), poison, device=cuda, dtype=torch.uint8)
    dbuf, ebuf = _guarded(B * pb.N * pb.O, cuda), _guarded(B * pb.M, cuda)
    loss = torch.zeros(1, device=cuda)
    s = op.struct()
    _lib.launch(cuda, lib.enf_mse_value_grad_a, _ptr(out), _ptr(y), B, pb.N, pb.O, ctypes.byref(s), _ptr(w), _ptr(cw), pb.gs,
                _ptr(dbuf) if want_dout else None, _ptr(loss), _ptr(ebuf), _ptr(scr), nscr, flags, _stream(cuda))
    torch.cuda.synchronize()
    nd, ne = B * pb.N * pb.O, B * pb.M
    r = scr[:4 * B * pb.M * pb.O].view(torch.float32).view(B, pb.M, pb.O).clone() if want_dout else None
    return NS(loss=loss, dout=dbuf[:nd].view(B, pb.N, pb.O), err=ebuf[:ne].view(B, pb.M), r=r, dguard=dbuf[nd:], eguard=ebuf[ne:])


@pytest.mark.parametrize("O", [2, 17, 4])
@pytest.mark.parametrize("name", list(OPERATORS))
def test_the_two_kernels_alone(cuda, name, O):
    pb = _kernel_problem(name, O)
    t = _t(cuda)
    op = SparseObservations.from_coo(pb.rows, pb.cols, pb.vals, pb.M, pb.N, device=cuda)
    assert np.array_equal(op.to_dense(), pb.A) and (np.diff(op.col_ptr.cpu().numpy())[-3:] == 0).all()
    lib = _lib.load()
    # the forward product alone
    obuf = _guarded(B * pb.M * O, cuda)
    s = op.struct(transposed=False)
    _lib.launch(cuda, lib.enf_obs_apply, _ptr(t(pb.out)), B, pb.N, O, ctypes.byref(s), _ptr(obuf), _stream(cuda))
    torch.cuda.synchronize()
    obs = obuf[:B * pb.M * O].view(B, pb.M, O)
    for label, w, cw in (("per observation", pb.w, None), ("per value", None, pb.cw), ("no weights", None, None)):
        wref = w if w is not None else cw
        ref = dense_loss(pb.A, pb.out, pb.y, wref, pb.gs)
        ybad = t(poisoned(pb.y, wref)) if wref is not None else t(pb.y)
        wt, cwt = (None if v is None else t(v) for v in (w, cw))
        got = _mse_a(cuda, pb, op, ybad, wt, cwt)
        errs = {"obs": np.abs(obs.double().cpu().numpy() - ref.obs).max() / np.abs(ref.obs).max(),
                "r": np.abs(got.r.double().cpu().numpy() - ref.r).max() / np.abs(ref.r).max(),
                "dout": np.abs(got.dout.double().cpu().numpy() - ref.dout).max() / np.abs(ref.dout).max(),
                "err_a": np.abs(got.err.double().cpu().numpy() - ref.err_a).max() / np.abs(ref.err_a).max(),
                "loss": abs(float(got.loss) - ref.loss) / ref.loss}
        print(f"kernels alone, {name}, O={O}, {label}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        # (the scalar loss: the fit step's f32 bound, 1e-5 -- a sum over B M O shares and, in this mode, float atomics)
        assert all(v <= 1e-6 for k, v in errs.items() if k != "loss") and errs["loss"] <= 1e-5, errs
        assert bool((got.dout[:, -3:] == 0).all()) and bool((obs[:, torch.tensor(np.asarray(OPERATORS[name]) == 0, device=cuda)] == 0).all())
        assert bool(torch.isnan(got.dguard).all()) and bool(torch.isnan(got.eguard).all()) and bool(torch.isnan(obuf[B * pb.M * O:]).all())
        assert bool(torch.isfinite(got.dout).all()) and bool(torch.isfinite(got.err).all()) and bool(torch.isfinite(got.loss).all())
        if wref is not None:                                           # zero weights with NaN / Inf targets leave exact zeros
            gone = torch.tensor(np.broadcast_to((wref == 0)[..., None] if wref.ndim == 2 else wref == 0, (B, pb.M, O)).copy(), device=cuda)
            assert bool(gone.any()) and bool((got.r[gone] == 0).all())
            clean = _mse_a(cuda, pb, op, t(pb.y), wt, cwt, poison=255)
            assert all(torch.equal(getattr(clean, k), getattr(got, k)) for k in ("dout", "err", "r"))
            if w is not None:
                assert bool((got.err[torch.tensor(w == 0, device=cuda)] == 0).all())
        # equal bits run to run and over scratch of 0x00 / 0xFF; obs, r, err_a and d out in every mode, the loss in deterministic mode
        d0, d1 = _mse_a(cuda, pb, op, ybad, wt, cwt, flags=DET, poison=0), _mse_a(cuda, pb, op, ybad, wt, cwt, flags=DET, poison=255)
        assert all(torch.equal(getattr(d0, k), getattr(d1, k)) for k in ("loss", "dout", "err", "r"))
        assert all(torch.equal(getattr(d0, k), getattr(got, k)) for k in ("dout", "err", "r"))
        assert abs(float(d0.loss) - float(got.loss)) <= 1e-6 * float(got.loss)
        only = _mse_a(cuda, pb, op, ybad, wt, cwt, flags=DET, want_dout=False)      # without d out: the loss and err_a, the same bits
        assert torch.equal(only.loss, d0.loss) and torch.equal(only.err, d0.err) and bool(torch.isnan(only.dout).all())


@pytest.mark.parametrize("O", [2, 4])
def test_rows_per_wave_change_no_bit(cuda, O):
    """The same nine rows in front of 52 other rows of 1 .. 4, of 20, of 40 and of 150 entries: M = 61 every time (so d out keeps its
    factor 2 / (B M O)), mean length 8, 23, 40 and 134 -- 64, 16, 4 rows per wave and one wave per row.  obs, r and err_a of the nine
    rows are equal bits, and with weight 0 on the other rows (their r is 0.0f, and a column's sum adds them behind the nine rows'
    entries) so is d out."""
    base = _kernel_problem("nine rows", O)
    t = _t(cuda)
    lib = _lib.load()
    got = {}
    for rpw, extra in ((64, [1 + (i % 4) for i in range(52)]), (16, [20] * 52), (4, [40] * 52), (1, [150] * 52)):
        er, ec, ev = ragged_entries(extra, base.N, 91, spare=3)
        rows, cols, vals = np.append(base.rows, er + base.M), np.append(base.cols, ec), np.append(base.vals, ev)
        M = base.M + len(extra)
        mean = rows.size // M
        assert rpw == (64 if mean <= 16 else 16 if mean <= 32 else 4 if mean < 65 else 1), (rpw, mean)      # (csrc/enf_obs.hip: obs_rows_per_wave)
        op = SparseObservations.from_coo(rows, cols, vals, M, base.N, device=cuda)
        pad = lambda v, fill: np.concatenate([v, np.full((B, len(extra)) + v.shape[2:], fill, dtype=v.dtype)], 1)
        pb = NS(**{**vars(base), "M": M})
        r = _mse_a(cuda, pb, op, t(pad(base.y, 0.5)), t(pad(np.maximum(base.w, 0.25), 0.0)), None, flags=DET)
        obuf = torch.empty(B, M, O, device=cuda)
        s = op.struct(transposed=False)
        _lib.launch(cuda, lib.enf_obs_apply, _ptr(t(base.out)), B, base.N, O, ctypes.byref(s), _ptr(obuf), _stream(cuda))
        torch.cuda.synchronize()
        got[rpw] = NS(obs=obuf[:, :base.M].clone(), r=r.r[:, :base.M].clone(), err=r.err[:, :base.M].clone(), dout=r.dout.clone(), loss=r.loss)
        assert bool((r.r[:, base.M:] == 0).all()) and bool(torch.isfinite(r.dout).all()) and bool((r.dout != 0).any())
    for rpw in (16, 4, 1):
        diff = [k for k in ("obs", "r", "err", "dout", "loss") if not torch.equal(getattr(got[rpw], k), getattr(got[64], k))]
        print(f"rows per wave {rpw} against 64, O={O}: differing {diff}")
        assert [k for k in diff if k != "loss"] == [], (rpw, diff)


# ---- 2 .. 6. the fit step and the evaluation
def _run(cuda, nef, params, c, op, kind="fit", flags=0, y=None, w="case", poison=255, want=("loss", "err", "loss_b"), x=None, xstride=None,
         gs=None):
    """One raw C-ABI call on a workspace filled with `poison`: kind "fit" = enf_fit_step_a, "eval" = enf_eval_loss_a.  err_a and loss_b
    sit in NaN-filled buffers with GUARD floats behind them."""
    lib, t = _lib.load(), _t(cuda)
    Bn, Zn = c.B, c.Z
    xt = t(c.x) if x is None else x
    p, a, s = t(c.p), t(c.a), t(c.s)
    wv = c.w if isinstance(w, str) else w
    yt = t(poisoned(c.y, wv) if wv is not None else c.y) if y is None else y
    wt = None if wv is None else t(wv)
    ow, cw = (wt, None) if wt is None or wt.dim() == 2 else (None, wt)
    desc = nef._desc(Bn, c.N, Zn)
    nbytes = int(lib.enf_obs_workspace_bytes(ctypes.byref(desc), c.M, flags))
    assert nbytes > 0
    ws = torch.full((nbytes,), poison, device=cuda, dtype=torch.uint8)
    packed = nef.pack(params)
    loss = torch.zeros(1, device=cuda)
    ebuf, lbuf = _guarded(Bn * c.M, cuda), _guarded(Bn, cuda)
    dp, da, ds = torch.full_like(p, float("nan")), torch.full_like(a, float("nan")), torch.full_like(s, float("nan"))
    sop = op.struct()
    head = (ctypes.byref(desc), _ptr(xt), c.N * xt.shape[-1] if xstride is None else xstride, _ptr(p), _ptr(a), _ptr(s), _ptr(packed), _ptr(yt),
            ctypes.byref(sop), _ptr(ow), _ptr(cw))
    e_, l_ = (_ptr(ebuf) if "err" in want else None), (_ptr(lbuf) if "loss_b" in want else None)
    if kind == "fit":
        _lib.launch(cuda, lib.enf_fit_step_a, *head, c.gs if gs is None else gs, _ptr(loss), _ptr(dp), _ptr(da), _ptr(ds), e_, l_, _ptr(ws), nbytes,
                    flags, _stream(cuda))
    else:
        _lib.launch(cuda, lib.enf_eval_loss_a, *head, _ptr(loss) if "loss" in want else None, e_, l_, _ptr(ws), nbytes, flags, _stream(cuda))
    torch.cuda.synchronize()
    return NS(loss=loss, dp=dp, da=da, ds=ds, err=ebuf[:Bn * c.M].view(Bn, c.M), loss_b=lbuf[:Bn], err_guard=ebuf[Bn * c.M:], loss_b_guard=lbuf[Bn:])


def _model(cuda, c, precision, variants=None):
    nef = build_nef(c.cfg, precision)
    if variants is not None:
        nef.pair_variants = variants
    return nef, nef.load_params(c.prm, device=cuda)


def _op_of(c, cuda):
    return SparseObservations.from_coo(c.rows, c.cols, c.vals, c.M, c.N, device=cuda)


def _same_bits(u, v, names=("loss", "dp", "da", "ds", "err", "loss_b")):
    return [n for n in names if not torch.equal(getattr(u, n), getattr(v, n))]


def _check_against_reference(cuda, c, precision, what, variants=None):
    nef, params = _model(cuda, c, precision, variants)
    op = _op_of(c, cuda)
    tol_l, tol_g = TOL[precision]
    fit, ev = _run(cuda, nef, params, c, op), _run(cuda, nef, params, c, op, "eval")
    e_loss = abs(float(fit.loss) - c.ref.loss) / c.ref.loss
    e_ev = abs(float(ev.loss) - c.ref.loss) / c.ref.loss
    e_g = [rel(g.cpu().numpy(), r) for g, r in zip((fit.dp, fit.da, fit.ds), c.ref.g)]
    own = BF16_OPERAND_ROUNDING.get(f"{what} {precision}", {})
    print(f"operators {what} {precision}: loss {e_loss:.2e} eval loss {e_ev:.2e} dp {e_g[0]:.2e} da {e_g[1]:.2e} dsigma {e_g[2]:.2e}"
          + "".join(f" ({k} holds {v:.3e}: twice the rounding build's error)" for k, v in own.items()))
    assert e_loss <= tol_l and e_ev <= tol_l, (e_loss, e_ev)
    assert all(e <= own.get(k, tol_g) for k, e in zip(("dp", "da", "dsigma"), e_g)), e_g
    for r in (fit, ev):
        assert bool(torch.isfinite(r.err).all()) and bool(torch.isfinite(r.loss_b).all())
        assert bool(torch.isnan(r.err_guard).all()) and bool(torch.isnan(r.loss_b_guard).all())
        # err_a and loss_b sum to the loss
        assert abs(float(r.loss_b.double().mean()) - float(r.loss)) <= 1e-5 * float(r.loss)
        assert torch.allclose(r.err.double().sum(1) / (c.M * c.O), r.loss_b.double(), rtol=1e-6, atol=0)
    assert all(bool(torch.isfinite(g).all()) for g in (fit.dp, fit.da, fit.ds))
    assert torch.equal(ev.err, fit.err) and torch.equal(ev.loss_b, fit.loss_b)
    assert np.allclose(fit.loss_b.double().cpu().numpy(), c.ref.loss_b, rtol=LOSS_TOL[precision], atol=0)
    return nef, params, op, fit


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("inv,weights", [("rel_pos_periodic", "obs"), ("rel_pos_periodic", "value"), ("latitude_periodic", "obs")])
def test_fit_step_and_evaluation_match_the_reference(cuda, inv, weights, precision):
    """a ragged operator over N = 50: rows of 1 .. 27 entries with overlaps and one empty row, O = 2, NaN / Inf targets under every zero
    weight; the nef methods give the raw calls' results"""
    c = case(inv, FIT_LENGTHS, 50, weights=weights)
    nef, params, op, fit = _check_against_reference(cuda, c, precision, f"{inv} weights per {weights}")
    t = _t(cuda)
    kw = {"obs_weight" if weights == "obs" else "obs_channel_weight": t(c.w)}
    y = t(poisoned(c.y, c.w))
    loss, dp, da, ds, err, lb = nef.mse_value_and_operator_grads(params, t(c.x), t(c.p), t(c.a), t(c.s), y, op, grad_scale=c.gs,
                                                                 return_errors=True, deterministic=False, **kw)
    lb2, err2 = nef.eval_operator_loss(params, t(c.x), t(c.p), t(c.a), t(c.s), y, op, **kw)
    torch.cuda.synchronize()
    assert torch.equal(err, fit.err) and torch.equal(lb, fit.loss_b) and torch.equal(err2, err) and torch.equal(lb2, lb)
    assert abs(float(loss) - float(fit.loss)) <= 1e-6 * float(fit.loss) and rel(da.cpu().numpy(), fit.da.cpu().numpy()) <= 1e-5
    obs = decode_observations(nef, params, t(c.x), op, t(c.p), t(c.a), t(c.s))
    tau = 2e-5 if precision == "f32" else 3e-2
    assert np.abs(obs.double().cpu().numpy() - c.ref.obs).max() <= tau * np.abs(c.ref.out).max() * np.abs(c.A).sum(1).max()


@pytest.mark.parametrize("variant", ["z_fold", "latent_split"])
def test_equal_groups_agree_with_the_grouped_step(cuda, variant):
    """from_groups with G = 4 and factors q, N = 80, f32: loss and gradients against enf_fit_step_g to 1e-5; and against the sequence
    apply (enf_forward_stages) + operator_mse (enf_mse_value_grad_a) + backward (enf_backward_latents) in deterministic mode, whose
    kernels and order are the fit step's -- equal bits are recorded, 1e-6 is asserted"""
    from tests import cells_ref
    cc = cells_ref.case("rel_pos_periodic", 4, 80)
    nef, params = _model(cuda, cc, "f32", variants=("auto", variant))
    desc = nef._desc(B, 80, Z)
    assert _lib.load().enf_pair_variant(ctypes.byref(desc), 1) == _lib.VARIANT[variant]
    t = _t(cuda)
    q0 = cc.q[0]
    op = SparseObservations.from_groups(np.full(cc.M, 4), q0, device=cuda)
    x, p, a, s, y, w = (t(v) for v in (cc.x, cc.p, cc.a, cc.s, cc.y, cc.w))
    qb = t(np.repeat(q0[None], B, 0))
    grp = nef.mse_value_and_cell_grads(params, x, p, a, s, y, 4, qweight=qb, obs_weight=w, grad_scale=cc.gs, return_errors=True)
    new = nef.mse_value_and_operator_grads(params, x, p, a, s, y, op, obs_weight=w, grad_scale=cc.gs, return_errors=True)
    torch.cuda.synchronize()
    names = ("loss", "dp", "da", "dsigma", "err", "loss_b")
    errs = {n: rel(u.cpu().numpy(), v.cpu().numpy()) for n, u, v in zip(names, new, grp)}
    print(f"operator step against enf_fit_step_g ({variant}): {errs}")
    assert all(e <= 1e-5 for e in errs.values()), errs
    nef.deterministic = True
    one = nef.mse_value_and_operator_grads(params, x, p, a, s, y, op, obs_weight=w, grad_scale=1.0)
    leaves = [v.clone().requires_grad_(True) for v in (p, a, s)]
    loss = nef.operator_mse(nef.apply(params, x, *leaves), y, op, obs_weight=w)
    loss.backward()
    torch.cuda.synchronize()
    comp = (loss.detach().reshape(1), leaves[0].grad, leaves[1].grad, leaves[2].grad)
    bits = {n: torch.equal(u, v.reshape(u.shape)) for n, u, v in zip(names, one, comp)}
    dev = {n: rel(u.cpu().numpy(), v.reshape(u.shape).cpu().numpy()) for n, u, v in zip(names, one, comp)}
    print(f"operator step against forward_stages + mse_value_grad_a + backward_latents ({variant}): equal bits {bits}, deviation {dev}")
    assert all(e <= 1e-6 for e in dev.values()), dev


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("variant", ["z_fold", "latent_split"])
def test_deterministic_mode_gives_equal_bits(cuda, variant, precision):
    """ENF_FIT_DETERMINISTIC: equal bits run to run and over a workspace of 0x00 and 0xFF, with any subset of the optional outputs;
    err_a and loss_b are the same bits in the default mode and in the evaluation"""
    c = case("rel_pos_periodic", FIT_LENGTHS, 50, weights="obs")
    nef, params = _model(cuda, c, precision, variants=("auto", variant))
    op = _op_of(c, cuda)
    one, two = _run(cuda, nef, params, c, op, flags=DET, poison=255), _run(cuda, nef, params, c, op, flags=DET, poison=0)
    again = _run(cuda, nef, params, c, op, flags=DET, poison=255)
    assert _same_bits(one, two) == [] and _same_bits(one, again) == []
    assert all(bool(torch.isfinite(getattr(one, n)).all()) for n in ("loss", "dp", "da", "ds"))
    plain = _run(cuda, nef, params, c, op)
    assert _same_bits(one, plain, ("err", "loss_b")) == []
    ev0, ev1 = _run(cuda, nef, params, c, op, "eval", flags=DET, poison=0), _run(cuda, nef, params, c, op, "eval", flags=DET, poison=255)
    assert _same_bits(ev0, ev1, ("loss", "err", "loss_b")) == [] and _same_bits(one, ev0, ("loss", "err", "loss_b")) == []
    nofit = _run(cuda, nef, params, c, op, flags=DET, want=())
    assert _same_bits(one, nofit, ("loss", "dp", "da", "ds")) == [] and bool(torch.isnan(nofit.err).all())
    only_b = _run(cuda, nef, params, c, op, flags=DET, want=("loss_b",), poison=0)       # loss_b without err_a: allowed, through the workspace
    assert _same_bits(one, only_b, ("loss", "dp", "da", "ds", "loss_b")) == [] and bool(torch.isnan(only_b.err).all())
    ev_b = _run(cuda, nef, params, c, op, "eval", want=("loss_b",))
    assert torch.equal(ev_b.loss_b, one.loss_b) and float(ev_b.loss) == 0.0


def test_zero_weight_rows_do_not_exist(cuda):
    """one more row of weight 0 (for every signal) on two columns no other row references and on column 0, which others do: moving x at
    its own columns, or at a column in no row, changes no bit; moving column 0 changes da"""
    c = case("rel_pos_periodic", FIT_LENGTHS, 50, weights="obs")
    rows = np.append(c.rows, [c.M] * 3)
    cols, vals = np.append(c.cols, [47, 48, 0]), np.append(c.vals, f32([0.7, -0.4, 1.1]))
    assert not np.isin([47, 48, 49], c.cols).any() and (c.cols == 0).any()
    op = SparseObservations.from_coo(rows, cols, vals, c.M + 1, c.N, device=cuda)
    w = np.concatenate([np.maximum(c.w, 0.5), np.zeros((B, 1))], 1)
    y = np.concatenate([c.y, np.full((B, 1, c.O), np.nan)], 1)
    c2 = NS(**{**vars(c), "M": c.M + 1, "w": w, "y": y})
    nef, params = _model(cuda, c2, "f32")
    t = _t(cuda)
    base = _run(cuda, nef, params, c2, op, flags=DET)
    for col, moves in ((47, False), (48, False), (49, False), (0, True)):
        x = t(c.x)
        x[:, col] += 0.3
        got = _run(cuda, nef, params, c2, op, flags=DET, x=x)
        diff = _same_bits(base, got)
        assert (("da" in diff) and ("loss" in diff)) if moves else diff == [], (col, diff)
    assert bool((base.err[:, -1] == 0).all()) and bool(torch.isfinite(base.da).all())


@pytest.mark.parametrize("D,H,Bn,N,Zn,precision", [(128, 2, 2, 144, 9, "f32"), (128, 2, 2, 144, 9, "bf16"), (128, 1, 2, 40, 5, "f32"),
                                                   (64, 4, 2, 40, 5, "f32"), (64, 1, 2, 40, 5, "f32"), (16, 2, 2, 40, 5, "f32")])
def test_other_instantiations(cuda, D, H, Bn, N, Zn, precision):
    """the other (width, heads) of the pair and tail kernels, and one padded width (D = 16)"""
    lengths = FIT_LENGTHS + ([40, 66, 4] if N == 144 else [])
    c = case("rel_pos_periodic", lengths, N, D=D, H=H, weights="obs", Bn=Bn, Zn=Zn)
    _check_against_reference(cuda, c, precision, f"{D}x{H} B={Bn} N={N} Z={Zn}")


def test_stride_zero_grid_equals_the_materialised_one(cuda):
    c = case("rel_pos_periodic", FIT_LENGTHS, 50, weights="value")
    nef, params = _model(cuda, c, "f32")
    op = _op_of(c, cuda)
    t = _t(cuda)
    x0 = t(c.x[0])
    full = _run(cuda, nef, params, c, op, flags=DET, x=x0[None].repeat(B, 1, 1).contiguous())
    shared = _run(cuda, nef, params, c, op, flags=DET, x=x0, xstride=0)
    assert _same_bits(full, shared) == [] and bool(torch.isfinite(full.dp).all())
    ev_full = _run(cuda, nef, params, c, op, "eval", x=x0[None].repeat(B, 1, 1).contiguous())
    ev_shared = _run(cuda, nef, params, c, op, "eval", x=x0, xstride=0)
    assert _same_bits(ev_full, ev_shared, ("err", "loss_b")) == []


# ---- 7. fit_linear_observations
def _loop_problem(cuda, precision):
    C, Zl, steps = 8, 4, 6
    cfg = make_cfg("rel_pos_periodic", D=64, H=2, C=C, O=2)
    prm = R.init_params(7, cfg, jitter=0.1)
    rng = np.random.default_rng(8)
    x, op = cell_operator((-1.0, 1.0, (4, 4)), 3)                        # 16 cells of 9 Gauss points: N = 144
    x64 = f32(x.numpy())
    A = op.to_dense(dtype=np.float32).astype(np.float64)
    cx = x64.reshape(16, 9, 2).mean(1)
    y = np.stack([np.stack([np.sin(2.0 * cx[:, 0] + b) * np.cos(1.5 * cx[:, 1]), 0.5 * cx[:, 0] * cx[:, 1] + 0.1 * b], -1) for b in range(B)])
    y = f32(y + 0.05 * rng.standard_normal(y.shape))
    w = f32(rng.uniform(0.5, 1.5, (B, 16)))
    w[rng.uniform(size=(B, 16)) < 0.2] = 0.0
    lat0 = (f32(R.init_positions_grid(1, Zl, 2) + 0.02 * rng.standard_normal((1, Zl, 2))), f32(1 + 0.1 * rng.standard_normal((1, Zl, C))),
            f32(np.full((1, Zl, 1), 2.0 / 3)))
    lr_p, lr_a = 2.0, np.full((C,), 30.0)                              # (tests/test_gpu_cells.py: the loss falls by about a tenth per step)
    t = _t(cuda)
    nef = build_nef(cfg, precision)
    nef.deterministic = True
    lat0_t = {"p_pos": t(lat0[0]), "a": t(lat0[1]), "gaussian_window": t(lat0[2])}
    lrs = {"p_pos": t([lr_p]), "a": t(lr_a), "gaussian_window": t([0.0])}
    # the same cells for the grouped tail: every group padded from 9 to 16 rows with q = 0 (at the cell's first point)
    xp = np.concatenate([x64.reshape(16, 9, 2), np.repeat(x64.reshape(16, 9, 2)[:, :1], 7, 1)], 1).reshape(256, 2)
    qp = np.concatenate([op.val.numpy().reshape(16, 9), np.zeros((16, 7), dtype=np.float32)], 1).reshape(256)
    return NS(cfg=cfg, prm=prm, x=x64, A=A, y=y, w=w, lat0=lat0, lr=(lr_p, lr_a), steps=steps, nef=nef, params=nef.load_params(prm, device=cuda),
              lat0_t=lat0_t, lrs=lrs, xt=t(x64), op=op.to(cuda), yt=t(y), wt=t(w), xp=t(xp), qp=t(qp))


_LOOP_REF = {}


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_fit_linear_observations_follows_the_reference_loop_and_the_padded_grouped_fit(cuda, precision):
    pb = _loop_problem(cuda, precision)
    if "ref" not in _LOOP_REF:
        _LOOP_REF["ref"] = fit_loop(pb.cfg, pb.prm, pb.x, pb.A, pb.y, pb.w, pb.lat0, pb.lr, pb.steps)
    ref_losses, (rp, ra, _) = _LOOP_REF["ref"]
    y = pb.yt.clone()
    y[pb.wt == 0] = float("nan")
    loss, lat, loss_b = fit_linear_observations(pb.nef, pb.params, pb.lat0_t, pb.lrs, pb.xt, pb.op, y, pb.steps, obs_weight=pb.wt, per_signal_loss=True)
    loss2, lat2 = fit_linear_observations(pb.nef, pb.params, pb.lat0_t, pb.lrs, pb.xt, pb.op, y, pb.steps, obs_weight=pb.wt)
    gl, glat, glb = fit_cell_averages(pb.nef, pb.params, pb.lat0_t, pb.lrs, pb.xp, pb.qp, 16, y, pb.steps, obs_weight=pb.wt, per_signal_loss=True)
    torch.cuda.synchronize()
    tol_l, tol_u = LOOP_TOL[precision]
    got, grouped = loss_b.double().mean(1).cpu().numpy(), glb.double().mean(1).cpu().numpy()
    upd = lambda L: [rel(L[k].double().cpu().numpy() - np.repeat(l0, B, 0), r - np.repeat(l0, B, 0))
                     for k, l0, r in (("p_pos", pb.lat0[0], rp), ("a", pb.lat0[1], ra))]
    print(f"fit_linear_observations {precision}: losses {got.tolist()} padded grouped {grouped.tolist()} reference {ref_losses.tolist()} "
          f"updates {upd(lat)} padded grouped {upd(glat)}")
    assert loss_b.shape == (pb.steps + 1, B) and bool(torch.isfinite(loss_b).all()) and all(bool(torch.isfinite(v).all()) for v in lat.values())
    assert ref_losses[-1] < ref_losses[0] and np.all(np.diff(got) < 0)
    for name, ls, L in (("operator", got, lat), ("padded grouped", grouped, glat)):
        assert np.all(np.abs(ls - ref_losses) <= tol_l * ref_losses), (name, ls, ref_losses)
        assert all(u <= tol_u for u in upd(L)), (name, upd(L))
    # the two routes agree with each other: both lie within the bound of the same reference, so within twice the bound of each other
    assert np.all(np.abs(got - grouped) <= 2 * tol_l * ref_losses)
    assert abs(float(loss) - ref_losses[-1]) <= tol_l * ref_losses[-1]
    assert torch.equal(loss, loss2) and all(torch.equal(lat[k], lat2[k]) for k in lat)


# ---- 8. operator_mse through apply(): the weight-gradient path
def test_operator_mse_weight_gradients_match_the_oracle(cuda):
    """loss and d loss / d (every weight tensor, p, a, sigma) of operator_mse(apply(...)) against fp64 autograd of the oracle: 1e-3 per
    tensor, small tensors measured against the largest (tests/test_gpu_cells_train.py: test_autodecoder_train_step_on_cells)"""
    c = case("rel_pos_periodic", FIT_LENGTHS, 50, weights="value")
    tp = T.to_torch(c.prm, torch.float64, requires_grad=True)
    lv = [torch.tensor(v, requires_grad=True) for v in (c.p, c.a, c.s)]
    out = T.nef_apply(tp, c.cfg, torch.tensor(c.x), *lv)
    obs = torch.einsum("mn,bno->bmo", torch.tensor(c.A), out)
    wt = torch.tensor(c.w)
    dd = torch.where(wt > 0, obs - torch.tensor(c.y), torch.zeros_like(obs))
    lref = (wt * dd * dd).sum() / (B * c.M * c.O)
    get = lambda tree, path: get(tree[path[0]], path[1:]) if path else tree
    leaves = [get(tp["params"], p) for p in TENSOR_PATHS]
    g = torch.autograd.grad(lref, leaves + lv, allow_unused=True)
    nef, params = _model(cuda, c, "f32")
    op = _op_of(c, cuda)
    t = _t(cuda)
    ws = nef.param_tensors(params)
    for v in ws:
        v.requires_grad_(True)
    hl = [t(v).requires_grad_(True) for v in (c.p, c.a, c.s)]
    loss = nef.operator_mse(nef.apply(params, t(c.x), *hl), t(poisoned(c.y, c.w)), op, obs_channel_weight=t(c.w))
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - float(lref.detach())) <= 1e-5 * float(lref.detach())
    gmax = max(float(v.norm()) for v in g[:len(leaves)] if v is not None)
    for path, a_, b_ in zip(TENSOR_PATHS, ws, g[:len(leaves)]):
        if b_ is None or path[-1] == "coefficients":
            assert a_.grad is None or float(a_.grad.abs().max()) == 0
            continue
        nb = float(b_.norm())
        e = float((a_.grad.cpu().double() - b_).norm()) / (nb if nb > 1e-3 * gmax else gmax)
        assert e < 1e-3, ("/".join(path), e)
    for name, h, b_ in zip(("p", "a", "sigma"), hl, g[len(leaves):]):
        assert float((h.grad.cpu().double() - b_).norm() / b_.norm()) < 1e-3, name
