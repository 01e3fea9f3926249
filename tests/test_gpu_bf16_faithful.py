"""The bf16 instantiations against a reference that rounds where they round.

The fp64 oracle does not round its operands, so the bf16 bounds of the other files (3e-2 forward, 7e-2 latent gradients, 3e-2 .. 2e-1
weight gradients) are the size of bf16 operand rounding and a bf16-only defect below that noise passes them.  Here every case is
evaluated three times --

  oracle   oracle/enf_ref_np.py / enf_ref_torch.py in fp64
  f32r     precision="f32" through libenf_hip_f32r.so (csrc/Makefile, -DENF_F32_ROUNDED=1): the fp32 instantiations -- fp32 layouts,
           v_mfma_f32_16x16x4_f32, compiler-scheduled GEMMs -- with every value rounded to bf16 that the bf16 instantiations hold as bf16
           ("Rounding sites"); tests/test_gpu_layout.py shows that its conversion is the bf16 kernels' bit for bit
  bf16     precision="bf16" through the product library

-- under the same forced pair-kernel variant on both sides (the folds move the rounding points), plus once through the plain f32 library.
With |.| the L2 norm over a tensor and o, f, r, b the four results:

  reference-only conditions   E_f = |f - o| / |o| inside the f32 tolerance of the file that owns the quantity, and
                              E_r = |r - o| / |o| >= 20 E_f: the rounding is on
  the assertions              |b - r| / |o| <= E_r / R per tensor;
                              for the worst single row (a query of an output, tangent or query gradient; a latent of a latent
                              gradient), max_row |b - r|_row / rms_row |o|_row <= E_r,row / R_ROW, E_r,row the same statistic of r - o;
                              for tensors with one row per query, the same with the MEDIAN row and R_MEDIAN = 20

R starts at 5: a CPU model of the chain (8 stages of 128 x 128 GEMMs with gelu, bf16 operands, fp32 sums) puts the residual of two
summation orders 20 times below the rounding error, and 5 leaves 4x for the number of re-rounded activations that flip by one ulp, which
varies with seed and device.  R_ROW starts at 2: in the same model the flips put the MAXIMUM of the residual only 2-3 times below the
rounding noise, and a worst row is a maximum over rows; 2 is the smallest ratio that still says "below the rounding noise".  E_r is
measured in the test from the two references.  Every figure is printed before anything is asserted.

What the MI355X showed (profiles/bf16_faithful.json: E_r / residual of every case and tensor; DESIGN.md, "bf16 against f32r").  The
smallest ratios are 3 - 8 at the 128-wide, two-head shape and 10 - 30 at the 64-wide ones, not 20 throughout.  The residual was traced
before any ratio was touched: between the two paths lse agrees to fp32 rounding (median difference 0), ybar to 1e-7 of its row norm in
the median row and 1e-5 .. 9e-5 in L2, and `out` to 4e-8 .. 8e-8 in the MEDIAN row -- while 1 % (64 x 2) to 21 % (128 x 2) of the
rows of `out` differ by 1e-3 .. 1e-2.  No rounding site is unmatched (one would move every row by about 4e-3).  What remains is the
flip the model knew, and its cascade, which the model did not have: an fp32-rounding difference lets one activation round to the other
neighbour, that ulp (4e-3) moves every output of the next GEMM by 3e-4 relative, about a tenth of THOSE then round the other way, and
the rest of that column's chain -- above all the tail, H D = 256 wide with five rounding stages per query -- carries rounding-sized noise of
its own.  The share of rows with a first flip grows with D and H D; it is a property of comparing two summation orders and cannot be
reduced from either side.  Hence, by the rule the work was specified with, per class (kind of call / tensor class / shape row):
  smallest recorded ratio >= 15      R = 5 stands (>= 6: R_ROW = 2 stands)
  lower, the difference traced       a third of the smallest recorded ratio
  that third below 2                 "not achieved": printed and recorded, NOT asserted with a loose bound -- R_CLASS holds None
and the median row carries what the flips take from the other two statistics: a row that no flip touched differs by fp32 summation
noise, four orders below the rounding error (measured ratio >= 4e4), so the model's healthy ratio applies in full, R_MEDIAN = 20, as long
as fewer than half of the rows carry a flip (measured: at most 21 %).  A bf16-only defect that moves every row -- a conversion that
truncates, a scaled operand row -- moves the median row; the flips do not.

Smallest recorded ratios per class (MI355X; cases = figures in the class; R / R_ROW as asserted, - = not achieved or no such statistic):
  class                                                    n  E_r/res      R      row  R_ROW     median
  forward / out / 128x2                                   27     3.08      -     1.72      -   4.24e+04
  forward / out / 64x2                                     9    10.55   3.52      2.5      -   1.38e+05
  forward / out / 128x1                                    3     7.94   2.65     2.62      -   9.68e+04
  forward / out / 64x1                                     3     9.92   3.31     4.24      -    1.2e+05
  forward / out / 64x4                                     3     6.54   2.18     2.23      -   1.33e+05
  latent gradients / dp / 128x2                            4    16.68      5     16.7      2          -
  latent gradients / da / 128x2                            4     6.10   2.03     4.82      -          -
  latent gradients / dwindow / 128x2                       4    11.79   3.93     16.5      2          -
  latent gradients / dx / 128x2                            4    20.38      5     17.3      2   5.59e+04
  latent gradients / dp / 64x2                             2    45.03      5     45.6      2          -
  latent gradients / da / 64x2                             2    22.03      5     13.1      2          -
  latent gradients / dwindow / 64x2                        2    33.42      5     21.9      2          -
  latent gradients / dx / 64x2                             2    39.74      5     24.2      2   1.14e+05
  latent gradients / dp / 128x1                            2    15.16      5     14.9      2          -
  latent gradients / da / 128x1                            2    12.97   4.32     9.21      2          -
  latent gradients / dwindow / 128x1                       2    16.89      5     14.2      2          -
  latent gradients / dx / 128x1                            2    13.74   4.58       12      2   7.04e+04
  latent gradients / dp / 64x1                             2    18.22      5     15.2      2          -
  latent gradients / da / 64x1                             2    31.01      5     26.5      2          -
  latent gradients / dwindow / 64x1                        2    53.19      5     27.7      2          -
  latent gradients / dx / 64x1                             2    26.25      5       10      2   1.39e+05
  latent gradients / dp / 64x4                             2    15.05      5     12.9      2          -
  latent gradients / da / 64x4                             2     8.61   2.87     4.14      -          -
  latent gradients / dwindow / 64x4                        2    13.07   4.36     14.8      2          -
  latent gradients / dx / 64x4                             2    22.21      5     20.8      2    9.4e+04
  fit step / dp / 128x2                                   13     9.63   3.21      8.4      2          -
  fit step / da / 128x2                                   13     5.43      -     2.69      -          -
  fit step / dwindow / 128x2                              13     5.06      -     4.59      -          -
  weight gradients / weights, other / 128x2               66     5.96      -        -      -          -
  weight gradients / weights, query relu layer / 128x2     4    30.33      5        -      -          -
  weight gradients / weights, query branch / 128x2        12     7.01   2.34        -      -          -
  weight gradients / weights, value relu layer / 128x2     4    21.84      5        -      -          -
  weight gradients / dp / 128x2                            2    16.08      5        -      -          -
  weight gradients / da / 128x2                            2     8.61   2.87        -      -          -
  weight gradients / dwindow / 128x2                       2     7.68   2.56        -      -          -
  weight gradients / weights, other / 64x2                66    27.03      5        -      -          -
  weight gradients / weights, query relu layer / 64x2      4   287.23      5        -      -          -
  weight gradients / weights, query branch / 64x2         12   102.53      5        -      -          -
  weight gradients / weights, value relu layer / 64x2      4    40.70      5        -      -          -
  weight gradients / dp / 64x2                             2    38.67      5        -      -          -
  weight gradients / da / 64x2                             2    35.32      5        -      -          -
  weight gradients / dwindow / 64x2                        2   125.61      5        -      -          -
  tangent / tan / 128x2                                    1    17.71      5     22.7      2   1.83e+05
  tangent / tan with xdot / 128x2                          1    10.54   3.51     8.54      2   1.26e+05
  tangent / out / 128x2                                    1     7.85   2.62     1.72      -   1.83e+05
  gn product / gp / 128x2                                  1     8.07   2.69      4.8      -          -
  gn product / ga / 128x2                                  1     9.58   3.19     6.41      2          -
  gn product / gwindow / 128x2                             1     7.71   2.57     10.9      2          -
  tangent / tan / 64x1                                     1    29.93      5     13.1      2   1.84e+05
  tangent / tan with xdot / 64x1                           1    56.72      5       34      2   2.97e+05
  tangent / out / 64x1                                     1    30.88      5     6.04      2    1.2e+05
  gn product / gp / 64x1                                   1    22.24      5     16.4      2          -
  gn product / ga / 64x1                                   1    29.09      5     33.1      2          -
  gn product / gwindow / 64x1                              1    32.00      5     32.9      2          -"""
import contextlib
import ctypes
import re

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from tests import ffn_ref
from tests.helpers import make_cfg, make_inputs, build_nef
from tests.test_gpu_forward import TOL as FWD_TOL
from tests.test_gpu_backward import TOL as GRAD_TOL
from tests.test_gpu_weight_grads import TOL as WGRAD_TOL, ref as oracle_weight_grads
from tests.test_gpu_weighted_fit import LOSS_TOL
from tests.test_gpu_tangent_x import TOL as TAN_TOL
from tests.test_gpu_gn import TOL as GN_TOL
from enf_pde_amd import _lib
from enf_pde_amd.enf.models import TENSOR_PATHS

pytestmark = pytest.mark.gpu

R_START, R_ROW_START, R_MEDIAN, ON = 5.0, 2.0, 20.0, 20.0
# (R, R_ROW) per class, by the rule of this file's docstring from the smallest ratios recorded on MI355X (profiles/bf16_faithful.json);
# None: the class would need a ratio below 2 -- "not achieved": its figures are printed and recorded, not asserted loosely.
# A class that is not listed starts at (R_START, R_ROW_START).
R_CLASS = {
    "forward / out / 128x2": (None, None),
    "forward / out / 64x2": (3.52, None),
    "forward / out / 128x1": (2.65, None),
    "forward / out / 64x1": (3.31, None),
    "forward / out / 64x4": (2.18, None),
    "latent gradients / da / 128x2": (2.03, None),
    "latent gradients / dwindow / 128x2": (3.93, 2.0),
    "latent gradients / da / 128x1": (4.32, 2.0),
    "latent gradients / dx / 128x1": (4.58, 2.0),
    "latent gradients / da / 64x4": (2.87, None),
    "latent gradients / dwindow / 64x4": (4.36, 2.0),
    "fit step / dp / 128x2": (3.21, 2.0),
    "fit step / da / 128x2": (None, None),
    "fit step / dwindow / 128x2": (None, None),
    "weight gradients / weights, other / 128x2": (None, None),
    "weight gradients / weights, query branch / 128x2": (2.34, None),
    "weight gradients / da / 128x2": (2.87, None),
    "weight gradients / dwindow / 128x2": (2.56, None),
    "tangent / tan with xdot / 128x2": (3.51, 2.0),
    "tangent / out / 128x2": (2.62, None),
    "gn product / gp / 128x2": (2.69, None),
    "gn product / ga / 128x2": (3.19, 2.0),
    "gn product / gwindow / 128x2": (2.57, 2.0),
}
# tensors with one row per QUERY: a flip stays inside its row, so the median row is free of flips (see the docstring)
QUERY_ROWS = {"out", "out written", "out read", "tan", "tan with xdot", "dx"}
# d loss / d (bias of the last layer) = sum of d out over the queries: no rounded operand enters it, in any precision
UNROUNDED = {"out_proj/layers_4/bias"}
SHAPE_ROWS = [(128, 2), (64, 2), (128, 1), (64, 1), (64, 4)]           # ENF_SHAPES (csrc/enf_layout.h)
_ORACLE = {}


def _once(key, fn):
    """an oracle result, computed once per session and never modified"""
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


def _np(t):
    return t.detach().double().cpu().numpy()


def _three(build, run):
    """run(nef, params) -> {name: fp64 array} through the plain f32 library, the f32r library and the bf16 product kernels;
    build(precision) -> (nef, params) is called inside the library's scope: the packed panels are that library's"""
    res = {}
    for tag, prec, lib in (("f32", "f32", None), ("f32r", "f32", _lib.load_f32r()), ("bf16", "bf16", None)):
        with (_lib.using(lib) if lib is not None else contextlib.nullcontext()):
            nef, params = build(prec)
            res[tag] = run(nef, params)
            torch.cuda.synchronize()
    return res


def _rows(v):
    """per-row L2 norms (rows: all but the last axis)"""
    return np.linalg.norm(v.reshape(-1, v.shape[-1]), axis=1)


def _class(what, name):
    """the class a figure is recorded and bounded under: kind of call / tensor class / shape row.  The 46 weight tensors form the four
    groups of tests/test_gpu_bf16_contract.py; the shape row is part of the class because the share of rows that carry a flip grows
    with the widths D and H D (see the docstring)."""
    kind = next(k for k in ("forward", "latent gradients", "fit step", "weight gradients", "tangent", "gn product") if what.startswith(k))
    if "/" in name:
        name = "weights, query relu layer" if "invariant_embedding_query" in name and "layers_0" in name else \
               "weights, value relu layer" if "invariant_embedding_value" in name and "layers_0" in name else \
               "weights, query branch" if any(k in name for k in ("invariant_embedding_query", "inv_emb_to_q", "a_to_k")) else "weights, other"
    elif name.startswith("out"):
        name = "out"
    return f"{kind} / {name} / {re.search(r'[0-9]+x[0-9]', what).group(0)}"


def _judge(what, oracle, res, f32_tol, rows=True, f32_max_norm=False, skip=()):
    """Print the figures of every tensor of a case, then assert the reference-only conditions and the bf16 bounds."""
    bad = []
    gmax = max(np.linalg.norm(o) for o in oracle.values())
    for name, o in oracle.items():
        f, r, b = res["f32"][name], res["f32r"][name], res["bf16"][name]
        assert f.shape == o.shape == r.shape == b.shape, (what, name, f.shape, o.shape)
        no = np.linalg.norm(o)
        if name in skip or no <= 1e-6 * gmax:
            print(f"bf16-faithful | {what} | {name} | skipped (|o| = {no:.3e})")
            continue
        finite = all(np.isfinite(v).all() for v in (f, r, b))
        e_f = np.abs(f - o).max() / np.abs(o).max() if f32_max_norm else np.linalg.norm(f - o) / no
        e_r, d = np.linalg.norm(r - o) / no, np.linalg.norm(b - r) / no
        if name in UNROUNDED:           # nothing to round: all three agree with the oracle to fp32 accuracy
            print(f"bf16-faithful | {what} | {name} | unrounded | E_f {e_f:.3e} | f32r {e_r:.3e} | bf16 - f32r {d:.3e}")
            if not (finite and max(e_f, e_r, d) < f32_tol):
                bad.append((name, "a tensor without rounded operands is off", e_f, e_r, d))
            continue
        R, R_ROW = R_CLASS.get(_class(what, name), (R_START, R_ROW_START))
        line = f"bf16-faithful | {what} | {name} | E_f {e_f:.3e} | E_r {e_r:.3e} | residual {d:.3e} | ratio {e_r / max(d, 1e-300):.2f}"
        if rows:
            rms = np.sqrt(np.mean(_rows(o) ** 2))
            er_rows, d_rows = _rows(r - o) / rms, _rows(b - r) / rms
            er_row, d_row = er_rows.max(), d_rows.max()
            line += f" | E_r,row {er_row:.3e} | residual,row {d_row:.3e} | ratio,row {er_row / max(d_row, 1e-300):.2f}"
            if name in QUERY_ROWS:
                er_med, d_med = np.median(er_rows), np.median(d_rows)
                line += f" | E_r,median {er_med:.3e} | residual,median {d_med:.3e} | ratio,median {er_med / max(d_med, 1e-300):.2f}"
        print(line + f" | R {R} R_ROW {R_ROW if rows else None}")
        if not finite:
            bad.append((name, "not finite"))
        if not e_f < f32_tol:
            bad.append((name, "plain f32 outside its tolerance", e_f, f32_tol))
        if not e_r >= ON * e_f:
            bad.append((name, "f32r is not rounding: E_r < 20 E_f", e_r, e_f))
        if R is not None and not d <= e_r / R:
            bad.append((name, "bf16 - f32r above E_r / R", d, e_r / R))
        if rows and R_ROW is not None and not d_row <= er_row / R_ROW:
            bad.append((name, "worst row of bf16 - f32r above E_r,row / R_ROW", d_row, er_row / R_ROW))
        if rows and name in QUERY_ROWS and not d_med <= er_med / R_MEDIAN:
            bad.append((name, "median row of bf16 - f32r above E_r,median / R_MEDIAN", d_med, er_med / R_MEDIAN))
    assert not bad, (what, bad)


def _t(cuda):
    return lambda v, g=False: torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda, requires_grad=g)


def _f32(v):
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def _builder(cuda, cfg, prm, ffn=False, variants=None, deterministic=None):
    def build(precision):
        nef = (ffn_ref.build_nef_ffn if ffn else build_nef)(cfg, precision)
        if variants is not None:
            nef.pair_variants = variants
        if deterministic is not None:
            nef.deterministic = deterministic
        return nef, nef.load_params(prm, device=cuda)
    return build


# ------------------------------------------------------------------------------------------------ forward
def _fwd_case(inv, D, H, B, N, Z, ffn=False, C=12, O=2, freq=(0.3, 0.6)):
    """weights, fp32-rounded inputs and the oracle's output (the caller has patched the oracle's embedding for ffn)"""
    def make():
        cfg = make_cfg(inv, D=D, H=H, C=C, O=O, freq=freq)
        prm = (ffn_ref.init_params_ffn if ffn else R.init_params)(D + Z, cfg, jitter=0.1)
        x, p, a, s = (_f32(v) for v in make_inputs(cfg, B, N, Z, D + Z + 1))
        return cfg, prm, (x, p, a, s), R.nef_apply(prm, cfg, x, p, a, s)
    return _once(("fwd", inv, D, H, B, N, Z, ffn, C, O, freq), make)


FWD_CASES = [("rel_pos_periodic", D, H, 2, 70, 9) for D, H in SHAPE_ROWS] + \
            [("latitude_periodic", 128, 2, 2, 70, 9), ("polar_periodic", 128, 2, 2, 70, 9), ("ponita", 64, 2, 2, 70, 9),   # enf_spec_rule
             ("rel_pos", 128, 2, 2, 70, 9),                     # a run-time invariant
             ("ball", 64, 2, 2, 70, 9),
             ("rel_pos_periodic", 128, 2, 3, 130, 20)]          # a forced split z-fold run crosses a tile boundary


@pytest.mark.parametrize("inv,D,H,B,N,Z", FWD_CASES)
def test_forward(cuda, pair_variant, inv, D, H, B, N, Z):
    cfg, prm, (x, p, a, s), ref = _fwd_case(inv, D, H, B, N, Z)
    t = _t(cuda)

    ran = []

    def run(nef, params):
        ran.append(int(_lib.load().enf_pair_variant(ctypes.byref(nef._desc(B, N, Z)), 0)))
        return {"out": _np(nef.apply(params, t(x), t(p, True), t(a), t(s)))}      # (a latent that wants a gradient: no bf16 hand-off)
    res = _three(_builder(cuda, cfg, prm), run)
    assert ran == [_lib.VARIANT[pair_variant]] * 3, (pair_variant, ran)            # the forced variant, on all three sides
    _judge(f"forward {inv} {D}x{H} {(B, N, Z)} {pair_variant}", {"out": ref}, res, FWD_TOL["f32"], f32_max_norm=True)


def test_forward_ffn(cuda, pair_variant, monkeypatch):
    monkeypatch.setattr(R, "rff_net", ffn_ref.ffn_net_np)
    cfg, prm, (x, p, a, s), ref = _fwd_case("rel_pos_periodic", 128, 2, 2, 70, 9, ffn=True)
    t = _t(cuda)
    run = lambda nef, params: {"out": _np(nef.apply(params, t(x), t(p, True), t(a), t(s)))}
    _judge(f"forward ffn 128x2 {pair_variant}", {"out": ref}, _three(_builder(cuda, cfg, prm, ffn=True), run), FWD_TOL["f32"], f32_max_norm=True)


def test_forward_inside_relu_masks(cuda, pair_variant):
    """the MASKS instantiations: a forward that writes the relu masks and one that reads them back at the same point, where the
    linearised relu is the relu"""
    B, N, Z = 2, 70, 9
    cfg, prm, (x, p, a, s), ref = _fwd_case("rel_pos_periodic", 128, 2, B, N, Z)
    t = _t(cuda)

    def run(nef, params):
        buf = nef.relu_mask_buffer(B, N, Z, cuda).zero_()
        with torch.no_grad():
            with nef.relu_masks(buf, "write", B):
                w = _np(nef.apply(params, t(x), t(p), t(a), t(s)))
            with nef.relu_masks(buf, "read", B):
                r = _np(nef.apply(params, t(x), t(p), t(a), t(s)))
        return {"out written": w, "out read": r}
    _judge(f"forward relu masks 128x2 {pair_variant}", {"out written": ref, "out read": ref}, _three(_builder(cuda, cfg, prm), run),
           FWD_TOL["f32"], f32_max_norm=True)


def test_forward_with_the_bf16_hand_off(cuda, pair_variant):
    """a no_grad decode: ENF_STAGE_YBAR_HALF is set, the bf16 pair kernel hands ybar to the tail as bf16 (the split z-fold ignores it)"""
    B, N, Z = 2, 70, 9
    cfg, prm, (x, p, a, s), ref = _fwd_case("rel_pos_periodic", 128, 2, B, N, Z)
    t = _t(cuda)
    flags = []

    def run(nef, params):
        lib = _lib.load()
        orig = lib.enf_forward_stages

        class Spy:
            def __call__(self, *args):
                flags.append(int(args[-2]))
                return orig(*args)
        try:
            lib.enf_forward_stages = Spy()
            with torch.no_grad():
                return {"out": _np(nef.apply(params, t(x), t(p), t(a), t(s)))}
        finally:
            lib.enf_forward_stages = orig
    res = _three(_builder(cuda, cfg, prm), run)
    print("bf16-faithful | hand-off | stages of the three forwards", flags)
    assert len(flags) == 3 and all(f & _lib.ENF_STAGE_YBAR_HALF for f in flags)
    _judge(f"forward bf16 hand-off 128x2 {pair_variant}", {"out": ref}, res, FWD_TOL["f32"], f32_max_norm=True)


# ------------------------------------------------------------------------------------------------ latent and query gradients
def _grad_case(D, H, B=2, N=70, Z=9, O=2, C=12):
    def make():
        cfg = make_cfg("rel_pos_periodic", D=D, H=H, C=C, O=O, freq=(0.3, 0.6))
        prm = R.init_params(D + Z, cfg, jitter=0.1)
        x, p, a, s = (_f32(v) for v in make_inputs(cfg, B, N, Z, D + Z + 1))
        w = _f32(np.random.default_rng(D + Z + 2).standard_normal((B, N, O)))
        tp = T.to_torch(prm, torch.float64)
        tx, tpp, ta, ts = (torch.tensor(v, requires_grad=True) for v in (x, p, a, s))
        (T.nef_apply(tp, cfg, tx, tpp, ta, ts) * torch.tensor(w)).sum().backward()
        return cfg, prm, (x, p, a, s, w), {"dp": tpp.grad.numpy(), "da": ta.grad.numpy(), "dwindow": ts.grad.numpy(), "dx": tx.grad.numpy()}
    return _once(("grad", D, H, B, N, Z, O, C), make)


def _grads(cuda, D, H, bwd_variant, deterministic=None):
    cfg, prm, (x, p, a, s, w), ref = _grad_case(D, H)
    t = _t(cuda)

    def run(nef, params):
        tp, ta, ts = t(p, True), t(a, True), t(s, True)
        (nef.apply(params, t(x), tp, ta, ts) * t(w)).sum().backward()            # enf_backward_latents
        tx = t(x, True)
        (nef.apply(params, tx, t(p), t(a), t(s)) * t(w)).sum().backward()        # the training path, query gradient
        return {"dp": _np(tp.grad), "da": _np(ta.grad), "dwindow": _np(ts.grad), "dx": _np(tx.grad)}
    what = f"latent gradients {D}x{H} {bwd_variant}" + (" deterministic" if deterministic else "")
    _judge(what, ref, _three(_builder(cuda, cfg, prm, deterministic=deterministic), run), GRAD_TOL["f32"])


@pytest.mark.parametrize("D,H", SHAPE_ROWS)
def test_latent_and_query_gradients(cuda, bwd_variant, D, H):
    _grads(cuda, D, H, bwd_variant)


def test_latent_and_query_gradients_deterministic(cuda, bwd_variant):
    _grads(cuda, 128, 2, bwd_variant, deterministic=True)


# ------------------------------------------------------------------------------------------------ the fused inner step
def _fit_case(kind, D=128, H=2, B=5, N=40, Z=9, O=2, C=12):
    """kind: "w" (per-point weights), "cw" (per-channel weights), "shared" (every signal holds signal 0's latents and points)"""
    def make():
        cfg = make_cfg("rel_pos_periodic", D=D, H=H, C=C, O=O, freq=(0.3, 0.6))
        prm = R.init_params(D + Z, cfg, jitter=0.1)
        x, p, a, s = (_f32(v) for v in make_inputs(cfg, B, N, Z, D + Z + 1))
        if kind == "shared":
            x, p, a, s = (np.repeat(v[:1], B, 0) for v in (x, p, a, s))
        rng = np.random.default_rng(D + Z + 2)
        y = _f32(rng.standard_normal((B, N, O)))
        w = _f32(rng.uniform(0.2, 2, (B, N, O) if kind == "cw" else (B, N)))
        tp = T.to_torch(prm, torch.float64)
        tpp, ta, ts = (torch.tensor(v, requires_grad=True) for v in (p, a, s))
        out = T.nef_apply(tp, cfg, torch.tensor(x), tpp, ta, ts)
        loss = (torch.tensor(w if kind == "cw" else w[..., None]) * (out - torch.tensor(y)) ** 2).mean()
        (B * loss).backward()
        return cfg, prm, (x, p, a, s, y, w), {"loss": loss.detach().numpy().reshape(1), "dp": tpp.grad.numpy(), "da": ta.grad.numpy(),
                                              "dwindow": ts.grad.numpy()}
    return _once(("fit", kind, D, H, B, N, Z, O, C), make)


def _fit(cuda, kind, variants, what):
    from enf_pde_amd.enf import models as M
    assert M.FUSED_FIT_STEP
    B, N, Z = 5, 40, 9
    cfg, prm, (x, p, a, s, y, w), ref = _fit_case(kind, O=1 if kind == "shared" else 2)
    t = _t(cuda)

    def run(nef, params):
        if kind == "shared":            # the shared forward and the one backward for all signals run (O = 1, latent-split forward, z-fold backward)
            assert _lib.load().enf_shared_backward_applies(ctypes.byref(nef._desc(B, N, Z)), _lib.ENF_FIT_SHARED_LATENTS) == 1
        tx = t(x[0])[None].expand(B, -1, -1) if kind == "shared" else t(x)
        loss, dp, da, ds = nef.mse_value_and_latent_grads(params, tx, t(p), t(a), t(s), t(y), grad_scale=float(B),
                                                          weight=t(w) if kind != "cw" else None, channel_weight=t(w) if kind == "cw" else None,
                                                          shared_latents=kind == "shared")
        return {"loss": _np(loss), "dp": _np(dp), "da": _np(da), "dwindow": _np(ds)}
    res = _three(_builder(cuda, cfg, prm, variants=variants), run)
    # the loss is one number: its error against the oracle is a difference of near-equal sums, not a rounding level to take a ratio of
    # -- it is held to the loss tolerances of tests/test_gpu_weighted_fit.py in all three evaluations and printed
    for tag, tol in (("f32", LOSS_TOL["f32"]), ("f32r", LOSS_TOL["bf16"]), ("bf16", LOSS_TOL["bf16"])):
        e = abs(float(res[tag]["loss"][0]) - float(ref["loss"][0])) / max(1.0, float(ref["loss"][0]))
        print(f"bf16-faithful | fit step {what} | loss {tag} | error {e:.3e} (bound {tol:.1e})")
        assert e < tol, (kind, tag, e)
    _judge(f"fit step {what} 128x2 {(B, N, Z)}", ref, res, GRAD_TOL["f32"], skip=("loss",))


@pytest.mark.parametrize("kind", ["w", "cw"])
def test_fit_step(cuda, kind, pair_variant, bwd_variant):
    _fit(cuda, kind, None, f"{kind} {pair_variant} {bwd_variant}")


def test_fit_step_shared_latents(cuda):
    _fit(cuda, "shared", ("latent_split", "z_fold"), "shared latents")


# ------------------------------------------------------------------------------------------------ all 46 weight gradients
def _wgrad_case(D, H, B=3, N=100, Z=16):
    def make():
        cfg = make_cfg("rel_pos_periodic", D=D, H=H, C=16, O=1)
        prm = R.init_params(D + Z, cfg, jitter=0.1)
        x, p, a, s = (_f32(v) for v in make_inputs(cfg, B, N, Z, D + Z + 1))
        w = _f32(np.random.default_rng(D + Z + 2).standard_normal((B, N, 1)))
        _, rg, rp, ra, rs = oracle_weight_grads(prm, cfg, x, p, a, s, w)
        ref = {"/".join(path): g for path, g in zip(TENSOR_PATHS, rg)}
        ref.update({"dp": rp, "da": ra, "dwindow": rs})
        return cfg, prm, (x, p, a, s, w), ref
    return _once(("wgrad", D, H, B, N, Z), make)


@pytest.mark.parametrize("D,H", [(128, 2), (64, 2)])
def test_weight_gradients(cuda, bwd_variant, D, H):
    cfg, prm, (x, p, a, s, w), ref = _wgrad_case(D, H)
    t = _t(cuda)

    def run(nef, params):
        ts_ = nef.param_tensors(params)
        for v in ts_:
            v.requires_grad_(True)
        tp, ta, tsg = t(p, True), t(a, True), t(s, True)
        (nef.apply(params, t(x), tp, ta, tsg) * t(w)).sum().backward()           # enf_backward_all
        g = lambda v: np.zeros(tuple(v.shape)) if v.grad is None else _np(v.grad)
        out = {"/".join(path): g(v) for path, v in zip(TENSOR_PATHS, ts_)}
        out.update({"dp": g(tp), "da": g(ta), "dwindow": g(tsg)})
        return out
    res = _three(_builder(cuda, cfg, prm), run)
    frozen = [k for k in ref if k.endswith("coefficients")]                      # stop_gradient (rff.py:87-90)
    for k in frozen:
        assert all(np.all(res[tag][k] == 0) for tag in res) and np.all(ref[k] == 0), k
    _judge(f"weight gradients {D}x{H} (3, 100, 16) {bwd_variant}", ref, res, WGRAD_TOL["f32"], rows=False, skip=frozen)


# ------------------------------------------------------------------------------------------------ forward mode and Gauss-Newton
def _tan_case(D, H):
    from tests.tangent_ref import case
    from tests.tangent_x_ref import oracle_jvp_x
    cfg, prm, xpas, tang, out_ref, tan_ref = case("rel_pos_periodic", D=D, H=H)

    def make():
        x, p, a, s = xpas
        xd = 0.5 * np.random.default_rng(D + H).standard_normal(x.shape)
        _, tan_x = oracle_jvp_x(cfg, prm, x, p, a, s, xd, *tang)
        # Gauss-Newton product: 2 / (B N O) J^T J v, by one jvp and one vjp of the oracle
        tp = T.to_torch(prm, torch.float64)
        prim = tuple(torch.tensor(v, requires_grad=True) for v in (p, a, s))
        out = T.nef_apply(tp, cfg, torch.tensor(x), *prim)
        g = torch.autograd.grad(out, prim, grad_outputs=torch.tensor(tan_ref) * (2.0 / tan_ref.size))
        return xd, tan_x, {"gp": g[0].numpy(), "ga": g[1].numpy(), "gwindow": g[2].numpy()}
    return (cfg, prm, xpas, tang, out_ref, tan_ref) + _once(("tan", D, H), make)


@pytest.mark.parametrize("D,H", [(128, 2), (64, 1)])
def test_tangent_and_gauss_newton(cuda, D, H):
    cfg, prm, (x, p, a, s), (dp, da, ds), out_ref, tan_ref, xd, tan_x_ref, gn_ref = _tan_case(D, H)
    t = _t(cuda)

    def run(nef, params):
        out, tan = nef.tangent(params, t(x), t(p), t(a), t(s), dp=t(dp), da=t(da), dwindow=t(ds))
        _, tan_x = nef.tangent(params, t(x), t(p), t(a), t(s), dp=t(dp), da=t(da), dwindow=t(ds), xdot=t(xd), return_out=False)
        gp, ga, gw = nef.gn_product(params, t(x), t(p), t(a), t(s), vp=t(dp), va=t(da), vwindow=t(ds))
        return {"out": _np(out), "tan": _np(tan), "tan with xdot": _np(tan_x), "gp": _np(gp), "ga": _np(ga), "gwindow": _np(gw)}
    res = _three(_builder(cuda, cfg, prm), run)
    fwd = {"out": out_ref, "tan": tan_ref, "tan with xdot": tan_x_ref}
    failed = []
    for args, kw in (((f"tangent {D}x{H}", {k: fwd[k] for k in ("tan", "tan with xdot")}, res, TAN_TOL["f32"]), {}),
                     ((f"tangent {D}x{H} decode", {"out": out_ref}, res, FWD_TOL["f32"]), dict(f32_max_norm=True)),
                     ((f"gn product {D}x{H}", gn_ref, res, GN_TOL["f32"]), {})):
        try:                            # (every group's figures are printed before the first failure is raised)
            _judge(*args, **kw)
        except AssertionError as e:
            failed.append(e)
    assert not failed, failed
