"""Cost of the Gauss-Newton product on a sparse observation operator (include/enf_hip.h, "Gauss-Newton product on sparse observations")
at the bench's FIT shape: 16 signals, 64 latents, D = 128, H = 2, O = 1, in bf16 and f32, for three operators shared by the signals:
  g4     128 groups of 4 consecutive rows (SparseObservations.from_groups), N = 512
  3x3    56 cells with a 3 x 3 Gauss rule, N = 504
  rays   4 rays of 128 Gauss nodes (line_integrals), N = 512: rows that take the wave form

Interleaved rounds on one box, hipEvent pairs on the launch stream, median of single calls after a warm-up; every round is recorded,
and every round first runs all its routes untimed (--settle calls each; scripts/bench_operators.py has the reason).
  product_a_<op>         nef.gn_operator_product (enf_gn_product_a) without and with the reuse of the point (ENF_GN_REUSE_POINT)
  composed_<op>          the same product by hand from shipped calls, one synchronisation at the end: nef.tangent, enf_obs_apply, the
                         weights in torch, the transposed product (enf_obs_apply on the CSC), the latent backward of nef.apply
  product_g              nef.gn_cell_product (enf_gn_product_g) at G = 4 on the rows, factors and weights of g4: the fused grouped tail
  lm_step_cg8_<op>       one step of lm_fit_linear_observations with eight CG iterations (fit step, eight products, one evaluation)
The one requirement is product_a <= composed; the ratio to product_g is reported.

Prints one JSON line; --out FILE also writes it there (profiles/gn_operators.json).

  python scripts/bench_gn_operators.py [--iters 30] [--warmup 3] [--rounds 3] [--out profiles/gn_operators.json]
"""
import argparse
import ctypes
import json
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from enf_pde_amd import _lib  # noqa: E402
from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF  # noqa: E402
from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant  # noqa: E402
from enf_pde_amd.fitting import SparseObservations, line_integrals, lm_fit_linear_observations  # noqa: E402

D, H, C, O = 128, 2, 16, 1
B, Z = 16, 64


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * iters)]
    for i in range(iters):
        ev[2 * i].record()
        fn()
        ev[2 * i + 1].record()
    torch.cuda.synchronize()
    ts = sorted(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(iters))
    return ts[iters // 2]


def operators(dev, g):
    """{name: (x (N, 2), op, the factors (N,) of equal groups or None)}"""
    x4 = torch.rand(512, 2, generator=g) * 2 - 1
    q4 = 0.2 + 1.8 * torch.rand(128, 4, generator=g)
    q4 = (q4 / q4.sum(-1, keepdim=True)).reshape(512)
    t, w1 = np.polynomial.legendre.leggauss(3)
    ex, ey = np.linspace(-1, 1, 9), np.linspace(-1, 1, 8)
    nodes = lambda e: (0.5 * (e[1:] + e[:-1]))[:, None] + (0.5 * (e[1:] - e[:-1]))[:, None] * t[None]
    nx, ny = nodes(ex), nodes(ey)
    x9 = torch.tensor(np.stack([np.broadcast_to(nx[:, None, :, None], (8, 7, 3, 3)), np.broadcast_to(ny[None, :, None, :], (8, 7, 3, 3))], -1)
                      .reshape(504, 2), dtype=torch.float32)
    q9 = np.broadcast_to(np.outer(w1, w1).reshape(1, 9) / 4.0, (56, 9)).reshape(504).copy()
    ends = torch.rand(2, 4, 2, generator=g).numpy() * 2 - 1
    xr, rays = line_integrals(ends[0], ends[1], 128, device=dev)
    return {"g4": (x4.to(dev), SparseObservations.from_groups(np.full(128, 4), q4.numpy(), device=dev), q4.to(dev)),
            "3x3": (x9.to(dev), SparseObservations.from_groups(np.full(56, 9), q9, device=dev), None),
            "rays": (xr.to(dev), rays, None)}


def transposed_struct(op):
    """A^T as an operator of its own for enf_obs_apply: the CSC arrays in the CSR's places (N rows, M columns)"""
    s = _lib.EnfSparseObs()
    s.M, s.nnz = op.N, op.nnz
    s.row_ptr, s.col, s.val = op.col_ptr.data_ptr(), op.trow.data_ptr(), op.tval.data_ptr()
    return s


def routes(dev, prec, ops):
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    g = torch.Generator().manual_seed(0)
    nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=O, latent_dim=C, cross_attn_invariant=inv,
                                       precision=prec, deterministic=False)
    P = nef.init(1, device=dev)
    p = (torch.rand(B, Z, 2, generator=g) * 2 - 1).to(dev)
    a = (1 + 0.1 * torch.randn(B, Z, C, generator=g)).to(dev)
    s = torch.full((B, Z, 1), 0.25, device=dev)
    vp, va = (0.3 * torch.randn(B, Z, 2, generator=g)).to(dev), torch.randn(B, Z, C, generator=g).to(dev)
    ps, as_ = p + 0.05 * torch.randn(B, Z, 2, generator=g).to(dev), a + 0.5 * torch.randn(B, Z, C, generator=g).to(dev)
    lib = _lib.load()
    st = _lib.stream(dev)
    fns, keep = {}, []
    for name, (x, op, q) in ops.items():
        N, M = op.N, op.M
        xb = x[None].expand(B, -1, -1)
        w = (0.2 + 1.8 * torch.rand(B, M, generator=g)).to(dev)
        coef = float(B) * 2.0 / (B * M * O)
        fwd, tr = op.struct(transposed=False), transposed_struct(op)
        obs_tan, dout = torch.empty(B, M, O, device=dev), torch.empty(B, N, O, device=dev)
        with torch.no_grad():
            f32 = nef.with_precision("f32") if prec != "f32" else nef
            target = torch.einsum("mn,bno->bmo", torch.tensor(op.to_dense(dtype=np.float32), device=dev), f32.apply(P, xb, ps, as_, s)).contiguous()
        keep.append((op, fwd, tr, obs_tan, dout, target))
        nef.gn_reserve(B, N, Z, dev, op=op)

        def product(reuse=False, xb=xb, op=op, w=w, last={}):       # (a tag from behind another route is stale: that call recomputes)
            nef.gn_operator_product(P, xb, p, a, s, op, obs_weight=w, vp=vp, va=va, grad_scale=float(B), reuse=last.get("tag") if reuse else None)
            last["tag"] = nef.workspace_tag(dev)

        def composed(xb=xb, op=op, w=w, fwd=fwd, tr=tr, obs_tan=obs_tan, dout=dout, N=N, M=M, coef=coef):
            _, tan = nef.tangent(P, xb, p, a, s, dp=vp, da=va, return_out=False)
            _lib.launch(dev, lib.enf_obs_apply, _lib.ptr(tan), B, N, O, ctypes.byref(fwd), _lib.ptr(obs_tan), st)
            r = torch.where(w[..., None] > 0, w[..., None] * obs_tan, torch.zeros_like(obs_tan))
            _lib.launch(dev, lib.enf_obs_apply, _lib.ptr(r), B, M, O, ctypes.byref(tr), _lib.ptr(dout), st)
            hp, ha, hs = (t.detach().clone().requires_grad_(True) for t in (p, a, s))
            nef.apply(P, xb, hp, ha, hs).backward(dout * coef)

        def lm_step(xb=xb, op=op, w=w, target=target):
            lm_fit_linear_observations(nef, P, xb, op, target, p, a, s, steps=1, cg_iters=8, obs_weight=w)
        fns.update({f"product_a_{name}_{prec}": product, f"product_a_reuse_{name}_{prec}": lambda product=product: product(True),
                    f"composed_{name}_{prec}": composed, f"lm_step_cg8_{name}_{prec}": lm_step})
        if q is not None:      # the grouped product on the same rows, factors and weights

            def product_g(reuse=False, xb=xb, w=w, qb=q[None].expand(B, -1).contiguous(), last={}):
                nef.gn_cell_product(P, xb, p, a, s, 4, qweight=qb, obs_weight=w, vp=vp, va=va, grad_scale=float(B),
                                    reuse=last.get("tag") if reuse else None)
                last["tag"] = nef.workspace_tag(dev)
            fns.update({f"product_g_{prec}": product_g, f"product_g_reuse_{prec}": lambda product_g=product_g: product_g(True)})
    return fns, keep


def settle(fns, calls):
    for fn in fns.values():
        for _ in range(calls):
            fn()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--settle", type=int, default=10, help="untimed calls of every route before the first timed one, in every round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ops = operators(dev, torch.Generator().manual_seed(2))
    res = {"shape": {"B": B, "Z": Z, "D": D, "H": H, "O": O, "g4": "128 groups of 4, N = 512", "3x3": "56 cells of 3 x 3, N = 504",
                     "rays": "4 rays of 128 nodes, N = 512"},
           "clock": "hipEvent pair around each call, median of the calls; medians of all rounds listed, the best reported",
           "iters": args.iters, "rounds": args.rounds}
    fns, keep = {}, []
    for prec in ("bf16", "f32"):
        f, k = routes(dev, prec, ops)
        fns.update(f)
        keep.append(k)
    times = {k: [] for k in fns}
    for _ in range(args.rounds):                     # interleaved: the routes see the same box state
        settle(fns, args.settle)
        for k, fn in fns.items():
            times[k].append(median_ms(fn, args.iters, args.warmup))
    ms = {k: round(min(v), 4) for k, v in times.items()}
    res["ms"] = ms
    res["rounds_ms"] = {k: [round(t, 4) for t in v] for k, v in times.items()}
    res["native_over_composed"] = {f"{n}_{p}": round(ms[f"product_a_{n}_{p}"] / ms[f"composed_{n}_{p}"], 3) for n in ops for p in ("bf16", "f32")}
    res["operator_over_grouped_g4"] = {p: round(ms[f"product_a_g4_{p}"] / ms[f"product_g_{p}"], 3) for p in ("bf16", "f32")}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
