"""Cost of the Gauss-Newton product on grouped observations (include/enf_hip.h, "Gauss-Newton product on grouped observations") at the
bench's FIT shape: 16 signals, 64 latents, D = 128, H = 2, O = 1, groups of G = 4 -- N = 512 rows, M = 128 observations per signal --
in bf16 and f32.

Interleaved rounds on one box, hipEvent pairs on the launch stream, median of single calls after a warm-up; every round is recorded.
  product_g        nef.gn_cell_product (enf_gn_product_g) without and with the reuse of the point (ENF_GN_REUSE_POINT)
  composed         the same product through public entry points: nef.tangent, the group sum and the seed in torch, the latent
                   backward of nef.apply -- the route a caller had to build by hand before
  cell_fit_step    one nef.mse_value_and_cell_grads (enf_fit_step_g): the unit a first-order fit pays per step
  lm_step          one step of lm_fit_cell_averages with eight CG iterations (fit step, eight products, one evaluation)
  parent_product   with --parent ROOT: the per-point nef.gn_product of the tree at ROOT (a checkout of the parent commit, built) on the
                   same 512 rows, timed in a CHILD process of its own in every round (this script with --child, importing ROOT's
                   package and library).  The spread of its rounds is the margin the grouped product is read against.

Prints one JSON line; --out FILE also writes it there (profiles/gn_cells.json).

  python scripts/bench_gn_cells.py [--iters 30] [--warmup 3] [--rounds 3] [--parent ROOT] [--out profiles/gn_cells.json]
"""
import argparse
import json
import os
import subprocess
import sys
from types import SimpleNamespace as NS

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _root():
    """--root ROOT (the child's tree) has to be known before the package is imported"""
    if "--root" in sys.argv:
        return os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
    return HERE


sys.path.insert(0, _root())
from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF  # noqa: E402
from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant  # noqa: E402

D, H, C, O = 128, 2, 16, 1
B, Z, G, M = 16, 64, 4, 128
N = M * G


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


def setup(dev, prec):
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(B, N, 2, generator=g) * 2 - 1).to(dev)
    p = (torch.rand(B, Z, 2, generator=g) * 2 - 1).to(dev)
    a = (1 + 0.1 * torch.randn(B, Z, C, generator=g)).to(dev)
    s = torch.full((B, Z, 1), 0.25, device=dev)
    vp, va = (0.3 * torch.randn(B, Z, 2, generator=g)).to(dev), torch.randn(B, Z, C, generator=g).to(dev)
    w = (0.2 + 1.8 * torch.rand(B, N, generator=g)).to(dev)                     # the parent's per-point weights
    q = 0.2 + 1.8 * torch.rand(B, M, G, generator=g)
    q = (q / q.sum(-1, keepdim=True)).reshape(B, N).to(dev)
    wo = (0.2 + 1.8 * torch.rand(B, M, generator=g)).to(dev)
    ps, as_ = p + 0.05 * torch.randn(B, Z, 2, generator=g).to(dev), a + 0.5 * torch.randn(B, Z, C, generator=g).to(dev)
    nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=O, latent_dim=C, cross_attn_invariant=inv,
                                       precision=prec, deterministic=False)
    params = nef.init(1, device=dev)
    return NS(nef=nef, params=params, x=x, p=p, a=a, s=s, vp=vp, va=va, w=w, q=q, wo=wo, ps=ps, as_=as_)


def parent_routes(c, prec):
    """the per-point product, through what the parent commit has"""
    nef, P = c.nef, c.params
    dev = c.p.device
    nef.gn_reserve(B, N, Z, dev)

    def product():
        nef.gn_product(P, c.x, c.p, c.a, c.s, vp=c.vp, va=c.va, weight=c.w, grad_scale=float(B))

    def product_reuse():
        nef.gn_product(P, c.x, c.p, c.a, c.s, vp=c.vp, va=c.va, weight=c.w, grad_scale=float(B), reuse=nef.workspace_tag(dev))
    return {f"parent_product_{prec}": product, f"parent_product_reuse_{prec}": product_reuse}


def cell_routes(c, prec):
    from enf_pde_amd.fitting import lm_fit_cell_averages
    nef, P = c.nef, c.params
    dev = c.p.device
    coef = float(B) * 2.0 / (B * M * O)
    nef.gn_reserve(B, N, Z, dev)
    with torch.no_grad():
        f32 = nef.with_precision("f32") if prec != "f32" else nef
        out = f32.apply(P, c.x, c.ps, c.as_, c.s)
        target = (c.q[..., None] * out).reshape(B, M, G, O).sum(2).contiguous()
    kw = dict(qweight=c.q, obs_weight=c.wo)

    def product_g():
        nef.gn_cell_product(P, c.x, c.p, c.a, c.s, G, vp=c.vp, va=c.va, grad_scale=float(B), **kw)

    def product_g_reuse():
        nef.gn_cell_product(P, c.x, c.p, c.a, c.s, G, vp=c.vp, va=c.va, grad_scale=float(B), reuse=nef.workspace_tag(dev), **kw)

    def composed():
        _, tan = nef.tangent(P, c.x, c.p, c.a, c.s, dp=c.vp, da=c.va, return_out=False)
        obs_tan = (c.q[..., None] * tan).reshape(B, M, G, O).sum(2)
        seed = c.q[..., None] * (c.wo[..., None] * obs_tan).repeat_interleave(G, dim=1) * coef
        hp, ha, hs = (t.detach().clone().requires_grad_(True) for t in (c.p, c.a, c.s))
        nef.apply(P, c.x, hp, ha, hs).backward(seed)

    def cell_fit_step():
        nef.mse_value_and_cell_grads(P, c.x, c.p, c.a, c.s, target, G, grad_scale=float(B), **kw)

    def lm_step():
        lm_fit_cell_averages(nef, P, c.x, c.q, G, target, c.p, c.a, c.s, steps=1, cg_iters=8, obs_weight=c.wo)
    return {f"product_g_{prec}": product_g, f"product_g_reuse_{prec}": product_g_reuse, f"composed_{prec}": composed,
            f"cell_fit_step_{prec}": cell_fit_step, f"lm_step_cg8_{prec}": lm_step}


def child(args):
    dev = torch.device("cuda:0")
    fns = {}
    for prec in ("bf16", "f32"):
        fns.update(parent_routes(setup(dev, prec), prec))
    print(json.dumps({k: median_ms(fn, args.iters, args.warmup) for k, fn in fns.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--root", default=None, help="(child) the tree whose package and library are imported")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    dev = torch.device("cuda:0")
    res = {"shape": {"B": B, "Z": Z, "N": N, "G": G, "M": M, "D": D, "H": H, "O": O},
           "clock": "hipEvent pair around each call, median of the calls; medians of all rounds listed, the best reported",
           "iters": args.iters, "rounds": args.rounds}
    fns = {}
    for prec in ("bf16", "f32"):
        c = setup(dev, prec)
        fns.update(cell_routes(c, prec))
        fns.update({k.replace("parent_", "this_tree_per_point_"): f for k, f in parent_routes(c, prec).items()})
    times = {k: [] for k in fns}
    for _ in range(args.rounds):                     # interleaved: the routes see the same box state
        for k, fn in fns.items():
            times[k].append(median_ms(fn, args.iters, args.warmup))
        if args.parent:                              # the parent commit's product, in a process of its own
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", args.parent, "--iters", str(args.iters),
                                  "--warmup", str(args.warmup)], check=True, capture_output=True, text=True).stdout
            for k, v in json.loads(out.strip().splitlines()[-1]).items():
                times.setdefault(k, []).append(v)
    res["ms"] = {k: round(min(v), 4) for k, v in times.items()}
    res["rounds_ms"] = {k: [round(t, 4) for t in v] for k, v in times.items()}
    if args.parent:
        res["parent_spread_ms"] = {k: round(max(v) - min(v), 4) for k, v in times.items() if k.startswith("parent_")}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
