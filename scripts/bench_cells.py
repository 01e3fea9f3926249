"""Cost of the grouped-observation fit step (include/enf_hip.h, "Grouped observations": enf_fit_step_g) at the bench's fit shape
(BASELINE config 2: 16 signals, 64 latents, 512 sampled points, D = 128, H = 2, bf16) with G = 4, so M = 128 observations per signal:

  cells      nef.mse_value_and_cell_grads (enf_fit_step_g) with quadrature factors and observation weights
  point      nef.mse_value_and_latent_grads with per-point weights (enf_fit_step_w) at the same N -- this tree's, and with --parent-tree
             DIR (a checkout of the parent commit with its library built) the parent's, in a child process of its own in every round
  autograd   the route there was before: nef.apply with autograd, the group sum and the loss in torch ops, backward to the latents

hipEvent pairs on the launch stream, median of --iters single calls after --warmup, --rounds interleaved rounds (parent, then this
tree's legs, in every round); the parent's fastest and slowest round are the margin the other figures are read against.
Prints one JSON line; with --out FILE also writes it there.

  python scripts/bench_cells.py [--iters 100] [--warmup 10] [--rounds 3] [--parent-tree DIR] [--out profiles/cells.json]
"""
import argparse
import json
import os
import subprocess
import sys
from types import SimpleNamespace as NS

HERE = os.path.dirname(os.path.abspath(__file__))

D, H, C, O = 128, 2, 16, 1
B, Z, N, G = 16, 64, 512, 4


def median_ms(fn, iters, warmup):
    import torch
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


def legs(cells):
    """{"point": fn[, "cells": fn, "autograd": fn]} on one set of inputs; ``cells`` False: the per-point leg only (the parent's tree)"""
    import torch
    from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF
    from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant
    dev = torch.device("cuda:0")
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(B, N, 2, generator=g) * 2 - 1).to(dev)
    p = (torch.rand(B, Z, 2, generator=g) * 2 - 1).to(dev)
    a = (1 + 0.1 * torch.randn(B, Z, C, generator=g)).to(dev)
    s = torch.full((B, Z, 1), 0.25, device=dev)
    M = N // G
    target = torch.randn(B, N, O, generator=g).to(dev)
    tg = target[:, :M].contiguous()
    q = (torch.rand(B, N, generator=g) / G + 0.5 / G).to(dev)
    w = (torch.rand(B, N, generator=g) * 2).to(dev)
    w[w < 0.5] = 0
    wg = w[:, :M].contiguous()
    nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=O, latent_dim=C, cross_attn_invariant=inv,
                                       precision="bf16")
    params = nef.init(1, device=dev)
    loss = torch.zeros(1, device=dev)

    def point():
        with torch.no_grad():
            nef.mse_value_and_latent_grads(params, x, p, a, s, target, grad_scale=B, loss_out=loss, weight=w)
    out = {"point": point}
    if not cells:
        return out

    def fused():
        nef.mse_value_and_cell_grads(params, x, p, a, s, tg, G, qweight=q, obs_weight=wg, grad_scale=B, loss_out=loss)

    def autograd():
        lv = [t.detach().requires_grad_(True) for t in (p, a, s)]
        o = nef.apply(params, x, *lv)
        obs = (q[..., None] * o).reshape(B, M, G, O).sum(2)
        dd = torch.where((wg > 0)[..., None], obs - tg, torch.zeros_like(obs))
        ((wg[..., None] * dd * dd).mean() * B).backward()
    out["cells"], out["autograd"] = fused, autograd
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit, library built: its enf_fit_step_w is measured too")
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)          # child mode: import the package from this checkout
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.tree is not None:                        # the child: the parent's package and library, the per-point leg, one round
        sys.path.insert(0, os.path.abspath(args.tree))
        print("RESULT " + json.dumps(round(median_ms(legs(False)["point"], args.iters, args.warmup), 4)))
        return
    sys.path.insert(0, os.path.dirname(HERE))

    def parent_round():
        cmd = [sys.executable, os.path.abspath(__file__), "--tree", args.parent_tree, "--iters", str(args.iters), "--warmup", str(args.warmup)]
        env = {k: v for k, v in os.environ.items() if k != "ENF_HIP_LIB"}      # the child loads the library of its own tree
        txt = subprocess.run(cmd, check=True, capture_output=True, text=True, env=env, timeout=300).stdout
        return json.loads([ln for ln in txt.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    own = legs(True)
    ms = {k: [] for k in own}
    parent = []
    for _ in range(args.rounds):                     # interleaved: the parent's child process, then this tree's legs
        if args.parent_tree is not None:
            parent.append(parent_round())
        for k, fn in own.items():
            ms[k].append(round(median_ms(fn, args.iters, args.warmup), 4))
    med = lambda v: sorted(v)[len(v) // 2]
    res = {"D": D, "H": H, "precision": "bf16", "B,Z,N": [B, Z, N], "G": G, "M": N // G, "iters": args.iters, "rounds": args.rounds,
           "clock": "hipEvent pair around each call, median per round", "fit_step_ms": ms,
           "cells_over_point": round(med(ms["cells"]) / med(ms["point"]), 4),
           "autograd_over_cells": round(med(ms["autograd"]) / med(ms["cells"]), 4)}
    if parent:
        res["parent_commit_point_fit_step_ms"] = parent
        res["parent_margin_ms"] = [min(parent), max(parent)]
        res["point_over_parent_point"] = round(med(ms["point"]) / med(parent), 4)
        res["cells_over_parent_point"] = round(med(ms["cells"]) / med(parent), 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
