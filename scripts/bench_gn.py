"""Cost of the Gauss-Newton product, of the batched CG step and of a Levenberg-Marquardt latent fit (include/enf_hip.h, "Gauss-Newton
product") at the bench's FIT shape: 16 signals, 64 latents, 512 sampled points, D = 128, H = 2, O = 1, in bf16 and f32.

ONE process, interleaved rounds, hipEvent pairs on the launch stream, median of single calls after a warm-up; every round is recorded.
  product    nef.gn_product without and with the reuse of the point (ENF_GN_REUSE_POINT)
  composed   the same product through public entry points: nef.tangent, w tan coef in torch, the latent backward of nef.apply
  fit_step   one nef.mse_value_and_latent_grads (enf_fit_step_w): the unit a first-order fit pays per step
  cg_update  enf_cg_update on (p, a) against the same step written in torch ops
  fit        per-signal losses of lm_fit_latents (4 steps, 4 and 8 CG iterations; target = the decode of perturbed latents) with the
             elapsed time of the whole call, and of the inner loop's SGD step (p -= g_p, a -= 5 g_a at gradient scale B) repeated for
             the same elapsed time

Prints one JSON line; --out FILE also writes it there (profiles/gn.json).

  python scripts/bench_gn.py [--iters 30] [--warmup 3] [--rounds 3] [--out profiles/gn.json]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace as NS

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF  # noqa: E402
from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant  # noqa: E402
from enf_pde_amd.fitting import gauss_newton as GN  # noqa: E402
from scripts.bench_determinism import median_ms  # noqa: E402

D, H, C, O = 128, 2, 16, 1
B, Z, N = 16, 64, 512


def setup(dev, prec):
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(B, N, 2, generator=g) * 2 - 1).to(dev)
    p = (torch.rand(B, Z, 2, generator=g) * 2 - 1).to(dev)
    a = (1 + 0.1 * torch.randn(B, Z, C, generator=g)).to(dev)
    s = torch.full((B, Z, 1), 0.25, device=dev)
    vp, va = (0.3 * torch.randn(B, Z, 2, generator=g)).to(dev), torch.randn(B, Z, C, generator=g).to(dev)
    w = (0.2 + 1.8 * torch.rand(B, N, generator=g)).to(dev)
    ps, as_ = p + 0.05 * torch.randn(B, Z, 2, generator=g).to(dev), a + 0.5 * torch.randn(B, Z, C, generator=g).to(dev)
    nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=O, latent_dim=C, cross_attn_invariant=inv,
                                       precision=prec, deterministic=False)
    params = nef.init(1, device=dev)
    with torch.no_grad():
        target = nef.with_precision("f32").apply(params, x, ps, as_, s) if prec != "f32" else nef.apply(params, x, ps, as_, s)
    return NS(nef=nef, params=params, x=x, p=p, a=a, s=s, vp=vp, va=va, w=w, target=target.contiguous())


def product_routes(c, prec):
    nef, P = c.nef, c.params
    dev = c.p.device
    coef = float(B) * 2.0 / (B * N * O)
    nef.gn_reserve(B, N, Z, dev)

    def product():
        nef.gn_product(P, c.x, c.p, c.a, c.s, vp=c.vp, va=c.va, weight=c.w, grad_scale=float(B))

    def product_reuse():
        nef.gn_product(P, c.x, c.p, c.a, c.s, vp=c.vp, va=c.va, weight=c.w, grad_scale=float(B), reuse=nef.workspace_tag(dev))

    def composed():
        _, tan = nef.tangent(P, c.x, c.p, c.a, c.s, dp=c.vp, da=c.va, return_out=False)
        seed = c.w[..., None] * tan * coef
        hp, ha, hs = (t.detach().clone().requires_grad_(True) for t in (c.p, c.a, c.s))
        nef.apply(P, c.x, hp, ha, hs).backward(seed)

    def fit_step():
        nef.mse_value_and_latent_grads(P, c.x, c.p, c.a, c.s, c.target, grad_scale=float(B), weight=c.w)
    return {f"product_{prec}": product, f"product_reuse_{prec}": product_reuse, f"composed_{prec}": composed, f"fit_step_{prec}": fit_step}


def cg_routes(dev):
    g = torch.Generator().manual_seed(2)
    mk = lambda w: torch.randn(B, Z, w, generator=g).to(dev)
    segs = [(mk(2), mk(2), mk(2)), (mk(C), mk(C), mk(C))]
    q = [2.0 * d + 0.1 * mk(d.shape[2]) for _, _, d in segs]
    lam = torch.full((B,), 1e-2, device=dev)
    rho = torch.ones(B, device=dev)

    def native():
        GN._cg_update(segs, B, Z, lam, rho, q)

    def torch_ops():
        bdot = lambda u, v: sum((ui * vi).sum(dim=(1, 2)) for ui, vi in zip(u, v))
        d = [s_[2] for s_ in segs]
        qd = [qi + lam[:, None, None] * di for qi, di in zip(q, d)]
        kappa = bdot(d, qd)
        live = (rho > 0) & torch.isfinite(rho) & (kappa > 0) & torch.isfinite(kappa)
        alpha = torch.where(live, rho / kappa, torch.zeros_like(rho))[:, None, None]
        r2 = []
        for (x, r, di), qi in zip(segs, qd):
            x.add_(alpha * di)
            r2.append(r - alpha * qi)
        rho2 = torch.where(live, bdot(r2, r2), rho)
        beta = torch.where(live, rho2 / rho, torch.zeros_like(rho))[:, None, None]
        for (x, r, di), ri in zip(segs, r2):
            di.copy_(torch.where(live[:, None, None], ri + beta * di, di))
    return {"cg_update_native": native, "cg_update_torch": torch_ops}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def fit_curves(c, prec):
    nef, P = c.nef, c.params
    res = {}
    for cg in (4, 8):
        run = lambda: GN.lm_fit_latents(nef, P, c.x, c.target, c.p, c.a, c.s, steps=4, cg_iters=cg)
        run()                                       # warm-up (kernel attributes, caches)
        (_, loss_b, lam, acc), ms = timed(run)
        res[f"lm_cg{cg}"] = {"ms": round(ms, 3), "mean_loss_by_step": [float(f"{v:.4e}") for v in loss_b.mean(1).cpu()],
                             "max_loss_by_step": [float(f"{v:.4e}") for v in loss_b.max(1).values.cpu()],
                             "accepted_by_step": [int(v) for v in acc.sum(1).cpu()]}

    def sgd(steps):
        p, a = c.p, c.a
        for _ in range(steps):
            _, gp, ga, _ = nef.mse_value_and_latent_grads(P, c.x, p, a, c.s, c.target, grad_scale=float(B))
            p, a = p - gp, a - 5.0 * ga
        return nef.eval_loss(P, c.x, p, a, c.s, c.target)[0]
    sgd(3)
    _, ms16 = timed(lambda: sgd(16))
    per = ms16 / 16
    for cg in (4, 8):
        n = max(1, int(res[f"lm_cg{cg}"]["ms"] / per))
        lb, ms = timed(lambda: sgd(n))
        res[f"sgd_for_the_time_of_lm_cg{cg}"] = {"steps": n, "ms": round(ms, 3), "mean_loss": float(f"{float(lb.mean()):.4e}"),
                                                 "max_loss": float(f"{float(lb.max()):.4e}")}
    res["sgd_step_ms"] = round(per, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"shape": {"B": B, "Z": Z, "N": N, "D": D, "H": H, "O": O},
           "clock": "hipEvent pair around each call, median of the calls; medians of all rounds listed, the best reported",
           "iters": args.iters, "rounds": args.rounds}
    cases = {prec: setup(dev, prec) for prec in ("bf16", "f32")}
    fns = {}
    for prec, c in cases.items():
        fns.update(product_routes(c, prec))
    fns.update(cg_routes(dev))
    times = {k: [] for k in fns}
    for _ in range(args.rounds):                     # interleaved: the routes see the same box state
        for k, fn in fns.items():
            times[k].append(median_ms(fn, args.iters, args.warmup))
    best = {k: min(v) for k, v in times.items()}
    res["ms"] = {k: round(v, 4) for k, v in best.items()}
    res["rounds_ms"] = {k: [round(t, 4) for t in v] for k, v in times.items()}
    res["fit"] = {prec: fit_curves(c, prec) for prec, c in cases.items()}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
