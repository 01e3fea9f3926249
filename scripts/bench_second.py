"""Cost and accuracy of a second directional derivative (include/enf_hip.h, "Second directional derivatives") at bench config 2's DECODE
shape (16 signals, 64 latents, the 64 x 64 grid shared by the signals, D = 128, H = 2, O = 1), hipEvent pairs on the launch stream,
median of single calls after a warm-up, interleaved rounds, every round recorded.

Routes (one process), in bf16 and f32:
  tangent_x_{prec}      nef.tangent with xdot alone (enf_field_tangent_x): the first-order pass on the same box
  second_{prec}         nef.second_derivative (enf_field_second_x): ONE second-order pass
  laplacian_{prec}      fitting.decode_laplacian: dx = 2 second-order passes
  central_diff_f32      the only earlier route to a second directional derivative: two f32 nef.tangent(xdot=) calls at x +- h xdot and
                        their difference in torch
  second_*_D64 / tangent_x_*_D64   the same calls at D = 64, H = 2: the f32 D = 128 pair kernel spills to scratch, its D = 64 neighbour
                        does not; the bf16 pair (no scratch at either width) gives the ratio the width alone costs
Accuracy (--accuracy, at the test shape of tests/second_ref.py: D = 64, H = 2, B = 3, N = 50, Z = 7, against the fp64 oracle):
  the central difference's error at every step h of a sweep and at its best, beside the second-order pass's;
  per case class of tests/test_gpu_second.py: E_r of libenf_hip_f32r.so, bf16's error, bf16 - f32r overall and in the median query row.

Prints one JSON line; --out FILE also writes it there (profiles/second_x.json).

  python scripts/bench_second.py [--iters 30] [--warmup 3] [--rounds 3] [--accuracy] [--out profiles/second_x.json]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, C = 2, 16
B, Z, GRID = 16, 64, 64
CD_STEP = 1e-3


def routes(dev):
    import torch
    sys.path.insert(0, ROOT)
    from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF
    from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant
    from enf_pde_amd.fitting import decode_laplacian
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    g = torch.Generator().manual_seed(0)
    lin = torch.linspace(-1, 1, GRID)
    coords = torch.stack(torch.meshgrid(lin, lin, indexing="xy"), -1).reshape(-1, 2).to(dev)     # (4096, 2), one grid for the batch
    p = (torch.rand(B, Z, 2, generator=g) * 2 - 1).to(dev)
    a = (1 + 0.1 * torch.randn(B, Z, C, generator=g)).to(dev)
    s = torch.full((B, Z, 1), 0.25, device=dev)
    vel = torch.randn(B, GRID * GRID, 2, generator=g).to(dev)                                   # a direction field per signal
    grid = coords[None].expand(B, -1, -1)
    fns = {}
    for D in (128, 64):
        tag = "" if D == 128 else "_D64"
        for prec in ("bf16", "f32"):
            nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=1, latent_dim=C, cross_attn_invariant=inv,
                                               precision=prec, deterministic=False)
            params = nef.init(1, device=dev)
            fns[f"tangent_x_{prec}{tag}"] = lambda nef=nef, params=params: nef.tangent(params, grid, p, a, s, xdot=vel)
            fns[f"second_{prec}{tag}"] = lambda nef=nef, params=params: nef.second_derivative(params, grid, p, a, s, vel)
            if D == 128:
                fns[f"laplacian_{prec}"] = lambda nef=nef, params=params: decode_laplacian(nef, params, coords, p, a, s)
            if D == 128 and prec == "f32":
                def central(nef=nef, params=params):
                    hi = nef.tangent(params, grid + CD_STEP * vel, p, a, s, xdot=vel, return_out=False)[1]
                    lo = nef.tangent(params, grid - CD_STEP * vel, p, a, s, xdot=vel, return_out=False)[1]
                    return (hi - lo) / (2 * CD_STEP)
                fns["central_diff_f32"] = central
    return fns


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


def measure(args):
    import torch
    fns = routes(torch.device("cuda:0"))
    times = {k: [] for k in fns}
    for _ in range(args.rounds):                     # interleaved: the routes see the same box state
        for k, fn in fns.items():
            times[k].append(median_ms(fn, args.iters, args.warmup))
    best = {k: min(v) for k, v in times.items()}
    res = {"ms": {k: round(v, 4) for k, v in best.items()}, "rounds_ms": {k: [round(t, 4) for t in v] for k, v in times.items()}}
    r = res["ratios"] = {}
    for prec in ("bf16", "f32"):
        r[f"second_over_tangent_x_{prec}"] = round(best[f"second_{prec}"] / best[f"tangent_x_{prec}"], 3)
        r[f"laplacian_over_second_{prec}"] = round(best[f"laplacian_{prec}"] / best[f"second_{prec}"], 3)
        r[f"second_over_tangent_x_{prec}_D64"] = round(best[f"second_{prec}_D64"] / best[f"tangent_x_{prec}_D64"], 3)
        r[f"second_D128_over_D64_{prec}"] = round(best[f"second_{prec}"] / best[f"second_{prec}_D64"], 3)
    r["central_diff_over_second_f32"] = round(best["central_diff_f32"] / best["second_f32"], 3)
    # what the scratch of the f32 D = 128 pair kernel costs: its width ratio against the ratio of the bf16 pair, which has none
    r["f32_width_ratio_over_bf16_width_ratio"] = round(r["second_D128_over_D64_f32"] / r["second_D128_over_D64_bf16"], 3)
    return res


def accuracy():
    """errors against the fp64 oracle at the test shape: the central difference of two f32 first-order passes over a sweep of steps, and
    the figures the bf16 bounds of tests/test_gpu_second.py are made of"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from enf_pde_amd import _lib
    from tests.helpers import build_nef
    from tests.second_ref import INVARIANTS, case, rel
    dev = torch.device("cuda:0")
    t = lambda v: torch.tensor(np.asarray(v), dtype=torch.float32, device=dev)
    npy = lambda v: v.double().cpu().numpy()
    rows = lambda v: np.linalg.norm(v.reshape(-1, v.shape[-1]), axis=1)

    def second(c, prec):
        nef = build_nef(c[0], prec)
        return npy(nef.second_derivative(nef.load_params(c[1], device=dev), *(t(v) for v in c[2]), t(c[3]))[2])
    c = case("rel_pos_periodic")
    nef = build_nef(c[0], "f32")
    P = nef.load_params(c[1], device=dev)
    x, p, a, s = (t(v) for v in c[2])
    xd = t(c[3])
    sweep = {}
    for h in (1e-1, 3e-2, 1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5):
        hi, lo = (nef.tangent(P, x + sg * h * xd, p, a, s, xdot=xd, return_out=False)[1] for sg in (1, -1))
        sweep[f"{h:g}"] = float(rel(npy((hi - lo) / (2 * h)), c[6]))
    best = min(sweep, key=sweep.get)
    res = {"central_difference_f32": {"case": "rel_pos_periodic, D 64, H 2, B 3, N 50, Z 7", "error_by_step": sweep, "best_step": best,
                                      "best_error": sweep[best], "second_order_pass_f32_error": float(rel(second(c, "f32"), c[6]))}}
    classes = [(inv, inv, dict(use_window=w)) for inv in INVARIANTS for w in (True, False)] + \
              [("128x2", "rel_pos_periodic", dict(D=128, H=2, B=2, N=130, Z=9)), ("128x1", "rel_pos_periodic", dict(D=128, H=1, B=2, N=20, Z=7)),
               ("64x1", "rel_pos_periodic", dict(D=64, H=1, B=2, N=20, Z=7)), ("64x4", "rel_pos_periodic", dict(D=64, H=4, B=2, N=20, Z=7))]
    table = res["bf16"] = {}
    for cls, inv, kw in classes:
        c = case(inv, **kw)
        ref = c[6]
        b = second(c, "bf16")
        with _lib.using(_lib.load_f32r()):
            r = second(c, "f32")
            torch.cuda.synchronize()
        rms = np.sqrt(np.mean(rows(ref) ** 2))
        table.setdefault(cls, []).append({
            "case": kw, "E_r": float(rel(r, ref)), "bf16": float(rel(b, ref)), "f32": float(rel(second(c, "f32"), ref)),
            "bf16_minus_f32r": float(np.linalg.norm(b - r) / np.linalg.norm(ref)),
            "E_r_median_row": float(np.median(rows(r - ref) / rms)), "bf16_minus_f32r_median_row": float(np.median(rows(b - r) / rms))})
    res["bf16_bounds"] = {cls: 2 * max(e["E_r"] for e in v) for cls, v in table.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"shape": {"B": B, "Z": Z, "N": GRID * GRID, "D": 128, "H": H, "O": 1, "grid": "shared by the signals (x_bstride = 0)",
                     "xdot": "per signal (B, N, 2)", "central_difference_step": CD_STEP},
           "clock": "hipEvent pair around each call, median of the calls; medians of all rounds listed, the best reported",
           "iters": args.iters, "rounds": args.rounds}
    res.update(measure(args))
    if args.accuracy:
        res["accuracy"] = accuracy()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
