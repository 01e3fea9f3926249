"""Cost of a directional derivative (include/enf_hip.h, "Directional derivatives") at bench config 2's DECODE shape (16 signals, 64
latents, the 64 x 64 grid shared by the signals, D = 128, H = 2), hipEvent pairs on the launch stream, median of single calls after a
warm-up, interleaved rounds, every round recorded.

Routes (one process):
  tangent_{bf16,f32}           nef.tangent without xdot (enf_field_tangent, the call it was), O = 1
  tangent_x_alone_{bf16,f32}   nef.tangent with xdot alone (enf_field_tangent_x), a per-signal direction field
  tangent_x_all_{bf16,f32}     ... with xdot and (dp, da, dwindow)
  material_O{1,2}_bf16         fitting.decode_material_derivative: ONE tangent pass for Du/Dt = u_t + c . grad u
  composed_O{1,2}_bf16         the route there was: decode_tendency (a tangent pass), decode_jacobian, the contraction with c in torch
(the latent ODE is a stand-in that returns a fixed dz/dt, the same for both routes: its cost is not the subject.)
The ratio composed / material is reported beside the ratio predicted from the separate times of DESIGN.md 7 (2.1x at O = 1, 3x at O = 2).

--ab PARENT_ROOT: the A/B of the call WITHOUT xdot against a checkout of the parent commit built in place: `scripts/bench_tangent.py`
of each tree in a fresh process, alternated parent / new, --procs of each; the rule of profiles/tangent_refactor_ab.json: the new
build's median over its rounds must lie inside the parent's own slowest-to-fastest round.

Prints one JSON line; --out FILE also writes it there (profiles/tangent_x.json).

  python scripts/bench_tangent_x.py [--iters 30] [--warmup 3] [--rounds 3] [--ab PARENT_ROOT [--procs 3]] [--out profiles/tangent_x.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, H, C = 128, 2, 16
B, Z, GRID = 16, 64, 64
PREDICTED = {1: round((3.93 + 4.47) / 3.93, 2), 2: round((3.93 + 7.67) / 3.93, 2)}      # from DESIGN.md 7's separate times


class _FixedOde:
    """a latent ODE whose right-hand side is a stored direction"""

    def __init__(self, dz):
        self.dz = dz

    def apply(self, params, latents):
        return self.dz


def routes(dev):
    import torch
    sys.path.insert(0, ROOT)
    from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF
    from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant
    from enf_pde_amd.fitting import decode_material_derivative, decode_tendency, decode_jacobian
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    g = torch.Generator().manual_seed(0)
    lin = torch.linspace(-1, 1, GRID)
    coords = torch.stack(torch.meshgrid(lin, lin, indexing="xy"), -1).reshape(-1, 2).to(dev)     # (4096, 2), one grid for the batch
    p = (torch.rand(B, Z, 2, generator=g) * 2 - 1).to(dev)
    a = (1 + 0.1 * torch.randn(B, Z, C, generator=g)).to(dev)
    s = torch.full((B, Z, 1), 0.25, device=dev)
    dp, da = (0.3 * torch.randn(B, Z, 2, generator=g)).to(dev), torch.randn(B, Z, C, generator=g).to(dev)
    ds = (0.02 * torch.randn(B, Z, 1, generator=g)).to(dev)
    vel = torch.randn(B, GRID * GRID, 2, generator=g).to(dev)                                   # a velocity field per signal
    grid = coords[None].expand(B, -1, -1)
    ode = _FixedOde((dp, da, ds))
    fns = {}

    def model(prec, O):
        nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=O, latent_dim=C, cross_attn_invariant=inv,
                                           precision=prec, deterministic=False)
        return nef, nef.init(1, device=dev)

    for prec in ("bf16", "f32"):
        nef, params = model(prec, 1)
        fns[f"tangent_{prec}"] = lambda nef=nef, params=params: nef.tangent(params, grid, p, a, s, dp=dp, da=da, dwindow=ds)
        fns[f"tangent_x_alone_{prec}"] = lambda nef=nef, params=params: nef.tangent(params, grid, p, a, s, xdot=vel)
        fns[f"tangent_x_all_{prec}"] = lambda nef=nef, params=params: nef.tangent(params, grid, p, a, s, dp=dp, da=da, dwindow=ds, xdot=vel)
    for O in (1, 2):
        nef, params = model("bf16", O)

        def material(nef=nef, params=params):
            return decode_material_derivative(nef, params, ode, None, coords, p, a, s, vel)

        def composed(nef=nef, params=params):
            u, ut = decode_tendency(nef, params, ode, None, coords, p, a, s)
            _, jac = decode_jacobian(nef, params, coords, p, a, s)
            return u, ut + (jac * vel[:, :, None, :]).sum(-1)
        fns[f"material_O{O}_bf16"], fns[f"composed_O{O}_bf16"] = material, composed
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
    dev = torch.device("cuda:0")
    fns = routes(dev)
    times = {k: [] for k in fns}
    for _ in range(args.rounds):                     # interleaved: the routes see the same box state
        for k, fn in fns.items():
            times[k].append(median_ms(fn, args.iters, args.warmup))
    best = {k: min(v) for k, v in times.items()}
    res = {"ms": {k: round(v, 4) for k, v in best.items()}, "rounds_ms": {k: [round(t, 4) for t in v] for k, v in times.items()}}
    res["ratios"] = {}
    for prec in ("bf16", "f32"):
        res["ratios"][f"x_alone_over_tangent_{prec}"] = round(best[f"tangent_x_alone_{prec}"] / best[f"tangent_{prec}"], 4)
        res["ratios"][f"x_all_over_tangent_{prec}"] = round(best[f"tangent_x_all_{prec}"] / best[f"tangent_{prec}"], 4)
    for O in (1, 2):
        res["ratios"][f"composed_over_material_O{O}_bf16"] = round(best[f"composed_O{O}_bf16"] / best[f"material_O{O}_bf16"], 3)
        res["ratios"][f"predicted_O{O}"] = PREDICTED[O]
    return res


def ab(args):
    """bench_tangent.py of the parent's tree and of this one in fresh processes, alternated"""
    keys = ("tangent_bf16", "tangent_f32")
    rounds = {"parent": {k: [] for k in keys}, "new": {k: [] for k in keys}}
    for _ in range(args.procs):
        for side, root in (("parent", os.path.abspath(args.ab)), ("new", ROOT)):
            env = dict(os.environ)
            env.pop("ENF_HIP_LIB", None)
            r = subprocess.run([sys.executable, os.path.join(root, "scripts", "bench_tangent.py"), "--iters", str(args.iters), "--warmup",
                                str(args.warmup), "--rounds", str(args.rounds)], cwd=root, env=env, capture_output=True, text=True,
                               timeout=300)
            if r.returncode != 0:
                raise RuntimeError(f"{side}: bench_tangent.py exited with {r.returncode}\n{r.stderr[-2000:]}")
            got = json.loads(r.stdout.strip().splitlines()[-1])["rounds_ms"]
            for k in keys:
                rounds[side][k] += got[k]
    res = {"what": "same-box A/B of nef.tangent WITHOUT xdot, processes alternated parent / new; ms, every round's median of single calls",
           "rule": "the new build's median over its rounds must lie inside the parent's own slowest-to-fastest round", "keys": {}}
    for k in keys:
        pr, nr = rounds["parent"][k], rounds["new"][k]
        pm, nm = statistics.median(pr), statistics.median(nr)
        res["keys"][k] = {"parent_rounds": pr, "new_rounds": nr, "parent_median": pm, "new_median": nm, "parent_min": min(pr),
                          "parent_max": max(pr), "new_vs_parent_median_pct": round(100 * (nm / pm - 1), 2),
                          "within_parent_range": bool(min(pr) <= nm <= max(pr)), "not_slower_than_parent_max": bool(nm <= max(pr))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ab", default=None, metavar="PARENT_ROOT")
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"shape": {"B": B, "Z": Z, "N": GRID * GRID, "D": D, "H": H, "grid": "shared by the signals (x_bstride = 0)",
                     "xdot": "per signal (B, N, 2)"},
           "clock": "hipEvent pair around each call, median of the calls; medians of all rounds listed, the best reported",
           "iters": args.iters, "rounds": args.rounds}
    if args.ab:                                      # first, and from a process that has not touched the GPU: the children are fresh
        res["ab_without_xdot"] = ab(args)
    res.update(measure(args))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
