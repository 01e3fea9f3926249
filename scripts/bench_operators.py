"""Cost of fitting against a sparse linear observation operator (include/enf_hip.h, "Sparse linear observations") at the bench's FIT shape:
16 signals, 64 latents, D = 128, H = 2, O = 1, in bf16 and f32.

Interleaved rounds on one box, hipEvent pairs on the launch stream, median of single calls after a warm-up; every round is recorded.
Every process, and this one again in every round, first runs ALL its routes untimed (--settle calls each): the route that is timed
first after a process starts, or after the GPU sat idle while the child started, otherwise reads about 7 % high at the 0.7 ms of the
bf16 step (three warm-up calls do not bring the clocks back).
  (a) the price of not fusing   fit_step_a_g4: nef.mse_value_and_operator_grads (enf_fit_step_a) with the G = 4 operator on 512 rows,
                                against fit_step_g (enf_fit_step_g, the fused grouped tail) and composed_g (nef.apply + nef.cell_mse +
                                backward: enf_forward_stages, enf_mse_value_grad_g, enf_backward_latents) on the same rows
  (b) what it buys              fit_step_a_3x3: a 3 x 3 Gauss rule on 56 cells, N = 504, against fit_step_g_padded: the same cells padded
                                to groups of 16 with q = 0, N = 896
  (c) the two kernels alone     kernel1_*: enf_mse_value_grad_a without d out (the forward product with the loss, one launch);
                                kernels12_*: with d out (both launches) -- at (a), (b) and 64 rays of 128 nodes (B = 16, O = 1).  A
                                hipEvent pair around one small launch reads the launch floor, so each figure is also taken as the time
                                per call of 50 back-to-back calls (*_x50): an upper bound of the kernels' own time
  parent_*                      with --parent ROOT: fit_step_g, composed_g and fit_step_g_padded of the tree at ROOT (a checkout of the
                                parent commit, built), timed in a CHILD process of its own in every round (this script with --child).  The
                                spread of its rounds is the margin the new call is read against.

Prints one JSON line; --out FILE also writes it there (profiles/operators.json).

  python scripts/bench_operators.py [--iters 30] [--warmup 3] [--rounds 3] [--parent ROOT] [--out profiles/operators.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _root():
    """--root ROOT (the child's tree) has to be known before the package is imported"""
    if "--root" in sys.argv:
        return os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
    return HERE


sys.path.insert(0, _root())
from enf_pde_amd import _lib  # noqa: E402
from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF  # noqa: E402
from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant  # noqa: E402

D, H, C, O = 128, 2, 16, 1
B, Z = 16, 64


def median_ms(fn, iters, warmup, batch=1):
    """median over `iters` event pairs, each around `batch` back-to-back calls; per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * iters)]
    for i in range(iters):
        ev[2 * i].record()
        for _ in range(batch):
            fn()
        ev[2 * i + 1].record()
    torch.cuda.synchronize()
    ts = sorted(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(iters))
    return ts[iters // 2] / batch


def _pad16(x, q, G):
    """groups of G rows padded to 16 with q = 0 at the group's first point"""
    M = x.shape[0] // G
    xg, qg = x.reshape(M, G, -1), q.reshape(M, G)
    return (torch.cat([xg, xg[:, :1].expand(-1, 16 - G, -1)], 1).reshape(M * 16, -1).contiguous(),
            torch.cat([qg, torch.zeros(M, 16 - G)], 1).reshape(M * 16).contiguous())


def setup(dev, prec):
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    g = torch.Generator().manual_seed(0)
    nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=O, latent_dim=C, cross_attn_invariant=inv,
                                       precision=prec, deterministic=False)
    p = (torch.rand(B, Z, 2, generator=g) * 2 - 1).to(dev)
    a = (1 + 0.1 * torch.randn(B, Z, C, generator=g)).to(dev)
    s = torch.full((B, Z, 1), 0.25, device=dev)
    # (a): 128 groups of 4 consecutive rows, factors that sum to 1, one set for all signals
    x4 = torch.rand(512, 2, generator=g) * 2 - 1
    q4 = 0.2 + 1.8 * torch.rand(128, 4, generator=g)
    q4 = (q4 / q4.sum(-1, keepdim=True)).reshape(512)
    # (b): 56 cells with a 3 x 3 Gauss rule, N = 504; the grouped tail needs them padded to 16 rows, N = 896
    t, w1 = np.polynomial.legendre.leggauss(3)
    ex, ey = np.linspace(-1, 1, 9), np.linspace(-1, 1, 8)
    nodes = lambda e: (0.5 * (e[1:] + e[:-1]))[:, None] + (0.5 * (e[1:] - e[:-1]))[:, None] * t[None]
    nx, ny = nodes(ex), nodes(ey)
    x9 = torch.tensor(np.stack([np.broadcast_to(nx[:, None, :, None], (8, 7, 3, 3)), np.broadcast_to(ny[None, :, None, :], (8, 7, 3, 3))], -1)
                      .reshape(504, 2), dtype=torch.float32)
    q9 = torch.tensor(np.broadcast_to(np.outer(w1, w1).reshape(1, 9) / 4.0, (56, 9)).reshape(504).copy(), dtype=torch.float32)
    xp, qp = _pad16(x9, q9, 9)
    tgt = lambda M: torch.randn(B, M, O, generator=g).to(dev)
    wo = lambda M: (0.2 + 1.8 * torch.rand(B, M, generator=g)).to(dev)
    return NS(nef=nef, params=nef.init(1, device=dev), p=p, a=a, s=s, x4=x4.to(dev), q4=q4.to(dev), x9=x9.to(dev), q9=q9.to(dev), xp=xp.to(dev),
              qp=qp.to(dev), y128=tgt(128), w128=wo(128), y56=tgt(56), w56=wo(56))


def grouped_routes(c, prec, tag):
    """what the parent commit has: the fused grouped step, the composed grouped route, the padded 3 x 3 cells"""
    nef, P = c.nef, c.params
    xb = lambda x: x[None].expand(B, -1, -1)
    qb = lambda q: q[None].expand(B, -1).contiguous()
    x4, q4, xp, qp = xb(c.x4), qb(c.q4), xb(c.xp), qb(c.qp)

    def fit_step_g():
        nef.mse_value_and_cell_grads(P, x4, c.p, c.a, c.s, c.y128, 4, qweight=q4, obs_weight=c.w128, grad_scale=float(B))

    def composed_g():
        hp, ha, hs = (t.detach().clone().requires_grad_(True) for t in (c.p, c.a, c.s))
        (nef.cell_mse(nef.apply(P, x4, hp, ha, hs), c.y128, 4, q4, c.w128) * float(B)).backward()

    def fit_step_g_padded():
        nef.mse_value_and_cell_grads(P, xp, c.p, c.a, c.s, c.y56, 16, qweight=qp, obs_weight=c.w56, grad_scale=float(B))
    return {f"{tag}fit_step_g_{prec}": fit_step_g, f"{tag}composed_g_{prec}": composed_g, f"{tag}fit_step_g_padded_{prec}": fit_step_g_padded}


def operator_routes(c, prec):
    from enf_pde_amd.fitting import SparseObservations
    nef, P = c.nef, c.params
    dev = c.p.device
    op4 = SparseObservations.from_groups(np.full(128, 4), c.q4.cpu(), device=dev)
    op9 = SparseObservations.from_groups(np.full(56, 9), c.q9.cpu(), device=dev)
    x4, x9 = c.x4[None].expand(B, -1, -1), c.x9[None].expand(B, -1, -1)

    def fit_step_a_g4():
        nef.mse_value_and_operator_grads(P, x4, c.p, c.a, c.s, c.y128, op4, obs_weight=c.w128, grad_scale=float(B))

    def fit_step_a_3x3():
        nef.mse_value_and_operator_grads(P, x9, c.p, c.a, c.s, c.y56, op9, obs_weight=c.w56, grad_scale=float(B))
    return {f"fit_step_a_g4_{prec}": fit_step_a_g4, f"fit_step_a_3x3_{prec}": fit_step_a_3x3}, {"g4": (op4, 512), "3x3": (op9, 504)}


def kernel_routes(dev, ops):
    """enf_mse_value_grad_a on a decode that exists, without (kernel 1) and with d out (kernels 1 and 2): B = 16, O = 1"""
    from enf_pde_amd.fitting import SparseObservations
    lib = _lib.load()
    g = torch.Generator().manual_seed(1)
    ops = dict(ops)
    rays = SparseObservations.from_groups(np.full(64, 128), (torch.rand(64 * 128, generator=g) / 128).numpy(), device=dev)
    ops["rays64x128"] = (rays, 64 * 128)
    fns, keep = {}, []
    for name, (op, N) in ops.items():
        out, y = torch.randn(B, N, O, generator=g).to(dev), torch.randn(B, op.M, O, generator=g).to(dev)
        w, dout, loss = torch.rand(B, op.M, generator=g).to(dev), torch.empty(B, N, O, device=dev), torch.zeros(1, device=dev)
        scr = torch.empty(int(lib.enf_mse_a_scratch_bytes(B, op.M, O, 1, 0)), device=dev, dtype=torch.uint8)
        s = op.struct()
        keep.append((op, out, y, w, dout, loss, scr, s))
        st = _lib.stream(dev)

        def call(with_dout, out=out, y=y, w=w, dout=dout, loss=loss, scr=scr, s=s, N=N):
            _lib.check(lib.enf_mse_value_grad_a(_lib.ptr(out), _lib.ptr(y), B, N, O, ctypes.byref(s), _lib.ptr(w), None, float(B),
                                                _lib.ptr(dout) if with_dout else None, _lib.ptr(loss), None, _lib.ptr(scr), scr.numel(), 0, st))
        fns[f"kernel1_{name}"] = lambda call=call: call(False)
        fns[f"kernels12_{name}"] = lambda call=call: call(True)
    return fns, keep


def settle(fns, calls):
    """every route untimed, before the first timed one"""
    for fn in fns.values():
        for _ in range(calls):
            fn()
    torch.cuda.synchronize()


def child(args):
    dev = torch.device("cuda:0")
    fns = {}
    for prec in ("bf16", "f32"):
        fns.update(grouped_routes(setup(dev, prec), prec, "parent_"))
    settle(fns, args.settle)
    print(json.dumps({k: median_ms(fn, args.iters, args.warmup) for k, fn in fns.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--settle", type=int, default=20, help="untimed calls of every route before the first timed one, in every process")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--root", default=None, help="(child) the tree whose package and library are imported")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    dev = torch.device("cuda:0")
    res = {"shape": {"B": B, "Z": Z, "D": D, "H": H, "O": O, "a": "128 groups of 4, N = 512", "b": "56 cells of 3 x 3, N = 504; padded to 16: N = 896",
                     "c": "B = 16, O = 1: the operators of (a) and (b), and 64 rays of 128 nodes (N = 8192)"},
           "clock": "hipEvent pair around each call, median of the calls; medians of all rounds listed, the best reported; *_x50: per call of 50 "
                    "back-to-back calls inside one event pair",
           "iters": args.iters, "rounds": args.rounds}
    fns, batch = {}, {}
    ops = None
    for prec in ("bf16", "f32"):
        c = setup(dev, prec)
        f, ops = operator_routes(c, prec)
        fns.update(f)
        fns.update(grouped_routes(c, prec, "this_tree_"))
    kf, keep = kernel_routes(dev, ops)
    fns.update(kf)
    for k, f in kf.items():
        fns[k + "_x50"], batch[k + "_x50"] = f, 50
    times = {k: [] for k in fns}
    for _ in range(args.rounds):                     # interleaved: the routes see the same box state
        settle(fns, args.settle)                     # (every round: the GPU sat idle while the child process started)
        for k, fn in fns.items():
            times[k].append(median_ms(fn, args.iters, args.warmup, batch.get(k, 1)))
        if args.parent:                              # the parent commit's calls, in a process of its own
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", args.parent, "--iters", str(args.iters),
                                  "--warmup", str(args.warmup), "--settle", str(args.settle)], check=True, capture_output=True, text=True,
                                 timeout=600).stdout
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
