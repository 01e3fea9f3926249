#!/usr/bin/env python3
"""Every host sequence of the decoder once, over the shapes at which the launchers choose differently: the driver of a kernel-name
trace.  Run it under `rocprofv3 --kernel-trace --stats -- python scripts/launch_forms.py` on two builds of the library (ENF_HIP_LIB)
and compare the (kernel name, call count) lists: a refactor of the launchers must leave them identical
(profiles/launch_refactor_trace.txt).

Calls, each once per case: nef.apply without and with grad (the latent backward), mse_value_and_latent_grads (plain, weight,
channel_weight, return_errors, shared_latents, deterministic), eval_loss, jacobian, query_vjp, tangent without and with xdot,
gn_product, and a weight-gradient backward.  Cases: (D, H) = (64, 2) and (128, 2) in bf16 and f32 with rel_pos_periodic and rff, one
run-time-invariant case (rel_pos) and one ffn case; Z = 8; B N in {512, 8192, 16384, 40000} (B = 2), so that the tail runs 1, 2, 4
and 8 active waves and both weight rings, and the pair kernels both variants."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import enf_ref_np as R  # noqa: E402
from tests.helpers import make_cfg, make_inputs, build_nef  # noqa: E402
from tests.ffn_ref import build_nef_ffn, init_params_ffn  # noqa: E402

B, Z, O = 2, 8, 2
CASES = [(64, 2, "bf16", "rel_pos_periodic", "rff"), (64, 2, "f32", "rel_pos_periodic", "rff"),
         (128, 2, "bf16", "rel_pos_periodic", "rff"), (128, 2, "f32", "rel_pos_periodic", "rff"),
         (128, 2, "bf16", "rel_pos", "rff"), (64, 2, "bf16", "rel_pos_periodic", "ffn")]


def run(dev, D, H, prec, inv, emb, N):
    cfg = make_cfg(inv, D=D, H=H, C=16, O=O)
    ffn = emb == "ffn"
    nef = (build_nef_ffn if ffn else build_nef)(cfg, prec)
    params = nef.load_params((init_params_ffn if ffn else R.init_params)(0, cfg, jitter=0.1), device=dev)
    t = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    x, p, a, s = (t(v) for v in make_inputs(cfg, B, N, Z, 1))
    g = torch.Generator(device="cpu").manual_seed(N)
    rnd = lambda *shape: torch.randn(shape, generator=g).to(dev)
    y, w, cw = rnd(B, N, O), rnd(B, N).abs(), rnd(B, N, O).abs()
    done = []

    def call(name, fn):
        r = fn()
        torch.cuda.synchronize()
        done.append(name)
        return r

    with torch.no_grad():
        call("apply", lambda: nef.apply(params, x, p, a, s))
    pg, ag, sg = (v.clone().requires_grad_(True) for v in (p, a, s))
    call("apply + latent backward", lambda: nef.apply(params, x, pg, ag, sg).sum().backward())
    fit = lambda **kw: nef.mse_value_and_latent_grads(params, x, p, a, s, y, grad_scale=float(B), **kw)
    with torch.no_grad():
        call("fit", fit)
        call("fit weight", lambda: fit(weight=w))
        call("fit channel_weight", lambda: fit(channel_weight=cw))
        call("fit return_errors", lambda: fit(return_errors=True))
        xs = x[:1].expand(B, N, x.shape[-1])
        ps, as_, ss = (v[:1].expand(B, *v.shape[1:]).contiguous() for v in (p, a, s))
        call("fit shared_latents", lambda: nef.mse_value_and_latent_grads(params, xs, ps, as_, ss, y,
                                                                         grad_scale=float(B), shared_latents=True))
        nef.deterministic = True
        call("fit deterministic", fit)
        nef.deterministic = None
        call("eval_loss", lambda: nef.eval_loss(params, x, p, a, s, y))
        call("jacobian", lambda: nef.jacobian(params, x, p, a, s))
        call("query_vjp", lambda: nef.query_vjp(params, x, p, a, s, rnd(B, N, O)))
        if not ffn:
            call("tangent", lambda: nef.tangent(params, x, p, a, s, dp=rnd(*p.shape), da=rnd(*a.shape)))
            call("tangent xdot", lambda: nef.tangent(params, x, p, a, s, dp=rnd(*p.shape), xdot=rnd(*x.shape)))
            call("gn_product", lambda: nef.gn_product(params, x, p, a, s, vp=rnd(*p.shape), va=rnd(*a.shape)))
    ts = [v for v in nef.param_tensors(params) if v.numel() and v.is_floating_point()]
    for v in ts:
        v.requires_grad_(True)
    call("weight-gradient backward", lambda: nef.apply(params, x, p, a, s).sum().backward())
    assert all(v.grad is None or bool(torch.isfinite(v.grad).all()) for v in ts)
    print(f"launch_forms D={D} H={H} {prec} {inv} {emb} B N = {B * N}: {len(done)} calls")


def main():
    dev = torch.device("cuda:0")
    np.random.seed(0)
    for N in (256, 4096, 8192, 20000):
        for D, H, prec, inv, emb in CASES:
            run(dev, D, H, prec, inv, emb, N)
    print("launch_forms: done")


if __name__ == "__main__":
    main()
