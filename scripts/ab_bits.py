#!/usr/bin/env python3
"""Bit-for-bit A/B of two builds of the library on a fixed, seeded list of calls.

  python scripts/ab_bits.py [--calls small|forward_mode] OLD/libenf_hip.so NEW/libenf_hip.so

  small (the default)   the small loss / gather / partial-sum kernels
  forward_mode          the forward-mode kernels of enf_tangent.hip and enf_second.hip: enf_field_tangent, enf_field_tangent_x,
                        enf_field_second_x and the three Gauss-Newton products (profiles/README.md, forward_mode_jet_ab.txt)

For each library one fresh child process (ENF_HIP_LIB set, enf_pde_amd/_lib.py) runs the fixed, seeded list of calls below and writes
every output's raw bytes; this process compares them and prints one line per call.  Exit status 1 if any output differs.
The shapes are the smallest that reach every branch of the kernels (profiles/README.md, small_kernels_ab.txt).  Outputs that a
float atomic forms in an order the hardware picks (the plain MSE loss over more than two blocks) are not comparable between two runs of
ONE library either: they are recorded under a name ending in '~' and reported, not compared."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def child(out_path):
    import ctypes
    import numpy as np
    import torch
    from enf_pde_amd import _lib
    from enf_pde_amd.fitting.ode_models import ponita_ode_g as G
    from enf_pde_amd.enf.models import _train
    from oracle import enf_ref_np as R
    from tests.helpers import make_cfg, make_inputs, build_nef

    dev = torch.device("cuda:0")
    lib, P, DET = _lib.load(), _lib.ptr, _lib.ENF_MSE_DETERMINISTIC
    st = _lib.stream(dev)
    res = {}

    def put(name, *ts):
        torch.cuda.synchronize()
        for i, t in enumerate(ts):
            res[f"{name} [{i}]"] = t.detach().cpu().contiguous().view(torch.uint8).numpy().copy()

    def rnd(seed, *shape):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)

    # ---- the MSE family: plain, one weight per O values (O = 1, 3), one weight per value; atomic and deterministic
    for n in (9, 258, 262146):
        out, tgt = rnd(n, n), rnd(n + 1, n)
        for form, O in (("plain", 1), ("w", 1), ("w", 3), ("cw", 1)):
            nw = n // O
            w = rnd(n + 2 + O, nw).abs()
            w[::3] = 0.0                                        # exact zeros, NaN targets under them
            t = tgt.clone()
            if form != "plain":
                t.view(nw, O)[w == 0] = float("nan")
            for flags in (0, DET):
                dout, loss = torch.empty(n, device=dev), torch.zeros(1, device=dev)
                nb = int(lib.enf_mse_scratch_bytes(n, flags))
                scr = torch.empty(max(nb, 1), device=dev, dtype=torch.uint8)
                if form == "plain" and not flags:
                    _lib.launch(dev, lib.enf_mse_value_grad, P(out), P(t), n, 1.5, P(dout), P(loss), st)
                elif form == "plain":
                    _lib.launch(dev, lib.enf_mse_value_grad_ex, P(out), P(t), n, 1.5, P(dout), P(loss), P(scr), nb, flags, st)
                elif form == "w":
                    _lib.launch(dev, lib.enf_mse_value_grad_w, P(out), P(t), P(w), n, O, 1.5, P(dout), P(loss), P(scr), nb, flags, st)
                else:
                    _lib.launch(dev, lib.enf_mse_value_grad_cw, P(out), P(t), P(w), n, 1.5, P(dout), P(loss), P(scr), nb, flags, st)
                name = f"mse {form} O={O} n={n} {'det' if flags else 'atomic'}"
                put(name + " dout", dout)
                put(name + " loss" + ("~" if not flags and n > 512 else ""), loss)

    # ---- enf_signal_sum
    for N in (1, 255, 256, 257, 1000):
        err = rnd(N, 3, N) * torch.logspace(-3, 3, N, device=dev)
        loss_b = torch.empty(3, device=dev)
        _lib.launch(dev, lib.enf_signal_sum, P(err), 3, N, 1.0 / (3.0 * N), P(loss_b), st)
        put(f"signal_sum N={N}", loss_b)

    # ---- the four gathers
    B, Z, N, Ns, S1, dx = 3, 5, 40, 7, 3, 2
    gen = torch.Generator().manual_seed(7)
    for O in (1, 3):
        coords, img = rnd(20, N, dx), rnd(21, B, N, O)
        lat0 = [rnd(22, 1, Z, 4), rnd(23, 1, Z, 9)]
        weight, cweight = rnd(24, B, N).abs(), rnd(25, B, N, O).abs()
        m2 = torch.randint(0, N, (Ns, S1), generator=gen).to(dev)
        m3 = torch.randint(0, N, (B, Ns, S1), generator=gen)
        m3[0, 1, 0], m3[1, 2, 1], m3[2, 6, 2] = -1, N, N + 5
        m3 = m3.to(dev)
        m2bad = m2.clone()
        m2bad[1, 0], m2bad[3, 2] = -1, N

        def gather(entry, masks, wgt, per_value=False):
            per_signal = masks.dim() == 3
            lat = [torch.full((B, Z, v.shape[2]), -7.0, device=dev) for v in lat0]
            comps = (_lib.EnfFitComponent * _lib.ENF_SGD_MAX_SEGMENTS)()
            for i, v in enumerate(lat0):
                comps[i] = _lib.EnfFitComponent(v.data_ptr(), lat[i].data_ptr(), v.shape[2], 0)
            xs = torch.full((S1, B, Ns, dx) if per_signal else (S1, Ns, dx), -7.0, device=dev)
            ys = torch.full((S1, B, Ns, O), -7.0, device=dev)
            ws = torch.full((S1, B, Ns, O) if per_value else (S1, B, Ns), -7.0, device=dev)
            losses = torch.full((S1,), -7.0, device=dev)
            head = (len(lat0), comps, B, Z, N, Ns, S1, dx, O, P(coords), P(img), P(masks), P(xs), P(ys), P(losses))
            if entry == "enf_fit_inputs":
                _lib.launch(dev, lib.enf_fit_inputs, *head, st)
            elif entry == "enf_fit_inputs_cw":
                _lib.launch(dev, lib.enf_fit_inputs_cw, *head, P(wgt), P(ws), 1 if per_signal else 0, st)
            else:
                _lib.launch(dev, getattr(lib, entry), *head, P(wgt), P(ws) if (wgt is not None or per_signal) else P(None), st)
            return (*lat, xs, ys, ws, losses)

        put(f"fit_inputs O={O}", *gather("enf_fit_inputs", m2, None))
        put(f"fit_inputs_w O={O}", *gather("enf_fit_inputs_w", m2, weight))
        put(f"fit_inputs_b O={O} weight", *gather("enf_fit_inputs_b", m3, weight))
        put(f"fit_inputs_b O={O} no weight", *gather("enf_fit_inputs_b", m3, None))
        put(f"fit_inputs_cw O={O} per-signal masks", *gather("enf_fit_inputs_cw", m3, cweight, True))
        put(f"fit_inputs_cw O={O} shared masks", *gather("enf_fit_inputs_cw", m2bad, cweight, True))

    # ---- the latent ODE's partial sums (through the autograd functions of fitting/ode_models/ponita_ode_g.py)
    for B_, Z_, J, C in ((2, 5, 16, 16), (16, 64, 64, 256)):
        a, kb, g = rnd(30, B_, Z_, C), rnd(31, B_, Z_, Z_, J), rnd(32, B_, Z_, C)
        W, bias = rnd(33, J, C).requires_grad_(True), rnd(34, C).requires_grad_(True)
        G.sep_gconv(a, kb, W, bias).backward(g)
        put(f"ode_conv_backward_weight B={B_} Z={Z_} J={J} C={C}", W.grad, bias.grad)
    H = 32
    for Rr in (40, 16 * 256 + 40):
        x = rnd(40, Rr, H).requires_grad_(True)
        prm = [t.requires_grad_(True) for t in (rnd(41, H), rnd(42, H), rnd(43, H, 2 * H) * 0.2, rnd(44, 2 * H), rnd(45, 2 * H, H) * 0.2,
                                                rnd(46, H))]
        G._LatentMLP.apply(x, *prm).backward(rnd(47, Rr, H))
        put(f"ode_block_backward H={H} R={Rr}", x.grad, *[t.grad for t in prm])
    I, H1, J = 2, 32, 32
    for Pn in (100, 16 * 4 * 12 + 5, 40000):
        inv = rnd(50, Pn, I).requires_grad_(True)
        prm = [t.requires_grad_(True) for t in (rnd(51, I + I * I + I ** 3 + I ** 4, H1) * 0.3, rnd(52, H1), rnd(53, H1, J) * 0.2, rnd(54, J))]
        G._KernelBasis.apply(inv, 3, *prm).backward(rnd(55, Pn, J))
        put(f"ode_basis_backward I={I} H1={H1} J={J} P={Pn}", inv.grad, *[t.grad for t in prm])

    # ---- the decoder: shared-latent fit step (enf_launch_mse_shared) and enf_backward_all (enf_xtd_reduce_kernel)
    def tt(v, grad=False):
        return torch.tensor(v, dtype=torch.float32, device=dev, requires_grad=grad)
    cfg = make_cfg("rel_pos_periodic", D=64, H=2, C=16, O=1)
    prm = R.init_params(3, cfg, jitter=0.1)
    B, N, Z = 3, 50, 7
    x, p, a, s = make_inputs(cfg, B, N, Z, 4)
    p, a, s = (np.repeat(v[:1], B, 0) for v in (p, a, s))
    rng = np.random.default_rng(5)
    y, w = rng.standard_normal((B, N, 1)), np.abs(rng.standard_normal((B, N)))
    w[:, ::4] = 0.0
    nef = build_nef(cfg, "bf16")
    nef.pair_variants = ("latent_split", "z_fold")
    params = nef.load_params(prm, device=dev)
    applies = int(lib.enf_shared_backward_applies(ctypes.byref(nef._desc(B, N, Z)), _lib.ENF_FIT_SHARED_LATENTS))
    for wt in (None, w):
        with torch.no_grad():
            r = nef.mse_value_and_latent_grads(params, tt(x[0])[None].expand(B, -1, -1), tt(p), tt(a), tt(s), tt(y), grad_scale=float(B),
                                               weight=None if wt is None else tt(wt), shared_latents=True)
        put(f"shared-latent fit step B={B} N={N} Z={Z} D=64 H=2 {'weight' if wt is not None else 'no weight'} (applies={applies}) loss", r[0])
        put(f"shared-latent fit step B={B} N={N} Z={Z} D=64 H=2 {'weight' if wt is not None else 'no weight'} (applies={applies}) grads~", *r[1:])

    B, N, Z = 2, 50, 7
    x, p, a, s = make_inputs(cfg, B, N, Z, 6)
    wo = np.random.default_rng(7).standard_normal((B, N, 1))
    budget = _train.STORE_BUDGET_BYTES
    for prec, chunked in (("f32", False), ("bf16", False), ("f32", True)):
        _train.STORE_BUDGET_BYTES = Z * N * 64 * (7 + 8) * 4 + (1 << 20) if chunked else budget      # chunked: one signal's store per pass
        nef = build_nef(cfg, prec)
        nef.deterministic = True
        params = nef.load_params(prm, device=dev)
        ts_ = nef.param_tensors(params)
        for t in ts_:
            t.requires_grad_(True)
        lp, la, ls = tt(p, True), tt(a, True), tt(s, True)
        (nef.apply(params, tt(x), lp, la, ls) * tt(wo)).sum().backward()
        put(f"backward_all B={B} N={N} Z={Z} D=64 H=2 {prec}{' chunked over signals' if chunked else ''}", lp.grad, la.grad, ls.grad,
            *[t.grad for t in ts_ if t.grad is not None])
    _train.STORE_BUDGET_BYTES = budget
    np.savez(out_path, **res)


def child_forward_mode(out_path):
    """Every compiled (D, H) in both precisions at B = 2, N = 50 (a partly filled query group, a clamped tail) and 70 (a second
    workgroup), Z = 1, 2, 7 (4, 2, 1 query groups; at Z = 7 one wave is inactive in the last iteration), O = 2; at (64, 2) also O = 32,
    the seven served invariants, rel_pos at dx = 1 and 3, the window off, x / xdot expanded with stride 0 and the far-logit case of
    tests/test_gpu_second.py (the softmax's rescale branch).  The products run deterministic (their backward pair kernel adds with
    float atomics otherwise) on weights with exact zeros.  No atomics anywhere: every output is compared."""
    import numpy as np
    import torch
    from enf_pde_amd.fitting.operators import SparseObservations
    from oracle import enf_ref_np as R
    from tests.helpers import make_cfg, make_inputs, build_nef

    dev = torch.device("cuda:0")
    res = {}

    def tt(v):
        return torch.tensor(v, dtype=torch.float32, device=dev)

    def put(name, *ts):
        torch.cuda.synchronize()
        for i, t in enumerate(t for t in ts if t is not None):
            res[f"{name} [{i}]"] = t.detach().cpu().contiguous().view(torch.uint8).numpy().copy()

    def run(tag, cfg, B, N, Z, inputs=None, expand=False, products=True):
        O = cfg["num_out"]
        prm = R.init_params(3, cfg, jitter=0.1)
        x, p, a, s = inputs or make_inputs(cfg, B, N, Z, 4)
        rng = np.random.default_rng(11)
        xd, dp, da, ds = (rng.standard_normal(v.shape) for v in (x, p, a, s))
        w, cw, ow = np.abs(rng.standard_normal((B, N))), np.abs(rng.standard_normal((B, N, O))), np.abs(rng.standard_normal((B, N // 2)))
        w[:, ::4], cw[:, ::3], ow[:, ::5] = 0.0, 0.0, 0.0          # exact zeros
        qw = np.abs(rng.standard_normal((B, N))) + 0.1
        G = 4 if N % 4 == 0 else 2                                 # G divides N: 2 at N = 50 and 70, 4 at N = 52 and 72
        rows = np.repeat(np.arange(N // 2), 3)                     # an operator of M = N / 2 rows, three entries each, across tiles
        op = SparseObservations.from_coo(rows, (rows * 2 + np.tile([0, 1, 17], N // 2)) % N, rng.standard_normal(rows.size), N // 2, N,
                                         device=dev)
        for prec in ("bf16", "f32"):
            nef = build_nef(cfg, prec)
            nef.deterministic = True
            P = nef.load_params(prm, device=dev)
            tx, txd = tt(x), tt(xd)
            if expand:
                tx, txd = tt(x[0])[None].expand(B, -1, -1), tt(xd[0])[None].expand(B, -1, -1)
            lat = (tt(p), tt(a), tt(s))
            v = dict(dp=tt(dp), da=tt(da), dwindow=tt(ds))
            name = f"{tag} B={B} N={N} Z={Z} O={O} {prec}"
            put(f"tangent {name}", *nef.tangent(P, tx, *lat, **v))
            put(f"tangent, no out {name}", *nef.tangent(P, tx, *lat, return_out=False, **v))
            put(f"tangent_x {name}", *nef.tangent(P, tx, *lat, xdot=txd, **v))
            put(f"tangent_x, xdot alone {name}", *nef.tangent(P, tx, *lat, xdot=txd))
            put(f"second_x {name}", *nef.second_derivative(P, tx, *lat, txd))
            put(f"second_x, no out, no tan {name}", *nef.second_derivative(P, tx, *lat, txd, return_out=False, return_first=False))
            if not products:
                continue
            gv = dict(vp=v["dp"], va=v["da"], vwindow=v["dwindow"], grad_scale=3.0)
            nef.gn_reserve(B, N, Z, dev, op=op)
            put(f"gn_product, weight {name}", *nef.gn_product(P, tx, *lat, weight=tt(w), **gv))
            put(f"gn_product, channel weight {name}", *nef.gn_product(P, tx, *lat, channel_weight=tt(cw), **gv))
            put(f"gn_product_g G={G} {name}", *nef.gn_cell_product(P, tx, *lat, G, qweight=tt(qw),
                                                                  obs_weight=tt(np.abs(rng.standard_normal((B, N // G))) * (np.arange(N // G) % 3 > 0)), **gv))
            put(f"gn_product_a {name}", *nef.gn_operator_product(P, tx, *lat, op, obs_weight=tt(ow), **gv))

    for D, H in ((64, 1), (64, 2), (64, 4), (128, 1), (128, 2)):
        for N in (50, 70):
            for Z in (1, 2, 7):
                run(f"rel_pos_periodic D={D} H={H}", make_cfg("rel_pos_periodic", D=D, H=H, C=8, O=2), 2, N, Z)
    run("rel_pos_periodic D=64 H=2, both output tiles", make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=32), 2, 50, 7)
    for N in (52, 72):                                             # enf_gn_product_g at G = 4, which has to divide N
        run("rel_pos_periodic D=64 H=2, G = 4", make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), 2, N, 7)
    for inv in ("latitude_periodic", "polar_periodic", "ponita", "abs_pos", "rel_pos", "norm_rel_pos"):
        run(f"{inv} D=64 H=2", make_cfg(inv, D=64, H=2, C=8, O=2), 2, 50, 7)
    for dx in (1, 3):
        run(f"rel_pos dx={dx} D=64 H=2", make_cfg("rel_pos", D=64, H=2, C=8, O=2, num_in=dx), 2, 50, 7)
    run("rel_pos_periodic D=64 H=2, no window", make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2, use_window=False), 2, 50, 7)
    run("rel_pos_periodic D=64 H=2, x and xdot stride 0", make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), 2, 50, 7, expand=True)
    cfg = make_cfg("rel_pos", D=64, H=2, C=8, O=2)                  # tests/test_gpu_second.py, _far_first_case
    x, p, a, s = make_inputs(cfg, 3, 50, 7, 1)
    p[:, :4] = 3.0 + 0.2 * p[:, :4]
    s[:] = 0.3
    run("rel_pos D=64 H=2, far latents first", cfg, 3, 50, 7, inputs=(x, p, a, s))
    np.savez(out_path, **res)


CALLS = {"small": child, "forward_mode": child_forward_mode}


def main():
    args = sys.argv[1:]
    calls = "small"
    if len(args) >= 2 and args[0] == "--calls":
        calls, args = args[1], args[2:]
    if calls not in CALLS:
        sys.exit(__doc__)
    if len(args) == 2 and args[0] == "--child":
        return CALLS[calls](args[1])
    if len(args) != 2:
        sys.exit(__doc__)
    import numpy as np
    got = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, path in enumerate(args):
            out = os.path.join(tmp, f"{i}.npz")
            env = dict(os.environ, ENF_HIP_LIB=os.path.abspath(path))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--calls", calls, "--child", out], check=True, env=env, timeout=900)
            with np.load(out) as z:
                got.append({k: z[k] for k in z.files})
    old, new = got
    calls, bad, free = {}, 0, 0
    for k in old:
        calls.setdefault(k.rsplit(" [", 1)[0], []).append(k)
    for call, keys in calls.items():
        nbytes = sum(old[k].size for k in keys)
        same = all(k in new and old[k].shape == new[k].shape and np.array_equal(old[k], new[k]) for k in keys)
        if call.endswith("~"):
            free += 1
            print(f"{'equal' if same else 'differs (float atomics: run-to-run order)':8s} {nbytes:9d} bytes  {call[:-1]}  [not compared]")
        else:
            bad += not same
            print(f"{'equal' if same else 'DIFFERS':8s} {nbytes:9d} bytes  {call}")
    print(f"# {len(calls) - free} calls compared, {len(calls) - free - bad} equal byte for byte, {bad} differ; {free} atomic-order outputs reported only")
    sys.exit(1 if bad or set(old) != set(new) else 0)


if __name__ == "__main__":
    main()
