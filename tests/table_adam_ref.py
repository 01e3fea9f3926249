"""Shared by tests/test_table_adam_host.py and tests/test_gpu_table_adam.py: seeded inputs of enf_table_adam_update / table_adam_update
and the float64 restatement of optax adam over a latent table (oracle/optim_ref_np.py) they are judged by.  Not a test module."""
import numpy as np
import torch

from oracle import optim_ref_np as OP

# the decay rates as the C-ABI carries them (float); the float64 reference computes with the same numbers
B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))
EPS = 1e-8
WIDTHS = (2, 1, 8, 1)                    # p_pos, p_ori, a, gaussian_window
NAMES = ("p_pos", "p_ori", "a", "gaussian_window")


def dense_gradient(grads, idx, S):
    """float64 (S, Z, width) per component: the sum of the rows j with idx[j] == s; an index outside [0, S) is dropped."""
    if idx is None:
        return [np.asarray(g, dtype=np.float64) for g in grads]
    out = []
    for g in grads:
        d = np.zeros((S,) + tuple(g.shape[1:]))
        for j, s in enumerate(idx):
            if 0 <= s < S:
                d[s] += np.asarray(g[j], dtype=np.float64)
        out.append(d)
    return out


def problem(idx, count, S=5, Z=5, widths=WIDTHS, seed=0, mixed_signs=False):
    """(tables, mu, nu, grads) as float32 torch tensors on the CPU.  ``idx``: a list of table rows, or None for a dense gradient.
    With four widths the gradients of the first two components are column slices of ONE (nidx, Z, w0 + w1) tensor, as the fit
    step returns the pose gradient.  count == 1 starts from zero moments; a later count from non-zero ones.  Unless
    ``mixed_signs``, every first moment carries the sign of the gradient it meets, as the moments of a consistent gradient history
    do: b1 mu + (1 - b1) g is then free of cancellation, and a relative bound can hold for every element (a sum that cancels has
    no relative accuracy in any arithmetic; ``mixed_signs`` cases are judged on the scale of the terms instead)."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * count + (0 if idx is None else len(idx)))
    nidx = S if idx is None else len(idx)
    r = lambda *s: torch.randn(*s, generator=g)
    tables = [r(S, Z, w) for w in widths]
    if len(widths) == 4:
        pose = r(nidx, Z, widths[0] + widths[1])
        grads = [pose[..., :widths[0]], pose[..., widths[0]:], r(nidx, Z, widths[2]), r(nidx, Z, widths[3])]
    else:
        grads = [r(nidx, Z, w) for w in widths]
    if count == 1:
        return tables, [torch.zeros_like(t) for t in tables], [torch.zeros_like(t) for t in tables], grads
    dense = dense_gradient([x.numpy() for x in grads], idx, S)
    mu, nu = [], []
    for t, d in zip(tables, dense):
        m = 0.5 * r(*t.shape).abs() + 0.01
        sign = torch.where(r(*t.shape) < 0, -torch.ones_like(m), torch.ones_like(m))
        if not mixed_signs:
            sign = torch.where(torch.tensor(d) != 0, torch.tensor(np.sign(d), dtype=torch.float32), sign)
        mu.append(m * sign)
        nu.append(0.3 * r(*t.shape) ** 2 + 1e-3)
    return tables, mu, nu, grads


def reference(tables, mu, nu, grads, idx, count, lr):
    """float64 optax adam on the same float32 inputs: (x', mu', nu', dense gradient) as lists of numpy arrays."""
    f = lambda ts: [t.detach().cpu().numpy().astype(np.float64) for t in ts]
    dense = dense_gradient(f(grads), idx, tables[0].shape[0])
    x, st = OP.adam_step(f(tables), dense, {"count": count - 1, "mu": f(mu), "nu": f(nu)}, lr=lr, b1=B1, b2=B2, eps=EPS)
    return x, st["mu"], st["nu"], dense


def check(got_x, got_mu, got_nu, ref, lr, label="", mu0=None):
    """mu' and nu' to rtol 1e-6, x' to 1e-5 lr + 1e-6 |x'|, every element (the issue's bounds: a few fp32 roundings of a
    six-operation expression).  With ``mu0`` (a mixed-sign case) mu' is judged on the scale of its terms,
    1e-6 (b1 |mu| + (1 - b1) |g|), the floating-point bound of a sum that may cancel, and x' through it likewise is not judged."""
    rx, rmu, rnu, dense = ref
    n = lambda t: t.detach().cpu().numpy().astype(np.float64)
    for k, (x, m, v) in enumerate(zip(got_x, got_mu, got_nu)):
        em, ev, ex = np.abs(n(m) - rmu[k]), np.abs(n(v) - rnu[k]), np.abs(n(x) - rx[k])
        scale_m = np.abs(rmu[k]) if mu0 is None else B1 * np.abs(n(mu0[k])) + (1 - B1) * np.abs(dense[k])
        print(f"{label} component {k}: max mu err / scale {np.max(em / np.maximum(scale_m, 1e-300)):.2e}, "
              f"max rel nu err {np.max(ev / np.maximum(np.abs(rnu[k]), 1e-300)):.2e}, max x err {ex.max():.2e} (lr {lr})")
        assert (em <= 1e-6 * scale_m).all(), (label, k, "mu")
        assert (ev <= 1e-6 * np.abs(rnu[k])).all(), (label, k, "nu")
        if mu0 is None:
            assert (ex <= 1e-5 * lr + 1e-6 * np.abs(rx[k])).all(), (label, k, "x")
