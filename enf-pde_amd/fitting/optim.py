"""Outer-loop optimisers with optax's update rules (the reference builds them in
experiments/fitting/trainers/pde_trainer.py:60-67):

    nef_opt          = optax.chain(optax.clip_by_global_norm(1.0), optax.adamw(lr_enf))
    autodecoder_opt  = optax.adam(lr_codes)
    meta_sgd_opt     = optax.adam(lr_meta_sgd)          # followed by clip(lrs, 1e-6, 10), pde_trainer.py:272

optax is not installed here and its version is un-pinned in the reference (README.md:31); the rules below are
optax's published ones (scale_by_adam with bias correction, eps outside the square root, eps_root = 0;
adamw = scale_by_adam -> add_decayed_weights(1e-4) -> scale(-lr); clip_by_global_norm: g / max(1, ||g|| / c)).
Functional style like optax: ``init(params) -> state``, ``update(grads, state, params) -> (new_params, state)``;
trees are flat lists of tensors.  Pure tensor code, device-agnostic (tested on CPU against oracle/optim_ref_np.py).

``table_adam_update`` is the one native piece: optax adam over an auto-decoder's whole latent table from the gathered gradient
rows of a batch, one HIP launch (enf_table_adam_update, include/enf_hip.h).
"""
import struct

import torch


def global_norm(tensors):
    norms = torch._foreach_norm([t.detach() for t in tensors])
    return torch.linalg.vector_norm(torch.stack(norms))


def clip_by_global_norm(grads, max_norm=1.0):
    """optax.clip_by_global_norm: every leaf scaled by 1 / max(1, ||g||_2 / max_norm)."""
    scale = 1.0 / torch.clamp(global_norm(grads) / max_norm, min=1.0)
    return list(torch._foreach_mul(list(grads), scale))


class Adam:
    """optax.adam(lr, b1=0.9, b2=0.999, eps=1e-8); weight_decay > 0 gives optax.adamw (decoupled, default 1e-4)."""

    def __init__(self, lr, b1=0.9, b2=0.999, eps=1e-8, weight_decay=0.0):
        self.lr, self.b1, self.b2, self.eps, self.wd = float(lr), b1, b2, eps, weight_decay

    def init(self, params):
        return {"count": 0, "mu": [torch.zeros_like(p) for p in params], "nu": [torch.zeros_like(p) for p in params]}

    @torch.no_grad()
    def update(self, grads, state, params):
        # multi-tensor (foreach) arithmetic: a handful of launches for the whole tree instead of ~10 per leaf
        count = state["count"] + 1
        grads = [g.to(p.dtype) for g, p in zip(grads, params)]
        mu = torch._foreach_mul(state["mu"], self.b1)
        torch._foreach_add_(mu, grads, alpha=1 - self.b1)
        nu = torch._foreach_mul(state["nu"], self.b2)
        torch._foreach_addcmul_(nu, grads, grads, value=1 - self.b2)
        c1, c2 = 1 - self.b1 ** count, 1 - self.b2 ** count
        den = torch._foreach_div(nu, c2)
        torch._foreach_sqrt_(den)
        torch._foreach_add_(den, self.eps)
        upd = torch._foreach_div(mu, den)
        torch._foreach_div_(upd, c1)
        if self.wd:
            torch._foreach_add_(upd, params, alpha=self.wd)
        new = torch._foreach_add(params, upd, alpha=-self.lr)
        return list(new), {"count": count, "mu": list(mu), "nu": list(nu)}


def scatter_rows(grads, idx, num_rows):
    """Gathered gradient rows (nidx, Z, width) -> dense (num_rows, Z, width): row s is the sum of the rows j with idx[j] == s,
    added in increasing j on CPU tensors (duplicates are summed); an index outside [0, num_rows) is dropped.  What enf_table_adam_update does
    per element, as torch ops: the CPU path below and the dense gradients a multi-rank step all-reduces use it."""
    idx = torch.as_tensor(idx, dtype=torch.int64)
    out = []
    for g in grads:
        d = torch.zeros((num_rows,) + tuple(g.shape[1:]), dtype=g.dtype, device=g.device)
        if g.is_cuda:        # no host round trip; index_add_ adds duplicates with atomics there, so their order is not fixed
            ok = ((idx >= 0) & (idx < num_rows)).to(g.device)
            d.index_add_(0, torch.where(ok, idx.to(g.device), torch.zeros_like(ok, dtype=torch.int64)), g * ok[:, None, None].to(g.dtype))
        else:
            for j, s in enumerate(idx.tolist()):         # a batch size: in index order, so that the sum's bits are the kernel's
                if 0 <= s < num_rows:
                    d[s] += g[j]
        out.append(d)
    return out


def _f32(v):
    return struct.unpack("f", struct.pack("f", float(v)))[0]


def _table_adam_scalars(opt, count):
    """(b1, b2, c1, c2) of one call: b1 and b2 as the float32 values the kernel receives, and the bias corrections
    c = 1 - b^count formed in double from THOSE, so that the step is exactly optax adam with the rounded decay rates (with the
    corrections of the unrounded ones the first step's nu' / c2 would be off by 1.3e-5: 0.999 is 0.99900001 in float32)."""
    b1, b2 = _f32(opt.b1), _f32(opt.b2)
    return b1, b2, 1.0 - b1 ** count, 1.0 - b2 ** count


@torch.no_grad()
def table_adam_update(opt, state, tables, grads, idx=None, inplace=False):
    """One optax adam step of ``opt`` (an Adam without weight decay) over a latent table, from the gradient rows of a batch.

    tables : list of (S, Z, width) float32 tensors (the components p_pos, p_ori, a, gaussian_window)
    state  : {"count", "mu", "nu"} as ``opt.init(tables)`` makes it
    grads  : list of (nidx, Z, width) tensors, the gradient w.r.t. the rows ``idx`` (nidx,) long of every table; a gradient may
             be a column slice of a wider tensor (the fit step's dp = [p_pos | p_ori]).  Duplicate indices are summed, an index
             outside [0, S) is ignored.  ``idx`` None: the gradients are dense, (S, Z, width), row j is table row j.
    Rows outside the batch get a zero gradient and move by their momentum alone (optax adam is dense).  Returns
    (new_tables, new_state) like ``Adam.update``; with ``inplace`` the tables and moments are overwritten and returned.
    On a GPU this is ONE launch of enf_table_adam_update for up to four components; on CPU tensors the same arithmetic in
    torch ops."""
    if opt.wd:
        raise ValueError("table_adam_update is optax.adam: the optimiser must not carry weight decay")
    tables, grads = list(tables), list(grads)
    if not tables or len(grads) != len(tables) or len(state["mu"]) != len(tables) or len(state["nu"]) != len(tables):
        raise ValueError("tables, grads and the optimiser state must hold the same, non-zero number of tensors")
    S, Z = tables[0].shape[0], tables[0].shape[1]
    nidx = S if idx is None else int(idx.numel())
    for x, g in zip(tables, grads):
        if x.dim() != 3 or tuple(x.shape[:2]) != (S, Z) or tuple(g.shape) != (nidx, Z, x.shape[2]):
            raise ValueError(f"table {tuple(x.shape)} / gradient {tuple(g.shape)}: expected (S, Z, width) and ({nidx}, Z, width)")
    count = state["count"] + 1
    b1, b2, c1, c2 = _table_adam_scalars(opt, count)
    if not tables[0].is_cuda:
        dense = [g.float() for g in grads] if idx is None else scatter_rows([g.float() for g in grads], idx, S)
        f = lambda v: torch.tensor(v, dtype=torch.float32)
        new_x, new_mu, new_nu = [], [], []
        for x, mu, nu, g in zip(tables, state["mu"], state["nu"], dense):
            m = f(b1) * mu + f(1.0 - b1) * g
            v = f(b2) * nu + f(1.0 - b2) * (g * g)
            xn = x - f(opt.lr) * (m / f(c1)) / (torch.sqrt(v / f(c2)) + f(opt.eps))
            if inplace:
                xn, m, v = x.copy_(xn), mu.copy_(m), nu.copy_(v)
            new_x.append(xn), new_mu.append(m), new_nu.append(v)
        return new_x, {"count": count, "mu": new_mu, "nu": new_nu}
    from .. import _lib
    lib = _lib.load()
    dev = tables[0].device
    keep, outs = [], ([], [], [])
    if idx is not None:
        idx = idx.to(device=dev, dtype=torch.int64).contiguous()
    st = _lib.stream(dev)
    for lo in range(0, len(tables), _lib.ENF_ADAM_MAX_SEGMENTS):
        segs = (_lib.EnfAdamSegment * _lib.ENF_ADAM_MAX_SEGMENTS)()
        n = 0
        for x, mu, nu, g in list(zip(tables, state["mu"], state["nu"], grads))[lo:lo + _lib.ENF_ADAM_MAX_SEGMENTS]:
            ins = [x, mu, nu]
            for t in ins:
                if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                    raise ValueError("tables and moments must be contiguous float32 tensors on one device")
            w = x.shape[2]
            if g.dtype != torch.float32 or g.device != dev or g.stride(2) != 1 or g.stride(0) != g.stride(1) * Z or g.stride(1) < w:
                g = g.to(device=dev, dtype=torch.float32).contiguous()
            new = ins if inplace else [torch.empty_like(t) for t in ins]
            keep += ins + [g]
            segs[n] = _lib.EnfAdamSegment(x.data_ptr(), mu.data_ptr(), nu.data_ptr(), g.data_ptr(), new[0].data_ptr(),
                                          new[1].data_ptr(), new[2].data_ptr(), w, g.stride(1))
            for o, t in zip(outs, new):
                o.append(t)
            n += 1
        _lib.launch(dev, lib.enf_table_adam_update, n, segs, S, Z, idx.data_ptr() if idx is not None else None, nidx,
                    opt.lr, b1, b2, opt.eps, c1, c2, st)
    return outs[0], {"count": count, "mu": outs[1], "nu": outs[2]}


def AdamW(lr, weight_decay=1e-4, **kw):
    return Adam(lr, weight_decay=weight_decay, **kw)
