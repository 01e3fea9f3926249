"""Every launch form of the per-query tail (csrc/enf_tail.hip: TailForm) on both weight pipelines, in one process.

The launcher picks the 3-slot weight ring (LA2) for grids of at most 256 workgroups or fewer than eight active waves, else the 2-slot
ring with two workgroups per CU.  The small-shape tests only ever reach LA2; here every form runs
  * once on NQ = 40000 queries: eight active waves, 313 workgroups, the 2-slot ring (LA2 = false), and
  * on the same rows in chunks of 4096 queries (the last 3136): the forms with fewer-active-wave instantiations run one active wave,
    the others eight waves on 32 workgroups -- the 3-slot ring (LA2 = true) either way,
all through ONE library handle, so that every kernel's dynamic-LDS attribute is set beside every other's.

Forms: forward, forward + stash, evaluation, evaluation with per-channel weights, seeded backward from the stash, forward + seeded
backward, fused loss, fused loss with per-channel weights (the test library's enf_test_tail); the d out backward with the recompute
and from the stash (enf_backward_latents_ex), the weight-gradient backward likewise (enf_backward_all).  Every call returns ENF_OK.

The arithmetic of a query does not depend on the active waves, and the ring changes how weights are staged, not what is multiplied:
the per-query arrays (out, the stash, d ybar, delta, err; for the weight-gradient form the layer inputs it leaves in the stash region)
of the whole run EQUAL the concatenated chunks bit for bit.  Measured on the parent of the change that added this file (the hand-written
launcher ladder), MI355X: bit-equal for every form, shape and precision below, so equality is asserted, not a tolerance.

The fused loss scales d out by 1 / (n O) of its own launch, so a chunk's d ybar and delta are other numbers than the whole run's: for
that form the chunks are compared on the stash and err, and d ybar / delta against the whole run on the 3-slot ring with four active
waves (the test library's switch), same queries, same scale.

The scalar loss.  The other test's comparison (1e-6 relative in default mode, where the loss is a sum of float atomics in free order;
equal bits with loss_part) holds per launch geometry: a chunk's partial sums carry another 1 / n than the whole run's, so no bits can
be compared across the two.  Asserted: per chunk (at most 256 partials) default against deterministic mode within 1e-6 relative; on
the whole run equal bits from two deterministic launches, and the default-mode loss within LOSS_BOUND of the deterministic sum.  At
2500 partials the order of the atomics alone moves the sum by more than 1e-6: the parent commit measured 2.2e-6 (D = 64, H = 1, f32,
evaluation; 4.6e-7 .. 2.2e-6 over the four cases, this tree 4.6e-7 .. 1.5e-6 in the same run), so LOSS_BOUND is four times the
parent's largest figure, 8.8e-6, not 1e-6."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from tests.helpers import make_cfg, make_inputs, build_nef
from enf_pde_amd import _lib
from enf_pde_amd.enf.models._train import FROZEN

pytestmark = pytest.mark.gpu

NQ, CHUNK, Z, O = 40000, 4096, 2, 2
FWD, SAVE, EVAL, SEED, FWD_SEED, LOSS = range(6)
STAGES_PAIR, STAGES_STASH = 1 | 8 | 2, 1 | 4 | 16          # prologue + fold + pair; prologue + tail with the stash (on the caller's ybar)
REUSE = 1 | 2                                             # ENF_BWD_REUSE_PROLOGUE | ENF_BWD_REUSE_TAIL
LOSS_BOUND = 8.8e-6                                        # (see the docstring)


def _ptr(v):
    return ctypes.c_void_p(v.data_ptr()) if v is not None and v.numel() else ctypes.c_void_p(0)


def _regions(nef, ws, N):
    """the d ybar, delta and tail-stash regions of a B = 1 workspace as int32 rows (enf_layout.h: EnfWorkspace, 256-byte aligned)"""
    H, D = nef._Hp, nef._Dp
    HD, ACT = H * D, 2 * H * D + 2 * D + 2
    al = lambda v: (v + 255) & ~255
    stride = ((2 * HD + 32 + D) + 63) & ~63
    o, off = 0, {}
    for name, nb in (("lt", Z * stride), ("an", Z * (2 * D + 2)), ("kv", Z * 2 * HD), ("ybar", N * HD), ("lse", N * H), ("dybar", N * HD),
                     ("delta", N * H), ("act", N * ACT)):
        off[name] = o
        o = al(o + 4 * nb)
    cut = lambda name, w: ws[off[name]:off[name] + 4 * N * w].view(torch.int32).view(N, w).clone()
    return dict(dybar=cut("dybar", HD), delta=cut("delta", H), act=cut("act", ACT))


class _Case:
    """one decoder, its inputs, and the whole run's ybar / lse (one forward), shared by every form"""

    def __init__(self, cuda, D, H, precision):
        self.cuda, self.lib = cuda, _lib.load_test()
        cfg = make_cfg("rel_pos_periodic", D=D, H=H, C=12, O=O)
        self.nef = nef = build_nef(cfg, precision)
        params = nef.load_params(R.init_params(3, cfg, jitter=0.1), device=cuda)
        x, p, a, s = make_inputs(cfg, 1, NQ, Z, 5)
        t = lambda v: torch.tensor(v, dtype=torch.float32, device=cuda).contiguous()
        self.x, self.p, self.a, self.s = t(x), t(p), t(a), t(s)
        self.ts = [v.contiguous() for v in nef.param_tensors(params)]
        self.arrT = (ctypes.c_void_p * len(self.ts))(*[_ptr(v) for v in self.ts])
        self.st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
        desc = nef._desc(1, NQ, Z)
        self.blob = torch.empty(int(self.lib.enf_packed_weight_bytes(ctypes.byref(desc))), device=cuda, dtype=torch.uint8)
        _lib.launch(cuda, self.lib.enf_pack_weights, ctypes.byref(desc), self.arrT, _ptr(self.blob), self.st)
        HD = nef._Hp * nef._Dp
        self.ybar, self.lse = torch.empty((NQ, HD), device=cuda), torch.empty((NQ, nef._Hp), device=cuda)
        out = torch.empty((NQ, O), device=cuda)
        ws = self.workspace(desc)
        _lib.launch(cuda, self.lib.enf_forward_stages, ctypes.byref(desc), _ptr(self.x), NQ * 2, _ptr(self.p), _ptr(self.a), _ptr(self.s),
                    _ptr(self.blob), _ptr(out), _ptr(self.ybar), _ptr(self.lse), _ptr(ws), ws.numel(), STAGES_PAIR, self.st)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(self.ybar).all()) and bool(torch.isfinite(self.lse).all())
        g = torch.Generator(device="cpu").manual_seed(D + H)
        self.target = torch.randn((NQ, O), generator=g).to(cuda)
        self.dout = torch.randn((NQ, O), generator=g).to(cuda)
        self.wq = (torch.rand((NQ,), generator=g) * 2).to(cuda)
        self.wq[::5] = 0.0                                       # a weight of 0: the query does not exist
        self.wv = (torch.rand((NQ, O), generator=g) * 2).to(cuda)

    def workspace(self, desc):
        return torch.full((int(self.lib.enf_workspace_bytes(ctypes.byref(desc))),), 255, device=self.cuda, dtype=torch.uint8)

    def tail(self, q0, q1, form, act=None, weight=None, per_value=False, det=False):
        """enf_test_tail on queries [q0, q1) with 0xFF-filled outputs: what the form writes as int32 words, and the loss"""
        n, nef, cuda, lib = q1 - q0, self.nef, self.cuda, self.lib
        HD, D = nef._Hp * nef._Dp, nef._Dp
        desc = nef._desc(1, n, 1)
        fill = lambda *shape: torch.full(shape, -1, device=cuda, dtype=torch.int32)
        out, dybar, delta, err = fill(n, O), fill(n, HD), fill(n, nef._Hp), fill(n)
        act = act.clone() if act is not None else fill(n, 2 * HD + 2 * D + 2)
        loss = torch.zeros(1, device=cuda)
        part = fill(int(lib.enf_test_tail_parts(ctypes.byref(desc)))) if det else None
        w = weight[q0:q1].contiguous() if weight is not None else None
        _lib.launch(cuda, lib.enf_test_tail, ctypes.byref(desc), _ptr(self.blob), form, O - 1, _ptr(self.ybar[q0:q1]),
                    _ptr(self.target[q0:q1]), _ptr(w), int(per_value), _ptr(out), _ptr(act), _ptr(dybar), _ptr(delta), _ptr(err), _ptr(loss),
                    _ptr(part), self.st)
        torch.cuda.synchronize()
        wrote = {FWD: dict(out=out), SAVE: dict(out=out, act=act), EVAL: dict(err=err), SEED: dict(dybar=dybar, delta=delta),
                 FWD_SEED: dict(out=out, act=act, dybar=dybar, delta=delta), LOSS: dict(act=act, dybar=dybar, delta=delta, err=err)}[form]
        return wrote, float(loss)

    def backward(self, q0, q1, wg, stash):
        """the d out backward (enf_backward_latents_ex) or the weight-gradient backward (enf_backward_all) of queries [q0, q1) on the
        whole run's ybar / lse rows; stash: behind a forward tail that left its pre-activations in the workspace.  Returns the
        workspace's d ybar, delta and stash regions."""
        n, nef, cuda, lib = q1 - q0, self.nef, self.cuda, self.lib
        desc = nef._desc(1, n, Z)
        ws = self.workspace(desc)
        x, ybar, lse, dout = (v[q0:q1].contiguous() for v in (self.x[0], self.ybar, self.lse, self.dout))
        head = (ctypes.byref(desc), _ptr(x), n * 2, _ptr(self.p), _ptr(self.a), _ptr(self.s))
        if stash:
            out = torch.empty((n, O), device=cuda)
            _lib.launch(cuda, lib.enf_forward_stages, *head, _ptr(self.blob), _ptr(out), _ptr(ybar), _ptr(lse), _ptr(ws), ws.numel(),
                        STAGES_STASH, self.st)
        dp, da, ds = torch.empty_like(self.p), torch.empty_like(self.a), torch.empty_like(self.s)
        flags = REUSE if stash else 0
        if wg:
            nscr = int(lib.enf_backward_all_scratch_bytes(ctypes.byref(desc), 1))
            scratch = torch.empty(nscr, device=cuda, dtype=torch.uint8)
            grads = [None if i in FROZEN or v.numel() == 0 else torch.empty_like(v) for i, v in enumerate(self.ts)]     # (rff coefficients: frozen)
            arrG = (ctypes.c_void_p * len(grads))(*[_ptr(g) for g in grads])
            _lib.launch(cuda, lib.enf_backward_all, *head, self.arrT, _ptr(self.blob), _ptr(ybar), _ptr(lse), _ptr(dout), _ptr(dp), _ptr(da),
                        _ptr(ds), arrG, ctypes.c_void_p(0), _ptr(ws), ws.numel(), _ptr(scratch), nscr, flags, self.st)
        else:
            _lib.launch(cuda, lib.enf_backward_latents_ex, *head, _ptr(self.blob), _ptr(ybar), _ptr(lse), _ptr(dout), _ptr(dp), _ptr(da),
                        _ptr(ds), _ptr(ws), ws.numel(), flags, self.st)
        torch.cuda.synchronize()
        got = _regions(nef, ws, n)
        if not (wg or stash):
            del got["act"]              # (the recomputing d out backward keeps its forward chain in registers)
        return got


def _chunks():
    return [(q, min(q + CHUNK, NQ)) for q in range(0, NQ, CHUNK)]


def _compare(fails, tag, whole, parts, keys=None):
    keys = list(whole) if keys is None else keys
    same = {k: bool(torch.equal(whole[k], torch.cat([p[k] for p in parts]))) for k in keys}
    wrote = {k: not bool((v == -1).all()) for k, v in whole.items()}
    print("tail forms", tag, "whole run (2-slot ring) against the 3-slot ring, bit-equal:", same)
    if not (all(wrote.values()) and all(same.values())):
        fails.append((tag, "wrote", wrote, "bit-equal", same))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("D,H", [(64, 1), (128, 2)])
def test_every_form_on_both_rings(cuda, D, H, precision):
    c = _Case(cuda, D, H, precision)
    tag = (D, H, precision)
    runs = [("forward", FWD, {}), ("forward + stash", SAVE, {}), ("evaluation", EVAL, {}),
            ("evaluation, per-channel weights", EVAL, dict(weight=c.wv, per_value=True)), ("seeded backward from the stash", SEED, {}),
            ("forward + seeded backward", FWD_SEED, {}), ("fused loss", LOSS, dict(weight=c.wq)),
            ("fused loss, per-channel weights", LOSS, dict(weight=c.wv, per_value=True))]
    fails, worst = [], 0.0
    stash_whole = c.tail(0, NQ, SAVE)[0]["act"]
    for name, form, kw in runs:
        whole, loss = c.tail(0, NQ, form, act=stash_whole if form == SEED else None, **kw)
        parts = [c.tail(q0, q1, form, act=stash_whole[q0:q1] if form == SEED else None, **kw) for q0, q1 in _chunks()]
        # the fused loss scales d out by 1 / (n O): a chunk's d ybar and delta are other numbers than the whole run's.  Its 3-slot
        # ring on the SAME queries: four active waves, forced through the test library's switch
        _compare(fails, tag + (name,), whole, [p[0] for p in parts], keys=["act", "err"] if form == LOSS else None)
        if form == LOSS:
            c.lib.enf_test_tail_active_waves(4)
            try:
                ring3 = c.tail(0, NQ, form, **kw)[0]
            finally:
                c.lib.enf_test_tail_active_waves(0)
            _compare(fails, tag + (name, "four active waves"), whole, [ring3])
        if form in (EVAL, LOSS):
            det, det_loss = c.tail(0, NQ, form, det=True, **kw)
            det2, det_loss2 = c.tail(0, NQ, form, det=True, **kw)
            dev = abs(loss - det_loss) / abs(det_loss)
            worst = max(worst, dev)
            print("tail forms", tag, name, "loss", loss, "deterministic", det_loss, det_loss2, "relative difference", dev)
            if not (all(torch.equal(whole[k], det[k]) for k in whole) and det_loss == det_loss2 and np.isfinite(det_loss)):
                fails.append((tag, name, "deterministic mode", det_loss, det_loss2))
            if dev > LOSS_BOUND:
                fails.append((tag, name, "loss against the deterministic sum", loss, det_loss, dev))
            for (q0, q1), (_, closs) in zip(_chunks(), parts):         # a chunk: at most 256 partials, the other test's comparison
                cdet = c.tail(q0, q1, form, det=True, **kw)[1]
                if not abs(closs - cdet) <= 1e-6 * abs(cdet):
                    fails.append((tag, name, "chunk", q0, closs, cdet))
    for wg in (False, True):
        for stash in (False, True):
            name = ("weight-gradient backward" if wg else "d out backward") + (" from the stash" if stash else "")
            _compare(fails, tag + (name,), c.backward(0, NQ, wg, stash), [c.backward(q0, q1, wg, stash) for q0, q1 in _chunks()])
    print("tail forms", tag, "largest relative difference of a whole run's loss from its deterministic sum:", worst)
    assert not fails, fails
