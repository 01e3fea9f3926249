#!/usr/bin/env python3
"""Print what the host-only part of the C-ABI returns: every size query over a grid of descriptors, and the error code of
the workspace entry points for calls that are refused before anything is launched.  No GPU is touched.

Run it on two builds (ENF_HIP_LIB selects the library) and diff the outputs: a refactor of the host side of csrc/ must
leave every line as it was.

    python scripts/host_abi_probe.py > new.txt
    ENF_HIP_LIB=/path/to/other/libenf_hip.so python scripts/host_abi_probe.py > old.txt
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from enf_pde_amd import _lib  # noqa: E402

# (name, B, N, Z, C, O, dx, invariant): the fit / decode shapes of the five BASELINE.json configs and one small shape
SHAPES = [
    ("c1_fit", 32, 1024, 16, 16, 1, 2, "ponita"),
    ("c2_fit", 16, 512, 64, 16, 1, 2, "rel_pos_periodic"),
    ("c2_decode", 16, 4096, 64, 16, 1, 2, "rel_pos_periodic"),
    ("c3_fit", 4, 4096, 128, 32, 3, 2, "latitude_periodic"),
    ("c3_decode", 4, 96 * 48, 128, 32, 3, 2, "latitude_periodic"),
    ("c4_fit", 8, 512, 128, 16, 1, 2, "rel_pos_periodic"),
    ("c4_decode", 8, 128 * 128, 128, 16, 1, 2, "rel_pos_periodic"),
    ("c5_decode", 2, 256 * 256, 64, 16, 1, 2, "rel_pos_periodic"),
    ("small", 2, 100, 25, 8, 2, 2, "rel_pos_periodic"),
]
WIDTHS = [(64, 1), (64, 2), (64, 4), (128, 1), (128, 2)]


def sizes(lib):
    for name, B, N, Z, C, O, dx, inv in SHAPES:
        for D, H in WIDTHS:
            for prec in (0, 1):
                for emb in (0, 1):
                    for vf in (0, 1, 2, 3):
                        d = _lib.make_desc(B, N, Z, H, D, C, O, dx, _lib.INVARIANT_IDS[inv], 1, prec, variants=(vf, 0), embedding=emb)
                        r = ctypes.byref(d)
                        row = [lib.enf_workspace_bytes(r), lib.enf_packed_weight_bytes(r), lib.enf_pair_scratch_bytes(r),
                               lib.enf_relu_mask_bytes(r)]
                        for cb in sorted({1, max(B // 2, 1), B}):
                            bw, ba = lib.enf_backward_weights_scratch_bytes(r, cb), lib.enf_backward_all_scratch_bytes(r, cb)
                            assert ba >= bw, (name, D, H, cb)
                            row += [cb, bw, ba]
                        print(name, f"D{D} H{H} prec{prec} emb{emb} fwd{vf}", *row)
    bad = _lib.make_desc(2, 100, 25, 3, 32, 8, 2, 2, 0, 1, 1)
    r = ctypes.byref(bad)
    print("invalid", lib.enf_workspace_bytes(r), lib.enf_packed_weight_bytes(r), lib.enf_pair_scratch_bytes(r), lib.enf_relu_mask_bytes(r),
          lib.enf_backward_weights_scratch_bytes(r, 1), lib.enf_backward_all_scratch_bytes(r, 1))
    ok = _lib.make_desc(2, 100, 25, 2, 64, 8, 2, 2, 0, 1, 1)
    r = ctypes.byref(ok)
    print("chunk out of range", [lib.enf_backward_weights_scratch_bytes(r, cb) for cb in (0, 3)],
          [lib.enf_backward_all_scratch_bytes(r, cb) for cb in (0, 3)])


def errors(lib):
    """Calls that return before the first HIP call.  Non-NULL pointers are the dummy address 4096: never dereferenced here."""
    vp = ctypes.c_void_p
    tensors = (vp * _lib.ENF_NUM_TENSORS)(*([4096] * _lib.ENF_NUM_TENSORS))
    holes = (vp * _lib.ENF_NUM_TENSORS)(*([4096] * (_lib.ENF_NUM_TENSORS - 1) + [None]))

    def args(fn, null=(), sigma=True, ws_bytes=0, arrays=tensors):
        out = []
        for i, t in enumerate(fn.argtypes[1:], 1):
            if t is ctypes.c_float:
                out.append(0.0)
            elif t in (ctypes.c_int64, ctypes.c_uint):
                out.append(0)
            elif t is ctypes.c_size_t:
                out.append(ws_bytes)        # (enf_backward_all: workspace_bytes and scratch_bytes alike)
            elif t is ctypes.POINTER(vp):
                out.append(None if i in null else arrays)
            else:
                out.append(None if i in null else 4096)
        if not sigma:
            out[4] = None                    # sigma is the sixth argument of all four
        return out

    fns = [lib.enf_forward_stages, lib.enf_backward_latents_ex, lib.enf_fit_step, lib.enf_backward_all]
    valid = _lib.make_desc(2, 100, 25, 2, 64, 8, 2, 2, 0, 1, 1)
    nowin = _lib.make_desc(2, 100, 25, 2, 64, 8, 2, 2, 0, 0, 1)
    unsupported = _lib.make_desc(2, 100, 25, 3, 32, 8, 2, 2, 0, 1, 1)
    bad_dim = _lib.make_desc(2, 100, 25, 2, 64, 8, 2, 3, 0, 1, 1)
    for fn in fns:
        n = len(fn.argtypes)
        ws = next(i for i in range(n - 1, 0, -1) if fn.argtypes[i] is ctypes.c_size_t) - 1
        if fn is lib.enf_backward_all:
            ws -= 2                          # (workspace, workspace_bytes, scratch, scratch_bytes)
        row = []
        for desc in (unsupported, bad_dim):  # invalid descriptor AND a NULL pointer AND a short workspace
            row.append(fn(ctypes.byref(desc), *args(fn, null=(1, ws))))
            row.append(fn(ctypes.byref(desc), *args(fn)))
        row.append(fn(None, *args(fn)))
        for i in range(1, n):                # valid descriptor, each pointer NULL in turn, short workspace
            if fn.argtypes[i] in (vp, ctypes.POINTER(vp)) and i != n - 1 and i != 5:
                row.append((i, fn(ctypes.byref(valid), *args(fn, null=(i,)))))
        row.append(fn(ctypes.byref(valid), *args(fn, sigma=False)))          # window without sigma, short workspace
        row.append(fn(ctypes.byref(nowin), *args(fn, sigma=False)))          # no window: sigma may be NULL; short workspace
        row.append(fn(ctypes.byref(valid), *args(fn)))                       # every pointer given, short workspace
        if fn is lib.enf_backward_all:
            row.append(fn(ctypes.byref(valid), *args(fn, arrays=holes)))     # a NULL tensor, short workspace
            big = lib.enf_workspace_bytes(ctypes.byref(valid))               # workspace large enough, scratch too small for one signal
            a = args(fn, ws_bytes=big)
            a[-3] = lib.enf_backward_all_scratch_bytes(ctypes.byref(valid), 1) - 1
            row.append(fn(ctypes.byref(valid), *a))
        print(fn.__name__, *row)
    # enf_backward_weights: refused for a scratch below one signal's
    fn = lib.enf_backward_weights
    a = args(fn)
    print(fn.__name__, fn(ctypes.byref(unsupported), *a), fn(ctypes.byref(valid), *args(fn, null=(1,))), fn(ctypes.byref(valid), *a),
          fn(ctypes.byref(valid), *args(fn, ws_bytes=lib.enf_backward_weights_scratch_bytes(ctypes.byref(valid), 1) - 1)),
          fn(ctypes.byref(_lib.make_desc(2, 100, 25, 2, 64, 8, 2, 2, 0, 1, 1, embedding=1)), *a))
    fn = lib.enf_pair_forward                 # z-fold forced: scratch missing / short
    zf = _lib.make_desc(2, 100, 25, 2, 64, 8, 2, 2, 0, 1, 1, variants=(2, 0))
    print(fn.__name__, fn(ctypes.byref(unsupported), *args(fn)), fn(ctypes.byref(zf), *args(fn, null=(1,))),
          fn(ctypes.byref(zf), *args(fn, null=(7,))), fn(ctypes.byref(zf), *args(fn, ws_bytes=lib.enf_pair_scratch_bytes(ctypes.byref(zf)) - 1)))


def tangent(lib):
    """enf_field_tangent and enf_gn_product: their size queries (every flag word, and one with an unknown bit) and the calls they refuse
    before a launch.  enf_field_tangent takes no workspace size: every call here has a reason to be refused."""
    flag_words = (0, _lib.ENF_GN_REUSE_POINT, _lib.ENF_BWD_DETERMINISTIC, _lib.ENF_BWD_DETERMINISTIC | _lib.ENF_GN_REUSE_POINT, 1 << 30)
    for name, B, N, Z, C, O, dx, inv in SHAPES:
        for D, H in WIDTHS:
            for prec in (0, 1):
                for emb in (0, 1):
                    d = _lib.make_desc(B, N, Z, H, D, C, O, dx, _lib.INVARIANT_IDS[inv], 1, prec, embedding=emb)
                    r = ctypes.byref(d)
                    print("tangent", name, f"D{D} H{H} prec{prec} emb{emb}", lib.enf_field_tangent_workspace_bytes(r),
                          *[lib.enf_gn_workspace_bytes(r, f) for f in flag_words])
    valid = _lib.make_desc(2, 100, 25, 2, 64, 8, 2, 2, 0, 1, 1)
    nowin = _lib.make_desc(2, 100, 25, 2, 64, 8, 2, 2, 0, 0, 1)
    bad_dim = _lib.make_desc(2, 100, 25, 2, 64, 8, 2, 3, 0, 1, 1)
    ffn = _lib.make_desc(2, 100, 25, 2, 64, 8, 2, 2, 0, 1, 1, embedding=1)
    ball = _lib.make_desc(2, 100, 25, 2, 64, 8, 2, 2, _lib.INVARIANT_IDS["ball"], 1, 1)
    P = 4096
    # (x, x_bstride, p, a, sigma, dp, da, dsigma, blob, out, tan, workspace, stream)
    ft = lib.enf_field_tangent
    full = [P, 0, P, P, P, P, P, P, P, P, P, P, None]
    row = []
    for desc in (bad_dim, ffn, ball):               # descriptor / unsupported before a NULL pointer
        row.append(ft(ctypes.byref(desc), *[None if i == 0 else v for i, v in enumerate(full)]))
    for i in (0, 2, 3, 8, 10, 11):                  # each required pointer NULL in turn
        row.append((i, ft(ctypes.byref(valid), *[None if j == i else v for j, v in enumerate(full)])))
    row.append(ft(ctypes.byref(valid), *[None if j in (5, 6, 7) else v for j, v in enumerate(full)]))       # no direction
    row.append(ft(ctypes.byref(valid), *[None if j == 4 else v for j, v in enumerate(full)]))               # window without sigma
    print(ft.__name__, *row)
    # (x, x_bstride, p, a, sigma, vp, va, vsigma, packed, weight, cweight, grad_scale, gp, ga, gsigma, workspace, bytes, flags, stream)
    gn = lib.enf_gn_product
    full = [P, 0, P, P, P, P, P, P, P, None, None, 1.0, P, P, P, P, 0, 0, None]
    row = []
    for desc in (bad_dim, ffn, ball):
        row.append(gn(ctypes.byref(desc), *[None if i == 0 else v for i, v in enumerate(full)]))
    for i in (0, 2, 3, 8, 12, 13, 14, 15):          # each required pointer NULL in turn, short workspace
        row.append((i, gn(ctypes.byref(valid), *[None if j == i else v for j, v in enumerate(full)])))
    row.append(gn(ctypes.byref(valid), *[None if j in (5, 6, 7) else v for j, v in enumerate(full)]))       # no direction
    row.append(gn(ctypes.byref(valid), *[P if j in (9, 10) else v for j, v in enumerate(full)]))            # both kinds of weights
    row.append(gn(ctypes.byref(valid), *[1 << 30 if j == 17 else v for j, v in enumerate(full)]))           # an unknown flag
    row.append(gn(ctypes.byref(valid), *[None if j == 4 else v for j, v in enumerate(full)]))               # window without sigma
    row.append(gn(ctypes.byref(nowin), *[None if j == 4 else v for j, v in enumerate(full)]))               # no window: short workspace
    for f in flag_words[:4]:                        # every pointer given: a workspace one byte short
        a = list(full)
        a[16], a[17] = lib.enf_gn_workspace_bytes(ctypes.byref(valid), f) - 1, f
        row.append(gn(ctypes.byref(valid), *a))
    print(gn.__name__, *row)
    # (x, x_bstride, xdot, xdot_bstride, p, a, sigma, dp, da, dsigma, blob, out, tan, workspace, stream): enf_field_tangent's refusals, and
    # xdot counts as a direction.  Like enf_field_tangent it takes no workspace size: every call here has a reason to be refused.
    fx = lib.enf_field_tangent_x
    full = [P, 0, P, 0, P, P, P, P, P, P, P, P, P, P, None]
    row = []
    for desc in (bad_dim, ffn, ball):               # descriptor / unsupported before a NULL pointer
        row.append(fx(ctypes.byref(desc), *[None if i == 0 else v for i, v in enumerate(full)]))
    for i in (0, 4, 5, 10, 12, 13):                 # each required pointer NULL in turn
        row.append((i, fx(ctypes.byref(valid), *[None if j == i else v for j, v in enumerate(full)])))
    row.append(fx(ctypes.byref(valid), *[None if j in (2, 7, 8, 9) else v for j, v in enumerate(full)]))    # no direction at all
    row.append(fx(ctypes.byref(valid), *[None if j in (0, 7, 8, 9) else v for j, v in enumerate(full)]))    # xdot alone, x missing
    row.append(fx(ctypes.byref(valid), *[None if j == 6 else v for j, v in enumerate(full)]))               # window without sigma
    print(fx.__name__, *row)


def second(lib):
    """enf_field_second_x: its size query beside the tangent's over the same grid, and the calls it refuses before a launch (it takes no
    workspace size: every call here has a reason to be refused)."""
    for name, B, N, Z, C, O, dx, inv in SHAPES:
        for D, H in WIDTHS:
            for prec in (0, 1):
                for emb in (0, 1):
                    d = _lib.make_desc(B, N, Z, H, D, C, O, dx, _lib.INVARIANT_IDS[inv], 1, prec, embedding=emb)
                    print("second", name, f"D{D} H{H} prec{prec} emb{emb}", lib.enf_field_second_workspace_bytes(ctypes.byref(d)))
    valid = _lib.make_desc(2, 100, 25, 2, 64, 8, 2, 2, 0, 1, 1)
    bad_dim = _lib.make_desc(2, 100, 25, 2, 64, 8, 2, 3, 0, 1, 1)
    ffn = _lib.make_desc(2, 100, 25, 2, 64, 8, 2, 2, 0, 1, 1, embedding=1)
    ball = _lib.make_desc(2, 100, 25, 2, 64, 8, 2, 2, _lib.INVARIANT_IDS["ball"], 1, 1)
    P = 4096
    # (x, x_bstride, xdot, xdot_bstride, p, a, sigma, blob, out, tan, tan2, workspace, stream)
    f2 = lib.enf_field_second_x
    full = [P, 0, P, 0, P, P, P, P, P, P, P, P, None]
    row = []
    for desc in (bad_dim, ffn, ball):               # descriptor / unsupported before a NULL pointer
        row.append(f2(ctypes.byref(desc), *[None if i == 0 else v for i, v in enumerate(full)]))
    for i in (0, 2, 4, 5, 7, 10, 11):               # each required pointer NULL in turn
        row.append((i, f2(ctypes.byref(valid), *[None if j == i else v for j, v in enumerate(full)])))
    row.append(f2(ctypes.byref(valid), *[None if j == 6 else v for j, v in enumerate(full)]))               # window without sigma
    print(f2.__name__, *row)


if __name__ == "__main__":
    lib = _lib.load()
    sizes(lib)
    errors(lib)
    tangent(lib)
    second(lib)
