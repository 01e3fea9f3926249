"""CPU tests of the 'ffn' invariant embedding: parameter tree and count, the C-ABI's EnfDesc.embedding, the constructor's
limits, .npz round trip, and the patched fp64 oracle (invariances, finite differences)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from tests.helpers import make_cfg, make_inputs
from tests.ffn_ref import ffn_oracle, init_params_ffn, build_nef_ffn  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMB = ("cross_attention_blocks_0", "attn")


@pytest.fixture(scope="module")
def lib():
    from enf_pde_amd import _lib
    return _lib.load()


def small_cfg(inv, **kw):
    d = dict(invariant=inv, D=32, H=2, C=6, O=2, freq=(0.3, 0.7))
    d.update(kw)
    return make_cfg(**d)


def _leaves(tree, prefix=()):
    for k, v in tree.items():
        if isinstance(v, dict):
            yield from _leaves(v, prefix + (k,))
        else:
            yield prefix + (k,), v


def test_ffn_tree_names_shapes_and_count():
    cfg = make_cfg("rel_pos_periodic", D=128, H=2, C=16, O=1)
    nef = build_nef_ffn(cfg, "bf16")
    P = nef.init(0, device="cpu")["params"]
    for branch in ("query", "value"):
        emb = dict(_leaves(P[EMB[0]][EMB[1]]["invariant_embedding_" + branch]))
        assert {k: tuple(v.shape) for k, v in emb.items()} == {
            ("Dense_0", "kernel"): (4, 128), ("Dense_0", "bias"): (128,),
            ("Dense_1", "kernel"): (128, 128), ("Dense_1", "bias"): (128,)}
        assert all(float(emb[(d, "bias")].abs().max()) == 0.0 for d in ("Dense_0", "Dense_1"))     # flax Dense: zero bias
    count = sum(int(np.prod(v.shape)) for _, v in _leaves(P))
    assert count == 499329 == 531585 - 2 * (128 ** 2 - 4 * 128 // 2)
    # the test's fp64 restatement has the same tree
    prm = init_params_ffn(0, cfg)
    assert R.count_params(prm) == 499329
    assert sorted(p for p, _ in _leaves(prm["params"])) == sorted(p for p, _ in _leaves(P))
    # C-ABI slots: Dense_0 in R?_COEF / R?_B1, Dense_1 in R?_W2 / R?_B2, nothing in R?_W1
    ts = nef.param_tensors({"params": P})
    assert ts[5].numel() == 0 and ts[10].numel() == 0             # (empty placeholders: no tensor in the tree)
    emb_q = P[EMB[0]][EMB[1]]["invariant_embedding_query"]
    assert ts[4] is emb_q["Dense_0"]["kernel"] and ts[6] is emb_q["Dense_0"]["bias"]
    assert ts[7] is emb_q["Dense_1"]["kernel"] and ts[8] is emb_q["Dense_1"]["bias"]
    nef._check_shapes(ts)


def test_embedding_enum_and_field_match_header():
    from enf_pde_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "enf_hip.h")).read()
    assert {k.lower(): int(v) for k, v in re.findall(r"ENF_EMB_([A-Z]+) = (\d+)", hdr)} == _lib.EMB == {"rff": 0, "ffn": 1}
    assert re.search(r"int32_t embedding;", hdr) and "embedding" in [f[0] for f in _lib.EnfDesc._fields_]
    assert _lib.EnfDesc().embedding == 0                   # a zeroed descriptor is rff
    assert ctypes.sizeof(_lib.EnfDesc) == 80


def test_check_desc_embedding(lib):
    from enf_pde_amd import _lib
    ok = _lib.make_desc(2, 100, 64, 2, 128, 16, 1, 2, 0, 1, 1, embedding=1)
    assert lib.enf_check_desc(ctypes.byref(ok)) == 0
    assert lib.enf_packed_weight_bytes(ctypes.byref(ok)) > 0
    bad = _lib.make_desc(2, 100, 64, 2, 128, 16, 1, 2, 0, 1, 1, embedding=2)
    assert lib.enf_check_desc(ctypes.byref(bad)) == -1                                  # ENF_EINVAL
    bad.embedding = -1
    assert lib.enf_check_desc(ctypes.byref(bad)) == -1
    for inv in (7, 8):                                                                # ball, ball_lat
        ball = _lib.make_desc(2, 100, 64, 2, 64, 16, 1, 3, inv, 1, 1, embedding=1)
        assert lib.enf_check_desc(ctypes.byref(ball)) == -3                           # ENF_EUNSUPPORTED
        ball.embedding = 0
        assert lib.enf_check_desc(ctypes.byref(ball)) == 0
    # the new checks come after the existing ones: a descriptor rejected before keeps its code
    both = _lib.make_desc(2, 100, 64, 2, 128, 16, 1, 2, 10, 1, 1, embedding=5)
    assert lib.enf_check_desc(ctypes.byref(both)) == -2                               # ENF_EINVARIANT
    wide = _lib.make_desc(2, 100, 64, 2, 96, 16, 1, 2, 0, 1, 1, embedding=5)
    assert lib.enf_check_desc(ctypes.byref(wide)) == -3


def test_constructor_limits():
    from types import SimpleNamespace as NS
    from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant
    cfg = make_cfg("rel_pos_periodic", D=64, H=2)
    with pytest.raises(NotImplementedError, match="num_layers"):
        build_nef_ffn(cfg, "bf16", num_layers=1)
    for name in ("ball", "ball_lat"):
        with pytest.raises(NotImplementedError, match=name):
            build_nef_ffn(make_cfg(name, D=64, H=2), "bf16")
    from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    kw = dict(num_hidden=64, num_heads=2, num_layers=0, num_out=1, latent_dim=16, cross_attn_invariant=inv)
    with pytest.raises(NotImplementedError):
        EquivariantCrossAttentionNeF(embedding_type="polynomial", **kw)
    with pytest.raises(ValueError):
        EquivariantCrossAttentionNeF(embedding_type="mlp", **kw)
    assert EquivariantCrossAttentionNeF(embedding_type="ffn", embedding_freq_multiplier=(3.0, 4.0), **kw).embedding_type == "ffn"
    # an odd width: the kernels' zero-padded widths are even (EnfDesc.d_true), so the constructor says so instead of the pack
    with pytest.raises(NotImplementedError, match="even"):
        EquivariantCrossAttentionNeF(embedding_type="ffn", **dict(kw, num_hidden=33))


def test_npz_round_trip(tmp_path):
    from enf_pde_amd import checkpoint
    cfg = make_cfg("ponita", D=64, H=2, C=8, O=2)
    nef = build_nef_ffn(cfg, "f32")
    params = nef.init(3, device="cpu")
    path = str(tmp_path / "ffn.npz")
    checkpoint.save_tree(path, params)
    back = nef.load_params(checkpoint.load_tree(path), device="cpu")
    a, b = nef.param_tensors(params), nef.param_tensors(back)
    assert [t.numel() == 0 for t in a] == [t.numel() == 0 for t in b] == [i in (5, 10) for i in range(46)]
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # an exported tree of the test's fp64 restatement loads as well
    prm = init_params_ffn(4, cfg, jitter=0.1)
    ts = nef.param_tensors(nef.load_params(prm, device="cpu"))
    assert np.array_equal(ts[4].numpy(), prm["params"][EMB[0]][EMB[1]]["invariant_embedding_query"]["Dense_0"]["kernel"].astype(np.float32))


def _apply(cfg, prm, x, p, a, s):
    return R.nef_apply(prm, cfg, x, p, a, s)


@pytest.mark.parametrize("inv", ["rel_pos_periodic", "ponita", "rel_pos"])
def test_restatements_agree(ffn_oracle, inv):
    cfg = small_cfg(inv)
    prm = init_params_ffn(1, cfg, jitter=0.1)
    x, p, a, s = make_inputs(cfg, 2, 13, 5, 2)
    ref = _apply(cfg, prm, x, p, a, s)
    o64 = T.nef_apply(T.to_torch(prm, torch.float64), cfg, *(torch.tensor(v) for v in (x, p, a, s))).numpy()
    assert np.abs(o64 - ref).max() < 1e-11
    # and the patch took: the rff tree is not what is evaluated
    assert "Dense_0" in prm["params"][EMB[0]][EMB[1]]["invariant_embedding_value"]


@pytest.mark.parametrize("inv", ["rel_pos", "rel_pos_periodic", "norm_rel_pos"])
def test_translation_invariance(ffn_oracle, inv):
    cfg = small_cfg(inv)
    prm = init_params_ffn(7, cfg, jitter=0.1)
    x, p, a, s = make_inputs(cfg, 2, 9, 5, 8)
    t = np.array([0.37, -0.21])
    assert np.abs(_apply(cfg, prm, x, p, a, s) - _apply(cfg, prm, x + t, p + t, a, s)).max() < 1e-10


def test_periodic_shift_by_two(ffn_oracle):
    cfg = small_cfg("rel_pos_periodic")
    prm = init_params_ffn(9, cfg, jitter=0.1)
    x, p, a, s = make_inputs(cfg, 1, 9, 5, 10)
    x2, p2 = x.copy(), p.copy()
    x2[..., 0] += 2.0
    p2[:, 2, 1] -= 2.0
    assert np.abs(_apply(cfg, prm, x, p, a, s) - _apply(cfg, prm, x2, p2, a, s)).max() < 1e-10


def test_ponita_se2_invariance(ffn_oracle):
    cfg = small_cfg("ponita")
    prm = init_params_ffn(13, cfg, jitter=0.1)
    x, p, a, s = make_inputs(cfg, 2, 11, 5, 14)
    al, t = 0.7, np.array([0.3, -0.5])
    Rm = np.array([[np.cos(al), -np.sin(al)], [np.sin(al), np.cos(al)]])
    x2 = x @ Rm.T + t
    p2 = p.copy()
    p2[..., :2] = p[..., :2] @ Rm.T + t
    p2[..., 2] = p[..., 2] + al
    assert np.abs(_apply(cfg, prm, x, p, a, s) - _apply(cfg, prm, x2, p2, a, s)).max() < 1e-10


@pytest.mark.parametrize("inv", ["rel_pos_periodic", "ponita", "polar_periodic", "latitude_periodic"])
def test_latent_gradients_match_finite_differences(ffn_oracle, inv):
    cfg = small_cfg(inv, D=16, O=1)
    prm = T.to_torch(init_params_ffn(19, cfg, jitter=0.1), torch.float64)
    x, p, a, s = (torch.tensor(v) for v in make_inputs(cfg, 1, 6, 3, 20))
    w = torch.tensor(np.random.default_rng(4).standard_normal((1, 6, 1)))

    def f(p_, a_, s_):
        return (T.nef_apply(prm, cfg, x, p_, a_, s_) * w).sum()
    assert torch.autograd.gradcheck(f, (p.clone().requires_grad_(True), a.clone().requires_grad_(True),
                                        s.clone().requires_grad_(True)), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_weight_gradients_match_finite_differences(ffn_oracle):
    """The embedding's own weights: fp64 autograd of the patched oracle against finite differences."""
    cfg = small_cfg("rel_pos_periodic", D=8, O=1)
    prm = T.to_torch(init_params_ffn(21, cfg, jitter=0.1), torch.float64)
    x, p, a, s = (torch.tensor(v) for v in make_inputs(cfg, 1, 5, 3, 22))
    emb = prm["params"][EMB[0]][EMB[1]]["invariant_embedding_query"]
    leaves = [emb["Dense_0"]["kernel"], emb["Dense_0"]["bias"], emb["Dense_1"]["kernel"]]

    def f(*ws):
        emb["Dense_0"]["kernel"], emb["Dense_0"]["bias"], emb["Dense_1"]["kernel"] = ws
        return T.nef_apply(prm, cfg, x, p, a, s).sum()
    assert torch.autograd.gradcheck(f, tuple(t.clone().requires_grad_(True) for t in leaves), eps=1e-6, atol=1e-6, rtol=1e-4)
