"""MFMA fragment-layout self test: pack_panel + make_frags + gemm_stage against an exact matmul.
Integer-valued, asymmetric operands so a swapped row/col map or a wrong k permutation cannot hide
(cdna_hip_programming.md section 3, 'Always A=I-check with ASYMMETRIC B')."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("M,K", [(64, 64), (64, 128), (64, 32), (16, 64)])
def test_panel_gemm_exact(cuda, bf16, M, K):
    from enf_pde_amd import _lib
    lib = _lib.load_test()          # the layout self-test entry points live in the test library only
    g = torch.Generator().manual_seed(M * 1000 + K + bf16)
    W = torch.randint(-4, 5, (K, M), generator=g).float().to(cuda)       # plain (in, out)
    X = torch.randint(-4, 5, (K, 16), generator=g).float().to(cuda)      # (in, cols)
    packed = torch.zeros(M * K * (2 if bf16 else 4), dtype=torch.uint8, device=cuda)
    Y = torch.zeros(M, 16, device=cuda)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.enf_debug_pack(p(packed), p(W), M, K, bf16, st) == 0
    assert lib.enf_debug_gemm(p(packed), p(X), p(Y), M, K, bf16, st) == 0
    torch.cuda.synchronize()
    ref = W.t() @ X
    assert torch.equal(Y, ref), f"max err {(Y - ref).abs().max().item()}"


# ---------------------------------------------------------------------------------------------- conversions
# The integers above need no rounding.  Below, the same two entry points on values that do, against torch's CPU conversion
# t.to(torch.bfloat16).float() (round to nearest even) bit for bit, through
#   "bf16"   the test library's bf16 path: bf16_pack2 in make_frags<true>, (__bf16) in pack_panel_kernel
#   "f32r"   the f32r library's fp32 path (csrc/Makefile, -DENF_F32_ROUNDED=1): the same conversions, results kept as fp32 -- equal bits
#            here are what makes that library the bf16-faithful reference of tests/test_gpu_bf16_faithful.py
#   "f32"    the test library's fp32 path, which must NOT round
MODES = {"bf16": ("load_test", 1, True), "f32r": ("load_f32r", 0, True), "f32": ("load_test", 0, False)}


def _roundable(n, seed):
    """n fp32 values (a multiple of 8) of eight kinds, shuffled, both signs, exponents over 50 binades, none subnormal / inf / nan:
    randoms | exact ties with an even upper half | ties with an odd upper half | one ulp below a tie | one ulp above a tie |
    ties that round up into the next binade | values above such a tie | values exactly representable"""
    g = torch.Generator().manual_seed(seed)
    m = n // 8
    ri = lambda lo, hi, k=m: torch.randint(lo, hi, (k,), generator=g, dtype=torch.int64)
    sign, expo = ri(0, 2, n) << 31, ri(102, 152, n) << 23
    up = lambda: ri(0, 128)                                      # the 7 mantissa bits bf16 keeps
    upper = torch.cat([up(), up() & ~1, up() | 1, up(), up(), torch.full((m,), 127), torch.full((m,), 127), up()])
    lower = torch.cat([ri(0, 1 << 16), torch.full((m,), 0x8000), torch.full((m,), 0x8000), torch.full((m,), 0x7FFF),
                       torch.full((m,), 0x8001), torch.full((m,), 0x8000), ri(0x8001, 1 << 16), torch.zeros(m, dtype=torch.int64)])
    bits = sign | expo | (upper << 16) | lower
    bits = bits[torch.randperm(n, generator=g)]
    v = (bits & 0xFFFFFFFF).to(torch.int64)
    v = torch.where(v >= 1 << 31, v - (1 << 32), v).to(torch.int32).view(torch.float32)
    assert torch.isfinite(v).all() and (v.abs() > 1e-10).all()
    return v


def _bits(t):
    return t.contiguous().view(torch.int32)


def _debug_call(cuda, lib, W, X, M, K, bf16):
    """Y (M x 16) = W^T X through enf_debug_pack + enf_debug_gemm"""
    packed = torch.zeros(M * K * (2 if bf16 else 4), dtype=torch.uint8, device=cuda)
    Y = torch.full((M, 16), float("nan"), device=cuda)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    Wd, Xd = W.contiguous().to(cuda), X.contiguous().to(cuda)
    assert lib.enf_debug_pack(p(packed), p(Wd), M, K, bf16, st) == 0
    assert lib.enf_debug_gemm(p(packed), p(Xd), p(Y), M, K, bf16, st) == 0
    torch.cuda.synchronize()
    return Y.cpu()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("M,K", [(64, 64), (64, 128), (64, 32), (16, 64)])
def test_make_frags_conversion_is_round_to_nearest_even(cuda, mode, M, K):
    """A 0/1 selection panel (the identity where M = K; row m picks input (m + off) % K otherwise) returns make_frags' conversion of
    X: one product 1 * x per output and zeros, exact in fp32."""
    from enf_pde_amd import _lib
    loader, bf16, rounds = MODES[mode]
    lib = getattr(_lib, loader)()
    X = _roundable(K * 16, 7 * M + K).reshape(K, 16)
    want = X.to(torch.bfloat16).float() if rounds else X
    assert not rounds or int((_bits(want) != _bits(X)).sum()) > K * 16 // 2          # the values do need rounding
    for off in range(0, K, M):
        sel = (torch.arange(M) + off) % K
        W = torch.zeros(K, M)
        W[sel, torch.arange(M)] = 1.0
        Y = _debug_call(cuda, lib, W, X, M, K, bf16)
        differ = _bits(Y) != _bits(want[sel])
        assert not differ.any(), (mode, off, int(differ.sum()), X[sel][differ][:4].tolist(), Y[differ][:4].tolist(), want[sel][differ][:4].tolist())


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("M,K", [(64, 64), (64, 128), (64, 32), (16, 64)])
def test_pack_panel_conversion_is_round_to_nearest_even(cuda, mode, M, K):
    """One-hot columns (column c picks input k0 + c) return the packed W, 16 input rows per launch: every element of the panel."""
    from enf_pde_amd import _lib
    loader, bf16, rounds = MODES[mode]
    lib = getattr(_lib, loader)()
    W = _roundable(K * M, 11 * M + K).reshape(K, M)
    want = W.to(torch.bfloat16).float() if rounds else W
    for k0 in range(0, K, 16):
        X = torch.zeros(K, 16)
        X[k0 + torch.arange(16), torch.arange(16)] = 1.0
        Y = _debug_call(cuda, lib, W, X, M, K, bf16)                   # Y[m][c] = packed W[k0 + c][m]
        differ = _bits(Y) != _bits(want[k0:k0 + 16].t())
        assert not differ.any(), (mode, k0, int(differ.sum()))
