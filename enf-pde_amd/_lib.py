"""ctypes binding of the C-ABI in include/enf_hip.h (libenf_hip.so, built in-tree by
``make -C enf-pde_amd/csrc`` / ``__graft_entry__.build()``).  Fails loudly when the library is
missing: there is no fallback path."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ENF_HIP_LIB") or os.path.join(_HERE, "libenf_hip.so")   # ENF_HIP_LIB: A/B builds (scripts/build_variant.sh)
TEST_LIB_PATH = os.environ.get("ENF_HIP_TEST_LIB") or os.path.join(_HERE, "libenf_hip_test.so")    # same ABI + test hooks (csrc/Makefile); tests only
F32R_LIB_PATH = os.environ.get("ENF_HIP_F32R_LIB") or os.path.join(_HERE, "libenf_hip_f32r.so")    # same ABI, -DENF_F32_ROUNDED=1 (csrc/Makefile); tests only

ENF_NUM_TENSORS = 46
PREC = {"f32": 0, "fp32": 0, "float32": 0, "bf16": 1, "bfloat16": 1}
INVARIANT_IDS = {"rel_pos_periodic": 0, "latitude_periodic": 1, "polar_periodic": 2, "ponita": 3,
                 "abs_pos": 4, "rel_pos": 5, "norm_rel_pos": 6, "ball": 7, "ball_lat": 8, "ponita_full": 9}

EXPORTS = ["enf_abi_version", "enf_strerror", "enf_invariant_dim", "enf_invariant_pose_dim", "enf_check_desc",
           "enf_packed_weight_bytes", "enf_pack_weights", "enf_workspace_bytes", "enf_forward",
           "enf_backward_latents", "enf_backward_latents_ex", "enf_forward_stages", "enf_lt_layout", "enf_lt_layout_ext", "enf_pack_pair", "enf_pair_forward",
           "enf_pair_backward", "enf_pair_backward_ex", "enf_pair_scratch_bytes", "enf_pair_variant", "enf_pair_partition", "enf_shared_forward_parts", "enf_shared_backward_applies", "enf_backward_weights", "enf_backward_weights_scratch_bytes",
           "enf_backward_all", "enf_backward_all_scratch_bytes", "enf_fit_step", "enf_fit_inputs",
           "enf_mse_value_grad",
           "enf_workspace_bytes_ex", "enf_fit_step_ex", "enf_mse_value_grad_ex", "enf_mse_scratch_bytes", "enf_pair_backward_ex2",
           "enf_pair_backward_scratch_bytes", "enf_backward_all_scratch_bytes_ex", "enf_backward_weights_ex",
           "enf_backward_weights_scratch_bytes_ex",
           "enf_fit_step_w", "enf_mse_value_grad_w", "enf_fit_inputs_w", "enf_fit_inputs_b",
           "enf_fit_step_cw", "enf_mse_value_grad_cw", "enf_fit_inputs_cw",
           "enf_fit_step_e", "enf_eval_loss", "enf_signal_sum", "enf_fit_step_g", "enf_eval_loss_g",
           "enf_fit_step_gs", "enf_mse_value_grad_g", "enf_fit_inputs_g",
           "enf_fit_step_gc", "enf_eval_loss_gc", "enf_mse_value_grad_gc", "enf_fit_inputs_gc",
           "enf_obs_apply", "enf_mse_a_scratch_bytes", "enf_mse_value_grad_a", "enf_obs_workspace_bytes", "enf_fit_step_a", "enf_eval_loss_a",
           "enf_field_grad_workspace_bytes", "enf_field_grad", "enf_query_vjp",
           "enf_field_tangent_workspace_bytes", "enf_field_tangent", "enf_field_tangent_x",
           "enf_field_second_workspace_bytes", "enf_field_second_x",
           "enf_gn_workspace_bytes", "enf_gn_product", "enf_gn_product_g", "enf_gn_a_workspace_bytes", "enf_gn_product_a", "enf_cg_update",
           "enf_ode_conv_forward", "enf_ode_conv_backward_basis", "enf_ode_conv_backward_weight", "enf_ode_conv_backward_weight_scratch_bytes", "enf_ode_poly_num_features", "enf_ode_poly_forward",
           "enf_ode_poly_backward", "enf_ode_vec_readout_forward", "enf_ode_vec_readout_backward", "enf_ode_block_supported", "enf_ode_block_scratch_bytes", "enf_ode_block_forward", "enf_ode_block_backward",
           "enf_ode_basis_supported", "enf_ode_basis_scratch_bytes", "enf_ode_basis_forward",
           "enf_ode_basis_backward", "enf_relu_mask_bytes", "enf_meta_sgd_update", "enf_table_adam_update"]
ENF_NUM_PAIR_TENSORS = 12          # ENF_P_* of include/enf_hip.h
# every ENF_STAGE_* / ENF_BWD_* / ENF_FIT_* / ENF_MSE_* bit of include/enf_hip.h under the header's name (tests/test_host.py
# compares them): package code builds its stage and flag words from these, never from numbers
ENF_STAGE_PROLOGUE, ENF_STAGE_PAIR, ENF_STAGE_TAIL, ENF_STAGE_FOLD = 1, 2, 4, 8
ENF_STAGE_TAIL_SAVE = 16           # stash the tail's pre-activations for the backward (ENF_BWD_REUSE_TAIL)
ENF_STAGE_PREPARE_BWD = 32         # a backward on the same inputs and workspace follows (ENF_BWD_REUSE_PREPARED)
ENF_STAGE_YBAR_HALF = 64           # nothing reads this call's ybar: the pair kernel may hand it to the tail as bf16
ENF_STAGES_FORWARD = ENF_STAGE_PROLOGUE | ENF_STAGE_PAIR | ENF_STAGE_TAIL | ENF_STAGE_FOLD       # (not a macro: what enf_forward runs)
ENF_BWD_REUSE_PROLOGUE, ENF_BWD_REUSE_TAIL, ENF_BWD_REUSE_PREPARED, ENF_BWD_ONLY_PAIR = 1, 2, 4, 8
# deterministic mode (include/enf_hip.h, "Deterministic mode"): one bit for every entry point that takes flags
ENF_BWD_DETERMINISTIC = ENF_FIT_DETERMINISTIC = ENF_MSE_DETERMINISTIC = 16
ENF_FIT_SHARED_LATENTS = ENF_STAGE_SHARED_LATENTS = 128      # include/enf_hip.h: the signals share latents and points (first inner step)
ENF_BWD_QUERY_GRAD = 32            # size queries: a query gradient will be asked for
ENF_GN_REUSE_POINT = 1             # enf_gn_product: a fit step or a product at the same point was the workspace's last user
(ENF_S_EQ, ENF_S_EV, ENF_S_G1, ENF_S_NH, ENF_S_DA1, ENF_S_DA2, ENF_S_DA3, ENF_S_HEAD0) = range(8)


def num_store(H):
    """ENF_NUM_STORE(H)"""
    return 7 + 4 * H


class EnfDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ("B", "N", "Z", "H", "D", "C", "O", "dx", "invariant_id", "use_window", "precision")] + \
               [("h_true", ctypes.c_int32), ("d_true", ctypes.c_int32),
                # per-call options (include/enf_hip.h): the library keeps no settings
                ("pair_fwd_variant", ctypes.c_int32), ("pair_bwd_variant", ctypes.c_int32), ("mask_mode", ctypes.c_int32),
                ("mask_signals", ctypes.c_int32), ("embedding", ctypes.c_int32), ("relu_masks", ctypes.c_void_p)]


VARIANT = {"auto": 0, "latent_split": 1, "z_fold": 2, "z_fold_zsplit": 3}       # ENF_VARIANT_*
MASK_MODE = {"off": 0, "write": 1, "read": 2}                # ENF_MASK_*
EMB = {"rff": 0, "ffn": 1}                                   # ENF_EMB_*


class EnfSgdSegment(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("g", ctypes.c_void_p), ("lr", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("n", ctypes.c_int64), ("width", ctypes.c_int32), ("g_stride", ctypes.c_int32), ("lr_len", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


ENF_SGD_MAX_SEGMENTS = 4


ENF_ADAM_MAX_SEGMENTS = 4


class EnfAdamSegment(ctypes.Structure):
    """One component of a latent table for enf_table_adam_update (include/enf_hip.h)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("x", "mu", "nu", "g", "x_out", "mu_out", "nu_out")] + \
               [("width", ctypes.c_int32), ("g_stride", ctypes.c_int32)]


ENF_CG_MAX_SEGMENTS = 3


class EnfCgSegment(ctypes.Structure):
    """One latent component of a batched conjugate-gradient step (include/enf_hip.h: enf_cg_update)."""
    _fields_ = [("x", ctypes.c_void_p), ("r", ctypes.c_void_p), ("d", ctypes.c_void_p), ("q", ctypes.c_void_p),
                ("width", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class EnfSparseObs(ctypes.Structure):
    """A sparse linear observation operator, CSR and CSC on the device (include/enf_hip.h, "Sparse linear observations")."""
    _fields_ = [("M", ctypes.c_int32), ("nnz", ctypes.c_int64), ("row_ptr", ctypes.c_void_p), ("col", ctypes.c_void_p),
                ("val", ctypes.c_void_p), ("col_ptr", ctypes.c_void_p), ("trow", ctypes.c_void_p), ("tval", ctypes.c_void_p)]


class EnfFitComponent(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("width", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class EnfError(RuntimeError):
    pass


_lib = None
_test_lib = None
_f32r_lib = None
# the test-only entry points of the two test libraries
_DEBUG_HOOKS = ("enf_debug_gemm", "enf_debug_pack")
_TEST_HOOKS = _DEBUG_HOOKS + ("enf_test_read_wave_sums", "enf_test_pair_fwd_streamed", "enf_test_tail_active_waves", "enf_test_tail_parts",
                              "enf_test_tail")


def load():
    """Load libenf_hip.so once; raise if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    _lib = _bind(LIB_PATH, hooks=())
    return _lib


def load_test():
    """The test library (libenf_hip_test.so): the whole product ABI plus the test-only entry points.  Tests only."""
    global _test_lib
    if _test_lib is None:
        _test_lib = _bind(TEST_LIB_PATH, hooks=_TEST_HOOKS)
    return _test_lib


def load_f32r():
    """The bf16-faithful fp32 reference (libenf_hip_f32r.so): the product ABI built with -DENF_F32_ROUNDED=1, in which
    precision="f32" rounds to bf16 every value that precision="bf16" holds as bf16 and keeps fp32 layouts, MFMAs and sums
    (csrc/enf_layout.h), plus the layout self-test entry points.  Tests only: ``with _lib.using(_lib.load_f32r()): ...``."""
    global _f32r_lib
    if _f32r_lib is None:
        _f32r_lib = _bind(F32R_LIB_PATH, hooks=_DEBUG_HOOKS)
    return _f32r_lib


class using:
    """Context manager for tests: route the package's calls through another build of the library (e.g. load_test())."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        global _lib
        self.prev, _lib = _lib, self.lib
        return self.lib

    def __exit__(self, *exc):
        global _lib
        _lib = self.prev


def _bind(path, hooks):
    if not os.path.exists(path):
        raise EnfError(f"{path} not found: build it with `make -C enf-pde_amd/csrc` "
                       "(or python -c 'import __graft_entry__ as g; g.build()'). There is no fallback path.")
    lib = ctypes.CDLL(path)
    vp, i64, sz, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_size_t, ctypes.c_int
    dp = ctypes.POINTER(EnfDesc)
    lib.enf_abi_version.restype = ci
    lib.enf_strerror.restype = ctypes.c_char_p
    lib.enf_strerror.argtypes = [ci]
    lib.enf_invariant_dim.argtypes = [ci, ci]
    lib.enf_invariant_pose_dim.argtypes = [ci, ci]
    lib.enf_check_desc.argtypes = [dp]
    lib.enf_packed_weight_bytes.restype = sz
    lib.enf_packed_weight_bytes.argtypes = [dp]
    lib.enf_workspace_bytes.restype = sz
    lib.enf_workspace_bytes.argtypes = [dp]
    lib.enf_pack_weights.argtypes = [dp, ctypes.POINTER(vp), vp, vp]
    lib.enf_forward.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.enf_forward_stages.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, sz, ctypes.c_uint, vp]
    lib.enf_backward_latents.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.enf_backward_latents_ex.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, ctypes.c_uint, vp]
    ip = ctypes.POINTER(ci)
    lib.enf_lt_layout.argtypes = [dp, ip, ip, ip, ip, ip, ip]
    lib.enf_pack_pair.argtypes = [dp, ctypes.POINTER(vp), vp, vp]
    lib.enf_mse_value_grad.argtypes = [vp, vp, sz, ctypes.c_float, vp, vp, vp]
    lib.enf_meta_sgd_update.argtypes = [ctypes.c_int, ctypes.POINTER(EnfSgdSegment), ctypes.c_float, vp]
    lib.enf_table_adam_update.argtypes = [ctypes.c_int, ctypes.POINTER(EnfAdamSegment), i64, ctypes.c_int32, vp, ctypes.c_int32] + \
                                         [ctypes.c_float] * 6 + [vp]
    lib.enf_fit_inputs.argtypes = [ctypes.c_int, ctypes.POINTER(EnfFitComponent)] + [ctypes.c_int32] * 7 + [vp] * 7
    lib.enf_ode_conv_forward.argtypes = [ci, ci, ci, ci, vp, vp, i64, i64, vp, vp, vp, vp]
    lib.enf_ode_conv_backward_basis.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, vp]
    lib.enf_ode_conv_backward_weight_scratch_bytes.restype = sz
    lib.enf_ode_conv_backward_weight_scratch_bytes.argtypes = [ci, ci, ci, ci]
    lib.enf_ode_conv_backward_weight.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, vp, sz, vp]
    lib.enf_ode_poly_num_features.argtypes = [ci, ci]
    lib.enf_ode_poly_forward.argtypes = [i64, ci, ci, vp, vp, vp]
    lib.enf_ode_poly_backward.argtypes = [i64, ci, ci, vp, vp, vp, vp]
    lib.enf_ode_basis_supported.argtypes = [ci, ci, ci, ci, ci]
    cf = ctypes.c_float
    lib.enf_ode_vec_readout_forward.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, cf, cf, vp, vp, vp]
    lib.enf_ode_vec_readout_backward.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, cf, cf, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.enf_ode_block_supported.argtypes = [ci, ci]
    lib.enf_ode_block_scratch_bytes.restype = sz
    lib.enf_ode_block_scratch_bytes.argtypes = [i64, ci, ci]
    lib.enf_ode_block_forward.argtypes = [i64, ci, ci, vp, vp, vp, vp, vp, vp, vp, ctypes.c_float, vp, vp, vp]
    lib.enf_ode_block_backward.argtypes = [i64, ci, ci, vp, vp, vp, vp, vp, vp, vp, ctypes.c_float, vp, vp, vp, sz, vp]
    lib.enf_ode_basis_scratch_bytes.restype = sz
    lib.enf_ode_basis_scratch_bytes.argtypes = [i64, ci, ci, ci, ci]
    lib.enf_ode_basis_forward.argtypes = [i64, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.enf_ode_basis_backward.argtypes = [i64, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.enf_relu_mask_bytes.restype = sz
    lib.enf_relu_mask_bytes.argtypes = [dp]
    lib.enf_pair_variant.argtypes = [dp, ci]
    lib.enf_pair_partition.argtypes = [dp] + [ctypes.POINTER(ctypes.c_int32)] * 3
    lib.enf_shared_forward_parts.argtypes = [dp, ctypes.POINTER(ctypes.c_int32)]
    lib.enf_shared_backward_applies.argtypes = [dp, ctypes.c_uint]
    lib.enf_backward_weights_scratch_bytes.restype = sz
    lib.enf_backward_weights_scratch_bytes.argtypes = [dp, ci]
    lib.enf_backward_weights.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, vp, ctypes.POINTER(vp), vp, vp, sz, vp]
    lib.enf_fit_step.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, ctypes.c_float, vp, vp, vp, vp, vp, sz, vp]
    lib.enf_backward_all_scratch_bytes.restype = sz
    lib.enf_backward_all_scratch_bytes.argtypes = [dp, ci]
    lib.enf_backward_all.argtypes = [dp, vp, i64, vp, vp, vp, ctypes.POINTER(vp), vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(vp), vp,
                                     vp, sz, vp, sz, ctypes.c_uint, vp]
    lib.enf_pair_scratch_bytes.restype = sz
    lib.enf_pair_scratch_bytes.argtypes = [dp]
    lib.enf_pair_forward.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, sz, vp]
    lib.enf_pair_backward.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, vp, ctypes.POINTER(vp), vp]
    lib.enf_pair_backward_ex.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, vp, ctypes.POINTER(vp), vp, vp]
    cu = ctypes.c_uint
    lib.enf_workspace_bytes_ex.restype = sz
    lib.enf_workspace_bytes_ex.argtypes = [dp, cu]
    lib.enf_fit_step_ex.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, ctypes.c_float, vp, vp, vp, vp, vp, sz, cu, vp]
    lib.enf_mse_scratch_bytes.restype = sz
    lib.enf_mse_scratch_bytes.argtypes = [sz, cu]
    lib.enf_mse_value_grad_ex.argtypes = [vp, vp, sz, ctypes.c_float, vp, vp, vp, sz, cu, vp]
    # the weighted loss (include/enf_hip.h, "Weighted loss"): weight (B, N) fp32 or NULL
    lib.enf_fit_step_w.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, ctypes.c_float, vp, vp, vp, vp, vp, sz, vp, cu, vp]
    lib.enf_mse_value_grad_w.argtypes = [vp, vp, vp, sz, ctypes.c_int32, ctypes.c_float, vp, vp, vp, sz, cu, vp]
    lib.enf_fit_inputs_w.argtypes = [ctypes.c_int, ctypes.POINTER(EnfFitComponent)] + [ctypes.c_int32] * 7 + [vp] * 9
    # per-signal index sets, masks (B, Ns, S1); ws may be given without weight (include/enf_hip.h: the index contract)
    lib.enf_fit_inputs_b.argtypes = [ctypes.c_int, ctypes.POINTER(EnfFitComponent)] + [ctypes.c_int32] * 7 + [vp] * 9
    # per-channel loss weights (include/enf_hip.h, "Weighted loss"): cweight (B, N, O) fp32, required; the gather takes the mask
    # layout as its last integer (0: shared (Ns, S1), 1: per-signal (B, Ns, S1))
    lib.enf_fit_step_cw.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, ctypes.c_float, vp, vp, vp, vp, vp, sz, vp, cu, vp]
    lib.enf_mse_value_grad_cw.argtypes = [vp, vp, vp, sz, ctypes.c_float, vp, vp, vp, sz, cu, vp]
    lib.enf_fit_inputs_cw.argtypes = [ctypes.c_int, ctypes.POINTER(EnfFitComponent)] + [ctypes.c_int32] * 7 + [vp] * 8 + [ctypes.c_int32, vp]
    # per-signal and per-point errors (include/enf_hip.h): weight (B, N) | NULL, cweight (B, N, O) | NULL, err (B, N), loss_b (B) | NULL
    lib.enf_fit_step_e.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, ctypes.c_float, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, cu, vp]
    lib.enf_eval_loss.argtypes = [dp, vp, i64] + [vp] * 11 + [sz, cu, vp]
    lib.enf_signal_sum.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_float, vp, vp]
    lib.enf_fit_step_g.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, ctypes.c_int32, vp, vp, ctypes.c_float] + [vp] * 7 + [sz, cu, vp]
    lib.enf_eval_loss_g.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, ctypes.c_int32] + [vp] * 6 + [sz, cu, vp]
    # grouped observations in the trainers: the fit step that may carry ENF_FIT_SHARED_LATENTS (enf_fit_step_g's arguments); the unfused
    # loss out, target | B, N, O, G | qweight, oweight | grad_scale | dout, loss, err_g, scratch | bytes, flags, stream; the gather of
    # sampled cells: B, Z, M, Ms, S1, G, dx, O | xq, q, obs, masks, xs, qs, ys, losses, oweight, ws | per_signal_masks, stream
    lib.enf_fit_step_gs.argtypes = list(lib.enf_fit_step_g.argtypes)
    lib.enf_mse_value_grad_g.argtypes = [vp, vp] + [ctypes.c_int32] * 4 + [vp, vp, ctypes.c_float] + [vp] * 4 + [sz, cu, vp]
    lib.enf_fit_inputs_g.argtypes = [ctypes.c_int, ctypes.POINTER(EnfFitComponent)] + [ctypes.c_int32] * 8 + [vp] * 10 + [ctypes.c_int32, vp]
    # per-value weights on grouped observations: the _g calls' arguments with cweight_g (B, M, O), required, in place of oweight; the
    # gather's ws is (S1, B, Ms, O)
    lib.enf_fit_step_gc.argtypes = list(lib.enf_fit_step_g.argtypes)
    lib.enf_eval_loss_gc.argtypes = list(lib.enf_eval_loss_g.argtypes)
    lib.enf_mse_value_grad_gc.argtypes = list(lib.enf_mse_value_grad_g.argtypes)
    lib.enf_fit_inputs_gc.argtypes = list(lib.enf_fit_inputs_g.argtypes)
    # sparse linear observations (include/enf_hip.h): out, B, N, O, op, obs, stream | out, target, B, N, O, op, oweight, cweight,
    # grad_scale, dout, loss, err_a, scratch, bytes, flags, stream | the fit step and the evaluation: enf_fit_step_g's / enf_eval_loss_g's
    # arguments with (op, oweight, cweight) in place of (G, qweight, oweight)
    op = ctypes.POINTER(EnfSparseObs)
    lib.enf_obs_apply.argtypes = [vp] + [ctypes.c_int32] * 3 + [op, vp, vp]
    lib.enf_mse_a_scratch_bytes.restype = sz
    lib.enf_mse_a_scratch_bytes.argtypes = [ctypes.c_int32] * 3 + [ci, cu]
    lib.enf_mse_value_grad_a.argtypes = [vp, vp] + [ctypes.c_int32] * 3 + [op, vp, vp, ctypes.c_float] + [vp] * 4 + [sz, cu, vp]
    lib.enf_obs_workspace_bytes.restype = sz
    lib.enf_obs_workspace_bytes.argtypes = [dp, ctypes.c_int32, cu]
    lib.enf_fit_step_a.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, op, vp, vp, ctypes.c_float] + [vp] * 7 + [sz, cu, vp]
    lib.enf_eval_loss_a.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, op] + [vp] * 6 + [sz, cu, vp]
    # derivative fields (include/enf_hip.h, "Derivative fields"): out (B, N, O) | NULL, jac (O, B, N, dx); dout (B, N, O), dx (B, N, dx)
    lib.enf_field_grad_workspace_bytes.restype = sz
    lib.enf_field_grad_workspace_bytes.argtypes = [dp, cu]
    lib.enf_field_grad.argtypes = [dp, vp, i64] + [vp] * 7 + [sz, cu, vp]
    lib.enf_query_vjp.argtypes = [dp, vp, i64] + [vp] * 8 + [sz, cu, vp]
    # tendency fields (include/enf_hip.h, "Tendency fields"): p, a, sigma | dp, da, dsigma (each may be NULL) | blob, out | NULL, tan, workspace, stream
    lib.enf_field_tangent_workspace_bytes.restype = sz
    lib.enf_field_tangent_workspace_bytes.argtypes = [dp]
    lib.enf_field_tangent.argtypes = [dp, vp, i64] + [vp] * 11
    # directional derivatives: enf_field_tangent with (xdot, xdot_bstride) behind (x, x_bstride); xdot may be NULL like the other tangents
    lib.enf_field_tangent_x.argtypes = [dp, vp, i64, vp, i64] + [vp] * 11
    # second directional derivatives: x, x_bstride, xdot (required), xdot_bstride | p, a, sigma | blob | out | NULL, tan | NULL, tan2 |
    # workspace, stream
    lib.enf_field_second_workspace_bytes.restype = sz
    lib.enf_field_second_workspace_bytes.argtypes = [dp]
    lib.enf_field_second_x.argtypes = [dp, vp, i64, vp, i64] + [vp] * 9
    # Gauss-Newton product (include/enf_hip.h): p, a, sigma | vp, va, vsigma (each may be NULL) | packed, weight, cweight | grad_scale |
    # gp, ga, gsigma | workspace, bytes, flags, stream
    lib.enf_gn_workspace_bytes.restype = sz
    lib.enf_gn_workspace_bytes.argtypes = [dp, cu]
    lib.enf_gn_product.argtypes = [dp, vp, i64] + [vp] * 9 + [ctypes.c_float] + [vp] * 4 + [sz, cu, vp]
    # the product on grouped observations: (G, qweight, oweight) in place of (weight, cweight)
    lib.enf_gn_product_g.argtypes = [dp, vp, i64] + [vp] * 7 + [ctypes.c_int32, vp, vp, ctypes.c_float] + [vp] * 4 + [sz, cu, vp]
    # the product on sparse observations: (op, oweight, cweight) in their place; its size query takes M
    lib.enf_gn_a_workspace_bytes.restype = sz
    lib.enf_gn_a_workspace_bytes.argtypes = [dp, ctypes.c_int32, cu]
    lib.enf_gn_product_a.argtypes = [dp, vp, i64] + [vp] * 7 + [op, vp, vp, ctypes.c_float] + [vp] * 4 + [sz, cu, vp]
    lib.enf_cg_update.argtypes = [ci, ctypes.POINTER(EnfCgSegment), ctypes.c_int32, ctypes.c_int32, vp, vp, vp]
    lib.enf_pair_backward_scratch_bytes.restype = sz
    lib.enf_pair_backward_scratch_bytes.argtypes = [dp, cu]
    lib.enf_pair_backward_ex2.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, vp, ctypes.POINTER(vp), vp, vp, sz, cu, vp]
    lib.enf_backward_all_scratch_bytes_ex.restype = sz
    lib.enf_backward_all_scratch_bytes_ex.argtypes = [dp, ci, cu]
    lib.enf_backward_weights_scratch_bytes_ex.restype = sz
    lib.enf_backward_weights_scratch_bytes_ex.argtypes = [dp, ci, cu]
    lib.enf_backward_weights_ex.argtypes = [dp, vp, i64, vp, vp, vp, vp, vp, vp, ctypes.POINTER(vp), vp, vp, sz, cu, vp]
    for name in hooks:
        getattr(lib, name).restype = ci
    if "enf_debug_gemm" in hooks:
        lib.enf_debug_gemm.argtypes = [vp, vp, vp, ci, ci, ci, vp]
        lib.enf_debug_pack.argtypes = [vp, vp, ci, ci, ci, vp]
    if "enf_test_tail" in hooks:
        lib.enf_test_tail_active_waves.argtypes = [ci]      # 1, 2, 4, 8: the tail launches run with that many active waves; 0: the launcher's rule; returns the previous setting
        lib.enf_test_tail_parts.argtypes = [dp]
        lib.enf_test_tail.argtypes = [dp, vp, ci, ci, vp, vp, vp, ci] + [vp] * 8      # one tail launch on the caller's buffers (csrc/enf_tail.hip)
        lib.enf_test_pair_fwd_streamed.argtypes = [ci]      # 1: the forward pair kernels run with an empty resident set; returns the previous setting
        lib.enf_test_read_wave_sums.argtypes = [vp]
    if lib.enf_abi_version() != 2:
        raise EnfError(f"{path}: ABI version mismatch")
    return lib


def check(rc):
    """Map a negative return code to the exception the reference would raise."""
    if rc == 0:
        return
    msg = load().enf_strerror(rc).decode()
    if rc == -2:   # ENF_EINVARIANT: reference raises ValueError (invariant/__init__.py:44,78)
        raise ValueError(msg)
    if rc == -6:   # ENF_EDIM: reference asserts (invariant/__init__.py:28,31,62,65)
        raise AssertionError(msg)
    if rc == -3:
        raise NotImplementedError(msg)
    raise EnfError(f"libenf_hip error {rc}: {msg}")


def launch(dev, fn, *args):
    """Call a library entry point that enqueues work on a stream of ``dev`` (a torch.device) with ``dev`` as the calling
    thread's current device -- the library's per-device bookkeeping (side stream, kernel attributes) goes by it -- and map
    its return code like ``check``."""
    import torch
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx == torch.cuda.current_device():
        return check(fn(*args))
    with torch.cuda.device(idx):
        return check(fn(*args))


def ptr(t):
    """A tensor's address as a pointer argument; None is NULL."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream(dev):
    """The current torch stream of ``dev`` as the stream argument of an entry point."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def make_desc(B, N, Z, H, D, C, O, dx, invariant_id, use_window, precision, d_true=0, h_true=0, variants=(0, 0),
              masks=None, embedding=0):
    """``variants``: (forward, backward) ENF_VARIANT_*; ``masks``: None or (int32 device tensor, "write" | "read", signals);
    ``embedding``: ENF_EMB_*."""
    d = EnfDesc()
    d.B, d.N, d.Z, d.H, d.D, d.C, d.O, d.dx = int(B), int(N), int(Z), int(H), int(D), int(C), int(O), int(dx)
    d.invariant_id, d.use_window, d.precision = int(invariant_id), int(bool(use_window)), int(precision)
    d.d_true, d.h_true = int(d_true), int(h_true)
    d.pair_fwd_variant, d.pair_bwd_variant = int(variants[0]), int(variants[1])
    d.embedding = int(embedding)
    if masks is not None:
        buf, mode, signals = masks
        d.relu_masks, d.mask_mode, d.mask_signals = buf.data_ptr(), MASK_MODE[mode], int(signals)
    return d
