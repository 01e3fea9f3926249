"""EquivariantCrossAttentionNeF -- host-side mirror of enf/models/equivariant_cross_attention_nef.py:70-235.

Same constructor keywords (experiments/fitting/__init__.py:25-38), same ``init`` / ``apply``
call shapes as the Flax module, same parameter tree (names follow Flax's naming rules, SURVEY.md
8a), same latent conventions.  ``apply`` runs the fused HIP path through the C-ABI
(include/enf_hip.h); gradients w.r.t. the latents (p, a, gaussian_window) come from the
hand-written HIP backward; when the weights require grad, ``apply`` takes the training path of
``_train.py`` (same HIP pair kernels, weight gradients as well).  There is no eager / CPU path.
"""
import ctypes
import math

import torch

from .. import steerable_attention  # noqa: F401  (package layout parity)
from ..steerable_attention.invariant import BaseInvariant
from ... import _lib
from . import _pad
from ._obs_calls import Cells as _Cells, Operator as _Operator, Points as _Points, f32 as _f32

__all__ = ["EquivariantCrossAttentionNeF", "TENSOR_PATHS", "FFN_TENSOR_PATHS", "tensor_paths"]

_BLK = "cross_attention_blocks_0"
# ENF_W_* order of include/enf_hip.h -> path in the Flax parameter tree
TENSOR_PATHS = [
    ("latent_stem", "kernel"), ("latent_stem", "bias"),
    (_BLK, "layer_norm_attn", "scale"), (_BLK, "layer_norm_attn", "bias"),
    (_BLK, "attn", "invariant_embedding_query", "encoding", "coefficients"),
    (_BLK, "attn", "invariant_embedding_query", "layers_0", "linear", "kernel"),
    (_BLK, "attn", "invariant_embedding_query", "layers_0", "linear", "bias"),
    (_BLK, "attn", "invariant_embedding_query", "linear_final", "kernel"),
    (_BLK, "attn", "invariant_embedding_query", "linear_final", "bias"),
    (_BLK, "attn", "invariant_embedding_value", "encoding", "coefficients"),
    (_BLK, "attn", "invariant_embedding_value", "layers_0", "linear", "kernel"),
    (_BLK, "attn", "invariant_embedding_value", "layers_0", "linear", "bias"),
    (_BLK, "attn", "invariant_embedding_value", "linear_final", "kernel"),
    (_BLK, "attn", "invariant_embedding_value", "linear_final", "bias"),
    (_BLK, "attn", "inv_emb_to_q", "kernel"), (_BLK, "attn", "inv_emb_to_q", "bias"),
    (_BLK, "attn", "a_to_k", "kernel"), (_BLK, "attn", "a_to_k", "bias"),
    (_BLK, "attn", "a_to_v", "kernel"), (_BLK, "attn", "a_to_v", "bias"),
    (_BLK, "attn", "inv_emb_to_v", "Dense_0", "kernel"), (_BLK, "attn", "inv_emb_to_v", "Dense_0", "bias"),
    (_BLK, "attn", "inv_emb_to_v", "LayerNorm_0", "scale"), (_BLK, "attn", "inv_emb_to_v", "LayerNorm_0", "bias"),
    (_BLK, "attn", "inv_emb_to_v", "Dense_1", "kernel"), (_BLK, "attn", "inv_emb_to_v", "Dense_1", "bias"),
    (_BLK, "attn", "inv_emb_cond_mixer", "Dense_0", "kernel"), (_BLK, "attn", "inv_emb_cond_mixer", "Dense_0", "bias"),
    (_BLK, "attn", "inv_emb_cond_mixer", "LayerNorm_0", "scale"), (_BLK, "attn", "inv_emb_cond_mixer", "LayerNorm_0", "bias"),
    (_BLK, "attn", "inv_emb_cond_mixer", "Dense_1", "kernel"), (_BLK, "attn", "inv_emb_cond_mixer", "Dense_1", "bias"),
    (_BLK, "attn", "out_proj", "kernel"), (_BLK, "attn", "out_proj", "bias"),
    (_BLK, "pointwise_ffn", "Dense_0", "kernel"), (_BLK, "pointwise_ffn", "Dense_0", "bias"),
    (_BLK, "pointwise_ffn", "LayerNorm_0", "scale"), (_BLK, "pointwise_ffn", "LayerNorm_0", "bias"),
    (_BLK, "pointwise_ffn", "Dense_1", "kernel"), (_BLK, "pointwise_ffn", "Dense_1", "bias"),
    ("out_proj", "layers_0", "kernel"), ("out_proj", "layers_0", "bias"),
    ("out_proj", "layers_2", "kernel"), ("out_proj", "layers_2", "bias"),
    ("out_proj", "layers_4", "kernel"), ("out_proj", "layers_4", "bias"),
]
assert len(TENSOR_PATHS) == _lib.ENF_NUM_TENSORS
BLOCK_PATHS = [t[1:] for t in TENSOR_PATHS if t[0] == _BLK]       # the 38 tensors of one attention block


def _ffn_paths(branch):
    e = (_BLK, "attn", f"invariant_embedding_{branch}")
    return [e + ("Dense_0", "kernel"), None, e + ("Dense_0", "bias"), e + ("Dense_1", "kernel"), e + ("Dense_1", "bias")]


# the same list for embedding_type="ffn" (include/enf_hip.h, ENF_EMB_FFN): Dense_0 takes the R?_COEF / R?_B1 slots, Dense_1 the
# linear_final slots R?_W2 / R?_B2; the R?_W1 slots have no tensor (None)
FFN_TENSOR_PATHS = TENSOR_PATHS[:4] + _ffn_paths("query") + _ffn_paths("value") + TENSOR_PATHS[14:]
assert len(FFN_TENSOR_PATHS) == _lib.ENF_NUM_TENSORS


def tensor_paths(num_layers=0):
    """TENSOR_PATHS followed by the tensors of the latent self-attention blocks (NEF:137-167), layer by layer."""
    return TENSOR_PATHS + [(f"self_attention_blocks_{i}",) + t for i in range(num_layers) for t in BLOCK_PATHS]


def _get(tree, path):
    for k in path:
        tree = tree[k]
    return tree


def _set(tree, path, value):
    for k in path[:-1]:
        tree = tree.setdefault(k, {})
    tree[path[-1]] = value


_ptr = _lib.ptr
_POINTS = _Points()      # (the kind of the calls on points holds nothing of a call)


FUSED_FIT_STEP = __import__("os").environ.get("ENF_FIT_STEP") != "0"      # mse_value_and_latent_grads through enf_fit_step (one call)


class _EnfFunction(torch.autograd.Function):
    """nef.apply with the HIP forward (enf_forward) and backward-to-latents (enf_backward_latents)."""

    @staticmethod
    def forward(ctx, x, p, a, sigma, model, packed):
        lib = _lib.load()
        B, Z = p.shape[0], p.shape[1]
        N = x.shape[1]
        dev = p.device
        desc, ws, st = model._call_ctx(B, N, Z, dev, masks=model._masks)
        xb, xstride = model._x_arg(x)
        p_, a_, s_ = model._latent_args(p, a, sigma)
        out = torch.empty((B, N, model.num_out), device=dev, dtype=torch.float32)
        HD = model._Hp * model._Dp
        # no input needs a gradient (a decode): nothing will read this call's ybar / lse -- they stay in the workspace, and the pair
        # kernel may hand ybar to the tail as bf16 (ENF_STAGE_YBAR_HALF, include/enf_hip.h: same `out`, half the bytes)
        no_grad = not any(ctx.needs_input_grad[:4])
        ybar = None if no_grad else torch.empty((B, N, HD), device=dev, dtype=torch.float32)
        lse = None if no_grad else torch.empty((B, N, model._Hp), device=dev, dtype=torch.float32)
        # a backward follows when an input needs a gradient: stash the tail's pre-activations for it (ENF_STAGE_TAIL_SAVE)
        ctx.tail_saved = any(ctx.needs_input_grad[1:4])
        # the latent table depends on (p, a, sigma, weights) only and sits at the head of the workspace whatever N is: a
        # forward on the SAME latent tensors and weights as the last call on this workspace (the decode that follows a fit's
        # final-loss forward, pde_trainer.py:225-235 then :393-402) skips the prologue kernel
        lt_key = (ws.data_ptr(), packed.data_ptr(), B, Z) + tuple((t.data_ptr(), t._version) for t in (p_, a_) + ((s_,) if s_ is not None else ()))
        held = model._lt_held.get(ws.data_ptr())
        reuse_lt = held is not None and held[0] == lt_key and held[1] == model._ws_tags.get(ws.data_ptr())
        stages = _lib.ENF_STAGES_FORWARD | (_lib.ENF_STAGE_TAIL_SAVE if ctx.tail_saved else 0) | (_lib.ENF_STAGE_YBAR_HALF if no_grad else 0)
        if reuse_lt:
            stages &= ~_lib.ENF_STAGE_PROLOGUE
        _lib.launch(dev, lib.enf_forward_stages, ctypes.byref(desc), _ptr(xb), xstride, _ptr(p_), _ptr(a_), _ptr(s_), _ptr(packed),
                                          _ptr(out), _ptr(ybar), _ptr(lse), _ptr(ws), ws.numel(), stages, st)
        ctx.ws_tag = model._ws_touch(ws)      # backward may reuse the latent table if nothing else used the workspace
        # (the tensors are held with the entry: their addresses cannot come back under the same key with other values)
        model._lt_held[ws.data_ptr()] = (lt_key, ctx.ws_tag[1], (p_, a_, s_, packed))
        ctx.model = model
        ctx.has_sigma = sigma is not None
        ctx.xstride = xstride
        if not no_grad:
            ctx.save_for_backward(xb, p_, a_, s_ if s_ is not None else p_.new_empty(0), packed, ybar, lse)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        lib = _lib.load()
        model = ctx.model
        xb, p_, a_, s_, packed, ybar, lse = ctx.saved_tensors
        sigma = s_ if ctx.has_sigma else None
        B, Z = p_.shape[0], p_.shape[1]
        N = ybar.shape[1]
        dev = p_.device
        desc, ws, st = model._call_ctx(B, N, Z, dev)
        dout = dout.contiguous().float()
        dp = torch.empty_like(p_)
        da = torch.empty_like(a_)
        dsig = torch.empty((B, Z, 1), device=dev, dtype=torch.float32)
        reuse = _lib.ENF_BWD_REUSE_PROLOGUE if model._ws_tag(ws) == ctx.ws_tag else 0
        if reuse and ctx.tail_saved:
            reuse |= _lib.ENF_BWD_REUSE_TAIL
        reuse |= model._det_flag()
        _lib.launch(dev, lib.enf_backward_latents_ex, ctypes.byref(desc), _ptr(xb), ctx.xstride, _ptr(p_), _ptr(a_), _ptr(sigma),
                                               _ptr(packed), _ptr(ybar), _ptr(lse), _ptr(dout), _ptr(dp), _ptr(da),
                                               _ptr(dsig), _ptr(ws), ws.numel(), reuse, st)
        model._ws_touch(ws)
        return None, dp, da, (dsig if ctx.has_sigma else None), None, None


class EquivariantCrossAttentionNeF:
    """Equivariant cross-attention neural field (NEF:70-235) on the fused gfx950 path.

    Args mirror the Flax module's fields (NEF:85-96); ``precision`` ("bf16" | "f32") selects
    the MFMA arithmetic of the per-pair contractions (ENF_PREC_*).

    ``deterministic``: True = every native call of this model takes its deterministic form (include/enf_hip.h, "Deterministic
    mode": partial sums through scratch and fixed-order reductions instead of float atomics -- equal bits for equal inputs,
    shapes and kernel variants); False = the default (atomic) path; None = follow
    ``torch.are_deterministic_algorithms_enabled()`` at the time of each call.
    """

    default_pair_variants = ("auto", "auto")

    def __init__(self, num_hidden, num_heads, num_layers, num_out, latent_dim, cross_attn_invariant,
                 self_attn_invariant=None, embedding_type="rff", embedding_freq_multiplier=(0.05, 0.1),
                 condition_value_transform=True, use_gaussian_window=True, precision="bf16", deterministic=None):
        if not isinstance(cross_attn_invariant, BaseInvariant):
            raise TypeError("cross_attn_invariant must come from enf.steerable_attention.invariant.get_ca_invariant")
        if embedding_type not in ("rff", "ffn"):
            if embedding_type == "polynomial":
                raise NotImplementedError(f"embedding type '{embedding_type}' is outside the accelerated path "
                                          "(no shipped config selects it; SURVEY.md 2, row 2)")
            raise ValueError(f"Unknown embedding type: {embedding_type}.")          # EMB:33
        if embedding_type == "ffn":
            if int(num_layers) > 0:
                raise NotImplementedError("embedding type 'ffn' is built for num_layers = 0 only (no latent self-attention)")
            if cross_attn_invariant.name in ("ball", "ball_lat"):
                raise NotImplementedError(f"embedding type 'ffn' is not built for the '{cross_attn_invariant.name}' invariant")
        if not condition_value_transform:
            raise NotImplementedError("condition_value_transform=False is not on the accelerated path")
        if embedding_type == "rff":
            assert not num_hidden % 2, "For the Fourier Features hidden_dim should be even to calculate them correctly."  # RFF:75-77
        elif num_hidden % 2:
            # (the reference takes any width for ffn; the kernels' zero-padded widths are even: EnfDesc.d_true)
            raise NotImplementedError(f"embedding type 'ffn' is built for an even num_hidden, not {num_hidden}")
        if precision not in _lib.PREC:
            raise ValueError(f"unknown precision {precision!r}")
        if deterministic not in (None, True, False):
            raise ValueError("deterministic must be True, False or None (= follow torch.use_deterministic_algorithms)")
        self.deterministic = deterministic
        self.num_hidden, self.num_heads, self.num_layers = int(num_hidden), int(num_heads), int(num_layers)
        self._Dp = _pad.padded_width(self.num_hidden)      # width of the kernels that run it (zero-padded if wider)
        self._Hp = _pad.padded_heads(self.num_heads)       # heads of the kernels that run it (3 -> 4, one zero head)
        if self._Hp == 4 and self._Dp != 64:
            raise NotImplementedError("3 or 4 heads are built for num_hidden <= 64 only")
        self.num_out, self.latent_dim = int(num_out), int(latent_dim)
        self.cross_attn_invariant = cross_attn_invariant
        self.self_attn_invariant = self_attn_invariant if self_attn_invariant is not None else cross_attn_invariant
        if self.num_layers > 0:
            # latent self-attention (NEF:223-226) runs the same pair kernels with the latents' own positions as queries
            # (enf/models/_train.py: apply_layers); dormant in every shipped config, so only the plain shapes are served
            if self.self_attn_invariant.name not in _lib.INVARIANT_IDS:
                raise NotImplementedError(f"self-attention with the '{self.self_attn_invariant.name}' invariant is not built")
        self.embedding_type = embedding_type
        self.embedding_freq_multiplier = tuple(embedding_freq_multiplier)
        self.condition_value_transform = condition_value_transform
        self.use_gaussian_window = bool(use_gaussian_window)
        self.precision = precision
        self._pack_cache = {}
        self._ws_cache = {}
        self._ws_gen = 0
        self._ws_tags = {}
        self._lt_held = {}                      # workspace -> (key of the latent table it holds, its use tag, the tensors)
        self.pair_variants = None               # (forward, backward) pair-kernel variant of this model's calls (_lib.VARIANT
                                                # keys); None = the class default below (tests flip it to cover both kernels)
        self._masks = None                      # (buffer, "write" | "read", signals) inside relu_masks(), else None
        self._pair_key = self._pair_blob = self._train_blob = None      # the training path's packed blobs and their keys (_train.py)

    def with_precision(self, precision):
        """The same model (fields, invariants) running its per-pair contractions in another arithmetic ("f32" | "bf16"), with
        caches of its own; parameters are plain tensors, so both models take the same parameter tree."""
        import copy
        if precision not in _lib.PREC:
            raise ValueError(f"unknown precision {precision!r}")
        m = copy.copy(self)
        m.precision = precision
        m._pack_cache, m._ws_cache, m._ws_gen, m._ws_tags, m._masks, m._lt_held = {}, {}, 0, {}, None, {}
        m._pair_key = m._pair_blob = m._train_blob = None
        return m

    # ------------------------------------------------------------------ deterministic mode
    def is_deterministic(self):
        """Whether a native call made now takes its deterministic form: the constructor's ``deterministic``, or torch's global
        switch when that is None."""
        if self.deterministic is None:
            return bool(torch.are_deterministic_algorithms_enabled())
        return bool(self.deterministic)

    def _det_flag(self):
        """ENF_BWD_DETERMINISTIC / ENF_FIT_DETERMINISTIC / ENF_MSE_DETERMINISTIC (one bit) or 0."""
        return _lib.ENF_BWD_DETERMINISTIC if self.is_deterministic() else 0

    # ------------------------------------------------------------------ descriptors / buffers
    def _desc(self, B, N, Z, masks=None, inv=None, dx=None):
        """The call descriptor; ``masks`` = a (buffer, mode, signals) triple for calls whose pair kernels take relu masks.  ``inv`` and
        ``dx``: another invariant and coordinate width than the cross-attention's (the latent self-attention blocks of _train.py)."""
        inv = inv if inv is not None else self.cross_attn_invariant
        return _lib.make_desc(B, N, Z, self._Hp, self._Dp, self.latent_dim, self.num_out,
                              inv.num_x_pos_dims if dx is None else dx, inv.kernel_id, self.use_gaussian_window, _lib.PREC[self.precision],
                              d_true=self.num_hidden if self._Dp != self.num_hidden else 0,
                              h_true=self.num_heads if self._Hp != self.num_heads else 0,
                              variants=tuple(_lib.VARIANT[v] for v in (self.pair_variants or self.default_pair_variants)),
                              masks=masks, embedding=_lib.EMB[self.embedding_type])

    def _workspace(self, desc, device, size_query=None):
        # one cached scratch buffer per (shape, stream); the autograd graph never keeps it alive
        lib = _lib.load()
        # (sized for the deterministic form while the mode is on: its partial buffers sit behind the plain workspace)
        det = self._det_flag()
        if size_query is not None:          # an entry point with a size query of its own (desc, flags), e.g. enf_field_grad_workspace_bytes
            nbytes = size_query(ctypes.byref(desc), det)
        else:
            nbytes = lib.enf_workspace_bytes_ex(ctypes.byref(desc), det) if det else lib.enf_workspace_bytes(ctypes.byref(desc))
        if nbytes == 0:
            _lib.check(lib.enf_check_desc(ctypes.byref(desc)))
        key = (str(device), _lib.stream(device).value)
        ws = self._ws_cache.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(int(nbytes), device=device, dtype=torch.uint8)
            self._ws_cache[key] = ws
        return ws

    def _call_ctx(self, B, N, Z, dev, masks=None, size_query=None):
        """What every native call on this model starts from: (descriptor, workspace, stream argument) for a (B, N, Z) problem on the
        current stream of ``dev``; ``masks`` as in _desc, ``size_query`` as in _workspace."""
        desc = self._desc(B, N, Z, masks=masks)
        return desc, self._workspace(desc, dev, size_query), _lib.stream(dev)

    @staticmethod
    def _latent_args(p, a, sigma):
        """The latents as the library takes them: p, a float32 and contiguous, sigma (B, Z, 1) likewise or None."""
        p_ = p.float().contiguous()
        s_ = sigma.float().reshape(p_.shape[0], p_.shape[1], 1).contiguous() if sigma is not None else None
        return p_, a.float().contiguous(), s_

    def _ws_touch(self, ws):
        """Mark a use of workspace `ws`; returns the tag identifying this use."""
        self._ws_gen += 1
        self._ws_tags[ws.data_ptr()] = self._ws_gen
        return (ws.data_ptr(), self._ws_gen)

    def _ws_tag(self, ws):
        return (ws.data_ptr(), self._ws_tags.get(ws.data_ptr()))

    @staticmethod
    def _x_arg(x):
        """(tensor to pass, batch stride in elements); a stride-0 batch (broadcast grid) is legal (TR:197,393)."""
        if x.dim() != 3:
            raise ValueError("x must be (batch, num_coords, coord_dim)")
        if x.stride(0) == 0:
            return x[0].contiguous(), 0
        xc = x.contiguous()
        return xc, xc.shape[1] * xc.shape[2]

    # ------------------------------------------------------------------ parameters
    def init(self, key, x=None, p=None, a=None, gaussian_window_size=None, device=None):
        """Random parameters with the reference's initialisers.  ``key`` is an int
        seed or a torch.Generator (JAX PRNG keys cannot be reproduced).  The sample inputs are
        accepted for call-shape parity with ``nef.init(key, x, p, a, window)`` (TR:101) and only
        supply the device."""
        if device is None:
            device = p.device if p is not None else torch.device("cuda")
        g = key if isinstance(key, torch.Generator) else torch.Generator().manual_seed(int(key))
        D, H, C, O = self.num_hidden, self.num_heads, self.latent_dim, self.num_out
        I = self.cross_attn_invariant.dim
        HD = H * D

        def normal(shape, std):
            return torch.randn(shape, generator=g) * std

        def lecun(n_in, n_out):     # flax Dense default: truncated normal, std sqrt(1/fan_in) / .8796
            t = torch.empty(n_in, n_out)
            torch.nn.init.trunc_normal_(t, mean=0.0, std=1.0, a=-2.0, b=2.0, generator=g)
            return {"kernel": t * (math.sqrt(1.0 / n_in) / 0.87962566103423978), "bias": torch.zeros(n_out)}

        def ln(n):
            return {"scale": torch.ones(n), "bias": torch.zeros(n)}

        def ffn(n_in, n_hid, n_out):
            return {"Dense_0": lecun(n_in, n_hid), "LayerNorm_0": ln(n_hid), "Dense_1": lecun(n_hid, n_out)}

        def rff(std):
            lim = math.sqrt(3 * 2.0 / D)
            return {"encoding": {"coefficients": normal((I, D // 2), std)},                                   # RFF:83
                    "layers_0": {"linear": {"kernel": normal((D, D), math.sqrt(2.0 / D)), "bias": normal((D,), 1e-6)}},  # RFF:55-60
                    "linear_final": {"kernel": (torch.rand((D, D), generator=g) * 2 - 1) * lim, "bias": normal((D,), 1e-6)}}  # RFF:35-40

        def ffn_emb():      # FFNEmbedding (embedding/linear.py): Dense(I -> D) -> gelu -> Dense(D -> D), flax defaults
            return {"Dense_0": lecun(I, D), "Dense_1": lecun(D, D)}

        fq, fv = self.embedding_freq_multiplier        # (ignored by ffn, as in the reference: embedding/__init__.py:25-33)
        emb_q, emb_v = (ffn_emb(), ffn_emb()) if self.embedding_type == "ffn" else (rff(fq), rff(fv))
        attn = {"invariant_embedding_query": emb_q, "invariant_embedding_value": emb_v,
                "inv_emb_to_q": lecun(D, HD), "a_to_k": lecun(D, HD), "a_to_v": lecun(D, HD),
                "inv_emb_to_v": ffn(D, D, 2 * HD), "inv_emb_cond_mixer": ffn(D, D, D), "out_proj": lecun(HD, HD)}
        P = {"latent_stem": lecun(C, D),
             _BLK: {"layer_norm_attn": ln(D), "attn": attn, "pointwise_ffn": ffn(HD, HD, HD)},
             "out_proj": {"layers_0": lecun(HD, D), "layers_2": lecun(D, D), "layers_4": lecun(D, O)}}
        Is = self.self_attn_invariant.dim
        for i in range(self.num_layers):                                 # NEF:137-167 (project_heads=True: widths D)
            def rff_s(std):
                r = rff(std)
                r["encoding"]["coefficients"] = normal((Is, D // 2), std)
                return r
            P[f"self_attention_blocks_{i}"] = {
                "layer_norm_attn": ln(D),
                "attn": {"invariant_embedding_query": rff_s(fq), "invariant_embedding_value": rff_s(fv),
                         "inv_emb_to_q": lecun(D, HD), "a_to_k": lecun(D, HD), "a_to_v": lecun(D, HD),
                         "inv_emb_to_v": ffn(D, D, 2 * HD), "inv_emb_cond_mixer": ffn(D, D, D), "out_proj": lecun(HD, D)},
                "pointwise_ffn": ffn(D, D, D)}

        def to_dev(t):
            return {k: to_dev(v) for k, v in t.items()} if isinstance(t, dict) else t.to(device=device, dtype=torch.float32)
        return {"params": to_dev(P)}

    def tensor_paths(self):
        """This model's tensor paths in C-ABI order: ``tensor_paths(num_layers)`` for rff, FFN_TENSOR_PATHS (None in the unused
        ENF_W_R?_W1 slots) for ffn."""
        return FFN_TENSOR_PATHS if self.embedding_type == "ffn" else tensor_paths(self.num_layers)

    def param_tensors(self, params):
        """The ENF_NUM_TENSORS weight tensors in C-ABI order (then, for num_layers > 0, 38 per self-attention block); ffn: an
        empty tensor in each unused ENF_W_R?_W1 slot (so that optimiser states, all-reduces and the trainers' lists keep their
        46 entries; its gradient is None, like the frozen rff coefficients')."""
        P = params["params"] if "params" in params else params
        paths = self.tensor_paths()
        dev = _get(P, paths[0]).device
        return [torch.empty(0, device=dev) if path is None else _get(P, path) for path in paths]

    def invalidate_caches(self):
        """Forget the packed-weight blob, the packed pair panels of the training path and the latent tables held in workspaces.

        CONTRACT of the caches: reuse is decided from ``(tensor.data_ptr(), tensor._version)`` of the weight / latent tensors,
        so an update is seen when it goes through torch (in-place ops bump ``_version``; the optimisers and
        ``meta_sgd_update`` of this package return fresh tensors).  Writes torch cannot see -- through ``.data``, through a
        detached alias made before the call, by a raw-pointer kernel, ``hipMemcpy`` or a collective on an alias -- leave
        ``_version`` unchanged: call this method after such a write (``load_params`` does, for the tree it returns is new)."""
        self._pack_cache.clear()
        self._lt_held.clear()
        self._pair_key = self._pair_blob = self._train_blob = None

    def load_params(self, tree, device="cuda"):
        """Build a parameter tree from nested numpy / torch arrays (e.g. an exported Flax tree)."""
        self.invalidate_caches()
        P = tree["params"] if "params" in tree else tree
        out = {}
        for path in self.tensor_paths():
            if path is not None:
                _set(out, path, torch.as_tensor(_get(P, path)).to(device=device, dtype=torch.float32).contiguous())
        return {"params": out}

    def pack(self, params):
        """Packed weight blob (device uint8 tensor) for ``params``; cached until a tensor changes."""
        lib = _lib.load()
        ts = self.param_tensors(params)[:_lib.ENF_NUM_TENSORS]
        dev = ts[0].device
        if dev.type != "cuda":
            raise _lib.EnfError("parameters must live on the GPU: the decoder has no CPU path")
        key = (self.precision, tuple((t.data_ptr(), t._version) if t is not None else None for t in ts))
        hit = self._pack_cache.get("k")
        if hit is not None and hit[0] == key:
            return hit[1]
        desc = self._desc(1, 1, 1)
        _lib.check(lib.enf_check_desc(ctypes.byref(desc)))
        ts = [t.detach().to(torch.float32).contiguous() if t is not None else None for t in ts]
        self._check_shapes(ts)
        if self._Dp != self.num_hidden or self._Hp != self.num_heads:
            ts = [t.contiguous() if t is not None else None
                  for t in _pad.pad_tensors(ts, self.num_hidden, self._Dp, self.num_heads, self._Hp, ffn=self.embedding_type == "ffn")]
        nbytes = lib.enf_packed_weight_bytes(ctypes.byref(desc))
        blob = torch.empty(int(nbytes), device=dev, dtype=torch.uint8)
        arr = (ctypes.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])
        _lib.launch(dev, lib.enf_pack_weights, ctypes.byref(desc), arr, _ptr(blob), _lib.stream(dev))
        self._pack_cache["k"] = (key, blob, ts)   # keep the fp32 sources alive until the pack kernels ran
        return blob

    def _check_shapes(self, ts):
        shp_done = []
        for t, shp, path in zip(ts, self._expected_shapes(), self.tensor_paths()):
            if shp is None:           # ffn: an unused ENF_W_R?_W1 slot
                if t is not None and t.numel():
                    raise ValueError(f"the ffn embedding has no tensor in ENF_W_* slot {len(shp_done)}")
                shp_done.append(None)
                continue
            shp_done.append(shp)
            if t is None:
                raise ValueError(f"parameter {'/'.join(path)} is missing")
            if tuple(t.shape) != shp:
                raise ValueError(f"parameter {'/'.join(path)} has shape {tuple(t.shape)}, expected {shp}")

    def _expected_shapes(self):
        D, H, C, O, I = self.num_hidden, self.num_heads, self.latent_dim, self.num_out, self.cross_attn_invariant.dim
        HD = H * D
        rff = [(I, D), None, (D,), (D, D), (D,)] if self.embedding_type == "ffn" else [(I, D // 2), (D, D), (D,), (D, D), (D,)]
        return ([(C, D), (D,), (D,), (D,)] + rff + rff + [(D, HD), (HD,)] * 3 +
                [(D, D), (D,), (D,), (D,), (D, 2 * HD), (2 * HD,)] + [(D, D), (D,), (D,), (D,), (D, D), (D,)] +
                [(HD, HD), (HD,)] + [(HD, HD), (HD,), (HD,), (HD,), (HD, HD), (HD,)] +
                [(HD, D), (D,), (D, D), (D,), (D, O), (O,)])

    # ------------------------------------------------------------------ forward
    def _check_inputs(self, what, x, p, a, gaussian_window_size):
        """The input checks of the entry point ``what`` (apply and the derivative calls): device, coordinate / pose / latent widths,
        batch agreement and the presence of the window.  Returns sigma: the window as a tensor (a scalar is expanded to (B, Z, 1)), or
        None for a model without one."""
        if not (x.is_cuda and p.is_cuda and a.is_cuda):
            raise _lib.EnfError(f"EquivariantCrossAttentionNeF.{what} needs CUDA/HIP tensors: there is no CPU path")
        inv = self.cross_attn_invariant
        if x.shape[-1] != inv.num_x_pos_dims:
            raise AssertionError(f"x has coordinate width {x.shape[-1]}, invariant '{inv.name}' expects {inv.num_x_pos_dims}")
        if p.shape[-1] != inv.num_z_pos_dims + inv.num_z_ori_dims:
            raise AssertionError(f"p has width {p.shape[-1]}, expected {inv.num_z_pos_dims + inv.num_z_ori_dims}")
        if a.shape[-1] != self.latent_dim:
            raise AssertionError(f"a has width {a.shape[-1]}, expected latent_dim={self.latent_dim}")
        if x.shape[0] != p.shape[0] or a.shape[:2] != p.shape[:2]:
            raise AssertionError("batch / latent dimensions of x, p, a disagree")
        sigma = gaussian_window_size if self.use_gaussian_window else None
        if self.use_gaussian_window and sigma is None:
            raise AssertionError("gaussian_window_size is required when use_gaussian_window=True")
        if sigma is not None and not torch.is_tensor(sigma):
            sigma = torch.full((p.shape[0], p.shape[1], 1), float(sigma), device=p.device)
        return sigma

    def apply(self, params, x, p, a, gaussian_window_size=None):
        """nef.apply(params, x, p, a, gaussian_window) -> (B, N, num_out)   (NEF:204-235).

        x (B,N,dx) [stride-0 batch allowed], p (B,Z,z_pos+z_ori), a (B,Z,latent_dim),
        gaussian_window_size (B,Z,1).  Differentiable w.r.t. p, a, gaussian_window_size, the weights and x.
        """
        sigma = self._check_inputs("apply", x, p, a, gaussian_window_size)
        x = x.float()
        p, a, sigma = self._latent_args(p, a, sigma)
        ts = self.param_tensors(params)
        if self.num_layers > 0:
            from . import _train
            self._check_shapes(ts)
            return _train.apply_layers(self, ts, x, p, a, sigma)
        if torch.is_grad_enabled() and (x.requires_grad or any(t is not None and t.requires_grad for t in ts)):
            # training path: gradients w.r.t. the weights (TR:255, NTR:304-339) and / or the query coordinates
            from . import _train
            self._check_shapes(ts)
            return _train.apply_train(self, ts, x, p, a, sigma)
        packed = self.pack(params)
        return _EnfFunction.apply(x, p, a, sigma, self, packed)

    __call__ = apply

    # ------------------------------------------------------------------ derivative fields
    def _field_grad_args(self, what, x, p, a, gaussian_window_size):
        """The checks of ``apply`` for the derivative calls, then (x tensor, its batch stride, p, a, sigma or None) as the library
        takes them."""
        if self.num_layers > 0:
            raise NotImplementedError(f"{what} is built for num_layers = 0 (the fused decoder)")
        sigma = self._check_inputs(what, x, p, a, gaussian_window_size)
        if x.dim() != 3:
            raise AssertionError(f"x has shape {tuple(x.shape)}, expected (B, N, {x.shape[-1]})")
        p_, a_, s_ = self._latent_args(p, a, sigma)
        return (*self._x_arg(x.float()), p_, a_, s_)

    @torch.no_grad()
    def jacobian(self, params, x, p, a, gaussian_window_size=None, return_out=True):
        """The decode and its Jacobian w.r.t. the query coordinates in one native call (include/enf_hip.h: enf_field_grad):
        jac[b, n, o, i] = d out[b, n, o] / d x[b, n, i], returned as (out (B, N, O) or None, jac (B, N, O, dx)); ``jac`` is a permuted view
        of the call's (O, B, N, dx) buffer.  No autograd graph is built and none of the inputs gets a gradient; ``deterministic``
        selects the fixed-order sums (equal bits for equal inputs) in place of float atomics.
        Derivatives are w.r.t. the coordinates as given -- angles for the spherical and ball invariants, no metric factors -- and per
        signal also for a stride-0 (broadcast) ``x``: sum over the batch for the derivative w.r.t. a shared grid.
        ``return_out`` False skips the store of the decode."""
        xb, xstride, p_, a_, s_ = self._field_grad_args("jacobian", x, p, a, gaussian_window_size)
        lib = _lib.load()
        packed = self.pack(params)
        B, Z, N, dev = p_.shape[0], p_.shape[1], x.shape[1], p_.device
        desc, ws, st = self._call_ctx(B, N, Z, dev, size_query=lib.enf_field_grad_workspace_bytes)
        out = torch.empty((B, N, self.num_out), device=dev, dtype=torch.float32) if return_out else None
        jac = torch.empty((self.num_out, B, N, x.shape[-1]), device=dev, dtype=torch.float32)
        _lib.launch(dev, lib.enf_field_grad, ctypes.byref(desc), _ptr(xb), xstride, _ptr(p_), _ptr(a_), _ptr(s_), _ptr(packed), _ptr(out),
                    _ptr(jac), _ptr(ws), ws.numel(), self._det_flag(), st)
        self._ws_touch(ws)
        return out, jac.permute(1, 2, 0, 3)

    @torch.no_grad()
    def query_vjp(self, params, x, p, a, gaussian_window_size, dout):
        """dx (B, N, dx) = sum_o dout[b, n, o] * d out[b, n, o] / d x[b, n, :] for a seed ``dout`` (B, N, O), in one native call with one
        backward pass (include/enf_hip.h: enf_query_vjp); per signal, coordinates as given, no autograd -- see ``jacobian``."""
        xb, xstride, p_, a_, s_ = self._field_grad_args("query_vjp", x, p, a, gaussian_window_size)
        B, Z, N, dev = p_.shape[0], p_.shape[1], x.shape[1], p_.device
        if tuple(dout.shape) != (B, N, self.num_out):
            raise AssertionError(f"dout has shape {tuple(dout.shape)}, expected {(B, N, self.num_out)}")
        lib = _lib.load()
        packed = self.pack(params)
        g = dout.float().contiguous()
        desc, ws, st = self._call_ctx(B, N, Z, dev, size_query=lib.enf_field_grad_workspace_bytes)
        dx = torch.empty((B, N, x.shape[-1]), device=dev, dtype=torch.float32)
        _lib.launch(dev, lib.enf_query_vjp, ctypes.byref(desc), _ptr(xb), xstride, _ptr(p_), _ptr(a_), _ptr(s_), _ptr(packed), _ptr(g), None,
                    _ptr(dx), _ptr(ws), ws.numel(), self._det_flag(), st)
        self._ws_touch(ws)
        return dx

    # ------------------------------------------------------------------ tendency fields
    def _tangent_refusals(self, what, tangents, xdot=None):
        """What the forward-mode calls do not serve, and a call without any direction: the checks that look at no tensor's shape or
        device (``gn_cell_product`` runs them in front of its shape checks)."""
        if self.num_layers > 0:
            raise NotImplementedError(f"{what} is built for num_layers = 0 (the fused decoder)")
        if self.embedding_type != "rff":
            raise NotImplementedError(f"{what} serves the rff embedding, not '{self.embedding_type}'")
        name = self.cross_attn_invariant.name
        if name in ("ball", "ball_lat", "ponita_full"):
            raise NotImplementedError(f"{what} does not serve the '{name}' invariant (no tangent of the per-latent phase / rotation)")
        if xdot is None and all(t is None for _, t in tangents):
            raise ValueError(f"{what} needs at least one of " + ", ".join(n for n, _ in tangents) + (", xdot" if what == "tangent" else ""))

    def _tangent_args(self, what, x, p, a, gaussian_window_size, tangents, xdot=None):
        """The refusals and argument checks of the forward-mode calls (``tangent``, ``gn_product``), then _field_grad_args' tuple.
        ``tangents``: ((name, tensor or None) for p, a, window), shapes of p / a / (B, Z, 1).  ``xdot`` (``tangent`` only): a query
        direction or None; it counts as a tangent and is checked against x (shape, float32, the latents' device) before anything
        touches the device; its layout is handled as x's (_x_arg)."""
        self._tangent_refusals(what, tangents, xdot)
        if xdot is not None:
            if x.dim() != 3 or tuple(xdot.shape) != tuple(x.shape):
                raise AssertionError(f"xdot has shape {tuple(xdot.shape)}, expected x's {tuple(x.shape)}")
            if xdot.device != p.device or xdot.dtype != torch.float32:
                raise ValueError(f"xdot must be a float32 tensor on {p.device}")
        xb, xstride, p_, a_, s_ = self._field_grad_args(what, x, p, a, gaussian_window_size)
        B, Z, dev = p_.shape[0], p_.shape[1], p_.device
        for (label, t), shape in zip(tangents, (tuple(p_.shape), tuple(a_.shape), (B, Z, 1))):
            if t is None:
                continue
            if tuple(t.shape) != shape:
                raise AssertionError(f"{label} has shape {tuple(t.shape)}, expected {shape}")
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"{label} must be a contiguous float32 tensor on {dev}")
        if self._masks is not None:
            raise NotImplementedError(f"{what} does not take relu masks")
        return xb, xstride, p_, a_, s_

    # ------------------------------------------------------------------ Gauss-Newton product
    def gn_reserve(self, B, N, Z, device, op=None):
        """Size this stream's cached workspace for ``gn_product`` on a (B, N, Z) problem.  The cache grows by REPLACING a buffer, so a
        fit step whose workspace a following ``gn_product(reuse=...)`` is to reuse must already run on the larger buffer: call this
        first.  ``op``: a SparseObservations -- the buffer of ``gn_operator_product`` (enf_gn_a_workspace_bytes), which also holds
        ``mse_value_and_operator_grads`` and ``eval_operator_loss`` against that operator.  Returns the workspace's current tag
        (``workspace_tag``)."""
        lib = _lib.load()
        self._call_ctx(B, N, Z, torch.device(device), size_query=lib.enf_gn_workspace_bytes if op is None else _Operator(op).gn_size_query)
        return self.workspace_tag(device)

    def workspace_tag(self, device):
        """The tag of the last native call on this stream's cached workspace of ``device`` (None before the first): what
        ``gn_product(reuse=...)`` takes right after the fit step at the same point."""
        device = torch.device(device)
        ws = self._ws_cache.get((str(device), _lib.stream(device).value))
        return None if ws is None else self._ws_tag(ws)

    @torch.no_grad()
    def gn_product(self, params, x, p, a, gaussian_window_size, vp=None, va=None, vwindow=None, weight=None, channel_weight=None,
                   grad_scale=1.0, reuse=None):
        """The Gauss-Newton matrix of a latent fit applied to a direction, in one native call (include/enf_hip.h: enf_gn_product):
        (gp, ga, gwindow or None) = grad_scale * 2 / (B N O) * J^T W J (vp, va, vwindow) with J = d out / d (p, a, window) and W the
        loss weights of ``mse_value_and_latent_grads`` (``weight`` (B, N), ``channel_weight`` (B, N, O), or 1).  With the fit step's
        ``grad_scale`` this is the Gauss-Newton Hessian of that step's loss in the units of its gradient.  ``vp`` / ``va`` /
        ``vwindow`` as the tangents of ``tangent``: each may be None (= zero), not all three.  The model's deterministic mode selects
        the fixed-order sums of the backward pair kernel.
        ``reuse``: the ``workspace_tag`` taken right after the ``mse_value_and_latent_grads`` (not ``shared_latents``) or the
        ``gn_product`` that last ran at the SAME (x, p, a, window, params) on this stream -- the latent prologue is then not recomputed.
        A tag that is no longer the workspace's current one silently recomputes.  Size the buffer first: ``gn_reserve``."""
        latents = self._tangent_args("gn_product", x, p, a, gaussian_window_size, (("vp", vp), ("va", va), ("vwindow", vwindow)))
        if weight is not None and channel_weight is not None:
            raise _POINTS.both("gn_product")
        _POINTS.shapes(p.shape[0], x.shape[1], x.shape[1], self.num_out, None, weight, channel_weight)
        return self._gn_call(_POINTS, params, x.shape[1], latents, (vp, va, vwindow), weight, channel_weight, grad_scale, reuse)

    def _gn_call(self, kind, params, N, latents, v, weight, cweight, grad_scale, reuse):
        """The native call of ``gn_product`` / ``gn_cell_product`` / ``gn_operator_product`` behind their checks.  ``latents``: _tangent_args' tuple."""
        xb, xstride, p_, a_, s_ = latents
        B, Z, dev = p_.shape[0], p_.shape[1], p_.device
        lib = _lib.load()
        packed = self.pack(params)
        w_, cw_ = _f32(weight), _f32(cweight)
        desc, ws, st = self._call_ctx(B, N, Z, dev, size_query=kind.gn_size_query or lib.enf_gn_workspace_bytes)
        flags = self._det_flag()
        if reuse is not None and reuse == self._ws_tag(ws) and reuse[1] is not None:
            flags |= _lib.ENF_GN_REUSE_POINT
        gp, ga = torch.empty_like(p_), torch.empty_like(a_)
        gs = torch.empty((B, Z, 1), device=dev, dtype=torch.float32)
        fn, mid = kind.gn(lib, w_, cw_)
        _lib.launch(dev, fn, ctypes.byref(desc), _ptr(xb), xstride, _ptr(p_), _ptr(a_), _ptr(s_), _ptr(v[0]), _ptr(v[1]), _ptr(v[2]),
                    _ptr(packed), *mid, float(grad_scale), _ptr(gp), _ptr(ga), _ptr(gs), _ptr(ws), ws.numel(), flags, st)
        self._ws_touch(ws)
        return gp, ga, (gs if s_ is not None else None)

    @torch.no_grad()
    def tangent(self, params, x, p, a, gaussian_window_size, dp=None, da=None, dwindow=None, return_out=True, xdot=None):
        """The decode in forward mode along a latent direction, in one native call (include/enf_hip.h: enf_field_tangent):
        tan[b, n, o] = sum_z d out[b, n, o] / d (p, a, window)[b, z, :] . (dp, da, dwindow)[b, z, :], returned as (out (B, N, O) or
        None, tan (B, N, O)).  With (dp, da, dwindow) = the latent ODE's right-hand side this is d u / d t of the decoded field.
        ``dp`` / ``da`` / ``dwindow`` have the shapes of p / a / the window (B, Z, 1) and must be float32 and contiguous on the
        latents' device; each may be None (= zero).  ``dwindow`` of a model without a window contributes exactly zero.
        ``xdot``: None, or a direction in the query coordinates, float32 (B, N, dx) on the latents' device; a stride-0 batch
        expansion (one direction field for all signals) is passed as such, as for ``x``; the same pass then adds sum_i d out / d x[b, n, i] xdot[b, n, i]
        (include/enf_hip.h: enf_field_tangent_x) -- alone a directional derivative of the field, with the latent direction the
        material derivative.  In the coordinates as given, as ``jacobian``: angle rates on the sphere, no metric factors.  With
        ``xdot`` the three latent tangents may all be None; all four None is a ValueError.  Without it the call is
        enf_field_tangent's, bit for bit.
        No autograd graph is built and none of the inputs gets a gradient.  Every element is written once without atomics: equal
        inputs give equal bits.  ``return_out`` False skips the store of the decode."""
        xb, xstride, p_, a_, s_ = self._tangent_args("tangent", x, p, a, gaussian_window_size, (("dp", dp), ("da", da), ("dwindow", dwindow)),
                                                     xdot=xdot)
        B, Z, N, dev = p_.shape[0], p_.shape[1], x.shape[1], p_.device
        lib = _lib.load()
        packed = self.pack(params)
        desc, ws, st = self._call_ctx(B, N, Z, dev, size_query=lambda d, flags: lib.enf_field_tangent_workspace_bytes(d))
        out = torch.empty((B, N, self.num_out), device=dev, dtype=torch.float32) if return_out else None
        tan = torch.empty((B, N, self.num_out), device=dev, dtype=torch.float32)
        if xdot is None:
            _lib.launch(dev, lib.enf_field_tangent, ctypes.byref(desc), _ptr(xb), xstride, _ptr(p_), _ptr(a_), _ptr(s_), _ptr(dp), _ptr(da),
                        _ptr(dwindow), _ptr(packed), _ptr(out), _ptr(tan), _ptr(ws), st)
        else:
            xd, xdstride = self._x_arg(xdot)
            _lib.launch(dev, lib.enf_field_tangent_x, ctypes.byref(desc), _ptr(xb), xstride, _ptr(xd), xdstride, _ptr(p_), _ptr(a_), _ptr(s_),
                        _ptr(dp), _ptr(da), _ptr(dwindow), _ptr(packed), _ptr(out), _ptr(tan), _ptr(ws), st)
        self._ws_touch(ws)
        return out, tan

    @torch.no_grad()
    def second_derivative(self, params, x, p, a, gaussian_window_size, xdot, return_out=True, return_first=True):
        """The decode in forward mode to second order along a direction in the query coordinates, in one native call
        (include/enf_hip.h: enf_field_second_x): (out (B, N, O) or None, tan (B, N, O) or None, tan2 (B, N, O)) with
        tan[b, n, o] = sum_i d out / d x[b, n, i] xdot[b, n, i] (``tangent``'s value along ``xdot`` alone) and
        tan2[b, n, o] = sum_ij xdot[b, n, i] xdot[b, n, j] d^2 out / d x[b, n, i] d x[b, n, j].  With xdot = e_i tan2 is a diagonal entry of
        the Hessian; fitting.decode_laplacian / decode_hessian build the operators from such passes.
        ``xdot``: float32 (B, N, dx) on the latents' device, required, checked and passed as ``tangent`` does (a stride-0 batch expansion
        is passed as such).  In the coordinates as given, as ``jacobian``: angles on the sphere, no metric factors.  Second derivatives as
        autograd means them: almost everywhere, the relu kinks contribute nothing.
        No autograd graph is built and none of the inputs gets a gradient.  Every element is written once without atomics: equal
        inputs give equal bits.  ``return_out`` / ``return_first`` False skip the stores of the decode / the first derivative."""
        if xdot is None:
            raise ValueError("second_derivative needs xdot")
        xb, xstride, p_, a_, s_ = self._tangent_args("second_derivative", x, p, a, gaussian_window_size,
                                                     (("dp", None), ("da", None), ("dwindow", None)), xdot=xdot)
        B, Z, N, dev = p_.shape[0], p_.shape[1], x.shape[1], p_.device
        lib = _lib.load()
        packed = self.pack(params)
        desc, ws, st = self._call_ctx(B, N, Z, dev, size_query=lambda d, flags: lib.enf_field_second_workspace_bytes(d))
        new = lambda: torch.empty((B, N, self.num_out), device=dev, dtype=torch.float32)
        out, tan, tan2 = (new() if return_out else None), (new() if return_first else None), new()
        xd, xdstride = self._x_arg(xdot)
        _lib.launch(dev, lib.enf_field_second_x, ctypes.byref(desc), _ptr(xb), xstride, _ptr(xd), xdstride, _ptr(p_), _ptr(a_), _ptr(s_),
                    _ptr(packed), _ptr(out), _ptr(tan), _ptr(tan2), _ptr(ws), st)
        self._ws_touch(ws)
        return out, tan, tan2

    # ------------------------------------------------------------------ relu masks (second-order terms by differences)
    def relu_mask_buffer(self, B, N, Z, device):
        """Device buffer for the relu masks of a (B, N, Z) problem (enf_relu_mask_bytes)."""
        desc = self._desc(B, N, Z)
        return torch.empty(int(_lib.load().enf_relu_mask_bytes(ctypes.byref(desc))) // 4, device=device, dtype=torch.int32)

    def relu_masks(self, buf, mode, signals):
        """Context manager: inside it, THIS model's pair-kernel forwards (any path) WRITE ("write") the relu masks of their
        pre-activations into ``buf``, or its forwards and the weight-gradient backwards of those forwards READ ("read") them
        -- relu linearised at the point the masks were taken, for signals b, b + signals, ... alike (include/enf_hip.h:
        EnfDesc.mask_mode).  The masks travel in each call's descriptor: other models and streams are not affected."""
        import contextlib
        if mode not in ("write", "read"):
            raise ValueError("mode must be 'write' or 'read'")

        @contextlib.contextmanager
        def cm():
            prev, self._masks = self._masks, (buf, mode, int(signals))
            try:
                yield buf
            finally:
                self._masks = prev
        return cm()

    @torch.no_grad()
    def mse_value_and_latent_grads(self, params, x, p, a, gaussian_window_size, target, grad_scale=1.0, loss_out=None, weight=None,
                                   channel_weight=None, return_errors=False, shared_latents=False):
        """loss = mean((nef.apply(params, x, p, a, window) - target)^2) and grad_scale * d loss / d(p, a, window) in one
        sequence of HIP launches (forward, loss + d out, backward), without building an autograd graph: what one
        inner step of the MAML loop computes (pde_trainer.py:175-207; grad_scale = B there).
        ``loss_out``: an already ZEROED float32 (1,) tensor to accumulate the loss into (saves the fill per call).
        ``weight``: None, or (B, N) loss weights per signal and query point, finite and >= 0 (include/enf_hip.h, "Weighted
        loss"): loss = sum_{b,n} weight[b,n] sum_o (out - target)^2 / (B N O), not normalised here (fitting/weights.py does
        that); a point of weight 0 does not exist -- its target may be NaN.
        ``channel_weight``: None, or (B, N, O) loss weights per signal, query point and output channel (the same section:
        enf_fit_step_cw): loss = sum_{b,n,o} channel_weight[b,n,o] (out - target)^2 / (B N O); the rule holds per value.  Not
        together with ``weight`` (ValueError).
        ``return_errors``: also return the per-point errors err (B, N) = sum_o w (out - target)^2 and the per-signal losses loss_b (B,)
        = err.sum(1) / (N O) of this step (include/enf_hip.h, "Per-signal and per-point errors": enf_fit_step_e -- the same kernels
        with one store added, so loss and gradients are the bits of the call without it).  Needs the one-call step.
        ``shared_latents``: the caller's statement that every signal holds the same latents (p, a, window) and that ``x`` is one point
        set expanded over the signals with stride 0 -- the first inner step of a fit (include/enf_hip.h: ENF_FIT_SHARED_LATENTS).  The
        one-call step may then run its forward pair kernel once for all signals; ignored on the composed fallbacks.
        Returns (loss (1,), dp, da, dwindow or None), with ``return_errors`` followed by (err, loss_b)."""
        if return_errors and not (x.is_cuda and p.is_cuda and a.is_cuda and target.is_cuda):
            raise _lib.EnfError("mse_value_and_latent_grads(return_errors=True) needs CUDA/HIP tensors: there is no CPU path")
        if return_errors and (self.num_layers > 0 or not FUSED_FIT_STEP):
            raise NotImplementedError("return_errors needs the one-call inner step (enf_fit_step_e): num_layers = 0 and ENF_FIT_STEP on")
        B, N = p.shape[0], x.shape[1]
        if weight is not None and channel_weight is not None:
            raise _POINTS.both("mse_value_and_latent_grads")
        _POINTS.shapes(B, N, N, self.num_out, None, weight, channel_weight)
        if self.num_layers > 0:           # no fused sequence for the layered model: autograd through apply()
            weight, channel_weight = _f32(weight), _f32(channel_weight)
            sigma = gaussian_window_size if self.use_gaussian_window else None
            with torch.enable_grad():
                leaves = [t.detach().float().requires_grad_(True) for t in (p, a)] + \
                         ([sigma.detach().float().requires_grad_(True)] if sigma is not None else [])
                out = self.apply(params, x, leaves[0], leaves[1], leaves[2] if sigma is not None else None)
                if channel_weight is not None:
                    dd = torch.where(channel_weight > 0, out - target, torch.zeros_like(out))
                    loss = (channel_weight * dd * dd).mean()
                elif weight is None:
                    loss = ((out - target) ** 2).mean()
                else:
                    wgt = weight[..., None]
                    dd = torch.where(wgt > 0, out - target, torch.zeros_like(out))
                    loss = (wgt * dd * dd).mean()
                g = torch.autograd.grad(loss * grad_scale, leaves, allow_unused=True)
            g = [torch.zeros_like(t) if gi is None else gi for t, gi in zip(leaves, g)]
            if loss_out is not None:
                loss_out.add_(loss.detach().reshape(1))
            return loss.detach().reshape(1), g[0], g[1], (g[2] if sigma is not None else None)
        _POINTS.shapes(B, N, N, self.num_out, target, None, None)
        return self._fit_step(_POINTS, N, params, x, p, a, gaussian_window_size, target, weight, channel_weight, grad_scale, loss_out,
                              return_errors, shared_latents)

    def _fit_step(self, kind, M, params, x, p, a, gaussian_window_size, target, weight, cweight, grad_scale, loss_out, return_errors,
                  shared_latents=False, deterministic=None):
        """The one body of the fit steps (``mse_value_and_latent_grads`` / ``_cell_grads`` / ``_operator_grads``) behind their checks:
        the arguments as the library takes them, descriptor and workspace, the output buffers, the kind's native call (_obs_calls.py).
        Returns (loss (1,), dp, da, dwindow or None), with ``return_errors`` followed by (err (B, M), loss_b (B,))."""
        sigma = gaussian_window_size if self.use_gaussian_window else None
        if self.use_gaussian_window and sigma is None:
            raise AssertionError("gaussian_window_size is required when use_gaussian_window=True")
        lib = _lib.load()
        packed = self.pack(params)
        p_, a_, s_ = self._latent_args(p, a, sigma)
        B, Z, N, dev = p_.shape[0], p_.shape[1], x.shape[1], p_.device
        xb, xstride = self._x_arg(x.float())
        flags = self._det_flag() if deterministic is None else (_lib.ENF_FIT_DETERMINISTIC if deterministic else 0)
        desc, ws, st = self._call_ctx(B, N, Z, dev, masks=self._masks, size_query=kind.size_query)
        tgt = target.float().contiguous()
        w_ = weight.float().contiguous() if weight is not None else None
        cw_ = cweight.float().contiguous() if cweight is not None else None
        loss = loss_out if loss_out is not None else torch.zeros(1, device=dev, dtype=torch.float32)
        dp, da = torch.empty_like(p_), torch.empty_like(a_)
        dsig = torch.empty((B, Z, 1), device=dev, dtype=torch.float32)
        err = torch.empty((B, M), device=dev, dtype=torch.float32) if return_errors else None
        loss_b = torch.empty((B,), device=dev, dtype=torch.float32) if return_errors else None
        res = (loss, dp, da, dsig if sigma is not None else None)
        if kind is _POINTS and not FUSED_FIT_STEP:       # the same step as three library calls (cross-check in the tests, A/B in scripts/)
            HD = self._Hp * self._Dp
            out = torch.empty((B, N, self.num_out), device=dev, dtype=torch.float32)
            ybar = torch.empty((B, N, HD), device=dev, dtype=torch.float32)
            lse = torch.empty((B, N, self._Hp), device=dev, dtype=torch.float32)
            _lib.launch(dev, lib.enf_forward_stages, ctypes.byref(desc), _ptr(xb), xstride, _ptr(p_), _ptr(a_), _ptr(s_), _ptr(packed),
                        _ptr(out), _ptr(ybar), _ptr(lse), _ptr(ws), ws.numel(),
                        _lib.ENF_STAGES_FORWARD | _lib.ENF_STAGE_TAIL_SAVE | _lib.ENF_STAGE_PREPARE_BWD, st)
            dout = torch.empty_like(out)
            nmse = int(lib.enf_mse_scratch_bytes(out.numel(), flags))
            mse_scr = torch.empty(nmse, device=dev, dtype=torch.uint8) if nmse else None
            if cw_ is not None:
                _lib.launch(dev, lib.enf_mse_value_grad_cw, _ptr(out), _ptr(tgt), _ptr(cw_), out.numel(), float(grad_scale),
                            _ptr(dout), _ptr(loss), _ptr(mse_scr), nmse, flags, st)
            else:
                _lib.launch(dev, lib.enf_mse_value_grad_w, _ptr(out), _ptr(tgt), _ptr(w_), out.numel(), self.num_out, float(grad_scale),
                            _ptr(dout), _ptr(loss), _ptr(mse_scr), nmse, flags, st)
            _lib.launch(dev, lib.enf_backward_latents_ex, ctypes.byref(desc), _ptr(xb), xstride, _ptr(p_), _ptr(a_), _ptr(s_),
                        _ptr(packed), _ptr(ybar), _ptr(lse), _ptr(dout), _ptr(dp), _ptr(da), _ptr(dsig), _ptr(ws), ws.numel(),
                        _lib.ENF_BWD_REUSE_PROLOGUE | _lib.ENF_BWD_REUSE_TAIL | _lib.ENF_BWD_REUSE_PREPARED | flags, st)
            self._ws_touch(ws)
            return res
        # ONE library call per step (include/enf_hip.h: enf_fit_step): prologue, pair forward, the tail with the loss and its gradient
        # (on points and cells a single kernel that forms them in registers), pair backward, prologue backward
        if shared_latents:
            flags |= _lib.ENF_FIT_SHARED_LATENTS
        fn, rest = kind.fit(lib, w_, cw_, shared_latents, (float(grad_scale), _ptr(loss), _ptr(dp), _ptr(da), _ptr(dsig)), (err, loss_b),
                            (_ptr(ws), ws.numel()))
        _lib.launch(dev, fn, ctypes.byref(desc), _ptr(xb), xstride, _ptr(p_), _ptr(a_), _ptr(s_), _ptr(packed), _ptr(tgt), *rest, flags, st)
        self._ws_touch(ws)
        return res + (err, loss_b) if return_errors else res

    @torch.no_grad()
    def eval_loss(self, params, x, p, a, gaussian_window_size, target, weight=None, channel_weight=None, loss_out=None, per_signal=True):
        """Evaluation without a decode (include/enf_hip.h: enf_eval_loss): the per-point errors err (B, N) = sum_o w (out - target)^2
        and the per-signal losses loss_b (B,) = err.sum(1) / (N O) of nef.apply(params, x, p, a, window) against ``target`` (B, N, O),
        formed in the tail's registers -- no ``out``, no autograd.  ``weight`` (B, N) / ``channel_weight`` (B, N, O) as in
        mse_value_and_latent_grads: a value of weight 0 does not exist, its target may be NaN.  Both results are the same bits for the
        same inputs in every mode.
        ``loss_out``: an already ZEROED float32 (1,) tensor; the scalar loss (the mean over all B N O values) is added to it.
        ``per_signal`` False skips the per-signal sums (a caller that evaluates a grid in chunks sums once: ``signal_losses``).
        Returns (loss_b or None, err)."""
        if not (x.is_cuda and p.is_cuda and a.is_cuda and target.is_cuda):
            raise _lib.EnfError("EquivariantCrossAttentionNeF.eval_loss needs CUDA/HIP tensors: there is no CPU path")
        if self.num_layers > 0:
            raise NotImplementedError("eval_loss is built for num_layers = 0 (the fused decoder)")
        if weight is not None and channel_weight is not None:
            raise _POINTS.both("eval_loss")
        _POINTS.shapes(p.shape[0], x.shape[1], x.shape[1], self.num_out, target, weight, channel_weight)
        return self._eval(_POINTS, x.shape[1], params, x, p, a, gaussian_window_size, target, weight, channel_weight, loss_out, per_signal)

    def _eval(self, kind, M, params, x, p, a, gaussian_window_size, target, weight, cweight, loss_out, per_signal, deterministic=None):
        """The one body of the evaluations (``eval_loss`` / ``eval_cell_loss`` / ``eval_operator_loss``) behind their checks, as
        _fit_step.  Returns (loss_b (B,) or None, err (B, M))."""
        sigma = gaussian_window_size if self.use_gaussian_window else None
        if self.use_gaussian_window and sigma is None:
            raise AssertionError("gaussian_window_size is required when use_gaussian_window=True")
        lib = _lib.load()
        packed = self.pack(params)
        p_, a_, s_ = self._latent_args(p, a, sigma)
        B, Z, N, dev = p_.shape[0], p_.shape[1], x.shape[1], p_.device
        xb, xstride = self._x_arg(x.float())
        flags = self._det_flag() if deterministic is None else (_lib.ENF_FIT_DETERMINISTIC if deterministic else 0)
        desc, ws, st = self._call_ctx(B, N, Z, dev, masks=self._masks, size_query=kind.size_query)
        tgt = target.float().contiguous()
        w_ = weight.float().contiguous() if weight is not None else None
        cw_ = cweight.float().contiguous() if cweight is not None else None
        err = torch.empty((B, M), device=dev, dtype=torch.float32)
        loss_b = torch.empty((B,), device=dev, dtype=torch.float32) if per_signal else None
        fn, mid = kind.evaluate(lib, w_, cw_)
        _lib.launch(dev, fn, ctypes.byref(desc), _ptr(xb), xstride, _ptr(p_), _ptr(a_), _ptr(s_), _ptr(packed), _ptr(tgt), *mid,
                    _ptr(loss_out), _ptr(err), _ptr(loss_b), _ptr(ws), ws.numel(), flags, st)
        self._ws_touch(ws)
        return loss_b, err

    @torch.no_grad()
    def signal_losses(self, err):
        """loss_b (B,) = err.sum(1) / (N num_out) of per-point errors err (B, N), by the fixed-order sum enf_eval_loss itself runs
        (enf_signal_sum: one workgroup per signal, same inputs, same bits)."""
        if not err.is_cuda:
            raise _lib.EnfError("EquivariantCrossAttentionNeF.signal_losses needs CUDA/HIP tensors: there is no CPU path")
        e = err.float().contiguous()
        B, N = e.shape
        loss_b = torch.empty((B,), device=e.device, dtype=torch.float32)
        _lib.launch(e.device, _lib.load().enf_signal_sum, _ptr(e), B, N, 1.0 / (float(N) * float(self.num_out)), _ptr(loss_b),
                    _lib.stream(e.device))
        return loss_b

    # ------------------------------------------------------------------ observations that are not points: cells, sparse operators
    GROUP_SIZES = _Cells.GROUP_SIZES

    def _obs_args(self, what, kind, x, p, a, target, weight, cweight):
        """The one shape and refusal checker of the calls against cells and operators (_obs_calls.py: the kind), run before anything
        touches the device: never both weight forms, the fused decoder, the kind's own parameters, x (B, N, dx) against p and a, N
        against the kind, then target (B, M, O) -- None for a call that takes none (``gn_cell_product``) --, qweight (B, N), the
        weights (B, M) / (B, M, O), and the devices."""
        if weight is not None and cweight is not None:
            raise kind.both(what)
        if self.num_layers > 0:
            raise NotImplementedError(f"{what} is built for num_layers = 0 (the fused decoder)")
        if x.dim() != 3 or p.dim() != 3 or a.dim() != 3:
            raise ValueError("x, p and a must be (batch, ., .)")
        B, Z, N = p.shape[0], p.shape[1], x.shape[1]
        if x.shape[0] != B or a.shape[0] != B or a.shape[1] != Z:
            raise ValueError(f"x {tuple(x.shape)}, p {tuple(p.shape)} and a {tuple(a.shape)} disagree on the batch or the latents")
        M = kind.rows(N)
        kind.shapes(B, N, M, self.num_out, target, weight, cweight)
        if not (x.is_cuda and p.is_cuda and a.is_cuda and (target is None or target.is_cuda) and (kind.op is None or kind.op.val.is_cuda)):
            raise _lib.EnfError(f"EquivariantCrossAttentionNeF.{what} needs CUDA/HIP tensors: there is no CPU path")
        return M

    def _decode_loss(self, what, kind, out, target, weight, cweight):
        """``cell_mse`` / ``operator_mse``: the same checks on a decode out (B, N, O) in place of x, p and a, then the one Function."""
        if weight is not None and cweight is not None:
            raise kind.both(what)
        if out.dim() != 3:
            raise ValueError(f"out must be (B, N, O), got {tuple(out.shape)}")
        B, N, O = out.shape
        kind.shapes(B, N, kind.rows(N), O, target, weight, cweight)
        if not (out.is_cuda and target.is_cuda and (kind.op is None or kind.op.val.is_cuda)):
            raise _lib.EnfError(f"EquivariantCrossAttentionNeF.{what} needs CUDA/HIP tensors: there is no CPU path")
        return _ObsMseFunction.apply(out, target, kind, weight, cweight, self._det_flag())

    @torch.no_grad()
    def mse_value_and_cell_grads(self, params, x, p, a, gaussian_window_size, target, group, qweight=None, obs_weight=None,
                                 grad_scale=1.0, loss_out=None, return_errors=False, shared_latents=False, obs_channel_weight=None):
        """The fit step against GROUPED observations (include/enf_hip.h, "Grouped observations": enf_fit_step_g): observation m of a
        signal is obs[m] = sum_k qweight[m group + k] out[m group + k] over the ``group`` consecutive query rows it owns -- a quadrature
        rule over a cell (fitting/cells.py: cell_quadrature) -- and
            loss = sum_{b,m} obs_weight[b,m] sum_o (obs - target)^2 / (B M O),        target (B, M, O), M = N / group.
        ``group``: 1, 2, 4, 8 or 16.  ``qweight``: (B, N) finite factors, or None for 1 / group (the plain mean); ``obs_weight``: (B, M),
        finite and >= 0, or None for 1 -- an observation of weight 0 does not exist, its target may be NaN.  Nothing is normalised.
        The group sum, the loss and d out are formed in the fused tail's registers: no ``out`` in memory, no autograd graph.
        ``loss_out``: an already ZEROED float32 (1,) tensor the loss is added to.  ``return_errors``: also err_g (B, M) =
        obs_weight sum_o (obs - target)^2 and loss_b (B,) = err_g.sum(1) / (M O).
        ``shared_latents``: the caller's statement that every signal holds the same latents, that ``x`` is one set of cells expanded
        over the signals with stride 0 and that the rows of ``qweight`` are equal -- the first inner step of a fit on shared cells.  The
        call then goes to enf_fit_step_gs with ENF_FIT_SHARED_LATENTS: one forward for all signals and, where the library's rule holds,
        one backward.  Without it the call is enf_fit_step_g, as before.
        ``obs_channel_weight``: (B, M, O), finite and >= 0, one weight per observed VALUE in place of ``obs_weight`` (both: ValueError)
        -- loss = sum_{b,m,o} cw (obs - target)^2 / (B M O), err_g = sum_o cw (obs - target)^2, the zero-weight rule per value
        (enf_fit_step_gc).  With ``shared_latents`` it is NotImplementedError.
        Returns (loss (1,), dp, da, dwindow or None), with ``return_errors`` followed by (err_g, loss_b)."""
        if shared_latents and obs_channel_weight is not None:
            raise NotImplementedError("mse_value_and_cell_grads: shared_latents with obs_channel_weight is not built; run the step unshared")
        kind = _Cells(group, qweight)
        M = self._obs_args("mse_value_and_cell_grads", kind, x, p, a, target, obs_weight, obs_channel_weight)
        return self._fit_step(kind, M, params, x, p, a, gaussian_window_size, target, obs_weight, obs_channel_weight, grad_scale, loss_out,
                              return_errors, shared_latents)

    @torch.no_grad()
    def eval_cell_loss(self, params, x, p, a, gaussian_window_size, target, group, qweight=None, obs_weight=None, loss_out=None,
                       per_signal=True, obs_channel_weight=None):
        """Evaluation against grouped observations without a decode (include/enf_hip.h: enf_eval_loss_g): err_g (B, M) and loss_b (B,)
        as mse_value_and_cell_grads(return_errors=True) gives them at the same point -- the same bits, in every mode.  ``loss_out``: an
        already ZEROED float32 (1,) tensor; the scalar loss is added to it.  ``per_signal`` False skips loss_b.
        ``obs_channel_weight``: (B, M, O) in place of ``obs_weight``, as in mse_value_and_cell_grads (enf_eval_loss_gc).
        Returns (loss_b or None, err_g)."""
        kind = _Cells(group, qweight)
        M = self._obs_args("eval_cell_loss", kind, x, p, a, target, obs_weight, obs_channel_weight)
        return self._eval(kind, M, params, x, p, a, gaussian_window_size, target, obs_weight, obs_channel_weight, loss_out, per_signal)

    @torch.no_grad()
    def gn_cell_product(self, params, x, p, a, gaussian_window_size, group, qweight=None, obs_weight=None, vp=None, va=None,
                        vwindow=None, grad_scale=1.0, reuse=None):
        """The Gauss-Newton matrix of a latent fit on GROUPED observations applied to a direction, in one native call
        (include/enf_hip.h: enf_gn_product_g):
            (gp, ga, gwindow or None) = grad_scale * 2 / (B M O) * sum_m Jg^T w Jg (vp, va, vwindow),    Jg = sum_k qweight J
        with J = d out / d (p, a, window), the sum over the ``group`` consecutive rows of observation m, and w = ``obs_weight`` -- the
        observation model of ``mse_value_and_cell_grads``, whose ``grad_scale`` makes this the Gauss-Newton Hessian of that step's loss
        in the units of its gradient.  ``group``, ``qweight`` (B, N) or None for 1 / group, ``obs_weight`` (B, M) or None for 1 as
        there: an observation of weight 0 does not exist.  ``vp`` / ``va`` / ``vwindow`` and ``reuse`` as in ``gn_product``; the tag
        may also come from right behind ``mse_value_and_cell_grads`` (not ``shared_latents``) or an earlier ``gn_cell_product`` at the
        same point.  The group sum of the tangent and d out are formed in the tail's registers.  Size the buffer first: ``gn_reserve``."""
        tangents = (("vp", vp), ("va", va), ("vwindow", vwindow))
        self._tangent_refusals("gn_cell_product", tangents)
        kind = _Cells(group, qweight)
        self._obs_args("gn_cell_product", kind, x, p, a, None, obs_weight, None)
        latents = self._tangent_args("gn_cell_product", x, p, a, gaussian_window_size, tangents)
        return self._gn_call(kind, params, x.shape[1], latents, (vp, va, vwindow), obs_weight, None, grad_scale, reuse)

    def cell_fit_loss(self, params, x, p, a, gaussian_window_size, target, group, qweight=None, obs_weight=None, obs_channel_weight=None):
        """The grouped loss of the decode of latents as a function of the LATENTS, without a decode in memory and with the decoder's
        weights frozen: a torch.autograd.Function around mse_value_and_cell_grads.  The forward makes one enf_fit_step_g / _gc call
        (loss and d loss / d (p, a, window) at grad_scale 1); the backward multiplies the stored gradients by the incoming scalar.
        Differentiable once, with respect to ``p``, ``a`` and ``gaussian_window_size`` only -- ``params`` get no gradient (take
        apply + cell_mse where they need one).  Arguments as mse_value_and_cell_grads.  Returns the loss, a 0-d tensor."""
        self._obs_args("cell_fit_loss", _Cells(group, qweight), x, p, a, target, obs_weight, obs_channel_weight)
        if self.use_gaussian_window and gaussian_window_size is None:
            raise AssertionError("gaussian_window_size is required when use_gaussian_window=True")
        win = gaussian_window_size if self.use_gaussian_window else None
        return _CellFitLossFunction.apply(self, params, x, p, a, win, target, int(group), qweight, obs_weight, obs_channel_weight)

    def cell_mse(self, out, target, group, qweight=None, obs_weight=None, obs_channel_weight=None):
        """The grouped loss of a decode that exists in memory (include/enf_hip.h: enf_mse_value_grad_g), for the weight-gradient path:
            loss = sum_{b,m} obs_weight[b,m] sum_o (obs - target)^2 / (B M O),    obs[b,m] = sum_k qweight[b, m group + k] out[b, m group + k]
        with out (B, N, O), target (B, M, O), M = N / group; ``qweight`` (B, N) or None for 1 / group, ``obs_weight`` (B, M) or None for 1
        (an observation of weight 0 does not exist, its target may be NaN).  A torch.autograd.Function: loss and d out come from ONE
        kernel, the backward multiplies d out by the incoming scalar.  Differentiable once, and only with respect to ``out``.
        ``obs_channel_weight``: (B, M, O) in place of ``obs_weight`` (both: ValueError), one weight per observed value
        (enf_mse_value_grad_gc): loss = sum_{b,m,o} cw (obs - target)^2 / (B M O).
        Returns the loss, a 0-d tensor."""
        return self._decode_loss("cell_mse", _Cells(group, qweight), out, target, obs_weight, obs_channel_weight)

    @torch.no_grad()
    def mse_value_and_operator_grads(self, params, x, p, a, gaussian_window_size, target, op, obs_weight=None, obs_channel_weight=None,
                                     grad_scale=1.0, loss_out=None, return_errors=False, deterministic=None):
        """The fit step against observations obs = A out of a sparse linear operator ``op`` (fitting/operators.py: SparseObservations;
        include/enf_hip.h, "Sparse linear observations": enf_fit_step_a), shared by the signals:
            loss = sum_{b,m,o} w (obs - target)^2 / (B M O),        target (B, M, O), M = op.M, x (B, N, dx), N = op.N.
        ``obs_weight`` (B, M) or ``obs_channel_weight`` (B, M, O), finite and >= 0, or neither for 1 -- a weight of 0 is a select, the
        target under it may be NaN.  The decode exists only in the call's workspace; the pair and tail kernels are the point fit's.
        ``loss_out``: an already ZEROED float32 (1,) tensor the loss is added to.  ``return_errors``: also err_a (B, M) and loss_b (B,).
        ``deterministic``: None for the model's mode, or True / False for this call.
        Returns (loss (1,), dp, da, dwindow or None), with ``return_errors`` followed by (err_a, loss_b)."""
        kind = _Operator(op)
        M = self._obs_args("mse_value_and_operator_grads", kind, x, p, a, target, obs_weight, obs_channel_weight)
        return self._fit_step(kind, M, params, x, p, a, gaussian_window_size, target, obs_weight, obs_channel_weight, grad_scale, loss_out,
                              return_errors, deterministic=deterministic)

    @torch.no_grad()
    def eval_operator_loss(self, params, x, p, a, gaussian_window_size, target, op, obs_weight=None, obs_channel_weight=None,
                           loss_out=None, per_signal=True, deterministic=None):
        """Evaluation against an operator's observations without returning a decode (include/enf_hip.h: enf_eval_loss_a): err_a (B, M)
        and loss_b (B,) as mse_value_and_operator_grads(return_errors=True) gives them at the same point -- the same bits, in every mode.
        ``loss_out``: an already ZEROED float32 (1,) tensor; the scalar loss is added to it.  ``per_signal`` False skips loss_b.
        Returns (loss_b or None, err_a)."""
        kind = _Operator(op)
        M = self._obs_args("eval_operator_loss", kind, x, p, a, target, obs_weight, obs_channel_weight)
        return self._eval(kind, M, params, x, p, a, gaussian_window_size, target, obs_weight, obs_channel_weight, loss_out, per_signal,
                          deterministic)

    @torch.no_grad()
    def gn_operator_product(self, params, x, p, a, gaussian_window_size, op, obs_weight=None, obs_channel_weight=None, vp=None, va=None,
                            vwindow=None, grad_scale=1.0, reuse=None):
        """The Gauss-Newton matrix of a latent fit against a sparse operator's observations applied to a direction, in one native call
        (include/enf_hip.h: enf_gn_product_a):
            (gp, ga, gwindow or None) = grad_scale * 2 / (B M O) * J^T A^T W A J (vp, va, vwindow),    J = d out / d (p, a, window)
        with A = ``op`` and W = ``obs_weight`` (B, M), ``obs_channel_weight`` (B, M, O) or 1 -- the observation model of
        ``mse_value_and_operator_grads``, whose ``grad_scale`` makes this the Gauss-Newton Hessian of that step's loss in the units of
        its gradient; what has weight 0 does not exist.  ``vp`` / ``va`` / ``vwindow`` and ``reuse`` as in ``gn_product``; the tag may
        also come from right behind ``mse_value_and_operator_grads`` or an earlier ``gn_operator_product`` at the same point.  The
        tangent of the decode, the weighted observations' tangent and d out exist only in the call's workspace.  Size the buffer
        first: ``gn_reserve(..., op=op)``."""
        tangents = (("vp", vp), ("va", va), ("vwindow", vwindow))
        self._tangent_refusals("gn_operator_product", tangents)
        kind = _Operator(op)
        self._obs_args("gn_operator_product", kind, x, p, a, None, obs_weight, obs_channel_weight)
        latents = self._tangent_args("gn_operator_product", x, p, a, gaussian_window_size, tangents)
        return self._gn_call(kind, params, x.shape[1], latents, (vp, va, vwindow), obs_weight, obs_channel_weight, grad_scale, reuse)

    def operator_mse(self, out, target, op, obs_weight=None, obs_channel_weight=None):
        """The loss of a decode that exists in memory against an operator's observations (include/enf_hip.h: enf_mse_value_grad_a), for
        the weight-gradient path: loss = sum_{b,m,o} w (A out - target)^2 / (B M O) with out (B, N, O), target (B, M, O).  A
        torch.autograd.Function as cell_mse: loss and d out come from the two kernels of csrc/enf_obs.hip, the backward multiplies d out
        by the incoming scalar; differentiable once, with respect to ``out`` only.  Returns the loss, a 0-d tensor."""
        return self._decode_loss("operator_mse", _Operator(op), out, target, obs_weight, obs_channel_weight)


class _ObsMseFunction(torch.autograd.Function):
    """nef.cell_mse / nef.operator_mse: the kind's enf_mse_value_grad_* call once in the forward (loss and d out at grad_scale 1); the
    backward scales the stored d out."""

    @staticmethod
    def forward(ctx, out, target, kind, weight, cweight, det):
        lib = _lib.load()
        dev = out.device
        o_, t_, w_, c_ = _f32(out), _f32(target), _f32(weight), _f32(cweight)
        B, N, O = o_.shape
        need = ctx.needs_input_grad[0]
        dout = torch.empty_like(o_) if need else None
        loss = torch.zeros(1, device=dev, dtype=torch.float32)
        fn, nscr, mid = kind.mse(lib, B, N, O, w_, c_, need, det)
        scr = torch.empty(nscr, device=dev, dtype=torch.uint8) if nscr else None
        _lib.launch(dev, fn, _ptr(o_), _ptr(t_), B, N, O, *mid, 1.0, _ptr(dout), _ptr(loss), None, _ptr(scr), nscr, det, _lib.stream(dev))
        if need:
            ctx.save_for_backward(dout)
        ctx.out_dtype = out.dtype
        return loss.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (dout,) = ctx.saved_tensors
        return (dout * g).to(ctx.out_dtype), None, None, None, None, None


class _CellFitLossFunction(torch.autograd.Function):
    """nef.cell_fit_loss: one mse_value_and_cell_grads in the forward; the backward scales its dp, da, dwindow."""

    @staticmethod
    def forward(ctx, nef, params, x, p, a, window, target, group, qweight, obs_weight, obs_channel_weight):
        det = lambda t: t.detach() if t is not None else None
        loss, dp, da, dsig = nef.mse_value_and_cell_grads(params, x.detach(), p.detach(), a.detach(), det(window), target.detach(), group,
                                                          qweight=det(qweight), obs_weight=det(obs_weight),
                                                          obs_channel_weight=det(obs_channel_weight))
        ctx.save_for_backward(dp, da, dsig if dsig is not None else dp.new_zeros(()))
        ctx.has_window = dsig is not None
        ctx.shapes = (p.shape, a.shape, None if window is None else window.shape)
        ctx.dtypes = (p.dtype, a.dtype, None if window is None else window.dtype)
        return loss.reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        dp, da, dsig = ctx.saved_tensors
        gp = (dp * g).reshape(ctx.shapes[0]).to(ctx.dtypes[0]) if ctx.needs_input_grad[3] else None
        ga = (da * g).reshape(ctx.shapes[1]).to(ctx.dtypes[1]) if ctx.needs_input_grad[4] else None
        gw = (dsig * g).reshape(ctx.shapes[2]).to(ctx.dtypes[2]) if ctx.has_window and ctx.needs_input_grad[5] else None
        return None, None, None, gp, ga, gw, None, None, None, None, None
