/* enf_hip.h -- C-ABI of the MI355X (gfx950) Equivariant-Neural-Field decoder.
 *
 * The reference (david-knigge/enf-pde) exposes this path as a Flax module, not an FFI:
 *   nef.apply(params, x, p, a, gaussian_window)            enf/models/equivariant_cross_attention_nef.py:204-235
 *   jax.grad(loss)(latents)   (MAML inner step)            experiments/fitting/trainers/pde_trainer.py:175-200
 * The entry points below are what a binding for that module would bind: one
 * forward, one backward-to-latents, weight packing, and size queries.  Plain pointers and
 * sizes only; every buffer is owned by the caller and lives in device (HBM) memory; nothing
 * is allocated, freed or synchronised inside the library; all work is enqueued on `stream`
 * (a hipStream_t passed as void*; the calling thread's current device must be the stream's).  Functions return 0 or a
 * negative ENF_E* code.  The library keeps no settings: a call depends on its arguments only, calls on different
 * (workspace, stream) pairs are independent and may come from different host threads, models and devices.  A workspace
 * is scratch of ONE call sequence at a time (the REUSE flags below tie a backward to the forward before it).
 *
 * Layouts (all fp32, C-contiguous, batch first):
 *   x      (B, N, dx)   query coordinates; x_bstride = element stride between signals
 *                       (0 = one grid broadcast over B, pde_trainer.py:197,393)
 *   p      (B, Z, dp)   latent poses  (dp = z_pos + z_ori; ponita carries the raw angle,
 *                       the cos/sin embed of NEF:214-217 happens inside)
 *   a      (B, Z, C)    latent context codes
 *   sigma  (B, Z, 1)    gaussian window size per latent
 *   out    (B, N, O)
 */
#ifndef ENF_HIP_H
#define ENF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ENF_ABI_VERSION 2

/* cross-attention invariants: enf/steerable_attention/invariant/__init__.py:47-78 */
enum {
  ENF_INV_REL_POS_PERIODIC = 0,  /* rel_pos_periodic.py:35-60,  window _base_invariant.py:35-43 */
  ENF_INV_LATITUDE_PERIODIC = 1, /* spherical_longitude.py:57-85, window :34-55                  */
  ENF_INV_POLAR_PERIODIC = 2,    /* polar_periodic.py:40-68,    window :35-38                    */
  ENF_INV_PONITA = 3,            /* ponita.py:20-44 (PonitaPos2D), window _base_invariant.py:25-33 */
  ENF_INV_ABS_POS = 4,           /* abs_pos.py:42                                                */
  ENF_INV_REL_POS = 5,           /* rel_pos.py:41                                                */
  ENF_INV_NORM_REL_POS = 6,      /* norm_rel_pos.py:34                                           */
  ENF_INV_BALL = 7,              /* ball.py:54-96: [R(alpha,beta,gamma) x^, r_x, r_p], window :36-52 (64-wide kernels only) */
  ENF_INV_BALL_LAT = 8,          /* ball_lat.py:54-88: [th_x, th_p, cos dphi, sin dphi, r_x, r_p]                              */
  ENF_INV_PONITA_FULL = 9,       /* ponita.py:48-92 (Ponita2D): both sides carry an orientation, x = (pos_x, pos_y, theta_x), dx = 3:
                                    [ponita's two, cos(theta_x - theta_p)]; the self-attention invariant of `ponita` (INV/__init__.py:30-32) */
  ENF_INV_COUNT = 10
};

/* arithmetic of the per-pair contractions */
enum {
  ENF_PREC_F32 = 0,  /* v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulate (parity mode) */
  ENF_PREC_BF16 = 1  /* v_mfma_f32_16x16x32_bf16: bf16 operands, fp32 accumulate (throughput mode) */
};

/* pair-kernel variant of a call: latent-split / unfolded, or z-fold (per-latent folded matrices) */
enum {
  ENF_VARIANT_AUTO = 0,          /* by problem size */
  ENF_VARIANT_LATENT_SPLIT = 1,  /* forward: the 8 waves split Z; backward: one wave = one latent */
  ENF_VARIANT_ZFOLD = 2,         /* forward: >= 192 workgroups of 128 queries; backward: >= 192 latents */
  ENF_VARIANT_ZFOLD_ZSPLIT = 3   /* forward only: the z-fold kernel over equal runs of latent steps -- the (signal, 128-query tile, latent) space
                                    cut into <= 256 runs, one workgroup each, a tile's partial softmax sums merged by a small kernel
                                    (enf_pair_partition).  AUTO picks it when fewer than 192 tiles exist and Z >= 128 -- e.g. 128 latents on
                                    a 96 x 48 sphere grid, 4 signals: 144 tiles -> 256 runs of 72.  In this variant the last bits of a
                                    query's value depend on the call's shape (the run boundaries order the partial sums) */
};

/* invariant embedding (reference enf/steerable_attention/embedding/__init__.py:25-33), EnfDesc.embedding.
 * ENF_EMB_FFN is Dense(I -> D) -> gelu -> Dense(D -> D) (embedding/linear.py, FFNEmbedding; flax Dense, tanh gelu).  It reuses
 * the weight slots of the rff embedding of both branches (R? = RQ / RV):
 *   ENF_W_R?_COEF  Dense_0.kernel (I, D)      ENF_W_R?_B1  Dense_0.bias (D)
 *   ENF_W_R?_W2    Dense_1.kernel (D, D)      ENF_W_R?_B2  Dense_1.bias (D)   (the role of rff's linear_final)
 *   ENF_W_R?_W1    unused: NULL is accepted; enf_backward_all writes exact zeros to its gradient if a buffer is given.
 * ffn is built for the non-ball invariants; the relu-mask modes are accepted and do nothing (the chain has no relu).
 * enf_backward_all gives every weight gradient (d Dense_0 in the R?_COEF slots) and the query gradient; with a store,
 * enf_pair_backward_ex writes ENF_S_EQ / ENF_S_EV as the invariant in features 0..3 (zeros elsewhere) and ENF_S_DA1 / DA2 as
 * d of the Dense_0 pre-activation.  The composed path of the ENF_P_* tensors (enf_pack_pair, enf_backward_weights) returns
 * ENF_EUNSUPPORTED for ffn. */
enum {
  ENF_EMB_RFF = 0,
  ENF_EMB_FFN = 1
};

/* relu masks of a call (see "Relu masks" below) */
#define ENF_MASK_OFF 0
#define ENF_MASK_WRITE 1
#define ENF_MASK_READ 2

enum {
  ENF_OK = 0,
  ENF_EINVAL = -1,       /* NULL pointer / non-positive size */
  ENF_EINVARIANT = -2,   /* unknown invariant id (reference: ValueError, invariant/__init__.py:78) */
  ENF_EUNSUPPORTED = -3, /* shape outside the compiled kernel set (D in {64,128}; H in {1,2}, 4 at D = 64; O <= 32) */
  ENF_EWORKSPACE = -4,   /* workspace too small */
  ENF_ELAUNCH = -5,      /* HIP launch error */
  ENF_EDIM = -6          /* dx / dp inconsistent with the invariant (reference asserts, :62,65) */
};

typedef struct EnfDesc {
  int32_t B, N, Z;       /* signals, queries per signal, latents per signal */
  int32_t H, D, C, O;    /* num_heads, num_hidden, latent_dim, num_out (NEF:85-89) */
  int32_t dx;            /* coordinate width (cfg.nef.num_in) */
  int32_t invariant_id;  /* ENF_INV_* */
  int32_t use_window;    /* use_gaussian_window (NEF:96) */
  int32_t precision;     /* ENF_PREC_* */
  int32_t h_true;       /* 0, or the model's num_heads when H is padded with all-zero heads (num_heads = 3 runs as H = 4):
                           only the block FFN's LayerNorm, which normalises over num_heads * num_hidden, needs it */
  int32_t d_true;       /* 0, or the model's num_hidden when D is a zero-padded width (d_true < D): LayerNorm statistics and
                           the D^-1/2 logit scale use d_true; the caller pads every weight tensor with zeros (see
                           enf-pde_amd/enf/models/_pad.py).  Lets num_hidden 16 / 32 (config_diff_sphere.yaml) run on the D = 64 kernels */
  /* ---- per-call options.  Everything a call depends on is in its arguments: the library keeps no mutable settings. */
  int32_t pair_fwd_variant; /* ENF_VARIANT_*: forward pair kernel.  enf_workspace_bytes / enf_pair_scratch_bytes depend on it */
  int32_t pair_bwd_variant; /* ENF_VARIANT_*: backward pair kernel (the weight-gradient path always runs the unfolded one) */
  int32_t mask_mode;        /* ENF_MASK_*: what the pair kernels of THIS call do with `relu_masks` */
  int32_t mask_signals;     /* signals b, b + mask_signals, ... share the masks of signal b % mask_signals (0 = B) */
  int32_t embedding;        /* ENF_EMB_*: invariant embedding of both branches (a zeroed descriptor is rff) */
  void* relu_masks;         /* enf_relu_mask_bytes(d) bytes of device memory, or NULL with ENF_MASK_OFF */
} EnfDesc;

/* Weight tensors in the order `enf_pack_weights` expects them; names are the Flax tree of
 * EquivariantCrossAttentionNeF (SURVEY.md 8a "Weights"); kernels are (in, out), y = x@W + b. */
enum {
  ENF_W_STEM_W = 0, ENF_W_STEM_B,                 /* latent_stem                       NEF:134 */
  ENF_W_LNA_G, ENF_W_LNA_B,                       /* cross_attention_blocks_0/layer_norm_attn NEF:29 */
  ENF_W_RQ_COEF, ENF_W_RQ_W1, ENF_W_RQ_B1, ENF_W_RQ_W2, ENF_W_RQ_B2,  /* attn/invariant_embedding_query RFF:21-40 */
  ENF_W_RV_COEF, ENF_W_RV_W1, ENF_W_RV_B1, ENF_W_RV_W2, ENF_W_RV_B2,  /* attn/invariant_embedding_value */
  ENF_W_Q_W, ENF_W_Q_B,                           /* attn/inv_emb_to_q                 ECA:54 */
  ENF_W_K_W, ENF_W_K_B,                           /* attn/a_to_k                       ECA:55 */
  ENF_W_V_W, ENF_W_V_B,                           /* attn/a_to_v                       ECA:56 */
  ENF_W_F1_W0, ENF_W_F1_B0, ENF_W_F1_G, ENF_W_F1_BE, ENF_W_F1_W1, ENF_W_F1_B1,  /* attn/inv_emb_to_v  ECA:65 */
  ENF_W_MX_W0, ENF_W_MX_B0, ENF_W_MX_G, ENF_W_MX_BE, ENF_W_MX_W1, ENF_W_MX_B1,  /* attn/inv_emb_cond_mixer ECA:66 */
  ENF_W_AO_W, ENF_W_AO_B,                         /* attn/out_proj                     ECA:72 */
  ENF_W_FF_W0, ENF_W_FF_B0, ENF_W_FF_G, ENF_W_FF_BE, ENF_W_FF_W1, ENF_W_FF_B1,  /* pointwise_ffn     NEF:40-42 */
  ENF_W_O0_W, ENF_W_O0_B, ENF_W_O2_W, ENF_W_O2_B, ENF_W_O4_W, ENF_W_O4_B,       /* out_proj layers_0/2/4 NEF:196-202 */
  ENF_NUM_TENSORS
};

int enf_abi_version(void);
const char* enf_strerror(int code);

/* invariant metadata (mirrors BaseInvariant.dim / num_z_pos_dims / num_z_ori_dims, _base_invariant.py:7-23) */
int enf_invariant_dim(int invariant_id, int dx);        /* I, or ENF_EINVARIANT */
int enf_invariant_pose_dim(int invariant_id, int dx);   /* dp = z_pos + z_ori    */

/* validate a descriptor against the compiled kernel set */
int enf_check_desc(const EnfDesc* d);

/* bytes of the packed weight blob (MFMA-fragment-ordered panels + folded matrices) */
size_t enf_packed_weight_bytes(const EnfDesc* d);
/* Build the packed blob from ENF_NUM_TENSORS device pointers (fp32).  Runs the exact
 * algebraic folds of DESIGN.md ("folds") in fp32 on the device.  `tensors` is a host array. */
int enf_pack_weights(const EnfDesc* d, const float* const* tensors, void* packed, void* stream);

/* scratch the forward / backward need (latent table, per-query partials) */
size_t enf_workspace_bytes(const EnfDesc* d);
/* The same for a call that carries `flags`: 0 gives enf_workspace_bytes(d); ENF_BWD_DETERMINISTIC (= ENF_FIT_DETERMINISTIC, see
 * "Deterministic mode" below) adds the partial-sum buffers of enf_backward_latents_ex / enf_fit_step_ex (equal to the plain size
 * plus one gradient table where the backward pair kernel does not split the queries).  ENF_BWD_QUERY_GRAD is accepted so that one
 * flag word serves every size query; it adds nothing here (the query gradient's partials come from enf_backward_all's / enf_pair_backward_ex2's
 * scratch).  0 for a bad descriptor or an unknown flag bit. */
size_t enf_workspace_bytes_ex(const EnfDesc* d, unsigned flags);

/* Replaces nef.apply (NEF:204-235).  `ybar` (B,N,H*D) and `lse` (B,N,H) are optional
 * outputs (may be NULL): the attention-weighted value sum and the softmax log-sum-exp,
 * which enf_backward_latents takes back instead of recomputing the forward. */
int enf_forward(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a,
                const float* sigma, const void* packed, float* out, float* ybar, float* lse,
                void* workspace, size_t workspace_bytes, void* stream);

/* Measurement hook: the same call as enf_forward, restricted to a subset of its kernels so that ONE
 * kernel can be bracketed by events on `stream` (bench.py's roofline leg, rocprofv3 cross-check).
 * stages: bit 0 = latent prologue (K1), bit 1 = pair kernel (K2), bit 2 = tail.  The latent table
 * lives in `workspace` between calls, so run bit 0 once before timing bit 1. */
#define ENF_STAGE_PROLOGUE 1u
#define ENF_STAGE_PAIR 2u
#define ENF_STAGE_TAIL 4u
#define ENF_STAGE_FOLD 8u      /* enf_wz_kernel: per-latent folded matrices of the z-fold pair variant (no-op otherwise);
                                  runs between PROLOGUE and PAIR, PAIR alone reuses what the workspace holds */
#define ENF_STAGE_TAIL_SAVE 16u /* with ENF_STAGE_TAIL: stash the tail's pre-activations in the workspace; the backward
                                  that follows on the untouched workspace (ENF_BWD_REUSE_TAIL) then skips their recompute */
#define ENF_STAGE_PREPARE_BWD 32u /* a backward on the same inputs and WORKSPACE follows: what it needs from the latent table
                                  alone (its per-latent folded matrices, the zeroed gradient table) starts on the device's
                                  side stream behind the pair kernel; pass ENF_BWD_REUSE_PREPARED to that backward.  The
                                  pending work is recorded against this workspace: any later call on the same workspace
                                  joins it first, a call on another workspace neither sees nor consumes it */
#define ENF_STAGE_YBAR_HALF 64u /* with ENF_STAGE_PAIR | ENF_STAGE_TAIL in ONE call, bf16 mode, `ybar` == NULL: nothing after this call reads
                                   its `ybar` (a decode: no backward follows), so the pair kernel may hand it to the tail as bf16 in the
                                   workspace -- half the bytes of the largest tensor of a forward; the tail rounds `ybar` to bf16 for its
                                   first matrix product anyway, so `out` is the same bit for bit.  Ignored where it does not apply
                                   (f32 mode, ENF_STAGE_TAIL_SAVE, the split z-fold variant, a caller-owned `ybar`, relu masks:
                                   EnfDesc.mask_mode != ENF_MASK_OFF -- masked passes are training passes, their pair kernels hand
                                   over fp32 rows only). */
#define ENF_STAGE_SHARED_LATENTS 128u /* the forward's form of ENF_FIT_SHARED_LATENTS (below), same statement and same rules: with
                                   ENF_STAGE_PAIR the pair kernel may compute signal 0 alone and write its `ybar` / `lse` rows to every
                                   signal; B > 1 with x_bstride != 0 is ENF_EINVAL.  Where ENF_STAGE_YBAR_HALF applies in the same
                                   call, that hand-off runs instead.  The workspace's d ybar | delta region is overwritten. */
int enf_forward_stages(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a,
                       const float* sigma, const void* packed, float* out, float* ybar, float* lse,
                       void* workspace, size_t workspace_bytes, unsigned stages, void* stream);

/* Replaces jax.grad(loss)(latents) for one inner step (pde_trainer.py:188,200): given
 * dL/dout it returns dL/dp (B,Z,dp), dL/da (B,Z,C), dL/dsigma (B,Z,1).  Buffers are
 * overwritten, not accumulated.  `ybar`/`lse` come from enf_forward on the same inputs. */
int enf_backward_latents(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p,
                         const float* a, const float* sigma, const void* packed, const float* ybar,
                         const float* lse, const float* dout, float* dp, float* da, float* dsigma,
                         void* workspace, size_t workspace_bytes, void* stream);
/* flags: ENF_BWD_REUSE_PROLOGUE = the workspace still holds the latent table of the enf_forward call with the same
 * (p, a, sigma, weights) -- nothing else has used it since -- so the prologue is not recomputed. */
#define ENF_BWD_REUSE_PROLOGUE 1u
/* ENF_BWD_REUSE_TAIL (with ENF_BWD_REUSE_PROLOGUE): that forward also ran with ENF_STAGE_TAIL_SAVE: the tail backward
 * reads the stashed pre-activations instead of recomputing the tail's forward chain (half of its GEMM stages). */
#define ENF_BWD_REUSE_TAIL 2u
/* ENF_BWD_REUSE_PREPARED (with ENF_BWD_REUSE_PROLOGUE): that forward ran with ENF_STAGE_PREPARE_BWD: join its side-stream
 * work instead of repeating it (ignored when nothing is pending). */
#define ENF_BWD_REUSE_PREPARED 4u
/* ENF_BWD_ONLY_PAIR: measurement hook, the backward counterpart of enf_forward_stages(ENF_STAGE_PAIR): re-run ONLY the
 * backward pair kernel (preceded by the zero-fill of the 2 MB gradient table it accumulates into) on the workspace a
 * complete enf_backward_latents[_ex] call with the same arguments has just left; dp / da / dsigma are not written. */
#define ENF_BWD_ONLY_PAIR 8u
/* Deterministic mode.  By default the backward pair kernel adds its shares of a latent-table gradient row -- one per query split,
 * `nsplit` = 1, 2, 4, ... of them, until every compute unit has a workgroup -- and, for the query gradient, one share per latent,
 * with float atomics, and the loss kernels add one partial per wave / block the same way: the sums' order, and so their last
 * bits, follow the order in which workgroups finish.  With ENF_BWD_DETERMINISTIC (enf_backward_latents_ex, enf_backward_all,
 * enf_pair_backward_ex2), ENF_FIT_DETERMINISTIC (enf_fit_step_ex) or ENF_MSE_DETERMINISTIC (enf_mse_value_grad_ex) the same
 * kernels STORE those shares in scratch and a second pass adds them in index order: no float atomic runs, and the results are the
 * same bits for the same inputs, the same shape, the same resolved kernel variants and the same build of the library, whatever
 * the workspace's address, size or previous contents.  What is NOT promised: equal bits between the deterministic and the default
 * path (another summation order), across shapes (the split z-fold forward orders its partial sums by the call's shape; nsplit
 * follows B, Z, N) or across library builds.  The default path is unchanged: same kernels, same workspace sizes.  Cost: one or two
 * small kernels per call and the partial buffers, nsplit x B Z gradient rows (DESIGN.md 7 has the measured times).
 * A deterministic call needs enf_workspace_bytes_ex(d, flags) bytes of workspace (ENF_EWORKSPACE otherwise); flag bits an entry
 * point does not know are ENF_EINVAL. */
#define ENF_BWD_DETERMINISTIC 16u
#define ENF_BWD_QUERY_GRAD 32u     /* size queries only: a query gradient (`dx`) will be asked for */
int enf_backward_latents_ex(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p,
                         const float* a, const float* sigma, const void* packed, const float* ybar,
                         const float* lse, const float* dout, float* dp, float* da, float* dsigma,
                         void* workspace, size_t workspace_bytes, unsigned flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training path: gradients w.r.t. the network weights (value_and_grad over params['nef'],
 * pde_trainer.py:255; nonmaml_pde_trainer.py:304-339).  The per-pair chain (97 % of the FLOPs)
 * stays in HIP -- enf_pair_forward for the values, enf_backward_weights for d lt and the gradients of the ENF_P_* tensors --;
 * folds, latent prologue and tail (per-latent / per-query work) are run by the host framework as differentiable ops around
 * them.
 *   latent table `lt` (B*Z rows, enf_lt_layout): [ u (H*D) | v0 (H*D) | pose (4) | wcoef | pad | c (H) | pad ]
 *     u, c   : att[n,z,h] = h1[n,z,:].u[z,h,:] + c[z,h]        (fold 1)
 *     v0     : a_to_v(a_norm)                                   (ECA:94)
 *     pose   : periodic/rel/abs/norm (p0,p1,p2,-); ponita (px,py,cos t,sin t); sphere (phi,theta,sin theta,cos theta)
 *     wcoef  : 1/sigma^2 (sphere: 1/(2 sigma^2))
 * ------------------------------------------------------------------------------------------- */
enum {   /* effective per-pair parameters, plain fp32, kernels (in, out) */
  ENF_P_AQ1 = 0, ENF_P_BQ1,   /* query RFFNet layers_0                         (D,D), (D)  */
  ENF_P_AV1, ENF_P_BV1,       /* value RFFNet layers_0                         (D,D), (D)  */
  ENF_P_AF, ENF_P_BF,         /* linear_final . inv_emb_to_v.Dense_0 (fold 2)  (D,D), (D)  */
  ENF_P_AGB, ENF_P_BGB,       /* diag(LN.scale) Dense_1, LN.bias Dense_1 + b; Flax column order [gamma (HD) | beta (HD)]  (D,2HD), (2HD) */
  ENF_P_AM, ENF_P_BM,         /* inv_emb_cond_mixer.Dense_0                    (D,D), (D)  */
  ENF_P_COEFQ, ENF_P_COEFV,   /* RFF coefficients                              (I, D/2)    */
  ENF_NUM_PAIR_TENSORS
};
/* Per-pair activations / deltas the backward can materialise (rows = (b*Z + z)*N + n, D columns,
 * bf16 in ENF_PREC_BF16 and fp32 in ENF_PREC_F32) so that every per-pair weight gradient is a plain
 * GEMM dW = X^T delta over the pair axis:   AQ1: EQ^T DA1   AV1: EV^T DA2   AF: G1^T DA3
 *   AGB[:, gamma_h|beta_h]: NH^T DG_h | NH^T DB_h     AM: sum_h V_h^T DA5_h    biases: column sums of delta */
enum { ENF_S_EQ = 0, ENF_S_EV, ENF_S_G1, ENF_S_NH, ENF_S_DA1, ENF_S_DA2, ENF_S_DA3, ENF_S_HEAD0 /* + 4h: V, DA5, DG, DB */ };
/* Column order of the stored rows.  ENF_PREC_F32: natural.  ENF_PREC_BF16: permuted inside every block of 32 columns --
 * stored column 32 b + 8 q + j (q < 4, j < 8) holds feature 32 b + 4 q + j for j < 4 and 32 b + 16 + 4 q + (j - 4)
 * otherwise (the MFMA operand fragments go out as they sit in registers, one 16-byte store each).  All buffers share the
 * permutation, so X^T delta comes out with rows and columns permuted alike: un-permute the D x D result. */
#define ENF_NUM_STORE(H) (7 + 4 * (H))

int enf_lt_layout(const EnfDesc* d, int* stride, int* off_u, int* off_v0, int* off_pose, int* off_wcoef, int* off_c);
/* ball / ball_lat only (invariant/ball.py, ball_lat.py): further fields of a latent-table row.
 *   ext (16 floats): [ R (9, row-major; ball.py:76-84) | the latent-only invariants (2) | pad ]; in the GRADIENT table the
 *                    backward returns d R and d(latent-only invariants) in the same slots
 *   phase_q, phase_v (D/2 each): coeff[latent-only rows]^T (latent-only invariants), the per-latent part of the RFF
 *                    pre-activation of the query / value RFFNet */
int enf_lt_layout_ext(const EnfDesc* d, int* off_ext, int* off_phase_q, int* off_phase_v);
int enf_pack_pair(const EnfDesc* d, const float* const* pair_tensors, void* packed, void* stream);
/* K2 alone: lt -> ybar (B,N,H*D), lse (B,N,H).  `scratch` (enf_pair_scratch_bytes; may be 0 -> NULL) holds the
 * per-latent folded matrices of the large-N forward variant. */
size_t enf_pair_scratch_bytes(const EnfDesc* d);
int enf_pair_forward(const EnfDesc* d, const float* x, int64_t x_bstride, const float* lt, const void* packed,
                     float* ybar, float* lse, void* scratch, size_t scratch_bytes, void* stream);
/* K3 alone: d ybar, delta[n,h] = d ybar . ybar, lse -> d lt (same layout as lt, overwritten);
 * `store` = NULL or ENF_NUM_STORE(H) device buffers of B*Z*N rows (see ENF_S_*). */
int enf_pair_backward(const EnfDesc* d, const float* x, int64_t x_bstride, const float* lt, const void* packed,
                      const float* lse, const float* dybar, const float* delta, float* dlt, void* const* store,
                      void* stream);
/* The same with the gradient w.r.t. the QUERY coordinates (jax.grad of nef.apply w.r.t. x; the self-attention blocks of
 * NEF:223-226 need it, their queries being the latent poses): `dx` (B,N,dx) fp32, ACCUMULATED into with float atomics
 * (zero it first), or NULL. */
int enf_pair_backward_ex(const EnfDesc* d, const float* x, int64_t x_bstride, const float* lt, const void* packed,
                         const float* lse, const float* dybar, const float* delta, float* dlt, void* const* store,
                         float* dx, void* stream);
/* The same with flags (0 = enf_pair_backward_ex).  ENF_BWD_DETERMINISTIC: `dlt` and `dx` are summed in a fixed order from partials
 * in `scratch` (enf_pair_backward_scratch_bytes(d, flags); pass ENF_BWD_QUERY_GRAD to the size query when `dx` is not NULL), and
 * `dx` is then OVERWRITTEN, not accumulated into. */
size_t enf_pair_backward_scratch_bytes(const EnfDesc* d, unsigned flags);
int enf_pair_backward_ex2(const EnfDesc* d, const float* x, int64_t x_bstride, const float* lt, const void* packed,
                          const float* lse, const float* dybar, const float* delta, float* dlt, void* const* store,
                          float* dx, void* scratch, size_t scratch_bytes, unsigned flags, void* stream);

/* Relu masks.  Second-order terms taken as finite differences of FIRST-order gradients (the outer MAML step,
 * pde_trainer.py:255) converge to the DISTRIBUTIONAL second derivative: relu units whose sign changes between the two
 * perturbed points add a finite amount that automatic differentiation (relu'' = 0) never includes (20 % on the RFFNet
 * layer-0 weights in the tests).  With EnfDesc.mask_mode = ENF_MASK_WRITE the pair-kernel forward of the call records, per
 * pair and relu layer (the two RFFNet layers), which pre-activations are positive, into EnfDesc.relu_masks; with
 * ENF_MASK_READ the pair-kernel forward of the call, and enf_pair_backward[_ex] / enf_backward_weights, use the relu
 * LINEARISED at those masks (h = a where the bit is set) instead of max(a, 0), for signals b, b + mask_signals, ...
 * alike.  One 32-bit word per lane, 16-query tile, latent and layer: enf_relu_mask_bytes(d) for the shape that WRITES
 * them (same N, Z; B = mask_signals). */
size_t enf_relu_mask_bytes(const EnfDesc* d);

/* One inner step of the MAML loop (pde_trainer.py:175-207) in ONE call: forward on (x, p, a, sigma), *loss += mean((out - target)^2)
 * (the caller zeroes *loss; target (B,N,O) fp32), and grad_scale * d loss / d(p, a, sigma) into dp / da / dsigma (OVERWRITTEN).
 * Equals enf_forward + enf_mse_value_grad + enf_backward_latents on the same arguments; the per-query tail runs once, as a single
 * kernel (forward chain, loss and its gradient in registers, backward chain), so neither `out` nor `d out` is materialised.
 * `workspace`: enf_workspace_bytes(d), contents need not be kept. */
int enf_fit_step(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                 const void* packed, const float* target, float grad_scale, float* loss, float* dp, float* da, float* dsigma,
                 void* workspace, size_t workspace_bytes, void* stream);
/* The same with flags (0 = enf_fit_step).  ENF_FIT_DETERMINISTIC: loss and gradients are summed in a fixed order (same inputs,
 * same bits; "Deterministic mode" above); `workspace`: enf_workspace_bytes_ex(d, ENF_FIT_DETERMINISTIC). */
#define ENF_FIT_DETERMINISTIC 16u
/* ENF_FIT_SHARED_LATENTS (enf_fit_step_ex / _w / _cw / _e): the caller's statement that rows b Z + z of `p`, `a` and `sigma` are equal
 * for all b and that all signals share their query points -- the first inner step of a fit, which starts every signal from the one
 * latent initialisation on one shared mask.  B > 1 with x_bstride != 0 contradicts it: ENF_EINVAL.  B == 1: no-op.  The flag is a
 * permission, not a command: where the forward resolves to the latent-split pair kernel and relu masks are off, that kernel then
 * runs ONCE, for signal 0, with its latents cut into P parts over all compute units (enf_shared_forward_parts), and a merge kernel
 * writes the row to all B signals' `ybar` / `lse`; elsewhere the ordinary sequence runs unchanged.  What differs from the call without
 * the flag is the fp32 order in which the partial sums over a query's latents are added; the B copies are the same bits.  The parts borrow
 * the workspace's d ybar | delta region: the workspace sizes do not change (enf_workspace_bytes_ex accepts the bit and ignores it).
 * The shared backward.  With equal latents and points every activation the backward pair kernel recomputes, and the tail's Jacobian,
 * are the same for all signals too, and d out -> d(latent table) is linear in d out.  With ONE output channel the whole backward of a
 * fit step is dlt[b, z, f] = sum_n dout[b, n] c[n, z, f], c = the per-pair contributions for d out = 1 at every query, and
 * dout[b, n] = 2 w[b, n] (out[n] - target[b, n]) grad_scale / (B N) is the only per-signal quantity.  Where ALL of the following hold
 * (enf_shared_backward_applies), behind the shared forward the step therefore also runs ONCE, on signal 0: the tail forward, one loss
 * kernel (that row of outputs against all B targets and weights, which also writes d out (B, N)), the unit-seeded tail backward, the
 * per-latent matrices of Z latents (not B Z), and ONE backward pass of the pair kernel over (N queries x Z latents) that contracts its
 * sums over queries with d out (fp32 matrix instructions: fp32 sums) and adds the result to all B Z gradient rows:
 *     the shared forward runs;  O == 1;  no per-channel weights (enf_fit_step_cw);  no per-point errors asked for (enf_fit_step_e with
 *     err);  ENF_FIT_DETERMINISTIC not set;  the backward resolves to the z-fold pair kernel;  the rff embedding, an invariant without
 *     per-latent phases (not ball / ball_lat), and (D, H) one of (128, 2), (128, 1), (64, 2), in either precision.
 * Elsewhere everything behind the forward pair kernel is the ordinary sequence on per-signal targets and weights, bit for bit.  Loss
 * and gradients of the shared backward differ from the unflagged call's by rounding only: in fp32 mode by the order of the fp32 sums
 * over queries; in bf16 mode also by WHERE d out meets a bf16 rounding (the ordinary backward rounds every signal's d out and the
 * quantities scaled by it to bf16 operands, the shared one rounds the unit-seeded quantities and multiplies by d out in fp32).
 * Workspace: d out and the row of outputs borrow the d ybar region behind signal 0's rows -- floats [N HD, N HD + B N) and the N
 * after them; d ybar and delta are written for signal 0 only (floats [0, N HD) and [0, N H)): delta's floats [N H, B N H), which the
 * ordinary backward writes, keep what they held.  The sizes do not change.
 * The library does NOT check the statement: with unequal latents every signal gets signal 0's forward. */
#define ENF_FIT_SHARED_LATENTS 128u
/* 1 where a fit step (enf_fit_step_ex / _w, or _e without err) with `flags` on this descriptor takes the shared backward above, 0
 * where it runs the ordinary sequence behind the forward; negative ENF_E* on a bad descriptor, ENF_EINVAL on unknown flag bits. */
int enf_shared_backward_applies(const EnfDesc* d, unsigned flags);
/* 1 and *parts = P (a power of two; 1 = signal 0 in one pass, then the broadcast) where a call with ENF_FIT_SHARED_LATENTS /
 * ENF_STAGE_SHARED_LATENTS on this descriptor runs the shared forward; 0 and *parts = 1 where it runs the ordinary sequence (B == 1,
 * the z-fold forward, relu masks); negative ENF_E* on a bad descriptor. */
int enf_shared_forward_parts(const EnfDesc* d, int32_t* parts);
int enf_fit_step_ex(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                    const void* packed, const float* target, float grad_scale, float* loss, float* dp, float* da, float* dsigma,
                    void* workspace, size_t workspace_bytes, unsigned flags, void* stream);

/* Weighted loss (enf_fit_step_w, enf_mse_value_grad_w, enf_fit_inputs_w).  `weight` is fp32 of shape (B, N): one value per signal
 * and query point, finite and >= 0, or NULL for the unweighted calls above.
 *     loss  = 1 / (B N O) * sum_{b,n} weight[b,n] * sum_o (out[b,n,o] - target[b,n,o])^2
 *     d out = 2 * weight[b,n] * (out - target) / (B N O) * grad_scale
 * With weight == 1 everywhere this is the unweighted loss.  The library does NOT normalise the weights (no reduction pass over
 * them: a call stays a pure function of its arguments); a caller who wants a weighted MEAN passes weights of mean 1.
 * A point with weight == 0 does not exist: its `target` values are never used in arithmetic and may be NaN or Inf, and its
 * contribution to the loss and to d out is exactly 0.0f (not 0 * NaN) -- weight = isfinite(field) is usable as it stands.
 * A signal whose weights are all zero adds 0 to the loss and gets zero gradients; it is not an error.
 * Flags, workspace and scratch sizes are those of the unweighted calls; with weight == NULL the arithmetic is theirs, bit for bit. */
int enf_fit_step_w(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                   const void* packed, const float* target, float grad_scale, float* loss, float* dp, float* da, float* dsigma,
                   void* workspace, size_t workspace_bytes, const float* weight /* (B,N) or NULL */, unsigned flags, void* stream);

/* Per-channel weights (enf_fit_step_cw, enf_mse_value_grad_cw, enf_fit_inputs_cw): variables that are observed separately -- a buoy
 * that gives height but no vorticity, a retrieval that fails for one variable.  `cweight` is fp32 of shape (B, N, O): one value per
 * signal, query point and output channel, finite and >= 0.
 *     loss  = 1 / (B N O) * sum_{b,n,o} cweight[b,n,o] * (out[b,n,o] - target[b,n,o])^2
 *     d out = 2 * cweight[b,n,o] * (out - target) / (B N O) * grad_scale
 * The rule above holds per VALUE: an element of weight 0 does not exist, its target is never used in arithmetic and may be NaN or Inf,
 * and its share of the loss and of d out is exactly 0.0f (a select on the weight, not a product) -- cweight = isfinite(field) per value is
 * usable as it stands.  The library does not normalise.  A signal or a channel whose weights are all zero contributes zeros and is not
 * an error.  cweight[b,n,o] = weight[b,n] for every o is the per-point loss: every squared error is weighted BEFORE it is added to the
 * sum over o, not the sum afterwards, and the two calls are promised to agree to rounding, not bit for bit (they are different kernel
 * instantiations).
 * x_bstride, flags (ENF_FIT_DETERMINISTIC: same inputs, same bits), workspace and scratch sizes are those of enf_fit_step_w /
 * enf_mse_value_grad_w; both precisions and every width, head count and O <= 32 of the fit step are served.  cweight == NULL is
 * ENF_EINVAL: a caller without channel weights uses the calls above, whose signatures and arithmetic are unchanged. */
int enf_fit_step_cw(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                    const void* packed, const float* target, float grad_scale, float* loss, float* dp, float* da, float* dsigma,
                    void* workspace, size_t workspace_bytes, const float* cweight /* (B,N,O), required */, unsigned flags, void* stream);

/* Per-signal and per-point errors (enf_fit_step_e, enf_eval_loss): which signal did not fit, and where on the grid the error is,
 * without a decode.  With w[b,n,o] the per-channel weight, the per-point weight broadcast over o, or 1:
 *     err[b,n]  = sum_o w[b,n,o] * (out[b,n,o] - target[b,n,o])^2        (B, N) fp32, OVERWRITTEN
 *     loss_b[b] = 1 / (N O) * sum_n err[b,n]                              (B)    fp32, OVERWRITTEN
 * The zero-weight rule of "Weighted loss" holds unchanged: a value of weight 0 does not exist, its target may be NaN or Inf, and its share
 * of err is exactly 0.0f (a select, not a product); a point whose weights are all zero -- a padded index of enf_fit_inputs_b among them --
 * has err == 0.0f, a signal whose weights are all zero has loss_b == 0.0f.  Weights are not normalised.  mean_b loss_b equals the scalar
 * loss of the calls above up to rounding.  err and loss_b are caller-owned; nothing past [0, B N) and [0, B) is written.
 * Both are deterministic by construction, in the default mode too: the fused tail holds 16 queries' squared errors per wave in
 * registers, and after folding the output channels 16 lanes store one value per query (no atomic, nothing that depends on the signals a
 * wave straddles); enf_signal_sum_kernel, one workgroup per signal, adds a row of err in an order fixed by N alone.  (Their bits follow
 * `out`: the split z-fold forward variant orders its partial sums by the call's shape, see "Deterministic mode".)
 *
 * enf_fit_step_e: enf_fit_step_w (weight, or neither) / enf_fit_step_cw (cweight) on the same arguments -- the same host sequence and the
 * same kernel instantiations with a store added, so `loss`, dp, da and dsigma are those calls', bit for bit -- plus err (required) and,
 * with loss_b != NULL, one more small launch at the end of the sequence.  weight and cweight both non-NULL is ENF_EINVAL.  flags and
 * workspace as enf_fit_step_w (ENF_FIT_DETERMINISTIC concerns `loss` and the gradients; other bits are ENF_EINVAL). */
int enf_fit_step_e(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                   const void* packed, const float* target, float grad_scale, float* loss, float* dp, float* da, float* dsigma,
                   void* workspace, size_t workspace_bytes, const float* weight /* (B,N) or NULL */, const float* cweight /* (B,N,O) or NULL */,
                   float* err /* (B,N), required */, float* loss_b /* (B) or NULL */, unsigned flags, void* stream);
/* Evaluation without a decode: latent prologue, forward pair kernel (the variant the descriptor resolves to), and a tail whose epilogue
 * forms err -- and, with loss != NULL, *loss += the scalar loss of enf_mse_value_grad[_w|_cw] (the caller zeroes it) -- from the output
 * accumulators: no `out` in memory, no backward chain, no stash.  At least one of loss, err, loss_b must be given (all NULL is
 * ENF_EINVAL), weight and cweight both non-NULL is ENF_EINVAL.  loss_b WITHOUT err is allowed: the per-point errors then pass through a
 * region of the workspace this call does not otherwise use.  flags: 0 or ENF_FIT_DETERMINISTIC (the scalar loss through the workspace's
 * partials in a fixed order; `workspace` is then enf_workspace_bytes_ex(d, flags), else enf_workspace_bytes(d)); err and loss_b are the
 * same bits either way. */
int enf_eval_loss(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                  const void* packed, const float* target, const float* weight /* (B,N) or NULL */, const float* cweight /* (B,N,O) or NULL */,
                  float* loss /* scalar, accumulated, or NULL */, float* err /* (B,N) or NULL */, float* loss_b /* (B) or NULL */,
                  void* workspace, size_t workspace_bytes, unsigned flags, void* stream);

/* The per-signal sum on its own, for a caller that fills err (B, N) from several calls (a grid evaluated in chunks):
 *     loss_b[b] = scale * (err[b,0] + ... + err[b,N-1])        scale = 1 / (N O) for the definition above
 * One workgroup per signal: each of its 256 threads adds a fixed strided slice, then a fixed tree -- same inputs and N, same bits; no
 * atomics, no scratch, any N >= 1, 64-bit offsets.  The kernel enf_fit_step_e and enf_eval_loss run.  NULL or B, N < 1: ENF_EINVAL. */
int enf_signal_sum(const float* err, int32_t B, int32_t N, float scale, float* loss_b, void* stream);

/* Grouped observations (enf_fit_step_g, enf_eval_loss_g): data that are cell averages, not point values -- the cell means of a
 * finite-volume solver, the box means of a reanalysis, a footprint's weighted mean.  An observation is a fixed linear functional of the
 * decode, a quadrature rule over a few query points per cell, and the fused tail forms it in registers in front of the squared error.
 *     G is the group size, one of {1, 2, 4, 8, 16};  N = M * G queries per signal;  observation m of signal b owns the CONSECUTIVE
 *     query rows m G .. m G + G - 1 of x (B, N, dx; x_bstride as everywhere, 0 = one set of cells for all signals).
 *     obs[b,m,o] = sum_{k<G} q[b, mG+k] * out[b, mG+k, o]         q = qweight (B, N), or NULL = 1/G exactly
 *     loss       = 1/(B M O) * sum_{b,m} w[b,m] * sum_o (obs[b,m,o] - target[b,m,o])^2
 *     d out[b, mG+k, o] = 2 * q[b,mG+k] * w[b,m] * (obs - target)[b,m,o] / (B M O) * grad_scale
 *     err_g[b,m] = w[b,m] * sum_o (obs - target)^2                 loss_b[b] = sum_m err_g[b,m] / (M O)
 * target is (B, M, O); w = oweight (B, M), or NULL for 1.  The zero-weight rule of "Weighted loss" holds per OBSERVATION: w[b,m] == 0
 * is a select, so that observation's target may be NaN or Inf, and its share of the loss and of every d out of its group is exactly
 * 0.0f.  q is a plain factor: it must be finite (any sign; q == 0 is a product, not a select) and the kernel multiplies with it.
 * Nothing is normalised by the library: a caller who wants cell MEANS passes factors that sum to 1 per group (NULL does).
 * The group sum is a fixed xor tree over the 16 query lanes of a wave's tile -- a group never straddles a tile, a signal or the rows
 * beyond B N, because tiles start at multiples of 16, G divides 16 and G divides N -- so obs, err_g and d out are the same bits in
 * every mode, as err is ("Per-signal and per-point errors"); ENF_FIT_DETERMINISTIC concerns `loss` and the gradients, as there.
 * The host sequences, workspace sizes and served descriptors are those of enf_fit_step_w / enf_eval_loss (every width, head count,
 * embedding, invariant, precision, pair-kernel variant and relu-mask mode); the tail runs an instantiation of its own, one for every G.
 * flags: 0 or ENF_FIT_DETERMINISTIC.  ENF_FIT_SHARED_LATENTS is ENF_EINVAL in these two calls: enf_fit_step_gs below is the fit step
 * that takes it.  ENF_EINVAL, behind the descriptor's errors and before anything is launched, also for: G outside the
 * set; N % G != 0; target == NULL; enf_fit_step_g with loss_b but without err_g (the fit step's workspace has no free region for the
 * errors; enf_eval_loss_g allows it, through the region enf_eval_loss uses); enf_eval_loss_g with loss, err_g and loss_b all NULL.
 * G == 1 is legal: with q == 1 (or NULL) it is the per-point loss, and the result agrees with enf_fit_step_w(weight = w) to rounding --
 * not bit for bit, it is another instantiation.  (With q != 1 the residual is q out - target, not out - target.)
 * `loss` is accumulated (the caller zeroes it), err_g and loss_b are OVERWRITTEN; nothing past [0, B M) and [0, B) is written. */
int enf_fit_step_g(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                   const void* packed, const float* target /* (B,M,O) */, int32_t G, const float* qweight /* (B,N) or NULL */,
                   const float* oweight /* (B,M) or NULL */, float grad_scale, float* loss, float* dp, float* da, float* dsigma,
                   float* err_g /* (B,M) or NULL */, float* loss_b /* (B) or NULL, needs err_g */, void* workspace, size_t workspace_bytes,
                   unsigned flags, void* stream);
int enf_eval_loss_g(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                    const void* packed, const float* target /* (B,M,O) */, int32_t G, const float* qweight /* (B,N) or NULL */,
                    const float* oweight /* (B,M) or NULL */, float* loss /* scalar, accumulated, or NULL */, float* err_g /* (B,M) or NULL */,
                    float* loss_b /* (B) or NULL */, void* workspace, size_t workspace_bytes, unsigned flags, void* stream);

/* The first inner step on shared latents against grouped observations: enf_fit_step_g's arguments, and `flags` may also carry
 * ENF_FIT_SHARED_LATENTS -- the caller's statement that the latents, the cells (x_bstride == 0) and the rows of qweight are equal for all
 * signals, as at step 0 of a fit on shared cells.  With the flag clear the call runs enf_fit_step_g's sequence: its bits.  With the flag
 * set the one shared forward runs wherever enf_shared_forward_parts says it does, and the one shared backward where
 * enf_shared_backward_applies(d, flags) holds and err_g == NULL (O == 1, the z-fold backward, an invariant without phases, a (D, H) of
 * the rule's set, not deterministic): ONE tail pass, unit-seeded tail backward and backward pair pass on signal 0, contracted with d out
 * (B, N) -- which the grouped SHARED form of the loss kernel forms from signal 0's row of outputs, signal 0's factors qweight[0, :] and
 * all B signals' targets and observation weights.  Elsewhere the ordinary grouped tail runs behind the shared forward.  The results agree
 * with the unflagged call to rounding, not bit for bit.  Workspace sizes are unchanged; the borrowed regions are those documented for
 * the shared backward (d out and the row of outputs behind signal 0's rows of d ybar).  B == 1 with the flag: the flag says nothing, the
 * call is enf_fit_step_g.  B > 1 with the flag and x_bstride != 0: ENF_EINVAL.  Every other refusal is enf_fit_step_g's, in its order. */
int enf_fit_step_gs(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                    const void* packed, const float* target /* (B,M,O) */, int32_t G, const float* qweight /* (B,N) or NULL */,
                    const float* oweight /* (B,M) or NULL */, float grad_scale, float* loss, float* dp, float* da, float* dsigma,
                    float* err_g /* (B,M) or NULL */, float* loss_b /* (B) or NULL, needs err_g */, void* workspace, size_t workspace_bytes,
                    unsigned flags, void* stream);

/* The unfused grouped loss, for a caller that holds a decode out (B, N, O) in memory (the weight-gradient path): the definitions above,
 *     *loss += the grouped loss;   dout (B, N, O) or NULL = d out;   err_g (B, M) or NULL, OVERWRITTEN.
 * One thread owns one (group, channel): it forms obs as the tail does (products, then pairs at distance 1, 2, .. G / 2), the residual
 * under the select on w -- a NaN or Inf target under w == 0 is allowed and leaves exact zeros --, its share of the loss and the G values of
 * d out; err_g is stored by the thread of channel 0, which adds the O shares in channel order.  d out and err_g involve no atomics: the
 * same bits run to run, in every mode.  The scalar loss is added with one atomic per workgroup, or with flags = ENF_MSE_DETERMINISTIC
 * through `scratch` (enf_mse_scratch_bytes(B M O, flags) bytes) in a fixed order, as enf_mse_value_grad_w.  qweight NULL = 1 / G exactly,
 * oweight NULL = 1.  ENF_EINVAL: out, target or loss NULL; B, N, O < 1; G outside the set; N % G != 0; an unknown flag bit; deterministic
 * without scratch.  Then ENF_EWORKSPACE. */
int enf_mse_value_grad_g(const float* out /* (B,N,O) */, const float* target /* (B,M,O) */, int32_t B, int32_t N, int32_t O, int32_t G,
                         const float* qweight /* (B,N) or NULL */, const float* oweight /* (B,M) or NULL */, float grad_scale,
                         float* dout /* (B,N,O) or NULL */, float* loss, float* err_g /* (B,M) or NULL */, void* scratch,
                         size_t scratch_bytes, unsigned flags, void* stream);

/* Per-value weights on grouped observations (enf_fit_step_gc, enf_eval_loss_gc, enf_mse_value_grad_gc, enf_fit_inputs_gc): a cell that
 * lacks one variable counts with its others -- a masked sea-surface value under a valid wind, one NaN variable in a box.  With
 * cw = cweight_g (B, M, O), finite and >= 0, REQUIRED, in place of oweight:
 *     loss      = 1/(B M O) * sum_{b,m,o} cw[b,m,o] * (obs[b,m,o] - target[b,m,o])^2
 *     d out[b, mG+k, o] = 2 * q[b,mG+k] * cw[b,m,o] * (obs - target)[b,m,o] / (B M O) * grad_scale
 *     err_g[b,m] = sum_o cw[b,m,o] * (obs - target)^2              loss_b[b] = sum_m err_g[b,m] / (M O)
 * The zero-weight rule holds per VALUE: a value of weight 0 does not exist, its target may be NaN or Inf, and its share of the loss and
 * of every d out of its group is exactly 0.0f.  Nothing is normalised.
 * After the xor tree every lane of a group holds obs for its eight channels; the lane reads cw[m][o] where the per-observation form
 * reads oweight[m] and applies the select per value.  The arithmetic per value and its order are the per-observation form's, so with
 * cw[b,m,:] = w[b,m] the results are those of the _g call with oweight = w, bit for bit (under ENF_FIT_DETERMINISTIC for the loss and
 * the gradients).  The tail runs instantiations of their own on an argument block of their own: every other call keeps its kernels.
 * Each call takes its _g counterpart's arguments, refusals and workspace sizes; cweight_g == NULL is ENF_EINVAL.
 * ENF_FIT_SHARED_LATENTS on enf_fit_step_gc: ENF_EUNSUPPORTED (behind the descriptor's errors) -- the shared first step with per-value
 * weights is not built. */
int enf_fit_step_gc(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                    const void* packed, const float* target /* (B,M,O) */, int32_t G, const float* qweight /* (B,N) or NULL */,
                    const float* cweight_g /* (B,M,O), required */, float grad_scale, float* loss, float* dp, float* da, float* dsigma,
                    float* err_g /* (B,M) or NULL */, float* loss_b /* (B) or NULL, needs err_g */, void* workspace, size_t workspace_bytes,
                    unsigned flags, void* stream);
int enf_eval_loss_gc(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                     const void* packed, const float* target /* (B,M,O) */, int32_t G, const float* qweight /* (B,N) or NULL */,
                     const float* cweight_g /* (B,M,O), required */, float* loss /* scalar, accumulated, or NULL */,
                     float* err_g /* (B,M) or NULL */, float* loss_b /* (B) or NULL */, void* workspace, size_t workspace_bytes,
                     unsigned flags, void* stream);
/* enf_mse_value_grad_g with per-value weights: the same kernel, whose thread of (group, channel o) reads cw[b,m,o]; err_g adds the O
 * shares in channel order, each under its own weight. */
int enf_mse_value_grad_gc(const float* out /* (B,N,O) */, const float* target /* (B,M,O) */, int32_t B, int32_t N, int32_t O, int32_t G,
                          const float* qweight /* (B,N) or NULL */, const float* cweight_g /* (B,M,O), required */, float grad_scale,
                          float* dout /* (B,N,O) or NULL */, float* loss, float* err_g /* (B,M) or NULL */, void* scratch,
                          size_t scratch_bytes, unsigned flags, void* stream);

/* Derivative fields (enf_field_grad, enf_query_vjp): the Jacobian of a decode with respect to its query coordinates -- grad u, the
 * vorticity or divergence of a velocity field, a PDE residual on a decoded frame -- in one call, without the weight-gradient machinery.
 *     jac[o,b,n,i] = d out[b,n,o] / d x[b,n,i]        (O, B, N, dx) fp32, channel-major, required, OVERWRITTEN
 * The derivatives are with respect to the coordinates AS GIVEN: for the spherical and ball invariants x holds angles (and a radius), and
 * jac holds the plain partial derivatives w.r.t. those angles -- no metric factors (1 / sin theta, 1 / r) are applied; ponita_full's third
 * column is d / d theta_x.  jac is per SIGNAL also when x_bstride == 0: a caller who wants the derivative w.r.t. a grid shared by the
 * batch sums over b.  `out` (B, N, O) is the decode itself, or NULL; with out == NULL
 * nothing outside jac and the workspace is written.
 * Sequence: latent prologue; the z-fold backward's per-latent matrices where the descriptor resolves to that variant; the forward pair
 * kernel; the forward tail, stashing its pre-activations; then per output channel o the SEEDED tail backward -- d out = the unit vector
 * e_o formed in registers, no (B, N, O) seed tensor exists -- and the backward pair kernel without a store, its query gradient into
 * jac + o B N dx.  The call picks no pair-kernel variant of its own: pair_fwd_variant / pair_bwd_variant decide, as everywhere.
 * Default mode: jac is zeroed by the call and every latent's share of a query's gradient is ADDED with float atomics, so the last bits
 * follow the order in which wavefronts finish.  flags = ENF_BWD_DETERMINISTIC: the shares go to the workspace and are summed over the
 * latents in index order -- same inputs, same bits, with the promise and the limits of "Deterministic mode" above.  Other flag bits are
 * ENF_EINVAL.  The gradient of the latent table that the backward pair kernel also forms is scratch of the call and is not returned.
 * `workspace`: enf_field_grad_workspace_bytes(d, flags) bytes, ONE buffer for everything the call needs (flags = 0: equal to
 * enf_workspace_bytes(d); deterministic: enf_workspace_bytes_ex(d, flags) plus B Z N dx floats of query-gradient shares); contents need
 * not be kept.  The size query returns 0 for a bad descriptor, a mask mode or an unknown flag bit.
 * Errors in this order: the descriptor's; EnfDesc.mask_mode != ENF_MASK_OFF is ENF_EUNSUPPORTED (relu masks belong to the
 * meta-gradient, not to a decode); a NULL x, p, a, packed, workspace, jac / dx / dout (or sigma with a window) or an unknown flag bit is
 * ENF_EINVAL; then ENF_EWORKSPACE.  Every invariant, both embeddings, both precisions and every width, head count and O <= 32 of the
 * forward are served.  Cost: one forward plus O backward passes (DESIGN.md 7 has the measured times). */
size_t enf_field_grad_workspace_bytes(const EnfDesc* d, unsigned flags);
int enf_field_grad(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                   const void* packed, float* out /* (B,N,O) or NULL */, float* jac /* (O,B,N,dx), required */, void* workspace,
                   size_t workspace_bytes, unsigned flags, void* stream);
/* The vector-Jacobian product for a caller-given seed, the same sequence with ONE backward pass (the tail backward reads `dout`):
 *     dx[b,n,:] = sum_o dout[b,n,o] * d out[b,n,o] / d x[b,n,:]        (B, N, dx) fp32, required, OVERWRITTEN
 * per signal like jac.  dout (B, N, O) is required; out, flags, workspace (enf_field_grad_workspace_bytes) and errors as above. */
int enf_query_vjp(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                  const void* packed, const float* dout /* (B,N,O) */, float* out /* (B,N,O) or NULL */, float* dx /* (B,N,dx) */,
                  void* workspace, size_t workspace_bytes, unsigned flags, void* stream);

/* Tendency fields (enf_field_tangent): the decode in FORWARD mode along a latent direction -- the Jacobian-vector product of the
 * decoder with respect to its latents,
 *     tan[b,n,o] = sum_z  d out[b,n,o] / d (p, a, sigma)[b,z,:]  .  (dp, da, dsigma)[b,z,:]        (B, N, O) fp32, required, OVERWRITTEN
 * With (dp, da, dsigma) = dz/dt of a latent ODE this is the time derivative d u / d t of the decoded field (the other half of a PDE
 * residual next to enf_field_grad); it also pushes a latent perturbation to the field (linearised uncertainty, the sensitivity to one
 * latent, the J v of a Gauss-Newton fit whose J^T w is enf_backward_latents).
 * dp, da, dsigma have the shapes of p, a, sigma; each may be NULL (= zero), not all three.  dsigma without a window
 * (EnfDesc.use_window == 0) contributes exactly zero.  `out` (B, N, O) is the decode itself, or NULL.  x may have x_bstride == 0.
 * Sequence: latent prologue and its tangent (a second latent table), the tangent pair kernel (the latent-split layout; every weight
 * stage multiplies the primal and the tangent fragments; softmax sums T = sum e (dy + dl y), S = sum e dl beside Y, C, L), the tangent
 * tail.  In bf16 mode the tangent fragments are rounded to bf16 exactly where the primal ones are.
 * tan and out are written once per element, by one lane, with no atomics and a fixed order of operations: the call is bit-reproducible
 * run to run by construction, and independent of what the workspace held.
 * Caller-owned buffers, the caller's stream, no allocation, no host synchronisation, no settings.  `workspace`:
 * enf_field_tangent_workspace_bytes(d) bytes -- the plain workspace's regions (latent table, an, kv, ybar) followed by the table's
 * tangent and d ybar, so a buffer of this size also serves every plain call on the same descriptor; contents need not be kept.  The
 * size query returns 0 for a bad or unserved descriptor.
 * Served: embedding rff; rel_pos_periodic, latitude_periodic, polar_periodic, ponita, abs_pos, rel_pos, norm_rel_pos; every width and
 * head count of the forward (d_true / h_true included); both precisions.  ball, ball_lat, ponita_full, ENF_EMB_FFN and
 * mask_mode != ENF_MASK_OFF are ENF_EUNSUPPORTED.  Errors in this order: the descriptor's; ENF_EUNSUPPORTED as above; a NULL x, p, a,
 * blob, tan, workspace (or sigma with a window), or all three tangents NULL: ENF_EINVAL.  (DESIGN.md 7 has accuracy and times.) */
size_t enf_field_tangent_workspace_bytes(const EnfDesc* d);
int enf_field_tangent(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                      const float* dp, const float* da, const float* dsigma /* tangents: shapes of p / a / sigma, each may be NULL */,
                      const void* blob, float* out /* (B,N,O) or NULL */, float* tan /* (B,N,O), OVERWRITTEN */, void* workspace,
                      void* stream);

/* Directional derivatives (enf_field_tangent_x): enf_field_tangent with a direction in the QUERY coordinates carried by the same pass,
 *     tan[b,n,o] = sum_z  d out[b,n,o] / d (p, a, sigma)[b,z,:]  .  (dp, da, dsigma)[b,z,:]
 *                + sum_i  d out[b,n,o] / d x[b,n,i]  xdot[b,n,i]
 * Forward mode is linear in its direction, so one pass serves both halves of a first-order transport term: with (dp, da, dsigma) = dz/dt
 * and xdot = c(x) it is the material derivative Du/Dt = u_t + c . grad u; with xdot alone an advection term, the derivative along a
 * characteristic or a streamline, a normal derivative on a boundary; with xdot = e_i a column of enf_field_grad's Jacobian in forward
 * mode.  xdot is (B, N, dx) fp32 with a batch stride of its own, xdot_bstride (in elements; 0 = one direction field shared by the
 * signals, whatever x_bstride is); it is read at the rows x is read at and is never written.  The direction is in the coordinates AS
 * GIVEN, the convention of enf_field_grad: on the sphere xdot is (d phi / dt, d theta / dt), rates of the angles with no metric
 * factors -- a physical velocity (u, v) is divided by its metric factors by the caller.
 * xdot, dp, da, dsigma: each may be NULL (= zero), not all four.  With xdot == NULL the call IS enf_field_tangent (the same kernels,
 * the same bits); with xdot the pair kernel is an instantiation of its own that adds the query's terms to the tangent of (invariant,
 * window) in front of the first GEMM stage -- no further stage, accumulator, LDS region or workspace.
 * Everything else is enf_field_tangent's: the workspace (enf_field_tangent_workspace_bytes(d)), what is served, the order of the
 * errors (the descriptor's; ENF_EUNSUPPORTED; ENF_EINVAL for a NULL x, p, a, blob, tan, workspace, sigma with a window, or all four
 * tangents NULL), one store per element with no atomics, bit-reproducible run to run and independent of what the workspace held. */
int enf_field_tangent_x(const EnfDesc* d, const float* x, int64_t x_bstride, const float* xdot /* (B,N,dx) or NULL */,
                        int64_t xdot_bstride, const float* p, const float* a, const float* sigma, const float* dp, const float* da,
                        const float* dsigma, const void* blob, float* out /* (B,N,O) or NULL */, float* tan /* (B,N,O), OVERWRITTEN */,
                        void* workspace, void* stream);

/* Second directional derivatives (enf_field_second_x): the decode in forward mode to SECOND order along a direction in the query
 * coordinates,
 *     tan2[b,n,o] = sum_ij  xdot[b,n,i] xdot[b,n,j]  d^2 out[b,n,o] / d x[b,n,i] d x[b,n,j]        (B, N, O) fp32, required, OVERWRITTEN
 *     tan[b,n,o]  = sum_i   d out[b,n,o] / d x[b,n,i]  xdot[b,n,i]                                 (B, N, O) fp32 or NULL
 * tan is enf_field_tangent_x's value along xdot alone; `out` (B, N, O) is the decode itself, or NULL.  With xdot = e_i tan2 is a
 * diagonal entry of the Hessian (dx passes sum to the Laplacian), with e_i + e_j an off-diagonal one by polarisation
 * (H_ij = (D2(e_i + e_j) - D2 e_i - D2 e_j) / 2): the diffusion term of a PDE residual next to enf_field_tangent's u_t.  "Second
 * derivative" as autograd means it: almost everywhere, the relu kinks contribute nothing.  xdot is (B, N, dx) fp32, required, with a batch
 * stride of its own (xdot_bstride, in elements; 0 = one direction field for all signals), read at the rows x is read at and never
 * written.  Coordinates AS GIVEN, the convention of enf_field_grad: angles on the sphere, no metric factors -- a sum of second angle
 * derivatives is not the Laplace-Beltrami operator.  The direction is in the query coordinates only: the latents have no tangent here.
 * Sequence: latent prologue (no prologue tangent, no tangent table); the second-order pair kernel (the tangent pair kernel's latent-split
 * layout, heads over grid.z; every weight stage multiplies the primal, the first-order and the second-order fragments; softmax sums
 * U = sum e (d2y + 2 dl dy + (d2l + dl^2) y), R = sum e (d2l + dl^2) beside Y, C, L, T, S); the second-order tail.  In bf16 mode the
 * first- and second-order fragments are rounded to bf16 exactly where the primal ones are.
 * Every element of tan2, tan and out is written once, by one lane, with no atomics and a fixed order of operations: bit-reproducible
 * run to run and independent of what the workspace held.  Caller-owned buffers, the caller's stream, no allocation, no host
 * synchronisation, no settings.  `workspace`: enf_field_second_workspace_bytes(d) bytes -- enf_field_tangent_workspace_bytes' regions at
 * their offsets followed by d2 ybar, so one buffer of this size also serves the plain and the tangent calls on the same descriptor;
 * contents need not be kept.  The size query returns 0 for a bad or unserved descriptor.
 * Served: what enf_field_tangent_x serves.  Errors in this order: the descriptor's; ENF_EUNSUPPORTED for ENF_EMB_FFN, ball, ball_lat,
 * ponita_full and mask_mode != ENF_MASK_OFF; ENF_EINVAL for a NULL x, xdot, p, a, blob, tan2, workspace, or sigma with a window.
 * (DESIGN.md 7 has accuracy and times.) */
size_t enf_field_second_workspace_bytes(const EnfDesc* d);
int enf_field_second_x(const EnfDesc* d, const float* x, int64_t x_bstride, const float* xdot /* (B,N,dx), required */,
                       int64_t xdot_bstride, const float* p, const float* a, const float* sigma, const void* blob,
                       float* out /* (B,N,O) or NULL */, float* tan /* (B,N,O) or NULL */, float* tan2 /* (B,N,O), OVERWRITTEN */,
                       void* workspace, void* stream);

/* Gauss-Newton product (enf_gn_product): the matrix-vector product of a Gauss-Newton / Levenberg-Marquardt fit of the latents in one
 * call,
 *     gv = grad_scale * 2 / (B N O) * sum_{n,o} J[b,n,o,:]^T  w[b,n,o]  (J v)[b,n,o]
 *     J = d out / d (p, a, sigma),   v = (vp, va, vsigma),   gv = (gp, ga, gsigma)        shapes of p / a / sigma, fp32, OVERWRITTEN
 * w = `weight` (B, N) broadcast over o, `cweight` (B, N, O), or 1, with the definitions and the zero-weight select of "Weighted loss":
 * a value of weight 0 does not exist.  With the grad_scale of a fit step gv is the Gauss-Newton Hessian of that step's loss applied to
 * v, in the units of that step's gradient.  The call takes no target and no loss.  vp, va, vsigma: each may be NULL (= zero), not all
 * three; vsigma without a window contributes exactly zero.  gp, ga, gsigma are all required.  x may have x_bstride == 0.
 * Sequence: latent prologue; the prologue tangent; where pair_bwd_variant resolves to the z-fold backward, its per-latent matrices;
 * the tangent pair kernel of enf_field_tangent, which here also stores lse in the forward pair kernel's convention; the GN tail -- ONE
 * kernel that runs the tail's forward chain with tangents, forms d out = (w > 0 ? w tan : 0) * 2 grad_scale / (B N O) in registers and
 * runs the tail's backward chain on the primal pre-activations (stashed in the workspace): neither tan nor d out reaches memory and the
 * forward chain runs once; the backward pair kernel without a store; the prologue backward.
 * flags: ENF_BWD_DETERMINISTIC -- the backward pair kernel's fixed-order route: no float atomic runs, same inputs give the same bits,
 * independent of what the workspace held (the rest of the sequence is deterministic by construction).  ENF_GN_REUSE_POINT -- the
 * caller's statement that the last call on this workspace was enf_fit_step_w / _cw / _e / _ex / _g WITHOUT ENF_FIT_SHARED_LATENTS
 * (enf_fit_step_gs with the flag clear is enf_fit_step_g), or an earlier enf_gn_product or enf_gn_product_g, on the same
 * (d, x, p, a, sigma, packed) and the same deterministic bit -- the grouped step runs the per-point step's sequence around another
 * tail, so it leaves the latent table, `an`, `kv` and the z-fold backward's matrices as that step does: the prologue and the z-fold matrices
 * are not recomputed (a CG solve calls the product many times at one point, right behind the fit step that gave the gradient).  Any
 * other bit: ENF_EINVAL.
 * `workspace`: ONE buffer of enf_gn_workspace_bytes(d, flags) bytes.  It begins with the plain workspace's regions at their usual
 * offsets (with ENF_BWD_DETERMINISTIC: those of enf_workspace_bytes_ex), so the fit steps and enf_eval_loss with the same deterministic
 * bit run on the same buffer; contents need not be kept otherwise.  The size query returns 0 for a bad or unserved descriptor or an
 * unknown flag bit.
 * Served: what enf_field_tangent serves.  Errors in this order: the descriptor's; ENF_EUNSUPPORTED for ENF_EMB_FFN, ball, ball_lat,
 * ponita_full or mask_mode != ENF_MASK_OFF; ENF_EINVAL for a NULL x, p, a, packed, gp, ga, gsigma, workspace (or sigma with a window),
 * all three tangents NULL, weight and cweight both given, or an unknown flag bit; then ENF_EWORKSPACE. */
#define ENF_GN_REUSE_POINT 1u
size_t enf_gn_workspace_bytes(const EnfDesc* d, unsigned flags);
int enf_gn_product(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                   const float* vp, const float* va, const float* vsigma /* shapes of p / a / sigma; each may be NULL, not all */,
                   const void* packed, const float* weight /* (B,N) or NULL */, const float* cweight /* (B,N,O) or NULL */,
                   float grad_scale, float* gp, float* ga, float* gsigma /* shapes of p / a / sigma, required, OVERWRITTEN */,
                   void* workspace, size_t workspace_bytes, unsigned flags, void* stream);
/* Gauss-Newton product on grouped observations (enf_gn_product_g): the product above for a fit on cell averages, in the notation of
 * "Grouped observations" (G, M = N / G, q = qweight (B, N) or NULL = 1/G exactly, w = oweight (B, M) or NULL = 1),
 *     gv = grad_scale * 2 / (B M O) * sum_{m,o} Jg[b,m,o,:]^T  w[b,m]  (Jg v)[b,m,o]
 *     Jg[b,m,o,:] = sum_{k<G} q[b, mG+k] * J[b, mG+k, o, :]                the Jacobian of the group sums obs[b,m,o]
 * w is under the zero-weight select: an observation of weight 0 does not exist, and its G rows get d out == 0.0f exactly, whatever
 * their x and q hold (finite).  q is a plain finite factor; nothing is normalised.  With enf_fit_step_g's grad_scale gv is the
 * Gauss-Newton Hessian of that step's loss applied to v, in the units of its gradient -- an observation is linear in the decode, so the
 * matrix is exact up to the residual's curvature.
 * The sequence is enf_gn_product's with the grouped form of the GN tail: behind the tangent chain a wave forms obs_tan = sum_k q tan by
 * the fixed xor tree of the fused grouped loss over its 16 query lanes (a group never straddles a tile, a signal or the rows beyond
 * B N, see there) and d out = q * (w * obs_tan) * 2 grad_scale / (B M O) in every lane of the group, in registers: neither tan,
 * obs_tan nor d out reaches memory.  One instantiation serves every G.  G == 1 with q == 1 (or NULL) is the per-point product with
 * weight = w, to rounding -- not bit for bit, it is another instantiation.
 * Workspace and size query: enf_gn_workspace_bytes, unchanged.  flags: ENF_BWD_DETERMINISTIC, ENF_GN_REUSE_POINT, as above.
 * Errors in this order: the descriptor's; ENF_EUNSUPPORTED as enf_gn_product gives it; ENF_EINVAL for what enf_gn_product refuses
 * and for G outside {1, 2, 4, 8, 16} or N % G != 0; then ENF_EWORKSPACE. */
int enf_gn_product_g(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                     const float* vp, const float* va, const float* vsigma, const void* packed,
                     int32_t G, const float* qweight /* (B,N) or NULL = 1/G */, const float* oweight /* (B,M) or NULL = 1 */,
                     float grad_scale, float* gp, float* ga, float* gsigma,
                     void* workspace, size_t workspace_bytes, unsigned flags, void* stream);
/* One conjugate-gradient step for B independent systems in one launch: the Gauss-Newton matrix of a fit is block diagonal over the
 * signals, so a solve is B separate CG iterations with per-signal alpha, beta and damping.  The vectors are split over up to three
 * segments (the latent components), each (B, Z, width) fp32 contiguous.
 *   INIT (q == NULL in every segment):  x = 0,  d = r,  rho = r . r        (the caller has put -g in r)
 *   step, per signal b:  q' = q + lam_b d;  kappa = d . q';  alpha = rho / kappa;  x += alpha d;  r -= alpha q';  rho' = r . r;
 *                        d = r + (rho' / rho) d;  rho = rho'
 * A signal whose rho or kappa is not a finite positive number is FROZEN -- it has converged, its right-hand side is zero, or the matrix
 * is numerically indefinite (bf16): its x, r, d and rho stay exactly as they were, so one signal cannot poison the batch with a NaN.
 * One workgroup per signal; the dot products run as a fixed strided slice per thread plus a fixed tree: same inputs, same bits, no
 * atomics, any Z * width.  ENF_EINVAL: nseg outside 1..3, a NULL segs / rho / x / r / d, a width or B or Z < 1, q given in some
 * segments only. */
typedef struct EnfCgSegment {      /* one latent component: p, a or sigma */
  float* x; float* r; float* d;    /* iterate, residual, search direction: updated in place */
  const float* q;                  /* G d as enf_gn_product returned it (undamped), or NULL in every segment: INIT */
  int32_t width, reserved;
} EnfCgSegment;
int enf_cg_update(int nseg /* 1..3 */, const EnfCgSegment* segs, int32_t B, int32_t Z, const float* lam /* (B) damping, or NULL = 0 */,
                  float* rho /* (B) r . r, in/out */, void* stream);

/* Reconstruction loss of the inner loop and its gradient in one pass (pde_trainer.py:185):
 *   *loss += mean((out - target)^2)   (the caller zeroes *loss),   dout = 2 (out - target) / n * grad_scale  (dout may be NULL) */
int enf_mse_value_grad(const float* out, const float* target, size_t n, float grad_scale, float* dout, float* loss,
                       void* stream);
/* The same with flags (0 = enf_mse_value_grad, no scratch).  ENF_MSE_DETERMINISTIC: the blocks' partial sums go to `scratch`
 * (enf_mse_scratch_bytes(n, flags)) and one workgroup adds them to *loss in index order. */
#define ENF_MSE_DETERMINISTIC 16u
size_t enf_mse_scratch_bytes(size_t n, unsigned flags);
int enf_mse_value_grad_ex(const float* out, const float* target, size_t n, float grad_scale, float* dout, float* loss,
                          void* scratch, size_t scratch_bytes, unsigned flags, void* stream);

/* The same with the weighted loss above: `weight` holds one value per O consecutive elements (n / O of them; n % O != 0 is
 * ENF_EINVAL), or NULL (then O only has to divide n). */
int enf_mse_value_grad_w(const float* out, const float* target, const float* weight /* (n / O) or NULL */, size_t n, int32_t O,
                         float grad_scale, float* dout, float* loss, void* scratch, size_t scratch_bytes, unsigned flags, void* stream);

/* The same with one weight per ELEMENT, cweight (n floats, required): the per-channel weighted loss above.  Flags and scratch are
 * those of enf_mse_value_grad_w (enf_mse_scratch_bytes(n, flags)). */
int enf_mse_value_grad_cw(const float* out, const float* target, const float* cweight /* (n), required */, size_t n, float grad_scale,
                          float* dout, float* loss, void* scratch, size_t scratch_bytes, unsigned flags, void* stream);

/* The meta-SGD update of one inner step for all latent components in one launch (pde_trainer.py:206-219):
 *     out = x - lr * (scale * g)        scale = the batch size (:206); lr broadcasts over the leading dims
 * A segment is one component (p_pos, p_ori, a, gaussian_window): x, out contiguous (n elements, trailing dimension
 * `width`); g may be a column slice of a wider array: element (row, c) is g[row * g_stride + c]; lr holds 1 or `width`
 * values (trainers/pde_trainer.py:83-97).  A component whose update is zeroed (:209-212) is simply left out. */
#define ENF_SGD_MAX_SEGMENTS 4
typedef struct EnfSgdSegment {
  const float* x;
  const float* g;
  const float* lr;
  float* out;
  int64_t n;
  int32_t width, g_stride, lr_len, reserved;
} EnfSgdSegment;
int enf_meta_sgd_update(int nseg, const EnfSgdSegment* segs, float scale, void* stream);

/* The Adam counterpart for an auto-decoder's latent TABLE (nonmaml_pde_trainer.py:67,125-126,159-160: optax.adam over the whole
 * table): one optax `adam` step (scale_by_adam with bias correction, eps outside the root, no weight decay) over every component of
 * the table in one launch, straight from the GATHERED gradient rows a fit step returns.  Per table element (s, z, c) of a segment:
 *     g   = sum over j with idx[j] == s of g[(j, z, c)], added in increasing j; exact 0.0f when no j matches
 *     mu' = b1 mu + (1 - b1) g            nu' = b2 nu + (1 - b2) g g
 *     x'  = x - lr (mu' / c1) / (sqrt(nu' / c2) + eps)
 * c1 = 1 - b1^count and c2 = 1 - b2^count are formed by the caller (in double, passed as float): the library keeps no counter.
 * A row outside the batch moves by its momentum only, as optax's dense Adam over the whole table does -- this is no sparse update.
 * idx == NULL: the gradient is dense, nidx must equal S and row j is table row j (what a multi-rank run holds after its all-reduce).
 * One thread owns one element and scans the nidx indices (a batch size): no atomics, no scratch; duplicate indices are legal and
 * summed in a fixed order (same inputs, same bits); x_out == x, mu_out == mu, nu_out == nu (in place) is safe.  The gradient
 * buffers must not overlap an output.  An index outside [0, S) is never used as an offset: it matches no row and contributes
 * nothing (the rule of enf_fit_inputs_b).  Element offsets are 64-bit (S Z width may exceed 2^31).
 * ENF_EINVAL: a NULL pointer, a non-positive size (nseg outside 1..ENF_ADAM_MAX_SEGMENTS, S, Z, nidx, width), c1 <= 0 or c2 <= 0;
 * ENF_EDIM: g_stride < width, or idx == NULL with nidx != S. */
#define ENF_ADAM_MAX_SEGMENTS 4
typedef struct EnfAdamSegment {      /* one component: p_pos, p_ori, a, gaussian_window */
  const float* x;                    /* table (S, Z, width) ... */
  const float* mu;                   /* ... and its first ... */
  const float* nu;                   /* ... and second moment */
  const float* g;                    /* gradient rows (nidx, Z, width); may be a column slice of a wider array (g_stride) */
  float* x_out;                      /* (S, Z, width); each output may equal its input */
  float* mu_out;
  float* nu_out;
  int32_t width, g_stride;           /* g element (j, z, c) = g[(j * Z + z) * g_stride + c] */
} EnfAdamSegment;
int enf_table_adam_update(int nseg, const EnfAdamSegment* segs, int64_t S, int32_t Z,
                          const int64_t* idx /* (nidx) table rows of the gradient's signals, or NULL */, int32_t nidx,
                          float lr, float b1, float b2, float eps, float c1, float c2, void* stream);

/* What the inner loop prepares before its first step, in ONE launch (pde_trainer.py:157-159, 193-197; six framework kernels otherwise):
 *   - every latent component of the shared initialisation, (1, Z, width), repeated for the B signals -> (B, Z, width);
 *   - the coordinates and the targets of all S1 = S + 1 sampled point sets gathered once:
 *       xs[s, i, :] = coords[masks[i, s], :]     (S1, Ns, dx)       ys[s, b, i, :] = img[b, masks[i, s], :]     (S1, B, Ns, O)
 *     with masks (Ns, S1) int64 indices into the N grid points, coords (N, dx), img (B, N, O), all fp32 and contiguous;
 *   - the S1 loss accumulators zeroed. */
typedef struct EnfFitComponent {
  const float* src; /* (1, Z, width) */
  float* dst;       /* (B, Z, width) */
  int32_t width, reserved;
} EnfFitComponent;
int enf_fit_inputs(int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t N, int32_t Ns, int32_t S1, int32_t dx, int32_t O,
                   const float* coords, const float* img, const int64_t* masks, float* xs, float* ys, float* losses, void* stream);
/* The same, plus the loss weights of the S1 sampled sets gathered in the same launch:
 *       ws[s, b, i] = weight[b, masks[i, s]]     (S1, B, Ns)       weight (B, N)
 * (a plain copy: the NaN targets of zero-weight points pass through `ys` untouched).  weight and ws are given together or both
 * NULL (= enf_fit_inputs); one without the other is ENF_EINVAL. */
int enf_fit_inputs_w(int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t N, int32_t Ns, int32_t S1, int32_t dx, int32_t O,
                     const float* coords, const float* img, const int64_t* masks, float* xs, float* ys, float* losses,
                     const float* weight /* (B,N) or NULL */, float* ws /* (S1,B,Ns) */, void* stream);
/* The same for PER-SIGNAL index sets (signals observed at different places: sensor drop-out, land masks, cloud gaps), one launch:
 *       masks (B, Ns, S1) int64: one set of Ns indices into the N grid points per signal and step
 *       xs[s, b, i, :] = coords[masks[b, i, s], :]     (S1, B, Ns, dx)      -- the consumers take xs[s] with x_bstride = Ns * dx
 *       ys[s, b, i, :] = img[b, masks[b, i, s], :]     (S1, B, Ns, O)
 *       ws[s, b, i]    = weight[b, masks[b, i, s]]     (S1, B, Ns)
 * plus the latent broadcast and the zeroed loss accumulators of enf_fit_inputs.  Row offsets are 64-bit (B N O may exceed 2^31).
 * Index contract: an index < 0 or >= N is never dereferenced.  Its xs row is coords[0], its ys row is zeros and its ws is 0.0f, so
 * by the weighted-loss contract above the point does not exist; a sampler pads a signal that has fewer than Ns observed points
 * with -1.  ws is what expresses this, so it is REQUIRED (NULL is ENF_EINVAL, with or without weight); weight stays optional: without
 * it ws is 1.0f for an index in range and 0.0f for one outside.
 * The loss stays un-normalised, 1 / (B Ns O): a caller who wants a signal with few valid samples to take a step as long as a fully
 * sampled one rescales ws[s, b, :] to mean 1 (inner_loop(normalize_weights=True)); the library forms no sums over weights. */
int enf_fit_inputs_b(int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t N, int32_t Ns, int32_t S1, int32_t dx, int32_t O,
                     const float* coords, const float* img, const int64_t* masks /* (B,Ns,S1) */, float* xs, float* ys, float* losses,
                     const float* weight /* (B,N) or NULL */, float* ws /* (S1,B,Ns), required */, void* stream);

/* The counterpart of enf_fit_inputs_w (per_signal_masks == 0: masks (Ns, S1), xs (S1, Ns, dx)) and of enf_fit_inputs_b
 * (per_signal_masks != 0: masks (B, Ns, S1), xs (S1, B, Ns, dx)) for PER-CHANNEL weights, in the same single launch as the latent
 * broadcast, xs, ys and the zeroed loss accumulators:
 *       ws[s, b, i, o] = cweight[b, masks[..], o]      (S1, B, Ns, O)      cweight (B, N, O)
 * cweight and ws are both required (NULL is ENF_EINVAL).  The index contract of enf_fit_inputs_b holds for BOTH layouts: an index
 * < 0 or >= N is never dereferenced; its xs row is coords[0], its ys row is zeros and its ws row is O zeros.  Offsets are 64-bit. */
int enf_fit_inputs_cw(int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t N, int32_t Ns, int32_t S1, int32_t dx, int32_t O,
                      const float* coords, const float* img, const int64_t* masks, float* xs, float* ys, float* losses,
                      const float* cweight /* (B,N,O), required */, float* ws /* (S1,B,Ns,O), required */, int32_t per_signal_masks,
                      void* stream);

/* The inner loop's setup on sampled CELLS in one launch, the counterpart of enf_fit_inputs_w / _b / _cw for cell indices: the latent
 * broadcast and the zeroed loss accumulators of enf_fit_inputs, and the gather of S1 = S + 1 sets of Ms cells out of M.
 *     xq (M G, dx) the cells' quadrature points, q (M G) their factors or NULL, obs (B, M, O), oweight (B, M) or NULL
 *     per_signal_masks == 0: masks (Ms, S1),    xs (S1, Ms G, dx),    qs (S1, Ms G)
 *     per_signal_masks != 0: masks (B, Ms, S1), xs (S1, B, Ms G, dx), qs (S1, B, Ms G)
 *     ys (S1, B, Ms, O), ws (S1, B, Ms), losses (S1)
 * Row i G + k of a sampled set is row m G + k of cell m = masks[..]; ys[s,b,i,:] = obs[b,m,:]; ws[s,b,i] = oweight[b,m].
 * The index contract of enf_fit_inputs_b: an index outside [0, M) is never dereferenced; its xs / qs rows are cell 0's (finite: q is a
 * factor, not a select), its ys row zeros and its ws 0.0f.  ws is therefore required with per-signal masks (without oweight it is 1 for
 * an index in range and 0 outside); with shared masks ws and oweight are given together or both NULL.  q and qs likewise.  64-bit row
 * offsets.  ENF_EINVAL before any launch: a NULL required pointer, a size < 1, G outside {1, 2, 4, 8, 16}, q / qs or oweight / ws not
 * given as stated, ncomp outside [1, ENF_SGD_MAX_SEGMENTS] or a bad component. */
int enf_fit_inputs_g(int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t M, int32_t Ms, int32_t S1, int32_t G,
                     int32_t dx, int32_t O, const float* xq /* (M*G, dx) */, const float* q /* (M*G) or NULL */,
                     const float* obs /* (B, M, O) */, const int64_t* masks, float* xs, float* qs /* NULL iff q NULL */,
                     float* ys /* (S1, B, Ms, O) */, float* losses, const float* oweight /* (B, M) or NULL */,
                     float* ws /* (S1, B, Ms) */, int32_t per_signal_masks, void* stream);
/* enf_fit_inputs_g for per-value weights (include "Grouped observations", the _gc calls), in the same single launch by the same kernel:
 *       ws[s, b, i, o] = cweight_g[b, masks[..], o]      (S1, B, Ms, O)      cweight_g (B, M, O)
 * cweight_g and ws are both required (NULL is ENF_EINVAL), with either mask layout; an index outside [0, M) gives O zeros. */
int enf_fit_inputs_gc(int ncomp, const EnfFitComponent* comps, int32_t B, int32_t Z, int32_t M, int32_t Ms, int32_t S1, int32_t G,
                      int32_t dx, int32_t O, const float* xq /* (M*G, dx) */, const float* q /* (M*G) or NULL */,
                      const float* obs /* (B, M, O) */, const int64_t* masks, float* xs, float* qs /* NULL iff q NULL */,
                      float* ys /* (S1, B, Ms, O) */, float* losses, const float* cweight_g /* (B, M, O), required */,
                      float* ws /* (S1, B, Ms, O), required */, int32_t per_signal_masks, void* stream);

/* Sparse linear observations (enf_obs_apply, enf_mse_value_grad_a, enf_fit_step_a, enf_eval_loss_a): an observation is ANY fixed linear
 * functional of the decode -- a 9- or 27-point cell rule, a triangle of an unstructured mesh, a footprint whose size changes with
 * latitude, a closed rule that shares nodes with its neighbour, an increment u(x_i) - u(x_j), a line integral along a ray, a conserved
 * total.  One operator A (M x N) is shared by the B signals of a call, given as CSR for the forward product and as CSC (the same
 * entries sorted by column, stably) for the transposed one; with the notation of "Grouped observations":
 *     obs[b,m,o]    = sum_{e in [row_ptr[m], row_ptr[m+1])}  val[e] * out[b, col[e], o]
 *     loss          = 1/(B M O) * sum_{b,m,o} w * (obs - target)^2
 *     d out[b,n,o]  = grad_scale * 2/(B M O) * sum_{e in [col_ptr[n], col_ptr[n+1])}  tval[e] * (w * (obs - target))[b, trow[e], o]
 *     err_a[b,m]    = sum_o w * (obs - target)^2                    loss_b[b] = sum_m err_a[b,m] / (M O)
 * target is (B, M, O).  w is oweight (B, M), or cweight (B, M, O), or 1; both at once is ENF_EINVAL.  The zero-weight rule holds per
 * observation (oweight) or per value (cweight) exactly as for groups: w == 0 is a select, the target under it may be NaN or Inf, and
 * its share of the loss and of every d out is exactly 0.0f.  val is a plain finite factor of any sign; nothing is normalised.  An
 * empty row is legal: its obs is 0 and it counts in M.  A query row that no observation references gets d out == 0.0f exactly.
 * Indices are int32 (nnz <= 2^31 - 1); offsets into the (B, ., O) tensors are 64-bit.  The library cannot check that the CSC is the
 * transpose of the CSR (fitting/operators.py builds it; a host test checks it): a mismatch gives a wrong gradient, never an address --
 * a col or trow outside its range is SKIPPED before it becomes an offset, and row and column ranges are clamped to [0, nnz].
 * Nothing of the decoder's kernels changes: these calls run two memory-bound kernels (csrc/enf_obs.hip) between the existing launches.
 * Summation order, a function of a row's length alone (so obs, r = w (obs - target), err_a and d out are the same bits in every mode
 * and under every launch geometry; no atomics):
 *     forward, length <= 64:  the row's entries in entry order, one fma each
 *     forward, length >= 65:  64 partial sums, partial l over entries l, l + 64, l + 128, ... in order (fma), then the fixed xor tree
 *                             over the partials at distance 32, 16, 8, 4, 2, 1
 *     transposed, any length: the column's entries in the CSC's entry order, one fma each, then the factor grad_scale 2/(B M O)
 * err_a adds its O shares in channel order.  The scalar loss is added with one float atomic per workgroup, or in deterministic mode
 * through scratch and the fixed-order sum of "Deterministic mode". */
typedef struct EnfSparseObs {
  int32_t M;                /* observations (rows of A) */
  int64_t nnz;              /* entries */
  const int32_t* row_ptr;   /* (M + 1) */
  const int32_t* col;       /* (nnz) query rows, any order within a row, repeats allowed */
  const float* val;         /* (nnz) */
  const int32_t* col_ptr;   /* (N + 1): the CSC; the three may be NULL where no d out is formed */
  const int32_t* trow;      /* (nnz) observations */
  const float* tval;        /* (nnz) */
} EnfSparseObs;
/* obs (B, M, O) = A out, out (B, N, O): the forward product alone.  ENF_EINVAL: a NULL, B, N, O or M < 1, nnz < 0. */
int enf_obs_apply(const float* out, int32_t B, int32_t N, int32_t O, const EnfSparseObs* op, float* obs, void* stream);
/* The unfused loss for a caller that holds a decode, enf_mse_value_grad_g's counterpart: *loss += the loss; dout (B, N, O) or NULL
 * (then the CSC may be NULL); err_a (B, M) or NULL, OVERWRITTEN.  scratch: enf_mse_a_scratch_bytes(B, M, O, dout != NULL, flags) bytes
 * -- r (B, M, O) where d out is wanted, the loss partials with flags = ENF_MSE_DETERMINISTIC; its contents need not be kept.
 * ENF_EINVAL: out, target, loss or a needed part of op NULL; B, N, O, M < 1; nnz < 0; both weights; an unknown flag bit; scratch NULL
 * where bytes are needed.  Then ENF_EWORKSPACE. */
size_t enf_mse_a_scratch_bytes(int32_t B, int32_t M, int32_t O, int want_dout, unsigned flags);
int enf_mse_value_grad_a(const float* out /* (B,N,O) */, const float* target /* (B,M,O) */, int32_t B, int32_t N, int32_t O,
                         const EnfSparseObs* op, const float* oweight /* (B,M) or NULL */, const float* cweight /* (B,M,O) or NULL */,
                         float grad_scale, float* dout /* (B,N,O) or NULL */, float* loss, float* err_a /* (B,M) or NULL */,
                         void* scratch, size_t scratch_bytes, unsigned flags, void* stream);
/* The fit step and the evaluation against an operator.  enf_fit_step_a: prologue, forward pair kernel, the forward tail with its
 * stash (out into the workspace), the forward product with the loss, the transposed product, the tail backward on the stash, the
 * backward pair kernel, the prologue backward, and with loss_b the per-signal sums -- the pair and tail kernels of enf_fit_step_w,
 * for every descriptor it serves.  enf_eval_loss_a: prologue, forward pair kernel, plain forward tail, the forward product with the
 * loss, the per-signal sums.  `workspace`: ONE buffer of enf_obs_workspace_bytes(d, M, flags) bytes; it begins with the plain (or,
 * with ENF_FIT_DETERMINISTIC, the deterministic) workspace's regions at their usual offsets, followed by out and d out (B, N, O), r
 * (B, M, O), the errors (B, M) of a call that wants loss_b without err_a -- so that combination is allowed here -- and the loss
 * partials.  flags: 0 or ENF_FIT_DETERMINISTIC; ENF_FIT_SHARED_LATENTS is ENF_EINVAL.  ENF_EINVAL, behind the descriptor's errors and
 * before any launch: a NULL that is required, M < 1, nnz < 0, both weight kinds; enf_eval_loss_a with loss, err_a and loss_b all NULL.
 * `loss` is accumulated (the caller zeroes it); err_a and loss_b are OVERWRITTEN. */
size_t enf_obs_workspace_bytes(const EnfDesc* d, int32_t M, unsigned flags);
int enf_fit_step_a(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                   const void* packed, const float* target /* (B,M,O) */, const EnfSparseObs* op, const float* oweight /* (B,M) or NULL */,
                   const float* cweight /* (B,M,O) or NULL */, float grad_scale, float* loss, float* dp, float* da, float* dsigma,
                   float* err_a /* (B,M) or NULL */, float* loss_b /* (B) or NULL */, void* workspace, size_t workspace_bytes,
                   unsigned flags, void* stream);
int enf_eval_loss_a(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                    const void* packed, const float* target /* (B,M,O) */, const EnfSparseObs* op, const float* oweight /* (B,M) or NULL */,
                    const float* cweight /* (B,M,O) or NULL */, float* loss /* scalar, accumulated, or NULL */,
                    float* err_a /* (B,M) or NULL */, float* loss_b /* (B) or NULL */, void* workspace, size_t workspace_bytes,
                    unsigned flags, void* stream);
/* Gauss-Newton product on sparse observations (enf_gn_product_a): enf_gn_product for a fit against an operator, in the notation above,
 *     gv = grad_scale * 2 / (B M O) * J^T A^T W A J v,        J = d out / d (p, a, sigma),  v = (vp, va, vsigma),  gv = (gp, ga, gsigma)
 * W = oweight (B, M), cweight (B, M, O) or 1 under the zero-weight select, per observation or per value: what has weight 0 does not
 * exist.  The scale and sign are those of enf_fit_step_a's gradient, so with that step's grad_scale gv is the Gauss-Newton Hessian of
 * its loss applied to v -- exact up to the residual's curvature, an observation being linear in the decode.
 * An operator couples rows across tiles and waves, so the Gauss-Newton tail is cut open as the fit step's is.  Sequence: latent
 * prologue (skipped under ENF_GN_REUSE_POINT, with the z-fold backward's matrices); the prologue tangent; the tangent pair kernel, which
 * leaves lse; the tangent tail in its stash form -- tan (B, N, O) and the tail's activation stash, no out; the forward product with the
 * weights in the same pass, r = (w > 0 ? w (A tan) : 0) (B, M, O); the transposed product d out = grad_scale 2/(B M O) A^T r, every
 * element written (a query row in no observation gets 0.0f); the tail's backward on the stash (the kernel of enf_fit_step_a); the
 * backward pair kernel; the prologue backward.  The two products keep "Sparse linear observations"' summation order and safety rules
 * and are functions of their inputs in every mode; ENF_BWD_DETERMINISTIC selects the backward pair kernel's fixed-order route as in
 * enf_gn_product.  ENF_GN_REUSE_POINT: as there, the last call on this workspace being enf_fit_step_a (same deterministic bit) or an
 * earlier enf_gn_product_a at the same (d, x, p, a, sigma, packed).
 * `workspace`: ONE buffer of enf_gn_a_workspace_bytes(d, M, flags) bytes -- enf_gn_workspace_bytes' regions followed by tan, r and
 * d out, and never less than enf_obs_workspace_bytes(d, M, ENF_FIT_DETERMINISTIC): the fit step, the products and the evaluation of a
 * Levenberg-Marquardt step run on one buffer.  The size query returns 0 for a bad or unserved descriptor, M < 1 or an unknown flag bit.
 * Served: what enf_gn_product serves.  Errors in this order: the descriptor's; ENF_EUNSUPPORTED as enf_gn_product gives it; ENF_EINVAL
 * for what enf_gn_product refuses, a NULL op, M < 1, nnz < 0, a missing CSR or CSC array (the product reads both), both weight kinds;
 * then ENF_EWORKSPACE. */
size_t enf_gn_a_workspace_bytes(const EnfDesc* d, int32_t M, unsigned flags);
int enf_gn_product_a(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                     const float* vp, const float* va, const float* vsigma, const void* packed, const EnfSparseObs* op,
                     const float* oweight /* (B,M) or NULL */, const float* cweight /* (B,M,O) or NULL */, float grad_scale,
                     float* gp, float* ga, float* gsigma, void* workspace, size_t workspace_bytes, unsigned flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Latent ODE (experiments/fitting/ode_models/ponita_ode_g.py): the separable group convolution of a ConvBlock,
 * SepGconv.__call__ (:63-83), over the fully connected latent set of every signal:
 *     out[b,r,:] = bias + sum_s a[b,s,:] * (kb[b,r,s,:] @ W)        a (B,Z,C), kb (B,Z,Z,J), W (J,C), bias (C) or NULL
 * fused: the (B,Z,Z,C) `kernel` tensor the reference materialises (:72) never exists; the J -> C product runs as fp32
 * MFMA tiles consumed in registers.  kb element (b,r,s,j) is read at b*Z*Z*J + r*kb_stride_r + s*kb_stride_s + j, so
 * the same entry point gives the gradient w.r.t. the senders:  d a = conv(g, kb with the (r,s) strides swapped, W, NULL).
 * enf_ode_conv_backward_basis:  d kb[b,r,s,:] = W (g[b,r,:] * a[b,s,:])   (B,Z,Z,J).
 * enf_ode_conv_backward_weight: d W (J,C) = kb^T (g (x) a) over the pair axis, the (B,Z,Z,C) product formed in registers, and
 *   d bias (C) = sum_{b,r} g: `dW` is ONE buffer of J*C + C floats, d W followed by d bias;
 *   scratch: enf_ode_conv_backward_weight_scratch_bytes(B,Z,J,C) bytes (per-workgroup partials, summed in a fixed order).
 * J in {16, 32, 64, 128}, C in {16, 32, 64, 128, 256} (256: config_shallow_water.yaml's node), anything else ENF_EUNSUPPORTED;
 * all buffers fp32, contiguous, 16-byte aligned. */
int enf_ode_conv_forward(int B, int Z, int J, int C, const float* a, const float* kb, int64_t kb_stride_r,
                         int64_t kb_stride_s, const float* W, const float* bias, float* out, void* stream);
int enf_ode_conv_backward_basis(int B, int Z, int J, int C, const float* a, const float* g, const float* W, float* dkb,
                                void* stream);
size_t enf_ode_conv_backward_weight_scratch_bytes(int B, int Z, int J, int C);
int enf_ode_conv_backward_weight(int B, int Z, int J, int C, const float* a, const float* kb, const float* g, float* dW,
                                 void* scratch, size_t scratch_bytes, void* stream);
/* PolynomialFeatures (ponita_ode_g.py:15-26) of the P = B Z^2 pair invariants x (P, I): the Kronecker powers
 * [x, x(x)x, ..., x^(x)(degree+1)] concatenated, F = I + I^2 + ... + I^(degree+1) values per pair (enf_ode_poly_num_features;
 * 340 for I = 4, degree = 3), in the reference's order (each power appends its new factor as the last index).
 * forward: feat (P, F);  backward: dx (P, I) = J^T dfeat.  I <= 8, degree <= 7.  No intermediate power is materialised. */
int enf_ode_poly_num_features(int I, int degree);
int enf_ode_poly_forward(int64_t P, int I, int degree, const float* x, float* feat, void* stream);
int enf_ode_poly_backward(int64_t P, int I, int degree, const float* x, const float* dfeat, float* dx, void* stream);
/* The kernel basis of PonitaGen (ponita_ode_g.py:128-131, 158-160), fused:  kb = gelu(gelu(poly(inv) W1 + b1) W3 + b3)
 * over the P = B Z^2 pairs, inv (P, I), W1 (F, H1), b1 (H1), W3 (H1, J), b3 (J) as in the reference's parameter tree
 * (kernel_basis/layers_1, layers_3), kb (P, J); gelu = the tanh form (flax default).  Neither the (P, F) feature tensor nor
 * the (P, H1) hidden layer touch memory (csrc/enf_ode_basis.hip).  backward: given d kb (P, J) -> d inv (P, I), d W1, d b1,
 * d W3, d b3 (all OVERWRITTEN; weight gradients are summed in a fixed order: bitwise reproducible).
 * I in 1..4, degree = 3, H1 in {32, 64, 128} (forward also 256), J in {32, 64, 128} (enf_ode_basis_supported -> 1 / 0);
 * `scratch`: enf_ode_basis_scratch_bytes(P, I, H1, J, backward) bytes, 16-byte aligned, contents need not be kept. */
/* Vector readout of PonitaGen (ponita_ode_g.py:176-193) with one output channel, fused:
 *     out[b,r,:] = mean_s wgt[b,r,s] * (cr * u[b,r,:] + cs * w[b,s,:]),    wgt[b,r,s] = inv[b,r,s,:] . Wi + aw[b,s]
 * inv (B,Z,Z,I) the pair invariants, Wi (I) = the readout kernel's rows for the invariants, aw (B,Z) = a @ (its rows for the latent
 * features), u / w (B,Z,D) receiver / sender vectors (relative position: u = w = p_pos, cr = 1, cs = -1; sender orientation: cr = 0,
 * cs = 1).  backward: g = d out (B,Z,D) -> d inv, d aw, d u, d w (OVERWRITTEN) and dWi_part (B * ceil(Z/64), I): partial sums of
 * d Wi, to be added up by the caller.  I <= 6, D in {2, 3}; no atomics. */
int enf_ode_vec_readout_forward(int B, int Z, int I, int D, const float* inv, const float* aw, const float* u, const float* w,
                                float cr, float cs, const float* Wi, float* out, void* stream);
int enf_ode_vec_readout_backward(int B, int Z, int I, int D, const float* inv, const float* aw, const float* u, const float* w,
                                 float cr, float cs, const float* Wi, const float* g, float* dinv, float* daw, float* du,
                                 float* dw, float* dWi_part, void* stream);
/* The per-latent half of a ConvBlock (ponita_ode_g.py:44-48), fused:  out = Dense_2(gelu(Dense_1(LayerNorm_eps(x))))  over the
 * R = B Z latent rows, x (R, H), gamma / beta (H), W1 (H, M), b1 (M), W2 (M, H), b2 (H) as in the reference's tree
 * (norm/scale, norm/bias, linear_1, linear_2); gelu = the tanh form.  forward also writes pre = LayerNorm(x) W1 + b1 (R, M)
 * for the backward.  backward: d out g (R, H) -> d x (R, H) and, in ONE buffer of 2 H M + M + 3 H floats (OVERWRITTEN),
 * d W1 (H, M) | d W2 (M, H) | d b1 (M) | d b2 (H) | d gamma (H) | d beta (H), summed in a fixed order.
 * H in {32, 64, 128}, M = 2 H (enf_ode_block_supported); scratch: enf_ode_block_scratch_bytes(R, H, M) bytes, 16-byte aligned. */
int enf_ode_block_supported(int H, int M);
size_t enf_ode_block_scratch_bytes(int64_t R, int H, int M);
int enf_ode_block_forward(int64_t R, int H, int M, const float* x, const float* gamma, const float* beta, const float* W1,
                          const float* b1, const float* W2, const float* b2, float eps, float* out, float* pre, void* stream);
int enf_ode_block_backward(int64_t R, int H, int M, const float* x, const float* gamma, const float* beta, const float* W1,
                           const float* W2, const float* pre, const float* g, float eps, float* dx, float* dparams,
                           void* scratch, size_t scratch_bytes, void* stream);
int enf_ode_basis_supported(int I, int degree, int H1, int J, int backward);
size_t enf_ode_basis_scratch_bytes(int64_t P, int I, int H1, int J, int backward);
int enf_ode_basis_forward(int64_t P, int I, int degree, int H1, int J, const float* inv, const float* W1, const float* b1,
                          const float* W3, const float* b3, float* kb, void* scratch, size_t scratch_bytes, void* stream);
int enf_ode_basis_backward(int64_t P, int I, int degree, int H1, int J, const float* inv, const float* W1, const float* b1,
                           const float* W3, const float* b3, const float* dkb, float* dinv, float* dW1, float* db1,
                           float* dW3, float* db3, void* scratch, size_t scratch_bytes, void* stream);

/* EVERY weight gradient in one call (value_and_grad over params['nef'], pde_trainer.py:255; SURVEY.md 8b's
 * enf_backward_weights in full).  Given d out it returns d p, d a, d sigma AND the gradients of all ENF_NUM_TENSORS
 * Flax-named tensors, fp32, shaped like the tensors enf_pack_weights takes, OVERWRITTEN (`dW` = host array of device pointers;
 * the two frozen RFF coefficient entries -- rff.py:87-90 -- may be NULL, else they are zero-filled).  `tensors` are the same
 * weights `packed` was built from (the fold backward needs the unfolded factors), `ybar` / `lse` come from enf_forward[_stages]
 * on the same inputs, `workspace` is that call's workspace (flags: ENF_BWD_REUSE_PROLOGUE / ENF_BWD_REUSE_TAIL as for
 * enf_backward_latents_ex; 0 recomputes what it needs), `dx` (B,N,dx) or NULL accumulates the gradient w.r.t. the queries.
 * Kernels: the tail backward in its weight-gradient form, K3 with the activation store + K4 (enf_xtd_kernel), the prologue
 * backward, fp32 matrix-pipe X^T delta products over the query / latent rows, and the chain rule through the folds of
 * enf_pack_weights -- no library GEMM, no host framework op; slices are summed in a fixed order.  By default d lt and `dx` are
 * accumulated with float atomics, so the results are reproducible up to those sums' last bits; with ENF_BWD_DETERMINISTIC in
 * `flags` the store-variant pair kernel's shares of d lt and of `dx` go through partial buffers in `scratch` and fixed-order sums
 * -- same inputs, same bits, for every output -- and `dx` is OVERWRITTEN instead of accumulated into; size `scratch` with
 * enf_backward_all_scratch_bytes_ex(d, c, ENF_BWD_DETERMINISTIC [| ENF_BWD_QUERY_GRAD when `dx` is given]); the workspace is the
 * plain enf_workspace_bytes(d).  scratch_bytes >= enf_backward_all_scratch_bytes(d, c) for some chunk size c in 1..B
 * signals (the largest c that fits is used; with relu masks a multiple of mask_signals).  EnfDesc.mask_mode = ENF_MASK_READ
 * replays the relu masks in the pair kernel as enf_backward_weights does. */
size_t enf_backward_all_scratch_bytes(const EnfDesc* d, int chunk_signals);
size_t enf_backward_all_scratch_bytes_ex(const EnfDesc* d, int chunk_signals, unsigned flags);
int enf_backward_all(const EnfDesc* d, const float* x, int64_t x_bstride, const float* p, const float* a, const float* sigma,
                     const float* const* tensors, const void* packed, const float* ybar, const float* lse, const float* dout,
                     float* dp, float* da, float* dsigma, float* const* dW, float* dx, void* workspace, size_t workspace_bytes,
                     void* scratch, size_t scratch_bytes, unsigned flags, void* stream);

/* Weight gradients of the per-pair chain (enf_backward_weights).  enf_pair_backward_ex plus, in the same
 * call, the gradients of the loss w.r.t. the ten trainable ENF_P_* tensors:
 *     dpair[ENF_P_A*] = X^T delta  (in, out),   dpair[ENF_P_B*] = 1^T delta      over all B Z N pairs, fp32, OVERWRITTEN
 * (dpair = host array of ENF_NUM_PAIR_TENSORS device pointers laid out like the tensors enf_pack_pair takes; the two RFF
 * coefficient entries are ignored: frozen in the reference, rff.py:87-90).  Kernels: K3 in its STORE instantiation writes
 * every layer's input / delta fragments for a chunk of signals into `scratch` (ENF_S_* above), enf_xtd_kernel reads each of
 * them ONCE and forms all 3 + 3H products and bias sums on the matrix pipe, a reduction sums slices and chunks in a fixed
 * order (same inputs -> same bits).  No library GEMM, no host framework op.
 *   scratch_bytes >= enf_backward_weights_scratch_bytes(d, c) for some chunk size c in 1..B signals: the call uses the
 *   largest c that fits (with relu masks: a multiple of mask_signals).  c = B: one pass.
 * EnfDesc.mask_mode = ENF_MASK_READ replays the relu masks as in enf_pair_backward_ex with a store. */
size_t enf_backward_weights_scratch_bytes(const EnfDesc* d, int chunk_signals);
int enf_backward_weights(const EnfDesc* d, const float* x, int64_t x_bstride, const float* lt, const void* packed,
                         const float* lse, const float* dybar, const float* delta, float* dlt, float* const* dpair,
                         float* dx, void* scratch, size_t scratch_bytes, void* stream);
/* The same with flags (0 = enf_backward_weights): ENF_BWD_DETERMINISTIC sums `dlt` and `dx` in a fixed order from partials at the
 * end of `scratch` (enf_backward_weights_scratch_bytes_ex(d, c, flags), with ENF_BWD_QUERY_GRAD when `dx` is given); `dx` is then
 * OVERWRITTEN. */
size_t enf_backward_weights_scratch_bytes_ex(const EnfDesc* d, int chunk_signals, unsigned flags);
int enf_backward_weights_ex(const EnfDesc* d, const float* x, int64_t x_bstride, const float* lt, const void* packed,
                            const float* lse, const float* dybar, const float* delta, float* dlt, float* const* dpair,
                            float* dx, void* scratch, size_t scratch_bytes, unsigned flags, void* stream);

/* The pair-kernel variant a call with this descriptor runs (ENF_VARIANT_AUTO resolved): ENF_VARIANT_LATENT_SPLIT or
 * ENF_VARIANT_ZFOLD (or, forward only, ENF_VARIANT_ZFOLD_ZSPLIT); `backward` = 0 for the forward kernel, 1 for the backward kernel.
 * Negative ENF_E* on a bad descriptor. */
int enf_pair_variant(const EnfDesc* d, int backward);
/* How ENF_VARIANT_ZFOLD_ZSPLIT cuts the forward pair kernel's work: the flattened (signal, 128-query tile, latent) space of
 * tiles x Z latent steps is walked by `workgroups` workgroups of `run` consecutive steps each (the last one may be shorter); a query
 * tile's latents are met by at most `parts` of them (the partial-sum slots the workspace holds).  Returns 1 and fills the three values when
 * the descriptor resolves to that variant, 0 (values untouched) when it does not, negative ENF_E* on a bad descriptor. */
int enf_pair_partition(const EnfDesc* d, int32_t* run, int32_t* workgroups, int32_t* parts);

#ifdef __cplusplus
}
#endif
#endif /* ENF_HIP_H */
