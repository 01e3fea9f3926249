// enf_obs.hip -- sparse linear observations (include/enf_hip.h, "Sparse linear observations"): the two products of an operator
// A (M x N), shared by the B signals of a call, with a decode that exists in memory.
//   forward     obs[b,m,o] = sum_{e in row m} val[e] out[b, col[e], o]       with the loss: r = w (obs - target), err_a, loss
//                                                                            or with weights alone: r = w obs (enf_gn_product_a)
//   transposed  d out[b,n,o] = gs * sum_{e in column n} tval[e] r[b, trow[e], o]
// Both are ONE kernel body, enf_obs_kernel: y[b,i,:] = scale * sum_e v[e] x[b, idx[e], :] over the entries [ptr[i], ptr[i + 1]), the
// forward launches with the loss epilogue behind the sum.  Memory-bound work on a few hundred kilobytes; no atomics but the scalar
// loss's one per workgroup (none in deterministic mode), no LDS but the loss's block sum.
//
// The work split depends on a row's LENGTH alone, so obs, r, err_a and d out are functions of the inputs, never of the launch:
//   length <  ENF_OBS_TREE_MIN (0 .. 64)  the lane that owns the row adds its entries in entry order, one fma each
//   length >= ENF_OBS_TREE_MIN (65 ..)    the row's whole wave: lane l adds entries l, l + 64, ... in order (fma), then the fixed xor
//                                         tree over the 64 lanes at distance 32, 16, 8, 4, 2, 1
// The transposed product never takes the long form (`tree` = 0): a column is summed in the CSC's entry order.
// A wave owns `rpw` consecutive rows (a power of two, 1 .. 64; lanes >= rpw own none and only help with long rows); the launcher picks
// rpw from the MEAN length nnz / rows, which moves rows between waves and nothing else.
// Safety: row bounds are clamped to [0, nnz] and to each other; an index outside [0, ncols) is skipped before it becomes an offset.
// Offsets into the (B, ., O) tensors are 64-bit.
#include <hip/hip_runtime.h>
#include <climits>
#include "enf_launch.h"

// CH channels of one row of a (., O) tensor, of which the first kc exist (the last pass of an O that is no multiple of CH).  VEC: one
// 16-byte access (kc == CH == 4; the launcher vouches for O % 4 == 0 and the alignment); otherwise one access per channel.
template <int CH> struct ObsVec { float v[CH]; };
template <int CH, bool VEC> __device__ __forceinline__ ObsVec<CH> obs_load(const float* __restrict__ p, int kc) {
  ObsVec<CH> r;
  if constexpr (VEC) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < CH; ++k) r.v[k] = k < kc ? p[k] : 0.f;
  }
  return r;
}
template <int CH, bool VEC> __device__ __forceinline__ void obs_store(float* __restrict__ p, const ObsVec<CH>& r, int kc) {
  if constexpr (VEC) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else {
#pragma unroll
    for (int k = 0; k < CH; ++k)
      if (k < kc) p[k] = r.v[k];
  }
}

struct ObsArgs {
  const int32_t* ptr; const int32_t* idx; const float* v;      // the operator in the orientation of this product
  long long nnz;
  int rows, ncols, B, O;        // y is (B, rows, O), x is (B, ncols, O)
  int rpw, tree;                // tree: rows of at least ENF_OBS_TREE_MIN entries take the wave form (never in the transposed product)
  const float* x; float* y; float scale;      // y: the plain product's result (unused with LOSS)
  // LOSS: target (B, rows, O); oweight (B, rows) | cweight (B, rows, O) | neither; r, err NULL or written; loss / part as mse_block_sum
  const float* target; const float* oweight; const float* cweight;
  float* r; float* err; float* loss; float* part; float inv_n;
};

// s += the entries [lo, hi) at stride `step` from `lo + first`, in order: one fma per entry and channel.  An entry's index and factor
// are read once for the CH channels of a pass.
template <int CH, bool VEC>
__device__ __forceinline__ void obs_accumulate(const ObsArgs& A, const float* __restrict__ xb, int lo, int hi, int first, int step, int o,
                                               int kc, ObsVec<CH>& s) {
  for (long long e = (long long)lo + first; e < hi; e += step) {
    const int c = A.idx[e];
    if ((unsigned)c >= (unsigned)A.ncols) continue;
    const float f = A.v[e];
    const ObsVec<CH> t = obs_load<CH, VEC>(xb + (size_t)c * (size_t)A.O + o, kc);
#pragma unroll
    for (int k = 0; k < CH; ++k) s.v[k] = fmaf(f, t.v[k], s.v[k]);
  }
}

// WEIGH (the Gauss-Newton product's forward, enf_launch_obs_weigh): weights without a target -- r = (w > 0 ? w y : 0) stored in the
// sum's pass; no loss, no atomic, no LDS.  An instantiation of its own: the other two keep their code.
template <int CH, bool VEC, bool LOSS, bool WEIGH = false>
__global__ __launch_bounds__(256) void enf_obs_kernel(ObsArgs A) {
  static_assert(!(LOSS && WEIGH), "the weighted product has no target");
  const int lane = threadIdx.x & 63;
  const long long items = (long long)A.B * A.rows;
  const long long waves = (items + A.rpw - 1) / A.rpw;
  float ls = 0.f;                                            // the thread's share of the loss
  for (long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); wv < waves; wv += (long long)gridDim.x * 4) {      // wave-uniform
    const long long i = wv * A.rpw + lane;                   // the (signal, row) this lane owns
    const bool own = lane < A.rpw && i < items;
    int b = 0, row = 0, lo = 0, hi = 0;
    if (own) {
      b = (int)(i / A.rows);
      row = (int)(i - (long long)b * A.rows);
      const long long p0 = A.ptr[row], p1 = A.ptr[row + 1];
      lo = (int)(p0 < 0 ? 0 : (p0 > A.nnz ? A.nnz : p0));
      hi = (int)(p1 < lo ? lo : (p1 > A.nnz ? A.nnz : p1));
    }
    const bool is_long = own && A.tree && hi - lo >= ENF_OBS_TREE_MIN;
    const unsigned long long longs = __ballot(is_long);
    const float* __restrict__ xb = A.x + (size_t)b * (size_t)A.ncols * (size_t)A.O;
    float e_acc = 0.f;                                       // err[b, row]: the channels' shares in channel order
    for (int o = 0; o < A.O; o += CH) {
      const int kc = A.O - o < CH ? A.O - o : CH;             // the channels of this pass
      ObsVec<CH> s;
#pragma unroll
      for (int k = 0; k < CH; ++k) s.v[k] = 0.f;
      if (own && !is_long) obs_accumulate<CH, VEC>(A, xb, lo, hi, 0, 1, o, kc, s);
      for (unsigned long long todo = longs; todo; todo &= todo - 1) {      // the wave's long rows, one after the other, all 64 lanes each
        const int src = __ffsll((long long)todo) - 1;
        const int slo = __shfl(lo, src, 64), shi = __shfl(hi, src, 64), sb = __shfl(b, src, 64);
        ObsVec<CH> t;
#pragma unroll
        for (int k = 0; k < CH; ++k) t.v[k] = 0.f;
        obs_accumulate<CH, VEC>(A, A.x + (size_t)sb * (size_t)A.ncols * (size_t)A.O, slo, shi, lane, 64, o, kc, t);
#pragma unroll
        for (int k = 0; k < CH; ++k) {
          for (int d = 32; d > 0; d >>= 1) t.v[k] += __shfl_xor(t.v[k], d, 64);
          if (lane == src) s.v[k] = t.v[k];
        }
      }
      if (!own) continue;
      const size_t at = (size_t)i * (size_t)A.O + o;
      if constexpr (LOSS) {
        const ObsVec<CH> tg = obs_load<CH, VEC>(A.target + at, kc);
        ObsVec<CH> wv4{};
        if (A.cweight) wv4 = obs_load<CH, VEC>(A.cweight + at, kc);
        const float w1 = A.oweight ? A.oweight[i] : 1.f;
        ObsVec<CH> rr;
#pragma unroll
        for (int k = 0; k < CH; ++k) {
          rr.v[k] = 0.f;
          if (k < kc) {
            const float w = A.cweight ? wv4.v[k] : w1;
            const float dd = w > 0.f ? s.v[k] - tg.v[k] : 0.f;             // weight 0: the target is never used in arithmetic
            rr.v[k] = w * dd;
            ls = fmaf(rr.v[k], dd, ls);
            e_acc = fmaf(rr.v[k], dd, e_acc);
          }
        }
        if (A.r) obs_store<CH, VEC>(A.r + at, rr, kc);
      } else if constexpr (WEIGH) {
        ObsVec<CH> wv4{};
        if (A.cweight) wv4 = obs_load<CH, VEC>(A.cweight + at, kc);
        const float w1 = A.oweight ? A.oweight[i] : 1.f;
        ObsVec<CH> rr;
#pragma unroll
        for (int k = 0; k < CH; ++k) {
          const float w = A.cweight ? wv4.v[k] : w1;
          rr.v[k] = (k < kc && w > 0.f) ? w * s.v[k] : 0.f;               // weight 0: a select, the sum under it is not used
        }
        obs_store<CH, VEC>(A.r + at, rr, kc);
      } else {
#pragma unroll
        for (int k = 0; k < CH; ++k) s.v[k] *= A.scale;
        obs_store<CH, VEC>(A.y + at, s, kc);
      }
    }
    if (LOSS && own && A.err) A.err[i] = e_acc;
  }
  if constexpr (LOSS) {
    if (!A.loss) return;                                     // (uniform: the whole grid)
    // the block's sum of the threads' shares, times inv_n: stored in part[block] (deterministic mode) or added with one atomic
    __shared__ float red[4];
    for (int d = 32; d > 0; d >>= 1) ls += __shfl_xor(ls, d, 64);
    if (lane == 0) red[threadIdx.x >> 6] = ls;
    __syncthreads();
    if (threadIdx.x == 0) {
      const float t = (red[0] + red[1] + red[2] + red[3]) * A.inv_n;
      if (A.part) A.part[blockIdx.x] = t;
      else atomicAdd(A.loss, t);
    }
  }
}

// rows per wave from the mean row length: full waves of one-lane rows while rows are short, one wave per row once the mean is long
static int obs_rows_per_wave(long long nnz, int rows, bool tree) {
  if (!tree) return 64;
  const long long mean = nnz / (rows > 0 ? rows : 1);
  return mean <= 16 ? 64 : mean <= 32 ? 16 : mean < ENF_OBS_TREE_MIN ? 4 : 1;
}
static unsigned obs_blocks(long long items, int rpw) {
  const long long waves = (items + rpw - 1) / rpw, blocks = (waves + 3) / 4;
  return (unsigned)(blocks > ENF_OBS_MAX_BLOCKS ? ENF_OBS_MAX_BLOCKS : (blocks < 1 ? 1 : blocks));
}
// the 16-byte form: whole passes of four channels and every tensor the kernel touches per channel aligned (NULL counts as aligned)
static bool obs_vec4(const ObsArgs& A) {
  auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  return A.O % 4 == 0 && al(A.x) && al(A.y) && al(A.r) && al(A.target) && al(A.cweight);
}
// one channel per pass at O == 1, four otherwise (scalar accesses, the last pass short), the 16-byte form where obs_vec4 holds
template <bool LOSS, bool WEIGH = false> static int obs_launch(const ObsArgs& A, unsigned blocks, hipStream_t st) {
  if (obs_vec4(A)) hipLaunchKernelGGL((enf_obs_kernel<4, true, LOSS, WEIGH>), dim3(blocks), dim3(256), 0, st, A);
  else if (A.O > 1) hipLaunchKernelGGL((enf_obs_kernel<4, false, LOSS, WEIGH>), dim3(blocks), dim3(256), 0, st, A);
  else hipLaunchKernelGGL((enf_obs_kernel<1, false, LOSS, WEIGH>), dim3(blocks), dim3(256), 0, st, A);
  return hipGetLastError() == hipSuccess ? ENF_OK : ENF_ELAUNCH;
}

// y (B, rows, O) = scale * (the operator's rows applied to x (B, ncols, O)); tree: long rows take the wave form, else entry order
int enf_launch_obs_product(const int32_t* ptr, const int32_t* idx, const float* v, long long nnz, int rows, int ncols, int B, int O,
                           const float* x, float* y, float scale, bool tree, hipStream_t st) {
  ObsArgs A{};
  A.ptr = ptr; A.idx = idx; A.v = v; A.nnz = nnz; A.rows = rows; A.ncols = ncols; A.B = B; A.O = O;
  A.tree = tree ? 1 : 0; A.rpw = obs_rows_per_wave(nnz, rows, tree);
  A.x = x; A.y = y; A.scale = scale;
  return obs_launch<false>(A, obs_blocks((long long)B * rows, A.rpw), st);
}

// the forward product with the loss (kernel 1): r = w (obs - target) (NULL or stored), err_a (NULL or stored), *loss += the mean weighted
// squared error -- through `part` (ENF_OBS_MAX_BLOCKS floats) and enf_launch_loss_sum where part != NULL.  (obs alone: enf_obs_apply.)
int enf_launch_obs_loss(const EnfSparseObs& op, int N, int B, int O, const float* out, const float* target, const float* oweight,
                        const float* cweight, float* r, float* err_a, float* loss, float* part, hipStream_t st) {
  ObsArgs A{};
  A.ptr = op.row_ptr; A.idx = op.col; A.v = op.val; A.nnz = op.nnz; A.rows = op.M; A.ncols = N; A.B = B; A.O = O;
  A.tree = 1; A.rpw = obs_rows_per_wave(op.nnz, op.M, true);
  A.x = out; A.scale = 1.f;
  A.target = target; A.oweight = oweight; A.cweight = cweight; A.r = r; A.err = err_a; A.loss = loss; A.part = part;
  A.inv_n = 1.0f / ((float)B * (float)op.M * (float)O);
  const unsigned blocks = obs_blocks((long long)B * op.M, A.rpw);
  if (int rc = obs_launch<true>(A, blocks, st)) return rc;
  return loss && part ? enf_launch_loss_sum(part, (int)blocks, loss, st) : ENF_OK;
}

// the forward product with weights and no target (the Gauss-Newton product): r (B, M, O) = (w > 0 ? w (A x) : 0), w = oweight (B, M),
// cweight (B, M, O) or 1; kernel 1's work split and order of sums
int enf_launch_obs_weigh(const EnfSparseObs& op, int N, int B, int O, const float* x, const float* oweight, const float* cweight, float* r,
                         hipStream_t st) {
  ObsArgs A{};
  A.ptr = op.row_ptr; A.idx = op.col; A.v = op.val; A.nnz = op.nnz; A.rows = op.M; A.ncols = N; A.B = B; A.O = O;
  A.tree = 1; A.rpw = obs_rows_per_wave(op.nnz, op.M, true);
  A.x = x; A.scale = 1.f;
  A.oweight = oweight; A.cweight = cweight; A.r = r;
  return obs_launch<false, true>(A, obs_blocks((long long)B * op.M, A.rpw), st);
}

// the transposed product (kernel 2): d out (B, N, O) = gs * A^T r, every element written, a column in the CSC's entry order
int enf_launch_obs_transpose(const EnfSparseObs& op, int N, int B, int O, const float* r, float gs, float* dout, hipStream_t st) {
  return enf_launch_obs_product(op.col_ptr, op.trow, op.tval, op.nnz, N, op.M, B, O, r, dout, gs, false, st);
}

// what every entry point checks of an operator; `transposed`: the CSC is needed too
bool enf_obs_op_ok(const EnfSparseObs* op, bool transposed) {
  if (!op || op->M < 1 || op->nnz < 0 || op->nnz > (long long)INT_MAX || !op->row_ptr) return false;
  if (op->nnz > 0 && (!op->col || !op->val)) return false;
  if (transposed && (!op->col_ptr || (op->nnz > 0 && (!op->trow || !op->tval)))) return false;
  return true;
}

extern "C" int enf_obs_apply(const float* out, int32_t B, int32_t N, int32_t O, const EnfSparseObs* op, float* obs, void* stream) {
  if (!out || !obs || B < 1 || N < 1 || O < 1 || !enf_obs_op_ok(op, false)) return ENF_EINVAL;
  return enf_launch_obs_product(op->row_ptr, op->col, op->val, op->nnz, op->M, N, B, O, out, obs, 1.f, true, (hipStream_t)stream);
}

// scratch of enf_mse_value_grad_a: [r: B M O floats, with dout | the loss partials, deterministic mode]
static size_t obs_mse_r_bytes(int B, int M, int O) { return enf_align(sizeof(float) * (size_t)B * (size_t)M * (size_t)O); }
extern "C" size_t enf_mse_a_scratch_bytes(int32_t B, int32_t M, int32_t O, int want_dout, unsigned flags) {
  if (B < 1 || M < 1 || O < 1 || (flags & ~ENF_MSE_DETERMINISTIC)) return 0;
  return (want_dout ? obs_mse_r_bytes(B, M, O) : 0) + ((flags & ENF_MSE_DETERMINISTIC) ? enf_align(sizeof(float) * ENF_OBS_MAX_BLOCKS) : 0);
}

extern "C" int enf_mse_value_grad_a(const float* out, const float* target, int32_t B, int32_t N, int32_t O, const EnfSparseObs* op,
                                    const float* oweight, const float* cweight, float grad_scale, float* dout, float* loss, float* err_a,
                                    void* scratch, size_t scratch_bytes, unsigned flags, void* stream) {
  if (!out || !target || !loss || B < 1 || N < 1 || O < 1 || (oweight && cweight) || (flags & ~ENF_MSE_DETERMINISTIC) ||
      !enf_obs_op_ok(op, dout != nullptr))
    return ENF_EINVAL;
  const size_t need = enf_mse_a_scratch_bytes(B, op->M, O, dout != nullptr, flags);
  if (need && !scratch) return ENF_EINVAL;
  if (scratch_bytes < need) return ENF_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* r = dout ? (float*)scratch : nullptr;
  float* part = (flags & ENF_MSE_DETERMINISTIC) ? reinterpret_cast<float*>((char*)scratch + (dout ? obs_mse_r_bytes(B, op->M, O) : 0)) : nullptr;
  if (int rc = enf_launch_obs_loss(*op, N, B, O, out, target, oweight, cweight, r, err_a, loss, part, st)) return rc;
  if (!dout) return ENF_OK;
  const float gs = 2.0f * (1.0f / ((float)B * (float)op->M * (float)O)) * grad_scale;
  return enf_launch_obs_transpose(*op, N, B, O, r, gs, dout, st);
}
