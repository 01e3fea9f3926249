"""Sparse linear observation operators (include/enf_hip.h, "Sparse linear observations"; no counterpart in the reference).

An observation is a fixed linear functional of the decoded field, obs[m] = sum_e val[e] u(x[col[e]]) over the entries of row m of an
operator A (M x N) on N query points.  The grouped layout of fitting/cells.py is the special case of equal, consecutive, disjoint rows;
here rows may have any length (0 .. N), share query points and refer to them in any order: 9- and 27-point cell rules, closed rules
that share nodes between neighbouring cells, triangles, footprints of changing size, increments, line integrals, conserved totals.

``SparseObservations`` holds the CSR (forward product) and the CSC (transposed product) of one operator, validated on the host when it
is built; ``LinearObservations`` is the observation value of this kind (inner_loop.py: _Observed) and ``check_operator`` the one copy
of the argument checks.  ``cell_operator`` and ``line_integrals`` build (x, op) pairs; ``decode_observations`` and ``fit_linear_observations`` run a
decoder against them (nef.mse_value_and_operator_grads: the pair and tail kernels of the point fit with the two products of
csrc/enf_obs.hip between the tail's forward and backward)."""
import numpy as np
import torch

from .. import _lib
from .cells import _edges, _rule_1d, check_obs_weights
from .inner_loop import _Observed, _batched, _fit_given

CLOSED_RULES = ("trapezoid", "simpson")


class SparseObservations:
    """One operator A (M x N): ``row_ptr`` (M + 1), ``col`` (nnz), ``val`` (nnz) -- the CSR, entries of a row in the order given -- and
    ``col_ptr`` (N + 1), ``trow`` (nnz), ``tval`` (nnz), the same entries sorted by column with a STABLE sort, so that a column keeps its
    entries in CSR order.  Built once from host arrays; int32 / float32 tensors on ``device``; ``val64`` keeps the factors in fp64 for
    ``to_dense``.  ValueError for: M or N < 1, pointers that do not start at 0, decrease or do not end at nnz, a column outside
    [0, N), a factor that is not finite, nnz >= 2^31."""

    def __init__(self, row_ptr, col, val, N, device=None):
        row_ptr = np.asarray(row_ptr)
        col = np.asarray(col)
        val = np.asarray(val, dtype=np.float64)
        if row_ptr.ndim != 1 or row_ptr.size < 2 or int(N) < 1:
            raise ValueError("an operator needs M >= 1 rows (row_ptr of M + 1 entries) and N >= 1 columns")
        if col.ndim != 1 or val.shape != col.shape:
            raise ValueError(f"col {col.shape} and val {val.shape} must be 1-D and equally long")
        if not (np.issubdtype(row_ptr.dtype, np.integer) and (col.size == 0 or np.issubdtype(col.dtype, np.integer))):
            raise ValueError("row_ptr and col must hold integers")
        nnz = int(col.size)
        if nnz >= 2 ** 31:
            raise ValueError("indices are int32: nnz must be below 2^31")
        if int(row_ptr[0]) != 0 or int(row_ptr[-1]) != nnz or np.any(np.diff(row_ptr) < 0):
            raise ValueError("row_ptr must start at 0, never decrease and end at nnz")
        if nnz and (col.min() < 0 or col.max() >= int(N)):
            raise ValueError(f"col must lie in [0, {int(N)})")
        with np.errstate(over="ignore"):
            finite = np.all(np.isfinite(val)) and np.all(np.isfinite(val.astype(np.float32)))
        if not finite:
            raise ValueError("val must be finite (in float32)")
        self.M, self.N, self.nnz = int(row_ptr.size - 1), int(N), nnz
        rows = np.repeat(np.arange(self.M, dtype=np.int64), np.diff(row_ptr).astype(np.int64))
        order = np.argsort(col, kind="stable")
        col_ptr = np.zeros(self.N + 1, dtype=np.int64)
        np.cumsum(np.bincount(col.astype(np.int64), minlength=self.N), out=col_ptr[1:])
        self.val64 = val.copy()
        t = lambda v, dt: torch.tensor(np.ascontiguousarray(v), dtype=dt, device=device)
        self.row_ptr, self.col, self.val = t(row_ptr, torch.int32), t(col, torch.int32), t(val, torch.float32)
        self.col_ptr, self.trow, self.tval = t(col_ptr, torch.int32), t(rows[order], torch.int32), t(val[order], torch.float32)
        self._order = order

    # ---- constructors
    @classmethod
    def from_coo(cls, rows, cols, vals, M, N, device=None):
        """Entries (rows[e], cols[e], vals[e]) kept as given -- nothing is summed, a repeated (row, column) stays two entries; a row keeps
        its entries in the order they appear in."""
        rows, cols = np.asarray(rows), np.asarray(cols)
        if rows.ndim != 1 or rows.shape != cols.shape or rows.shape != np.asarray(vals).shape:
            raise ValueError("rows, cols and vals must be 1-D and equally long")
        if int(M) < 1:
            raise ValueError("an operator needs M >= 1 rows")
        if rows.size and not (np.issubdtype(rows.dtype, np.integer) and np.issubdtype(cols.dtype, np.integer)):
            raise ValueError("rows and cols must hold integers")
        if rows.size and (rows.min() < 0 or rows.max() >= int(M)):
            raise ValueError(f"rows must lie in [0, {int(M)})")
        order = np.argsort(rows, kind="stable")
        row_ptr = np.zeros(int(M) + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows.astype(np.int64), minlength=int(M)), out=row_ptr[1:])
        return cls(row_ptr, cols[order].astype(np.int64), np.asarray(vals, dtype=np.float64)[order], N, device=device)

    @classmethod
    def from_groups(cls, sizes, q, device=None):
        """Ragged consecutive groups: row m owns the next sizes[m] query rows, with the factors ``q`` (sum(sizes),) -- or None for the
        plain mean 1 / sizes[m].  Equal sizes give the grouped layout of fitting/cells.py."""
        sizes = np.asarray(sizes, dtype=np.int64)
        if sizes.ndim != 1 or sizes.size < 1 or np.any(sizes < 0):
            raise ValueError("sizes must be a 1-D array of group sizes >= 0")
        N = int(sizes.sum())
        if q is None:
            q = np.repeat(1.0 / np.maximum(sizes, 1), sizes)
        q = q.detach().cpu().numpy() if torch.is_tensor(q) else np.asarray(q)
        if q.shape != (N,):
            raise ValueError(f"q has shape {q.shape}, expected {(N,)}")
        return cls(np.concatenate([[0], np.cumsum(sizes)]), np.arange(N, dtype=np.int64), q, N, device=device)

    # ---- views
    def to(self, device):
        """The same operator with its arrays on ``device``."""
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        for k in ("row_ptr", "col", "val", "col_ptr", "trow", "tval"):
            setattr(new, k, getattr(self, k).to(device))
        return new

    @property
    def device(self):
        return self.val.device

    def to_dense(self, transposed=False, dtype=np.float64):
        """A (M, N) as a host array from the CSR -- or, ``transposed``, A^T (N, M) from the CSC; repeated entries add.  fp64 factors
        with dtype float64, the float32 ones the kernels read otherwise.  For tests and small problems."""
        exact = np.dtype(dtype) == np.float64
        if transposed:
            ptr, idx = self.col_ptr.cpu().numpy(), self.trow.cpu().numpy()
            v = self.val64[self._order] if exact else self.tval.cpu().numpy()
            out = np.zeros((self.N, self.M), dtype=dtype)
        else:
            ptr, idx = self.row_ptr.cpu().numpy(), self.col.cpu().numpy()
            v = self.val64 if exact else self.val.cpu().numpy()
            out = np.zeros((self.M, self.N), dtype=dtype)
        np.add.at(out, (np.repeat(np.arange(ptr.size - 1), np.diff(ptr)), idx), v.astype(dtype))
        return out

    def struct(self, transposed=True):
        """The operator as the library takes it (keep ``self`` alive while the call runs)."""
        if not self.val.is_cuda:
            raise _lib.EnfError("SparseObservations: the arrays are not on a GPU; move them with .to(device)")
        s = _lib.EnfSparseObs()
        s.M, s.nnz = self.M, self.nnz
        s.row_ptr, s.col, s.val = self.row_ptr.data_ptr(), self.col.data_ptr(), self.val.data_ptr()
        if transposed:
            s.col_ptr, s.trow, s.tval = self.col_ptr.data_ptr(), self.trow.data_ptr(), self.tval.data_ptr()
        return s


def _closed_rule_1d(k, rule):
    """Positions in [0, 1] and weights that sum to 1 of a k-point CLOSED rule (both end points are nodes)."""
    k = int(k)
    if rule == "trapezoid":
        if k < 2:
            raise ValueError(f"the trapezoid rule needs k >= 2 points per axis, got {k}")
        w = np.ones(k)
        w[0] = w[-1] = 0.5
        return np.arange(k) / (k - 1.0), w / (k - 1.0)
    if k < 3 or k % 2 == 0:
        raise ValueError(f"Simpson's rule needs an odd k >= 3 points per axis, got {k}")
    w = np.where(np.arange(k) % 2 == 1, 4.0, 2.0)
    w[0] = w[-1] = 1.0
    return np.arange(k) / (k - 1.0), w / (3.0 * (k - 1.0))


def cell_operator(cells, k, rule="gauss", kind="cartesian", dtype=torch.float32, device=None):
    """The means over every cell of a tensor-product grid as an operator: ``cell_quadrature``'s arguments, any k >= 1, and two more rules.

    rule : "gauss" / "midpoint" -- open rules, every cell owns its k ** dx points: x (M k^dx, dx) and the factors are those of
           cell_quadrature, bit for bit, where it serves k;  "trapezoid" (k >= 2) / "simpson" (odd k >= 3) -- closed composite rules on
           k - 1 sub-intervals per cell and axis, whose end nodes neighbouring cells SHARE: every axis has cells (k - 1) + 1 nodes, x
           holds their tensor product in C order, and a row refers to its k ** dx nodes by index.
    kind : "cartesian", or "sphere" (two axes (phi, theta): the factors carry sin(theta) and are normalised per cell).
    Returns (x (N, dx), op) with op.M = the number of cells, rows in C order over the axes; every row's factors sum to 1."""
    edges = _edges(cells)
    dx, k = len(edges), int(k)
    if kind not in ("cartesian", "sphere"):
        raise ValueError(f"kind must be 'cartesian' or 'sphere', got {kind!r}")
    if kind == "sphere" and dx != 2:
        raise ValueError("kind='sphere' needs two axes, (phi, theta)")
    closed = rule in CLOSED_RULES
    nodes, facs, index = [], [], []          # per axis: (cells, k) node positions, factors and node numbers
    for e in edges:
        c = e.size - 1
        if closed:
            t, w = _closed_rule_1d(k, rule)
            pos = e[:-1, None] + (e[1:] - e[:-1])[:, None] * t[None, :]
            pos[:-1, -1] = pos[1:, 0]                                    # a shared node has ONE position: its right cell's first
            pos[-1, -1] = e[-1]
            index.append(np.arange(c)[:, None] * (k - 1) + np.arange(k)[None, :])
        else:
            t, w = _rule_1d(k, rule)
            mid, half = 0.5 * (e[1:] + e[:-1]), 0.5 * (e[1:] - e[:-1])
            pos = mid[:, None] + half[:, None] * t[None, :]
        nodes.append(pos)
        facs.append(np.broadcast_to(w[None, :], pos.shape).copy())
    if kind == "sphere":
        facs[1] = facs[1] * np.sin(nodes[1])
        facs[1] = facs[1] / facs[1].sum(axis=1, keepdims=True)
    counts = [n.shape[0] for n in nodes]
    M, G = int(np.prod(counts)), k ** dx
    grids = np.meshgrid(*[np.arange(c) for c in counts], *[np.arange(k)] * dx, indexing="ij")
    q = np.ones(grids[0].shape)
    for ax in range(dx):
        q = q * facs[ax][grids[ax], grids[dx + ax]]
    q = q.reshape(M * G)
    if not closed:
        x = np.stack([nodes[ax][grids[ax], grids[dx + ax]] for ax in range(dx)], axis=-1).reshape(M * G, dx)
        return torch.tensor(x, dtype=dtype, device=device), SparseObservations.from_groups(np.full(M, G), q, device=device)
    per_axis = [c * (k - 1) + 1 for c in counts]
    axis_pos = []
    for ax in range(dx):
        p = np.empty(per_axis[ax])
        p[index[ax]] = nodes[ax]
        axis_pos.append(p)
    x = np.stack(np.meshgrid(*axis_pos, indexing="ij"), axis=-1).reshape(-1, dx)
    col = np.ravel_multi_index([index[ax][grids[ax], grids[dx + ax]] for ax in range(dx)], per_axis).reshape(M * G)
    op = SparseObservations(np.arange(M + 1, dtype=np.int64) * G, col, q, x.shape[0], device=device)
    return torch.tensor(x, dtype=dtype, device=device), op


def line_integrals(starts, ends, k, rule="gauss", dtype=torch.float32, device=None):
    """Line integrals along straight rays: ``starts``, ``ends`` (R, dx); every ray gets k nodes of ``rule`` ("gauss", "midpoint",
    "trapezoid", "simpson") and its factors carry the segment LENGTH, so that obs[r] approximates the integral of the field from
    starts[r] to ends[r] (exact for polynomials along the ray up to the rule's degree).  Nodes are not shared between rays.
    Returns (x (R k, dx), op) with op.M = R."""
    s, e = np.asarray(starts, dtype=np.float64), np.asarray(ends, dtype=np.float64)
    if s.ndim != 2 or s.shape != e.shape or s.shape[0] < 1:
        raise ValueError(f"starts {s.shape} and ends {e.shape} must both be (R, dx) with R >= 1")
    if rule in CLOSED_RULES:
        t, w = _closed_rule_1d(k, rule)
    else:
        t, w = _rule_1d(int(k), rule)
        t = 0.5 * (t + 1.0)
    R, k = s.shape[0], int(k)
    x = s[:, None, :] + (e - s)[:, None, :] * t[None, :, None]
    q = np.linalg.norm(e - s, axis=1)[:, None] * w[None, :]
    op = SparseObservations.from_groups(np.full(R, k), q.reshape(R * k), device=device)
    return torch.tensor(x.reshape(R * k, -1), dtype=dtype, device=device), op


def check_operator(x, op, B=None, target=None, target_wrong=None, shared=False):
    """The one check of query points and targets against an operator; ValueError otherwise, x first.
    ``shared``: ``x`` is the grid the signals share and must be (N, dx) with N = op.N; else it is that or a batch (B, N, dx).
    ``target``: must be (B, op.M, O); ``target_wrong``: the caller's words for it, a format of {shape}, {got}, {B} and {M}."""
    if shared:
        if x.dim() != 2 or x.shape[0] != op.N:
            raise ValueError(f"x must be (N, dx) = ({op.N}, dx) for this operator, got {tuple(x.shape)}")
    else:
        if x.dim() not in (2, 3):
            raise ValueError(f"x must be (N, dx) or (B, N, dx), got {tuple(x.shape)}")
        if x.dim() == 3 and x.shape[0] != B:
            raise ValueError(f"x holds {x.shape[0]} signals, the latents {B}")
        if x.shape[-2] != op.N:
            raise ValueError(f"x holds {x.shape[-2]} query points, the operator has {op.N} columns")
    if target is not None and (target.dim() != 3 or target.shape[0] != B or target.shape[1] != op.M):
        raise ValueError(target_wrong.format(shape=tuple(target.shape), got=target.shape[1] if target.dim() > 1 else "no", B=B, M=op.M))


class LinearObservations(_Observed):
    """Linear functionals of the field given by a sparse operator (SparseObservations) on the query points ``x`` (N, dx): observation m
    owns the entries of row m, of any number, shared or not.  It answers what the fits on an operator ask -- the step, the evaluation,
    the Gauss-Newton product and its buffer (fit_linear_observations, gauss_newton.lm_fit_linear_observations) -- and nothing of what
    sampling needs: there is no gather of rows, and ``observed`` and the trainers' steps refuse it."""
    WEIGHT_KW = ("obs_weight", "obs_channel_weight")
    STEP, EVAL, PRODUCT = "mse_value_and_operator_grads", "eval_operator_loss", "gn_operator_product"
    REFUSAL = ("a linear observation operator is served by fitting.fit_linear_observations and fitting.lm_fit_linear_observations only: "
               "the trainers' steps and inner_loop sampling do not take it yet")

    def __init__(self, x, op):
        check_operator(x, op, shared=True)
        self.x, self.op, self.num = x, op, op.M

    def _call(self, nef, name, params, xs, qs, p, a, window, *ys, **kw):
        return getattr(nef, name)(params, xs, p, a, window, *ys, self.op, **kw)

    def hints(self, channel):
        return False

    def reserve_kw(self):
        return {"op": self.op}


@torch.no_grad()
def decode_observations(nef, params, x, op, p, a, window):
    """obs (B, M, O) = A out of a decode at the operator's query points: nef.apply followed by the forward product (enf_obs_apply).
    x (N, dx) or (B, N, dx)."""
    B = p.shape[0]
    check_operator(x, op, B)
    xb, _ = _batched(x, None, B)
    out = nef.apply(params, xb, p, a, window).float().contiguous()
    obs = torch.empty((B, op.M, out.shape[2]), device=out.device, dtype=torch.float32)
    s = op.struct(transposed=False)
    _lib.launch(out.device, _lib.load().enf_obs_apply, _lib.ptr(out), B, op.N, out.shape[2], s, _lib.ptr(obs), _lib.stream(out.device))
    return obs


def fit_linear_observations(nef, params, latents0, lrs, x, op, targets, steps, obs_weight=None, obs_channel_weight=None,
                            optimize_gaussian_window=False, per_signal_loss=False):
    """Fit per-signal latents to linear observations of the field with ``steps`` steps of the inner loop's meta-SGD rule -- the loop of
    fit_cell_averages on an operator: every step sees all M observations and is one nef.mse_value_and_operator_grads, the final loss is
    nef.eval_operator_loss at the fitted latents (no decode is returned).

    latents0, lrs : as for inner_loop (leading dimension 1);  x: the operator's query points (N, dx), shared by the signals
    op            : a SparseObservations with N columns, on the targets' device
    targets       : (B, M, O);  obs_weight: None or (B, M), finite and >= 0 -- an observation of weight 0 does not exist and its
                    target may be NaN;  obs_channel_weight: None or (B, M, O), one weight per observed value (both: ValueError)
    Returns (loss at the fitted latents, latents dict with leading dimension B), with ``per_signal_loss`` followed by loss_b
    (steps + 1, B)."""
    B = targets.shape[0]
    check_operator(x, op, B, targets, "targets hold {got} observations, the operator {M}", shared=True)
    w, per_value = check_obs_weights("fit_linear_observations", obs_weight, obs_channel_weight, targets.shape)
    dev = targets.device
    given = (_batched(x.to(dev), None, B)[0], None, targets.float(), w)         # the caller's tensors themselves, a stride-0 batch
    return _fit_given(nef, params, LinearObservations.given(op=op), latents0, lrs, lambda s: given, B, int(steps), dev, per_value,
                      optimize_gaussian_window, per_signal_loss)
