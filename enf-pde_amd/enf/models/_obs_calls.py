"""What differs between the observation kinds in the loss calls of models/__init__.py -- points, cells (grouped observations) and sparse
operators: the number of values M a signal's loss is the mean of, the names and shapes of the two weight forms, the workspace size query
and, per verb (fit step, evaluation, loss of a decode, Gauss-Newton product), the entry point with the kind's middle arguments in the
order of include/enf_hip.h.  The call bodies are the model's (_fit_step, _eval, _gn_call, _decode_loss)."""
import ctypes

from ... import _lib

_ptr = _lib.ptr


def f32(t):
    """A tensor as the library takes it: float32 and contiguous (the callers run without a graph); None stays None."""
    return t.float().contiguous() if t is not None else None


def _bad(name, t, shape):
    return f"{name} has shape {tuple(t.shape)}, expected {shape}"


class _Kind:
    wname, cwname, target_error = "obs_weight", "obs_channel_weight", ValueError      # the weights' keywords; a wrong target's error
    qweight = op = None         # cells: the factors (B, N); operator: the SparseObservations
    size_query = None           # a (desc, flags) workspace query of the kind's own, or the model's plain / deterministic workspace
    gn_size_query = None        # the same for the Gauss-Newton product, or enf_gn_workspace_bytes

    def both(self, what):
        return ValueError(f"{what}: pass {self.wname} (one weight per observation) or {self.cwname} (one per value), not both")

    def shapes(self, B, N, M, O, target, weight, cweight):
        """The one shape check: target (B, M, O) or None, qweight (B, N), weight (B, M), cweight (B, M, O)."""
        if target is not None and tuple(target.shape) != (B, M, O):
            raise self.target_error(_bad("target", target, (B, M, O)))
        if self.qweight is not None and tuple(self.qweight.shape) != (B, N):
            raise ValueError(_bad("qweight", self.qweight, (B, N)))
        if weight is not None and tuple(weight.shape) != (B, M):
            raise ValueError(_bad(self.wname, weight, (B, M)))
        if cweight is not None and tuple(cweight.shape) != (B, M, O):
            raise ValueError(_bad(self.cwname, cweight, (B, M, O)))


class Points(_Kind):
    """Every query is an observation: M = N, ``weight`` (B, N) or ``channel_weight`` (B, N, O)."""
    wname, cwname, target_error = "weight", "channel_weight", AssertionError

    def fit(self, lib, w, cw, shared, grads, errs, ws):
        if errs[0] is not None:         # the same sequence and instantiations; the tail also stores its per-query errors
            return lib.enf_fit_step_e, (*grads, *ws, _ptr(w), _ptr(cw), _ptr(errs[0]), _ptr(errs[1]))
        if cw is not None:              # the same sequence, the tail's per-channel instantiation
            return lib.enf_fit_step_cw, (*grads, *ws, _ptr(cw))
        return lib.enf_fit_step_w, (*grads, *ws, _ptr(w))

    def evaluate(self, lib, w, cw):
        return lib.enf_eval_loss, (_ptr(w), _ptr(cw))

    def gn(self, lib, w, cw):
        return lib.enf_gn_product, (_ptr(w), _ptr(cw))


class Cells(_Kind):
    """Observation m is the qweight-ed sum of ``group`` consecutive queries: M = N / group, ``obs_weight`` (B, M) or
    ``obs_channel_weight`` (B, M, O), which takes obs_weight's place in the call."""
    GROUP_SIZES = (1, 2, 4, 8, 16)

    def __init__(self, group, qweight):
        self.group, self.qweight = group, qweight

    def rows(self, N):
        if int(self.group) not in self.GROUP_SIZES:
            raise ValueError(f"group must be one of {self.GROUP_SIZES}, got {self.group}")
        if N % int(self.group):
            raise ValueError(f"{N} query points per signal: not a multiple of group = {self.group}")
        return N // int(self.group)

    def mid(self, w, cw):
        self._q = self.qweight.float().contiguous() if self.qweight is not None else None      # (kept alive with the kind)
        return int(self.group), _ptr(self._q), _ptr(cw if cw is not None else w)

    def fit(self, lib, w, cw, shared, grads, errs, ws):
        fn = lib.enf_fit_step_gc if cw is not None else lib.enf_fit_step_gs if shared else lib.enf_fit_step_g
        return fn, (*self.mid(w, cw), *grads, _ptr(errs[0]), _ptr(errs[1]), *ws)

    def evaluate(self, lib, w, cw):
        return (lib.enf_eval_loss_gc if cw is not None else lib.enf_eval_loss_g), self.mid(w, cw)

    def mse(self, lib, B, N, O, w, cw, need, det):
        fn = lib.enf_mse_value_grad_gc if cw is not None else lib.enf_mse_value_grad_g
        return fn, int(lib.enf_mse_scratch_bytes(B * (N // int(self.group)) * O, det)), self.mid(w, cw)

    def gn(self, lib, w, cw):
        return lib.enf_gn_product_g, self.mid(w, None)


class Operator(_Kind):
    """obs = A out of a sparse operator (fitting/operators.py: SparseObservations) shared by the signals: N = op.N, M = op.M,
    ``obs_weight`` (B, M) or ``obs_channel_weight`` (B, M, O).  The fit reads the transposed arrays too."""

    def __init__(self, op):
        self.op = op

    def rows(self, N):
        if N != self.op.N:
            raise ValueError(f"{N} query points per signal, the operator has {self.op.N} columns")
        return self.op.M

    def size_query(self, desc, _flags):       # the workspace of the calls: sized for the deterministic form whatever the mode
        return _lib.load().enf_obs_workspace_bytes(desc, self.op.M, _lib.ENF_FIT_DETERMINISTIC)

    def mid(self, w, cw, transposed):
        return ctypes.byref(self.op.struct(transposed=transposed)), _ptr(w), _ptr(cw)

    def fit(self, lib, w, cw, shared, grads, errs, ws):
        return lib.enf_fit_step_a, (*self.mid(w, cw, True), *grads, _ptr(errs[0]), _ptr(errs[1]), *ws)

    def evaluate(self, lib, w, cw):
        return lib.enf_eval_loss_a, self.mid(w, cw, False)

    def gn_size_query(self, desc, flags):    # the product's buffer also holds the fit step's and the evaluation's regions
        return _lib.load().enf_gn_a_workspace_bytes(desc, self.op.M, flags)

    def gn(self, lib, w, cw):
        return lib.enf_gn_product_a, self.mid(w, cw, True)

    def mse(self, lib, B, N, O, w, cw, need, det):
        return lib.enf_mse_value_grad_a, int(lib.enf_mse_a_scratch_bytes(B, self.op.M, O, 1 if need else 0, det)), self.mid(w, cw, need)
