"""What a fit observes, and the one parser of a public step's observation keywords.

A kind of observation is a value that answers, for its kind, the questions the fits and both trainers ask of their data -- how many
observations there are and how many query rows each owns, how a step's inputs are gathered, which call of the decoder is its fit
step, its evaluation, its Gauss-Newton product and the loss of a decode, and how the frames of a roll-out are sampled -- so that the
code above the decoder has one body per step instead of one per kind.  Each kind lives beside the helpers of its observation model, and
the modules import one another in one direction only:
  inner_loop.py   ``_Observed`` (what the kinds share: the decoder's calls by name, the weight keywords) and ``Points(coords)``
  cells.py        ``Cells(x, q, group, num)``, cell averages (include/enf_hip.h, "Grouped observations")
  operators.py    ``LinearObservations(x, op)``, any sparse linear operator on the decode; it answers the calls and no sampling
  this module     ``observed``, the one parser of the four keywords (weights, channel_weights, cells, cell_channel_weights): it refuses
                  what is not served and returns the observation value with the prepared LossWeights
  gauss_newton.py, trainers/   the callers
"""
from .inner_loop import Points
from .cells import Cells
from .operators import LinearObservations, SparseObservations
from .weights import LossWeights

_NO_CHANNEL_WEIGHTS_ON_CELLS = ("cells= takes per-observation weights= (M,) / (B, M) or cell_channel_weights= (M, O) / (B, M, O); "
                                "channel_weights are not served on cells")


def cell_loss_weights(weights, cell_channel_weights, B, M, O, **kw):
    """LossWeights.build for data on cells: ``weights`` per observation, ``cell_channel_weights`` per observed value; both at once is
    a ValueError that names them."""
    if weights is not None and cell_channel_weights is not None:
        raise ValueError("pass weights= (one per observation) or cell_channel_weights= (one per observed value), not both")
    return LossWeights.build(weights, cell_channel_weights, B, M, O, **kw)


def observed(coords, weights, channel_weights, cells, cell_channel_weights, B, num, O, T=None, normalize=True, frames=None, device=None,
             nef=None):
    """What every public step does first with its four keywords: (obs, lw), the observation value -- ``Points(coords)``, or ``Cells``
    of ``cells`` = (x (M G, dx), q (M G,) or None, group) checked against ``num`` = M -- and the prepared LossWeights over (B, num[, O])
    (``T``: (B, T, num[, O]); ``frames``: cut first; LossWeights.build) or None.  The refusals, in this order: on points,
    ``cell_channel_weights``; on cells ``channel_weights``, a decoder with self-attention layers (``nef``: the grouped calls are built
    for num_layers = 0), a group or a number of quadrature rows that is not served; then both weight kinds at once and wrong shapes."""
    if cells is None:
        if cell_channel_weights is not None:
            raise ValueError("cell_channel_weights= goes with cells=")
        lw = LossWeights.build(weights, channel_weights, B, num, O, T=T, normalize=normalize, device=device, frames=frames)
        return Points(coords), lw
    if isinstance(cells, LinearObservations) or any(isinstance(c, SparseObservations) for c in (cells if isinstance(cells, (tuple, list)) else ())):
        raise NotImplementedError(LinearObservations.REFUSAL)
    if channel_weights is not None:
        raise ValueError(_NO_CHANNEL_WEIGHTS_ON_CELLS)
    if getattr(nef, "num_layers", 0) > 0:
        raise NotImplementedError("cells= is built for num_layers = 0 (the fused decoder)")
    return Cells(*cells, num), cell_loss_weights(weights, cell_channel_weights, B, num, O, T=T, normalize=normalize, device=device, frames=frames)
