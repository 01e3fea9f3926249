"""Host-side callers of the decoder, mirroring experiments/fitting (the "harness" rows of SURVEY.md 8):

  get_model_pde(cfg)   experiments/fitting/__init__.py:14-65   (nef, ode_model)
  inner_loop(...)      trainers/pde_trainer.py:122-235         MAML inner loop: per-signal latent SGD
  make_signal_masks    (no counterpart)                        per-signal point sets drawn from each signal's observed points
  decode(...)          trainers/pde_trainer.py:389-405         full-grid decode (chunking optional)
  decode_jacobian, divergence, curl_2d, gradient_norm  (no counterpart)  the decode's Jacobian w.r.t. the coordinates and operators on it
  decode_tangent, decode_tendency  (no counterpart)             the decode in forward mode along a latent direction; d u / d t under the latent ODE
  decode_directional, decode_material_derivative  (no counterpart)   the same pass along a query direction: c . grad u, and Du/Dt = u_t + c . grad u
  decode_second_directional, decode_laplacian, decode_hessian, decode_diffusion_residual  (no counterpart)   second derivatives in forward mode: c^T H c, the Laplacian, the Hessian, u_t - nu Lap u
  cg_solve, lm_fit_latents  (no counterpart)                   batched CG on the native Gauss-Newton product; Levenberg-Marquardt latent fits
  lm_fit_cell_averages  (no counterpart)                       the Levenberg-Marquardt fit against cell averages, on the grouped Gauss-Newton product
  lm_fit_linear_observations  (no counterpart)                 the Levenberg-Marquardt fit against a sparse linear observation operator, on its Gauss-Newton product
  cell_quadrature, decode_cell_averages, fit_cell_averages  (no counterpart)   fits against cell averages: quadrature groups in the fused tail
  inner_loop_cells, gather_cell_samples, cell_mse_torch  (no counterpart)   the inner loop on sampled cells (the trainers' cells=) and the torch-op mirrors of its kernels
  SparseObservations, cell_operator, line_integrals, decode_observations, fit_linear_observations  (no counterpart)   fits against any sparse linear observation operator (CSR): 9- / 27-point and closed cell rules, ragged or overlapping rows, line integrals
  Points (inner_loop), Cells (cells), LinearObservations (operators)  (no counterpart)   what a fit observes: one value per kind, beside its helpers; every meta-SGD fit runs inner_loop._fit_body on one, every Levenberg-Marquardt fit gauss_newton._lm_loop
  observations: observed  (no counterpart)                     the one parser of weights= / channel_weights= / cells= / cell_channel_weights=
  (imports go one way: weights <- inner_loop <- cells <- operators <- observations <- gauss_newton, trainers)
  shard_signals / allreduce_mean_  SURVEY.md 8e               meta-batch data parallelism over RCCL
  MetaSGDPDETrainer    trainers/pde_trainer.py:60-67,237-500   outer steps: nef (meta-gradient), ode, dual; val_step
  ode_models           ode_models/ponita_ode_g.py, mlp_ode.py  PonitaODEGen (fused SepGconv HIP kernels), MLPODE
  solve_latent_ode     trainers/trainer_utils/solvers.py:69-162 Euler / RK4 over the latent tuple
  NonMetaPDETrainer    trainers/nonmaml_pde_trainer.py:56-307  auto-decoder trainer: nef steps (first-order, exact), ode step, val_step
  draw_point_masks     nonmaml_pde_trainer.py:273-283          per-frame point subsets of the roll-out loss (shared by both trainers)
"""
from .model import get_model_pde
from .inner_loop import inner_loop, decode, make_masks, make_signal_masks, default_meta_sgd_lrs
from .derivatives import decode_jacobian, decode_tangent, decode_tendency, decode_directional, decode_material_derivative, divergence, curl_2d, gradient_norm
from .derivatives import decode_second_directional, decode_laplacian, decode_hessian, decode_diffusion_residual
from .gauss_newton import cg_solve, lm_fit_latents, lm_fit_cell_averages, lm_fit_linear_observations
from .cells import cell_quadrature, decode_cell_averages, fit_cell_averages, draw_cell_samples
from .cells import inner_loop_cells, gather_cell_samples, cell_mse_torch
from .operators import SparseObservations, cell_operator, line_integrals, decode_observations, fit_linear_observations
from .parallel import shard_range, allreduce_mean_, init_distributed
from .trainers import MetaSGDPDETrainer, TrainState, meta_gradients, NonMetaPDETrainer, NonMetaTrainState, draw_point_masks
from .trainers.trainer_utils import solve_latent_ode
from .ode_models import PonitaODEGen, MLPODE

__all__ = ["get_model_pde", "inner_loop", "decode", "make_masks", "make_signal_masks", "default_meta_sgd_lrs", "shard_range",
           "allreduce_mean_", "init_distributed", "MetaSGDPDETrainer", "TrainState", "meta_gradients", "NonMetaPDETrainer", "NonMetaTrainState",
           "solve_latent_ode", "PonitaODEGen", "MLPODE", "draw_point_masks", "decode_jacobian", "decode_tangent", "decode_tendency", "decode_directional", "decode_material_derivative",
           "divergence", "curl_2d", "gradient_norm", "cg_solve", "lm_fit_latents", "lm_fit_cell_averages", "cell_quadrature", "decode_cell_averages", "fit_cell_averages",
           "draw_cell_samples", "inner_loop_cells", "gather_cell_samples", "cell_mse_torch", "decode_second_directional", "decode_laplacian", "decode_hessian", "decode_diffusion_residual",
           "SparseObservations", "cell_operator", "line_integrals", "decode_observations", "fit_linear_observations", "lm_fit_linear_observations"]
