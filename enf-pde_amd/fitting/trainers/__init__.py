"""Host-side trainers mirroring experiments/fitting/trainers: the meta-learning trainer and the auto-decoder trainer, each with
its nef phase, latent-ODE phase and validation roll-out (the roll-out arithmetic they share: latent_ode.py)."""
from .pde_trainer import MetaSGDPDETrainer, TrainState, meta_gradients
from .nonmaml_pde_trainer import NonMetaPDETrainer, NonMetaTrainState
from .latent_ode import LatentODEMixin, draw_point_masks, sample_frames

__all__ = ["MetaSGDPDETrainer", "TrainState", "meta_gradients", "NonMetaPDETrainer", "NonMetaTrainState",
           "LatentODEMixin", "draw_point_masks", "sample_frames"]
