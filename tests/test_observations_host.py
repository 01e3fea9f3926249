"""The refusals of the one argument parser (fitting/observations.py: observed), seen through every public step that takes the four
keywords weights / channel_weights / cells / cell_channel_weights: each is a ValueError raised before anything reaches the decoder."""
from types import SimpleNamespace as NS

import pytest
import torch

from enf_pde_amd.fitting.trainers import MetaSGDPDETrainer, NonMetaPDETrainer, meta_gradients


class _NoDecoder:
    """A decoder that must not be reached: every call, every attribute but ``num_layers``, is an error."""
    num_layers = 0

    def __getattr__(self, name):
        raise AssertionError(f"the decoder was reached ({name}) before the refusal")


X = torch.zeros(16, 2)                                  # 4 cells of 4 quadrature rows
TRAJ = torch.zeros(2, 12, 4, 2)
IDX = torch.zeros(2, dtype=torch.long)
MASKS = torch.zeros(2, 3, dtype=torch.long)
STATE = NS(params={"nef": None, "ode_params": {"w": torch.zeros(1)}, "meta_sgd_lrs": {}, "autodecoder": {"params": {}}}, rng=None)


def _maml():
    conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=0.0, learning_rate_ode=1e-3),
              meta=NS(learning_rate_meta_sgd=1e-2, num_inner_steps=2, noise_pos_inner_loop=0.0), nef=NS(optimize_gaussian_window=False),
              training=NS(max_num_sampled_points=8), node=NS(dt=1, method="euler"), dataset=NS(traj_len_train=3, traj_len_out_horizon=2))
    return MetaSGDPDETrainer(conf, _NoDecoder(), None, torch.zeros(4, 2), ode_model=None)


def _autodec():
    conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=1e-2), nef=NS(optimize_gaussian_window=False),
              training=NS(max_num_sampled_points=8), node=NS(dt=1, method="euler"))
    shell = NS(apply=lambda params, idx: (None, None, None))                  # (the table is read before the roll-out loss parses)
    return NonMetaPDETrainer(conf, _NoDecoder(), shell, torch.zeros(4, 2), ode_model=object())


# (name, the call with the four keywords, whether the step takes channel_weights)
STEPS = [
    ("maml.nef_train_step", lambda **kw: _maml().nef_train_step(STATE, TRAJ[:, 0], **kw), True),
    ("maml.fit_errors", lambda **kw: _maml().fit_errors(STATE, TRAJ[:, 0], **kw), True),
    ("maml.ode_train_step", lambda **kw: _maml().ode_train_step(STATE, TRAJ, **kw), False),
    ("maml.dual_train_step", lambda **kw: _maml().dual_train_step(STATE, TRAJ, **kw), True),
    ("maml.val_step", lambda **kw: _maml().val_step(STATE, TRAJ, **kw), True),
    ("maml.rollout_loss", lambda **kw: _maml().rollout_loss(None, None, None, TRAJ, **kw), True),
    ("autodec.loss_and_grads", lambda **kw: _autodec().loss_and_grads(STATE, TRAJ[:, 0], IDX, **kw), True),
    ("autodec.fit_latents_step", lambda **kw: _autodec().fit_latents_step(STATE, (TRAJ[:, 0], IDX), **kw), True),
    ("autodec.ode_train_step", lambda **kw: _autodec().ode_train_step(STATE, (TRAJ, IDX), **kw), False),
    ("autodec.val_step", lambda **kw: _autodec().val_step(STATE, (TRAJ, IDX), **kw), True),
    ("meta_gradients", lambda **kw: meta_gradients(_NoDecoder(), None, {}, {}, None, TRAJ[:, 0], MASKS, **kw), True),
]
CELLS = (X, None, 4)
REFUSALS = [
    ("both weight kinds on points", dict(weights=torch.ones(4), channel_weights=torch.ones(4, 2)), "not both", True),
    ("both weight kinds on cells", dict(weights=torch.ones(4), cell_channel_weights=torch.ones(4, 2), cells=CELLS), "not both", False),
    ("channel_weights with cells", dict(channel_weights=torch.ones(4, 2), cells=CELLS), "channel_weights", True),
    ("cell_channel_weights without cells", dict(cell_channel_weights=torch.ones(4, 2)), "cell_channel_weights", False),
    ("a group the tail does not serve", dict(cells=(X, None, 3)), "group", False),
    ("quadrature rows that are not M * group", dict(cells=(X, None, 2)), "cells hold", False),
]


@pytest.mark.parametrize("what,kw,match,needs_channel_weights", REFUSALS, ids=[r[0] for r in REFUSALS])
@pytest.mark.parametrize("name,call,takes_channel_weights", STEPS, ids=[s[0] for s in STEPS])
def test_every_step_refuses_before_the_decoder(name, call, takes_channel_weights, what, kw, match, needs_channel_weights):
    if needs_channel_weights and not takes_channel_weights:
        with pytest.raises(TypeError, match="channel_weights"):             # the step has no such keyword
            call(**kw)
        return
    with pytest.raises(ValueError, match=match):
        call(**kw)
