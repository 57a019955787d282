"""Host side of the weight EMA, no GPU: the decay schedule, argument validation of the steppers and the CLI, and what a checkpoint
without an EMA does to a stepper that keeps one."""
import logging
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from lunaris_orion_amd import hostside

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ema_decay_at_without_warmup_is_the_decay():
    for t in (0, 1, 9, 10 ** 6):
        assert hostside.ema_decay_at(0.999, t, False) == 0.999
    assert hostside.ema_decay_at(0.0, 5) == 0.0


def test_ema_decay_at_with_warmup():
    d = hostside.ema_decay_at
    assert d(0.999, 0, True) == 1 / 10
    assert d(0.999, 9, True) == 10 / 19
    assert d(0.999, 10 ** 6, True) == 0.999                       # (1 + t) / (10 + t) = 0.999991 there: the cap holds
    assert d(0.5, 9, True) == 0.5 and d(0.5, 7, True) == 8 / 17   # 10 / 19 > 0.5 > 8 / 17
    ts = [d(0.9999, t, True) for t in range(0, 200000, 997)]
    assert all(a <= b for a, b in zip(ts, ts[1:])) and ts[-1] == 0.9999      # monotone up to the cap


def test_one_minus_decay_is_formed_in_double_and_raised_to_the_period():
    assert hostside.ema_one_minus_decay(0.9) == 1.0 - 0.9
    assert hostside.ema_one_minus_decay(0.9, 2) == 1.0 - 0.9 ** 2
    assert np.float32(hostside.ema_one_minus_decay(0.999, 1)) == np.float32(1.0 - 0.999) != np.float32(1.0) - np.float32(0.999)


def test_stepper_arguments_are_validated_before_anything_touches_the_gpu():
    from lunaris_orion_amd.trainer import HybridStepper, VAEStepper
    for bad in (dict(ema_decay=1.0), dict(ema_decay=-0.01), dict(ema_decay=float("nan")), dict(ema_decay=0.9, ema_every=0)):
        with pytest.raises(ValueError, match="ema_"):
            VAEStepper(None, **bad)
        with pytest.raises(ValueError, match="ema_"):
            HybridStepper(None, None, **bad)


def test_cli_flags_default_to_off_and_are_validated():
    sys.path.insert(0, ROOT)
    import train_hybrid
    args = train_hybrid.parse_args(["--data_dir", "x"])
    assert (args.ema_decay, args.ema_every, args.ema_warmup) == (0.0, 1, False)
    args = train_hybrid.parse_args(["--data_dir", "x", "--ema_decay", "0.999", "--ema_every", "4", "--ema_warmup"])
    assert (args.ema_decay, args.ema_every, args.ema_warmup) == (0.999, 4, True)
    for bad in (["--ema_decay", "1"], ["--ema_decay", "-0.5"], ["--ema_decay", "0.9", "--ema_every", "0"]):
        with pytest.raises(SystemExit):
            train_hybrid.parse_args(["--data_dir", "x", *bad])


class _StubVAE(torch.nn.Module):
    """Two parameters that are views of one flat buffer at offsets 0 and 64, as LunarisCoreVAE lays its own out."""

    def __init__(self):
        super().__init__()
        self._flat = torch.zeros(128)
        self.a, self.b = torch.nn.Parameter(torch.zeros(2, 3)), torch.nn.Parameter(torch.zeros(5))
        self.a.data, self.b.data = self._flat[0:6].view(2, 3), self._flat[64:69]
        self.loss_scale, self.noise_calls = 1.0, 0

    def flat_parameters(self):
        return self._flat


class _StubStepper:
    def __init__(self, vae, ema=True):
        self.exp_avg, self.exp_avg_sq, self.opt_steps = torch.zeros(128), torch.zeros(128), 0
        self.ema = torch.full((128,), 7.0) if ema else None
        self.ema_steps, self.ema_updates = 5, 5


def _checkpoint(**more):
    return {"global_step": 3, "best_loss": 0.5, "vae_state_dict": {"a": torch.arange(6.0).view(2, 3), "b": -torch.arange(5.0)}, **more}


def test_restore_without_an_ema_restarts_it_from_the_loaded_parameters(caplog):
    vae = _StubVAE()
    stepper = _StubStepper(vae)
    with caplog.at_level(logging.INFO, logger="TrainHybrid"):
        assert hostside.restore_checkpoint(_checkpoint(), stepper, vae, None) == (3, 0.5)
    assert torch.equal(stepper.ema, vae.flat_parameters()) and stepper.ema[5] == 5.0 and stepper.ema[64 + 4] == -4.0
    assert stepper.ema.data_ptr() != vae.flat_parameters().data_ptr()
    assert (stepper.ema_steps, stepper.ema_updates) == (0, 0)
    said = [r.getMessage() for r in caplog.records if "vae_ema_state_dict" in r.getMessage()]
    assert len(said) == 1 and "restarts" in said[0]


def test_restore_with_an_ema_fills_the_buffer_and_the_counts(caplog):
    vae = _StubVAE()
    stepper = _StubStepper(vae)
    ema_sd = OrderedDict(a=torch.full((2, 3), 0.25), b=torch.full((5,), -0.5))
    ck = _checkpoint(vae_ema_state_dict=ema_sd, lunaris_amd_extra={"ema_decay": 0.9, "ema_every": 2, "ema_warmup": False, "ema_steps": 8, "ema_updates": 4})
    with caplog.at_level(logging.INFO, logger="TrainHybrid"):
        hostside.restore_checkpoint(ck, stepper, vae, None)
    want = torch.zeros(128)
    want[0:6], want[64:69] = 0.25, -0.5
    assert torch.equal(stepper.ema, want) and (stepper.ema_steps, stepper.ema_updates) == (8, 4)
    assert vae.flat_parameters()[5] == 5.0                                     # the live weights are the checkpoint's live ones
    assert not [r for r in caplog.records if "vae_ema_state_dict" in r.getMessage()]
    with pytest.raises(KeyError, match="vae_ema_state_dict"):
        hostside.restore_checkpoint(_checkpoint(vae_ema_state_dict={"a": ema_sd["a"]}), stepper, vae, None)


def test_a_stepper_without_an_ema_ignores_the_entry():
    vae = _StubVAE()
    stepper = _StubStepper(vae, ema=False)
    hostside.restore_checkpoint(_checkpoint(vae_ema_state_dict={"a": torch.ones(2, 3), "b": torch.ones(5)}), stepper, vae, None)
    assert stepper.ema is None and (stepper.ema_steps, stepper.ema_updates) == (5, 5)
