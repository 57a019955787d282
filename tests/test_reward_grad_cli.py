"""--reward_grad_weight of train_hybrid.py: parsing, its default, the --vae_only argument error and its place in the checkpoint."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_flag_parses_and_defaults_to_off():
    import train_hybrid
    assert train_hybrid.parse_args(["--data_dir", "x"]).reward_grad_weight == 0.0
    args = train_hybrid.parse_args(["--data_dir", "x", "--reward_grad_weight", "0.25"])
    assert args.reward_grad_weight == 0.25 and not args.vae_only
    # the teacher's own objective may be switched off beside it: the reward needs the teacher, not the teacher's loss
    args = train_hybrid.parse_args(["--data_dir", "x", "--reward_grad_weight", "2", "--reward_scale", "0", "--quality_weight", "0"])
    assert args.reward_grad_weight == 2.0
    assert train_hybrid.parse_args(["--data_dir", "x", "--vae_only"]).vae_only           # --vae_only alone stays valid


def test_vae_only_with_a_reward_weight_is_an_argument_error_that_says_why(capsys):
    import train_hybrid
    with pytest.raises(SystemExit) as e:
        train_hybrid.parse_args(["--data_dir", "x", "--vae_only", "--reward_grad_weight", "0.5"])
    assert e.value.code == 2                                                             # argparse's argument error
    err = capsys.readouterr().err
    assert "--reward_grad_weight" in err and "--vae_only" in err and "teacher" in err
    with pytest.raises(SystemExit):
        train_hybrid.parse_args(["--data_dir", "x", "--reward_grad_weight", "-1"])
    assert "--reward_grad_weight" in capsys.readouterr().err


def test_flag_lands_in_the_checkpoint_args():
    import train_hybrid
    from lunaris_orion_amd import hostside

    class _V(torch.nn.Module):                    # the smallest objects checkpoint_dict() needs (tests/test_hostside.py)
        def __init__(self):
            super().__init__()
            self._flat = torch.zeros(64)
            self.w = torch.nn.Parameter(torch.zeros(4, 4))
            self.w.data = self._flat[:16].view(4, 4)
            self.loss_scale, self.noise_calls = 65536.0, 0

        def flat_parameters(self):
            return self._flat

    class _S:
        exp_avg, exp_avg_sq = torch.zeros(64), torch.zeros(64)
        opt_steps, lr, base_lr, betas, eps, weight_decay, t0, min_lr = 0, 1e-4, 1e-4, (0.9, 0.999), 1e-8, 0.01, 10, 1e-6
    args = train_hybrid.parse_args(["--data_dir", "x", "--reward_grad_weight", "0.25", "--feature_dim", "64"])
    with pytest.warns(UserWarning, match="without teacher entries"):
        ck = hostside.checkpoint_dict(_S(), _V(), None, 3, 1.0, vars(args))
    assert ck["args"]["reward_grad_weight"] == 0.25
    default = train_hybrid.parse_args(["--data_dir", "x", "--feature_dim", "64"])
    with pytest.warns(UserWarning, match="without teacher entries"):
        assert hostside.checkpoint_dict(_S(), _V(), None, 3, 1.0, vars(default))["args"]["reward_grad_weight"] == 0.0
