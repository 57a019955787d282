"""`train_hybrid.py --ema_decay D`: the averaged weights ride in the checkpoint, are what gets validated, survive a resume bit for bit, and
without the flag nothing of them shows.  The CLI is what is tested, so each run is a process (batch 2, latent 256, ten sprites).

The ten sprites are one sprite ten times: a resumed process shuffles its first epoch like the original's FIRST epoch, so only with
identical sprites does "resume and take one more step" see the batch the uninterrupted run sees at that step (the noise stream and the
optimizer state are restored; the order of the data is not part of a checkpoint)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--vae_only", "--batch_size", "2", "--latent_dim", "256", "--gradient_accumulation_steps", "1", "--log_every", "1"]
EMA = ["--ema_decay", "0.5", "--ema_warmup", "--validate_every", "1"]


def _make_data(d, n=10):
    rng = np.random.default_rng(0)
    one = rng.integers(0, 256, (1, 128, 128, 3), dtype=np.uint8)
    np.save(os.path.join(d, "sprites_000.npy"), np.repeat(one, n, axis=0))
    with open(os.path.join(d, "labels_000.csv"), "w") as f:
        f.write("filename,category,prompt,seed,pixel_size,guidance_scale,pag_scale,num_steps\n")
        for i in range(n):
            f.write(f"s{i}.png,cat,prompt {i},{i},4,5.0,2.0,20\n")


def _train(data, out, *extra, ok=True):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_hybrid.py"), "--data_dir", str(data), "--output_dir", str(out), *COMMON, *extra],
                       capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr[-2000:]
    return r


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


@pytest.fixture(scope="module")
def ema_run(tmp_path_factory):
    """One epoch = four steps (nine training sprites at batch 2, one held out) with the EMA on and a validation pass at its end."""
    data = tmp_path_factory.mktemp("data")
    _make_data(str(data))
    out = tmp_path_factory.mktemp("ema")
    _train(data, out, *EMA, "--num_epochs", "1")
    return data, out


def test_checkpoints_carry_the_averaged_weights_and_their_counts(ema_run):
    _, out = ema_run
    for tag in ("latest", "best"):
        ck = _load(out / "checkpoints" / f"{tag}.pt")
        ema, live = ck["vae_ema_state_dict"], ck["vae_state_dict"]
        assert list(ema.keys()) == list(live.keys()) and len(ema) == 72
        assert all(ema[k].shape == live[k].shape and ema[k].dtype == torch.float32 for k in live)
        assert sum(not torch.equal(ema[k], live[k]) for k in live) >= 60          # an average of four iterates, not a copy of the last
        extra = ck["lunaris_amd_extra"]
        assert (extra["ema_decay"], extra["ema_every"], extra["ema_warmup"], extra["ema_steps"], extra["ema_updates"]) == (0.5, 1, True, 4, 4)
        assert ck["args"]["ema_decay"] == 0.5
    log = (out / "training.log").read_text()
    # the log line carries the decay the NEXT step runs at; warm-up after one and after four steps: 2 / 11 and 5 / 14
    assert "weight EMA on" in log and "ema_decay 0.181818" in log and "ema_decay 0.357143" in log
    assert "val_weights ema" in log


def test_resume_and_one_more_step_equals_the_uninterrupted_run(ema_run):
    data, out = ema_run
    resumed, straight = out.parent / "resumed", out.parent / "straight"
    _train(data, resumed, *EMA, "--num_epochs", "1", "--max_steps", "5", "--resume_from", str(out / "checkpoints" / "latest.pt"))
    _train(data, straight, *EMA, "--num_epochs", "2", "--max_steps", "5")
    a, b = _load(resumed / "checkpoints" / "latest.pt"), _load(straight / "checkpoints" / "latest.pt")
    assert a["global_step"] == b["global_step"] == 5
    assert a["lunaris_amd_extra"]["ema_steps"] == b["lunaris_amd_extra"]["ema_steps"] == 5
    for k in b["vae_state_dict"]:
        assert torch.equal(a["vae_state_dict"][k], b["vae_state_dict"][k]), f"live {k}: the premise (same data, noise, optimizer state)"
    for k in b["vae_ema_state_dict"]:
        assert torch.equal(a["vae_ema_state_dict"][k], b["vae_ema_state_dict"][k]), f"ema {k}"
    before = _load(out / "checkpoints" / "latest.pt")["vae_ema_state_dict"]
    assert any(not torch.equal(before[k], b["vae_ema_state_dict"][k]) for k in before)      # the fifth step did move it


def test_validate_only_validates_the_averaged_weights(ema_run):
    data, out = ema_run
    path = out / "checkpoints" / "latest.pt"
    r = _train(data, out.parent / "only", "--validate_only", "--ema_decay", "0.5", "--resume_from", str(path))
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["val_weights"] == "ema" and res["n"] == 1 and res["global_step"] == 4
    # the averaged weights of the epoch's end: the logged validation is reproduced, and the live weights give another number
    logged = [ln for ln in (out / "training.log").read_text().splitlines() if "Validation:" in ln][-1]
    assert res["val_loss"] == pytest.approx(float(logged.split("val_loss ")[1].split()[0]), rel=1e-5)
    live = json.loads([ln for ln in _train(data, out.parent / "only_live", "--validate_only", "--resume_from", str(path)).stdout.splitlines()
                       if ln.strip()][0])
    assert "val_weights" not in live and live["val_loss"] != res["val_loss"]


def test_without_the_flag_nothing_mentions_the_ema_and_validating_its_checkpoint_with_it_fails(ema_run):
    data, _ = ema_run
    out = data.parent / "plain"
    _train(data, out, "--num_epochs", "1", "--max_steps", "1")
    ck = _load(out / "checkpoints" / "latest.pt")
    for keys in (ck, ck["lunaris_amd_extra"], ck["args"]):                        # ("semantic_weight" is an old key: match the prefix)
        assert not any(k.startswith("ema_") or "_ema_" in k for k in keys), sorted(keys)
    log = (out / "training.log").read_text()
    assert "ema_" not in log and "EMA" not in log and "val_weights" not in log
    r = _train(data, data.parent / "refused", "--validate_only", "--ema_decay", "0.5", "--resume_from", str(out / "checkpoints" / "latest.pt"), ok=False)
    assert "vae_ema_state_dict" in r.stderr and not r.stdout.strip()
