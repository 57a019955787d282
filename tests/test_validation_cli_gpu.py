"""`train_hybrid.py --validate_every N` / `--validate_only`: the held-out tenth is validated at epoch ends, decides early stopping and
best.pt, and rides in the checkpoint; without the flag nothing of it shows.  The CLI is what is tested, so each run is a process."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--vae_only", "--batch_size", "4", "--latent_dim", "256", "--num_epochs", "2", "--gradient_accumulation_steps", "1", "--log_every", "3"]


def _make_data(d, n=40):
    rng = np.random.default_rng(0)
    np.save(os.path.join(d, "sprites_000.npy"), rng.integers(0, 256, (n, 128, 128, 3), dtype=np.uint8))
    with open(os.path.join(d, "labels_000.csv"), "w") as f:
        f.write("filename,category,prompt,seed,pixel_size,guidance_scale,pag_scale,num_steps\n")
        for i in range(n):
            f.write(f"s{i}.png,cat,prompt {i},{i},4,5.0,2.0,20\n")


def _train(data, out, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_hybrid.py"), "--data_dir", str(data), "--output_dir", str(out), *COMMON, *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


@pytest.fixture(scope="module")
def validated_run(tmp_path_factory):
    """Two epochs on 40 synthetic sprites (36 train, 4 held out) with a validation pass after each."""
    data = tmp_path_factory.mktemp("data")
    _make_data(str(data))
    out = tmp_path_factory.mktemp("validated")
    _train(data, out, "--validate_every", "1")
    return data, out


def test_validate_every_logs_decides_and_checkpoints(validated_run):
    _, out = validated_run
    lines = [ln for ln in (out / "training.log").read_text().splitlines() if "Validation:" in ln]
    assert len(lines) == 2                                                    # once per epoch
    vals = []
    for ln in lines:
        fields = dict(re.findall(r"(\w+) (-?[\d.]+(?:e[-+]?\d+)?|nan|inf)", ln.split("Validation:")[1]))
        assert {"val_loss", "val_recon_loss", "val_kl_loss", "val_psnr", "val_psnr_min", "val_ssim", "n"} <= fields.keys(), ln
        assert int(fields["n"]) == 4                                          # the held-out tenth of 40
        assert 0.0 < float(fields["val_psnr"]) < 60.0 and -1.0 <= float(fields["val_ssim"]) <= 1.0
        vals.append(float(fields["val_loss"]))
    ck = torch.load(out / "checkpoints" / "latest.pt", map_location="cpu", weights_only=True)
    best = ck["lunaris_amd_extra"]["best_val_loss"]
    assert best == pytest.approx(min(vals), rel=1e-5)                         # the log prints six digits
    assert (out / "checkpoints" / "best.pt").exists()
    assert torch.load(out / "checkpoints" / "best.pt", map_location="cpu", weights_only=True)["lunaris_amd_extra"]["best_val_loss"] == best


def test_validate_only_prints_one_json_line_and_restores_best_val_loss(validated_run):
    data, out = validated_run
    path = out / "checkpoints" / "latest.pt"
    before = (hashlib.sha256(path.read_bytes()).hexdigest(), path.stat().st_mtime_ns)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    r = _train(data, out.parent / "only", "--validate_only", "--resume_from", str(path))
    assert (hashlib.sha256(path.read_bytes()).hexdigest(), path.stat().st_mtime_ns) == before
    assert not list((out.parent / "only" / "checkpoints").glob("*.pt"))       # nothing saved, no step taken
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n"] == 4 and res["global_step"] == ck["global_step"] == 18
    assert res["best_val_loss"] == ck["lunaris_amd_extra"]["best_val_loss"]   # --resume_from restored it
    # the weights are those of the second epoch's end: its logged validation is reproduced (z = mu: nothing random in a pass)
    last = [ln for ln in (out / "training.log").read_text().splitlines() if "Validation:" in ln][-1]
    logged = float(re.search(r"val_loss (\S+)", last).group(1))
    assert res["val_loss"] == pytest.approx(logged, rel=1e-5)
    assert {"val_recon_loss", "val_kl_loss", "val_psnr", "val_psnr_min", "val_ssim"} <= res.keys()


def test_without_the_flag_nothing_mentions_validation(validated_run):
    data, _ = validated_run
    out = data.parent / "plain"
    _train(data, out)
    log = (out / "training.log").read_text()
    assert "val_" not in log and "Validation" not in log
    ck = torch.load(out / "checkpoints" / "latest.pt", map_location="cpu", weights_only=True)
    assert not any("val" in k for k in ck["lunaris_amd_extra"]) and not any(k.startswith("val") or "best_val" in k for k in ck)
