"""train_hybrid.py --vae_attention: two optimizer steps on a tiny dataset, and what the checkpoint carries."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cli_two_steps_with_vae_attention(tmp_path):
    data = tmp_path / "data"
    data.mkdir()
    rng = np.random.default_rng(0)
    n = 9                                                  # 8 training sprites after the 90 % split: two steps of batch 4
    np.save(os.path.join(data, "sprites_000.npy"), rng.integers(0, 256, (n, 128, 128, 3), dtype=np.uint8))
    with open(os.path.join(data, "labels_000.csv"), "w") as f:
        f.write("filename,category,prompt,seed,pixel_size,guidance_scale,pag_scale,num_steps\n")
        for i in range(n):
            f.write(f"s{i}.png,cat,prompt {i},{i},4,5.0,2.0,20\n")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_hybrid.py"), "--data_dir", str(data), "--output_dir", str(out),
                        "--vae_only", "--vae_attention", "--batch_size", "4", "--gradient_accumulation_steps", "1", "--num_epochs", "1",
                        "--log_every", "1", "--latent_dim", "64"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    import torch
    ck = torch.load(out / "checkpoints" / "latest.pt", map_location="cpu", weights_only=False)
    assert ck["args"]["vae_attention"] is True
    assert ck["global_step"] == 2
    sd = ck["vae_state_dict"]
    assert len(sd) == 86
    from lunaris_orion_amd.vae import LunarisCoreVAE
    m = LunarisCoreVAE(64, attention=True)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert float(sd["encoder.attn.gamma"]) != 0.0 and float(sd["decoder.attn.gamma"]) != 0.0
    # the optimizer state covers the 86 tensors and loads into the object the reference builds
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=0.01, betas=(0.9, 0.999))
    opt.load_state_dict(ck["vae_optimizer"])
    assert len(opt.state_dict()["state"]) == 86 and int(float(opt.state_dict()["state"][0]["step"])) == 2
