#!/usr/bin/env python
"""Step time of the README High-End recipe (batch 64, latent 512, embedding 256, feature_dim 512, teacher dropout 0.1) with the
teacher's 3x3 convolutions on fp16 and on e4m3 operands, as interleaved pairs in one process.  The stepper is built the way
bench.py's hybrid_leg builds it (same seed, same sprite pool, pipelined optimizer); the VAE stays fp16 in both legs, so the pair
isolates the teacher's operand mode.

  python tools/highend_step_ab.py --pairs 3 --steps 3 --warmup 2 [--modes fp16,fp8] [--feature_dim 512]

Prints one JSON line per leg and a markdown summary row per mode.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lunaris_orion_amd.teacher import LunarMoETeacher  # noqa: E402
from lunaris_orion_amd.trainer import HybridStepper  # noqa: E402
from lunaris_orion_amd.vae import LunarisCoreVAE  # noqa: E402


def synth_sprites(n, seed):       # bench.py's pool
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, (n, 128, 128, 3), dtype=np.uint8)
    return (torch.from_numpy(u8).float() / 127.5 - 1.0).permute(0, 3, 1, 2).contiguous()


def leg(a, pool, precision):
    torch.manual_seed(42)
    kw = {} if precision == "fp16" else {"mfma_precision": precision}
    teacher = LunarMoETeacher(num_experts=4, feature_dim=a.feature_dim, embedding_dim=256, dropout_rate=0.1, **kw).to("cuda").train()
    vae = LunarisCoreVAE(latent_dim=a.latent).to("cuda")
    hs = HybridStepper(vae, teacher, gradient_accumulation_steps=1, pipeline_optimizer=True)
    hs.step(pool[0], batch_idx=0)
    first = hs.metrics()
    for i in range(1, a.warmup):
        hs.step(pool[i % len(pool)], batch_idx=i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        hs.step(pool[i % len(pool)], batch_idx=i)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / a.steps
    out = {"precision": precision, "ms_per_step": ms, "sprites_per_s": a.batch / ms * 1e3, "teacher_path": teacher.last_path(a.batch),
           "first_step": {k: first[k] for k in ("recon_loss", "kl_loss", "quality_scores", "teacher_loss")}}
    del hs, teacher, vae
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--latent", type=int, default=512)
    ap.add_argument("--feature_dim", type=int, default=512)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--modes", default="fp16,fp8")
    a = ap.parse_args()
    pool = [synth_sprites(a.batch, i).cuda() for i in range(4)]
    modes = a.modes.split(",")
    ms = {m: [] for m in modes}
    for _ in range(a.pairs):
        for m in modes:
            r = leg(a, pool, m)
            ms[m].append(r["ms_per_step"])
            print(json.dumps(r), flush=True)
    for m in modes:
        print(f"| {m} | {' / '.join(f'{t:.1f}' for t in ms[m])} | {a.batch / max(ms[m]) * 1e3:.1f}-{a.batch / min(ms[m]) * 1e3:.1f} |")
    if len(modes) == 2:
        print("every", modes[1], "step time below every", modes[0], "step time:", max(ms[modes[1]]) < min(ms[modes[0]]))


if __name__ == "__main__":
    main()
