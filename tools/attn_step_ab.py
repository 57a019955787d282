#!/usr/bin/env python
"""Step time of the fused VAE step with and without the bottleneck self-attention (LunarisCoreVAE(attention=True)), as interleaved
runs in one process, and the share of the attention launches in a profiled step.  The stepper is built the way bench.py builds it
(same seed, same sprite pool, pipelined optimizer).

  python tools/attn_step_ab.py [--batch 64] [--latent 512] [--runs 5] [--steps 20] [--warmup 5]

Prints one JSON line per run, the medians, and the per-launch rows of the attention sites (HIP-event profile, one stream).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lunaris_orion_amd import _lib  # noqa: E402
from lunaris_orion_amd.trainer import VAEStepper  # noqa: E402
from lunaris_orion_amd.vae import LunarisCoreVAE  # noqa: E402


def synth_sprites(n, seed):       # bench.py's pool
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, (n, 128, 128, 3), dtype=np.uint8)
    return (torch.from_numpy(u8).float() / 127.5 - 1.0).permute(0, 3, 1, 2).contiguous()


def make(a, attention):
    torch.manual_seed(42)
    vae = LunarisCoreVAE(latent_dim=a.latent, attention=attention).to("cuda")
    if attention:                 # gamma = 0 is the identity: give the sites something to do
        with torch.no_grad():
            vae.encoder.attn.gamma.fill_(0.5)
            vae.decoder.attn.gamma.fill_(0.5)
        vae.mark_weights_changed()
    return vae, VAEStepper(vae, gradient_accumulation_steps=1, pipeline_optimizer=True)


def leg(a, pool, attention):
    vae, st = make(a, attention)
    for i in range(a.warmup):
        st.step(pool[i % len(pool)], batch_idx=i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        st.step(pool[i % len(pool)], batch_idx=i)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / a.steps
    st.synchronize_parameters()
    del st, vae
    torch.cuda.empty_cache()
    return ms


def profile(a, pool, steps=3):
    vae, st = make(a, True)
    for i in range(a.warmup):
        st.step(pool[i % len(pool)], batch_idx=i)
    torch.cuda.synchronize()
    _lib.lib.lo_prof_enable(2)
    for i in range(steps):
        st.step(pool[i % len(pool)], batch_idx=i)
    torch.cuda.synchronize()
    rows, name = {}, C.create_string_buffer(128)
    ms, fl, by = C.c_double(), C.c_double(), C.c_double()
    for i in range(_lib.lib.lo_prof_count()):
        _lib.lib.lo_prof_get(i, name, 128, C.byref(ms), C.byref(fl), C.byref(by))
        if ms.value >= 0:
            r = rows.setdefault(name.value.decode(), [0.0, 0])
            r[0] += ms.value
            r[1] += 1
    _lib.lib.lo_prof_enable(0)
    total = sum(r[0] for r in rows.values())
    attn = {k: r for k, r in rows.items() if k.startswith("attn") or k.startswith("lo_attn8")}
    return total / steps, {k: (r[0] / steps, r[1] / steps) for k, r in attn.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--latent", type=int, default=512)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    pool = [synth_sprites(a.batch, i).cuda() for i in range(4)]
    ms = {False: [], True: []}
    for _ in range(a.runs):
        for attention in (False, True):
            t = leg(a, pool, attention)
            ms[attention].append(t)
            print(json.dumps({"attention": attention, "ms_per_step": t}), flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(f"| attention | ms per step ({a.runs} runs) | median |")
    for k in (False, True):
        print(f"| {'on' if k else 'off'} | {' / '.join(f'{t:.3f}' for t in ms[k])} | {med[k]:.3f} |")
    print(f"median on / off: {med[True] / med[False]:.4f}")
    total, attn = profile(a, pool)
    print(f"profiled step (launches one after the other, one stream): {total:.3f} ms in the library's launches; attention launches:")
    for k, (t, n) in sorted(attn.items()):
        print(f"| {k} | {n:.0f} per step | {1e3 * t:.1f} us |")
    s = sum(t for t, _ in attn.values())
    print(f"attention launches: {1e3 * s:.1f} us per step = {100 * s / total:.2f} % of the profiled step")


if __name__ == "__main__":
    main()
