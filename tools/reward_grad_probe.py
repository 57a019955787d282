#!/usr/bin/env python
"""The hybrid step with and without the reward gradient at batch 64, latent 512, timed with device events and alternated inside one
process; one JSON line.

  off       HybridStepper(reward_grad_weight=0): the step as it was
  on        HybridStepper(reward_grad_weight=W): + eval-mode teacher forward, its backward with the seeded image data gradient, fused = 2
  autograd  the same objective composed from the nn.Modules with autograd (what a user had to write before): vae(x), the train-mode
            teacher calls, teacher(recon) in eval mode with eval_input_grad=True, torch clip_grad_norm_ + AdamW for both models

  python tools/reward_grad_probe.py [--routes off,on,autograd] [--reps 7] [--warmup 3] [--batch 64] [--latent 512] [--weight 0.5] [--profile]

--profile: the library's per-launch table of one `on` step (what the step adds, by launch).  Results: profiles/reward_grad_ab.md.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from lunaris_orion_amd import _lib  # noqa: E402
from lunaris_orion_amd.teacher import LunarMoETeacher  # noqa: E402
from lunaris_orion_amd.trainer import HybridStepper  # noqa: E402
from lunaris_orion_amd.vae import LunarisCoreVAE  # noqa: E402


def _models(latent, **tkw):
    torch.manual_seed(42)
    vae = LunarisCoreVAE(latent).to("cuda")
    t = LunarMoETeacher(embedding_dim=256, **tkw).to("cuda").train()
    return vae, t


class _Autograd:
    """_process_batch with the reward term, from the modules: autograd, torch's clip and AdamW."""

    def __init__(self, latent, weight):
        self.vae, self.t = _models(latent, eval_input_grad=True)
        self.w = weight
        self.vopt = torch.optim.AdamW(self.vae.parameters(), lr=1e-4, weight_decay=0.01)
        self.topt = torch.optim.AdamW(self.t.live_parameters(), lr=1e-4, weight_decay=0.01)
        self.baseline = None

    def step(self, x, i):
        vae, t = self.vae, self.t
        recon, mu, logvar = vae(x)
        with torch.no_grad():
            t(x)                                                    # the dead call: its BatchNorm side effects are real
        rl = torch.nn.functional.mse_loss(recon, x)
        kl = -0.5 * torch.mean(1 + logvar - mu.pow(2) - logvar.exp())
        out = t(recon.detach())
        q, sem = out["quality_scores"], out["semantic_score"]
        total = (q.mean() + 0.5 * sem.mean()).detach()
        self.baseline = total if self.baseline is None else 0.9 * self.baseline + 0.1 * total
        adv = (total - self.baseline) * 0.1
        t.eval()
        q_eval = t(recon)["quality_scores"]                       # eval kept forward; x.grad through lo_teacher_eval_backward
        t.train()
        vae_loss = rl + 0.1 * kl - adv * rl - self.w * q_eval.mean()
        vgrads = torch.autograd.grad(vae_loss, list(vae.parameters()))     # the teacher's parameters are constants in this term
        (0.5 * -q.mean()).backward()
        for p, g in zip(vae.parameters(), vgrads):
            p.grad = g
        torch.nn.utils.clip_grad_norm_(vae.parameters(), 1.0)
        torch.nn.utils.clip_grad_norm_(t.live_parameters(), 1.0)
        self.vopt.step()
        self.topt.step()
        self.vopt.zero_grad(set_to_none=True)
        self.topt.zero_grad(set_to_none=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--routes", default="off,on,autograd")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--latent", type=int, default=512)
    ap.add_argument("--weight", type=float, default=0.5)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    routes = a.routes.split(",")
    x = bench.synth_sprites(a.batch, 1).cuda()
    runners = {}
    for r in routes:
        if r == "autograd":
            runners[r] = _Autograd(a.latent, a.weight)
        else:
            vae, t = _models(a.latent)
            runners[r] = HybridStepper(vae, t, gradient_accumulation_steps=1, reward_grad_weight=a.weight if r == "on" else 0.0)

    def timed(r, i):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        runners[r].step(x, i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for i in range(a.warmup):
        for r in routes:
            timed(r, i)
    ms = {r: [] for r in routes}
    for i in range(a.reps):
        for r in routes:                            # alternated: drift of the clocks hits every route alike
            ms[r].append(timed(r, i))
    res = {"batch": a.batch, "latent": a.latent, "weight": a.weight, "reps": a.reps, "unit": "ms"}
    for r in routes:
        res[r] = {"median": round(statistics.median(ms[r]), 3), "min": round(min(ms[r]), 3), "max": round(max(ms[r]), 3)}
        if r != "autograd":
            m = runners[r].metrics()
            res[r]["metrics"] = {k: round(m[k], 6) for k in ("vae_loss", "recon_loss", "reward_grad_loss", "eval_quality", "grad_norm", "grads_finite")}
    res["max_mem_GB"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    print(json.dumps(res))
    if a.profile and "on" in runners:
        _lib.lib.lo_prof_enable(1)
        runners["on"].step(x, 0)
        torch.cuda.synchronize()
        rows = bench.collect_profile(_lib.lib)
        _lib.lib.lo_prof_enable(0)
        for k, r in sorted(rows.items(), key=lambda kv: -kv[1][0])[:30]:
            print(f"{k:36s} {r[0]:9.3f} ms n={r[1]:3d}  avg {1e3 * r[0] / max(r[1], 1):7.1f} us")
        print("sum", round(sum(r[0] for r in rows.values()), 3))


if __name__ == "__main__":
    main()
