#!/usr/bin/env python
"""What a validation pass (lunaris_orion_amd.evaluate.Validator) costs, with HIP events, at `--batch` / `--latent` (64 / 512):

  forward+loss   lo_vae_forward (with the fused MSE / KL partial sums) + lo_vae_loss on a resident batch: the forward half of a training
                 step, as every checkout has it -- the base the validation batch is compared with
  val batch      one batch of a pass: lo_vae_forward at eps = 0, lo_eval_image_metrics, lo_eval_latent_kl, lo_eval_accumulate
  three kernels  the three lo_eval_* launches alone on the buffers of the batch before
  metrics / kl / accumulate   each of the three alone
  train step     one VAEStepper.step (pipelined optimizer) on the same batch: the epoch-level cost of validating a 10 % split every
                 epoch is (val batch) / (9 * train step)

The legs run one after the other inside a round, `--rounds` rounds, `--iters` calls per leg and round between two events; the
table gives the median, the smallest and the largest round.

  python tools/validation_ab.py [--batch 64] [--latent 512] [--rounds 5] [--iters 20] [--out profiles/validation_ab.md]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--latent", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from lunaris_orion_amd import _lib
    from lunaris_orion_amd.evaluate import Validator
    from lunaris_orion_amd.trainer import VAEStepper
    from lunaris_orion_amd.vae import LunarisCoreVAE
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured on a CPU"
    torch.manual_seed(42)
    B, L = a.batch, a.latent
    vae = LunarisCoreVAE(latent_dim=L).to("cuda")
    st = VAEStepper(vae, gradient_accumulation_steps=1, pipeline_optimizer=True)
    val = Validator(st)
    u8 = np.random.default_rng(0).integers(0, 256, (B, 128, 128, 3), dtype=np.uint8)
    x = (torch.from_numpy(u8).float() / 127.5 - 1.0).permute(0, 3, 1, 2).contiguous().cuda()
    eps0 = torch.zeros(B, L, device="cuda")
    val._acc = torch.zeros(8, dtype=torch.float64, device="cuda")
    lib, sp = _lib.lib, _lib.stream_ptr

    def forward_loss():
        _r, _m, _l, eng = vae._native_forward(x, eps0, target=x)
        _lib.check(lib.lo_vae_loss(eng.handle, eng.ws.data_ptr(), 1.0, 0.1, 0.0, None, 1.0, float(vae.loss_scale), st.losses.data_ptr(), sp()), "lo_vae_loss")

    def val_batch():
        val._add_batch(x, B)

    buf = val.forward(x)
    ops = {"metrics": lambda: _lib.check(lib.lo_eval_image_metrics(buf["recon"].data_ptr(), x.data_ptr(), B, B, buf["img"].data_ptr(), sp())),
           "kl": lambda: _lib.check(lib.lo_eval_latent_kl(buf["mu"].data_ptr(), buf["logvar"].data_ptr(), B, L, B, buf["kl"].data_ptr(), sp())),
           "accumulate": lambda: _lib.check(lib.lo_eval_accumulate(buf["img"].data_ptr(), buf["kl"].data_ptr(), None, B, val._acc.data_ptr(), sp()))}

    def three():
        for f in ops.values():
            f()

    legs = {"forward+loss": forward_loss, "val batch": val_batch, "three kernels": three, **ops, "train step": lambda: st.step(x, batch_idx=0)}
    times = {k: [] for k in legs}
    for rnd in range(a.rounds + 1):                          # round 0 warms every leg up
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rnd > 0:
                times[name].append(1e3 * e0.elapsed_time(e1) / a.iters)
    st.synchronize_parameters()
    assert st.metrics()["grads_finite"] == 1.0
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"| leg (batch {B}, latent {L}) | median us | min us | max us |", "|---|---|---|---|"]
    lines += [f"| {k} | {med[k]:.1f} | {min(v):.1f} | {max(v):.1f} |" for k, v in times.items()]
    lines += ["", f"val batch / forward+loss = {med['val batch'] / med['forward+loss']:.3f}; "
                  f"three kernels / val batch = {med['three kernels'] / med['val batch']:.3f}; "
                  f"epoch-level cost of a 10 % split validated every epoch = val batch / (9 * train step) = "
                  f"{100 * med['val batch'] / (9 * med['train step']):.2f} % of the epoch's training time"]
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
