#!/usr/bin/env python
"""What the weight EMA (VAEStepper(ema_decay=...)) costs, in ONE process at `--batch` / `--latent` (64 / 512):

  kernels   lo_prof (per-launch HIP events) on the two streaming passes over the whole flat buffer, alternating: lo_ema_update
            (12 B / parameter) and the AdamW pass lo_adamw_range (28 B / parameter), the yardstick with the same access pattern;
            then the records of `--prof-steps` profiled training steps with the EMA on (profiling runs everything on one stream)
  steps     VAEStepper.step with pipeline_optimizer=True on a resident batch: EMA off, on, on with ema_every=4 -- three steppers
            on three models, `--iters` steps per leg between two events, `--rounds` rounds, the order of the legs reversed every
            other round; round 0 warms every leg up
  swap      one `with stepper.ema_weights(): pass` (flat -> backup, EMA -> flat, and back) behind a finished step

  python tools/ema_ab.py [--batch 64] [--latent 512] [--rounds 6] [--iters 30] [--out profiles/ema_ab_table.md]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--latent", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--prof-steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from lunaris_orion_amd import _lib
    from lunaris_orion_amd.trainer import VAEStepper
    from lunaris_orion_amd.vae import LunarisCoreVAE
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured on a CPU"
    lib, sp = _lib.lib, _lib.stream_ptr
    B, L = a.batch, a.latent
    u8 = np.random.default_rng(0).integers(0, 256, (B, 128, 128, 3), dtype=np.uint8)
    x = (torch.from_numpy(u8).float() / 127.5 - 1.0).permute(0, 3, 1, 2).contiguous().cuda()

    def stepper(**kw):
        torch.manual_seed(42)
        return VAEStepper(LunarisCoreVAE(latent_dim=L).to("cuda"), gradient_accumulation_steps=1, pipeline_optimizer=True, **kw)

    def profile():
        rows, name = {}, C.create_string_buffer(128)
        ms, fl, by = C.c_double(), C.c_double(), C.c_double()
        for i in range(lib.lo_prof_count()):
            lib.lo_prof_get(i, name, 128, C.byref(ms), C.byref(fl), C.byref(by))
            if ms.value >= 0:
                rows.setdefault(name.value.decode(), []).append((ms.value, by.value))
        return rows

    def rate_rows(rows, keep, drop_first=0):
        out = []
        for k, v in rows.items():
            if not any(s in k for s in keep):
                continue
            v = v[drop_first:]
            t, byts = statistics.median(m for m, _ in v), statistics.median(b for _, b in v)
            out.append((k, len(v), 1e3 * t, 1e3 * min(m for m, _ in v), byts / 1e6, byts / (t * 1e-3) / 1e12))
        return out

    lines = []
    # ---- kernels: the two passes alone over the whole flat buffer, alternating, under lo_prof ------------------------------------------
    st_on = stepper(ema_decay=0.999)
    n = st_on.vae.flat_parameters().numel()
    p, g = st_on.vae.flat_parameters().clone(), torch.randn(n, device="cuda") * 1e-3
    m, v, e = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    lib.lo_prof_enable(1)
    for i in range(a.iters + 2):
        _lib.check(lib.lo_ema_update(e.data_ptr(), p.data_ptr(), n, 1e-3, None, sp()), "lo_ema_update")
        _lib.check(lib.lo_adamw_range(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, None, 1e-4, 0.9, 0.999, 1e-8, 0.01, i + 1, None, sp()),
                   "lo_adamw_range")
    torch.cuda.synchronize()
    alone = rate_rows(profile(), ("lo_ema_update", "lo_adamw"), drop_first=2)
    lib.lo_prof_enable(0)
    del p, g, m, v, e
    lines += [f"| pass alone over the flat buffer ({n:,} parameters, batch {B}, latent {L}) | launches | median us | min us | MB | TB/s at the median |",
              "|---|---|---|---|---|---|"]
    lines += [f"| {k} | {c} | {t:.1f} | {tm:.1f} | {mb:.1f} | {r:.2f} |" for k, c, t, tm, mb, r in alone]
    rates = {k: r for k, _c, _t, _tm, _mb, r in alone}
    if "lo_ema_update" in rates and "lo_adamw" in rates:
        lines += ["", f"lo_ema_update reaches {rates['lo_ema_update'] / rates['lo_adamw']:.2f} of lo_adamw's bandwidth in the same run"]
    # ---- ... and inside profiled steps (one stream, nothing overlaps) -----------------------------------------------------------------
    for i in range(3):
        st_on.step(x, batch_idx=i)
    torch.cuda.synchronize()
    lib.lo_prof_enable(1)
    for i in range(a.prof_steps):
        st_on.step(x, batch_idx=i)
    torch.cuda.synchronize()
    in_step = rate_rows(profile(), ("lo_ema_update", "lo_adamw"))
    lib.lo_prof_enable(0)
    lines += ["", f"| launch inside {a.prof_steps} profiled steps (EMA on) | launches | median us | min us | MB | TB/s at the median |", "|---|---|---|---|---|---|"]
    lines += [f"| {k} | {c} | {t:.1f} | {tm:.1f} | {mb:.1f} | {r:.2f} |" for k, c, t, tm, mb, r in in_step]
    # ---- steps: off / on / every 4, alternating order ---------------------------------------------------------------------------------
    legs = {"EMA off": stepper(), "EMA on": st_on, "EMA on, ema_every=4": stepper(ema_decay=0.999, ema_every=4)}
    times = {k: [] for k in legs}
    for rnd in range(a.rounds + 1):
        order = list(legs.items())
        if rnd % 2 == 0:
            order.reverse()
        for name, st in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for i in range(a.iters):
                st.step(x, batch_idx=i)
            st.synchronize_parameters()           # the window ends when the last step's side-stream work (AdamW tail, EMA) has
            e1.record()
            torch.cuda.synchronize()
            if rnd > 0:
                times[name].append(1e3 * e0.elapsed_time(e1) / a.iters)
    for st in legs.values():
        assert st.metrics()["grads_finite"] == 1.0
    med = {k: statistics.median(v) for k, v in times.items()}
    lines += ["", f"| VAEStepper.step, pipelined ({a.rounds} rounds of {a.iters} steps) | median us | min us | max us | against EMA off |", "|---|---|---|---|---|"]
    lines += [f"| {k} | {med[k]:.1f} | {min(v):.1f} | {max(v):.1f} | {100 * (med[k] / med['EMA off'] - 1):+.2f} % |" for k, v in times.items()]
    # ---- swap: one ema_weights() enter / exit -----------------------------------------------------------------------------------------
    swaps = []
    for rnd in range(a.rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        with st_on.ema_weights():
            pass
        e1.record()
        torch.cuda.synchronize()
        if rnd > 0:
            swaps.append(1e3 * e0.elapsed_time(e1))
    lines += ["", f"one ema_weights() enter + exit (three copies of {4 * n / 1e6:.0f} MB; the re-pack of the operands is paid by the next forward): "
                  f"median {statistics.median(swaps):.1f} us, min {min(swaps):.1f}, max {max(swaps):.1f}"]
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
