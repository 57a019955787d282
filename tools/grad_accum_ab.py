#!/usr/bin/env python
"""Wall time per window of real gradient accumulation (VAEStepper(accumulate_gradients=True)) against the steps it replaces, and the
rate of lo_grad_accumulate alone.  Per `--batch * --k` sprites (64 * 4 = 256 by default, latent 512):

  plain         k plain steps at gradient_accumulation_steps=1: k updates of `batch` samples each.  The leg passes no new argument:
                it runs unchanged on a checkout that does not have the mode
  factored      one accumulated window of k micro-batches: one update of k * batch samples, the two Linear matrices as factor blocks
  materialised  the same with LO_LINEAR_FACTORED=0: every gradient accumulated in the flat buffer
  op            lo_grad_accumulate at the two sizes a factored window calls it with (everything in front of fc_mu.weight; everything
                behind decoder.fc.weight) and on the whole flat buffer (the materialised window), and lo_adamw's streaming pass
                (lo_adamw_range) on the whole buffer in the same process, in GB/s of the bytes each pass moves

Every leg is a process of its own under its own time limit; the legs of a round run one after the other, the rounds alternate them,
and the first leg that fails, faults or runs out of time ends the script -- nothing is started on the GPU after it.

  python tools/grad_accum_ab.py [--batch 64] [--latent 512] [--k 4] [--rounds 3] [--windows 20] [--warmup 5] [--out profiles/grad_accum_ab.md]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEG_TIMEOUT_S = 240


def synth_sprites(n, seed):       # bench.py's pool
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, (n, 128, 128, 3), dtype=np.uint8)
    return (torch.from_numpy(u8).float() / 127.5 - 1.0).permute(0, 3, 1, 2).contiguous()


def leg_step(a):
    """One timed leg: `windows` windows of k calls, each window timed on the host clock around a device synchronise."""
    import torch
    sys.path.insert(0, ROOT)
    from lunaris_orion_amd.trainer import VAEStepper
    from lunaris_orion_amd.vae import LunarisCoreVAE
    torch.manual_seed(42)
    vae = LunarisCoreVAE(latent_dim=a.latent).to("cuda")
    if a.leg == "plain":
        st = VAEStepper(vae, gradient_accumulation_steps=1, pipeline_optimizer=True)
    else:
        st = VAEStepper(vae, gradient_accumulation_steps=a.k, pipeline_optimizer=True, accumulate_gradients=True)
    pool = [synth_sprites(a.batch, i).cuda() for i in range(a.k)]
    times = []
    for w in range(a.warmup + a.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.k):
            st.step(pool[i], batch_idx=i if a.leg != "plain" else 0)
        torch.cuda.synchronize()
        if w >= a.warmup:
            times.append(1e3 * (time.perf_counter() - t0))
    st.synchronize_parameters()
    met = st.metrics()
    assert met["grads_finite"] == 1.0, met
    if a.leg != "plain":
        assert st._window_factored(vae._engine(a.batch)) == (a.leg == "factored")
    print(json.dumps({"leg": a.leg, "ms_per_window": times, "opt_steps": st.opt_steps}), flush=True)


def leg_op(a):
    import ctypes as C
    import torch
    sys.path.insert(0, ROOT)
    from lunaris_orion_amd import _lib
    from lunaris_orion_amd.parallel import grad_range as _grad_range
    from lunaris_orion_amd.vae import LunarisCoreVAE
    vae = LunarisCoreVAE(latent_dim=a.latent).to("cuda")
    eng = vae._engine(a.batch)
    n = vae.flat_parameters().numel()
    lin_b, lin_e = _grad_range(eng, "lo_vae_linear_grad_range")
    sizes = {"encoder range [0, fc_mu.weight)": lin_b, "decoder range (behind decoder.fc.weight)": n - (lin_e - 32768), "whole flat buffer": n}
    acc, g = torch.zeros(n, device="cuda"), torch.randn(n, device="cuda")
    m, v, p = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.randn(n, device="cuda")
    st = _lib.stream_ptr()

    def timed(fn, reps=50, warm=10):
        for _ in range(warm):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for b, e in ev:
            b.record()
            fn()
            e.record()
        torch.cuda.synchronize()
        return sorted(b.elapsed_time(e) for b, e in ev)

    rows = []
    for what, cnt in sizes.items():
        for first in (1, 0):
            ms = timed(lambda: _lib.check(_lib.lib.lo_grad_accumulate(acc.data_ptr(), g.data_ptr(), cnt, 1.0, first, st), "lo_grad_accumulate"))
            nbytes = (8 if first else 12) * cnt
            rows.append({"pass": f"lo_grad_accumulate first={first}", "range": what, "elems": cnt, "us_median": 1e3 * ms[len(ms) // 2],
                         "us_min": 1e3 * ms[0], "us_max": 1e3 * ms[-1], "GBps_median": nbytes / (1e6 * ms[len(ms) // 2])})
    ms = timed(lambda: _lib.check(_lib.lib.lo_adamw_range(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, None, 1e-4, 0.9, 0.999, 1e-8,
                                                          0.01, 1, None, st), "lo_adamw_range"))
    rows.append({"pass": "lo_adamw_range (p, g, m, v: 28 B per element)", "range": "whole flat buffer", "elems": n, "us_median": 1e3 * ms[len(ms) // 2],
                 "us_min": 1e3 * ms[0], "us_max": 1e3 * ms[-1], "GBps_median": 28 * n / (1e6 * ms[len(ms) // 2])})
    print(json.dumps({"leg": "op", "rows": rows}), flush=True)


def run_leg(a, leg, env_extra):
    """A leg as a child process under its own time limit; any failure ends the script."""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--batch", str(a.batch), "--latent", str(a.latent), "--k", str(a.k),
           "--windows", str(a.windows), "--warmup", str(a.warmup)]
    env = dict(os.environ, **env_extra)
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=LEG_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"leg {leg}: no result after {LEG_TIMEOUT_S} s; stopping, nothing further is started")
    if r.returncode != 0:
        raise SystemExit(f"leg {leg}: exit status {r.returncode}; stopping, nothing further is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--latent", type=int, default=512)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the tables to this file (markdown)")
    ap.add_argument("--leg", choices=["plain", "factored", "materialised", "op"], default=None, help="run one leg in this process (the driver's children)")
    a = ap.parse_args()
    if a.leg == "op":
        return leg_op(a)
    if a.leg:
        return leg_step(a)
    legs = (("plain", {}), ("factored", {"LO_LINEAR_FACTORED": "1"}), ("materialised", {"LO_LINEAR_FACTORED": "0"}))
    ms = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, env in legs:
            ms[name].append(run_leg(a, name, env)["ms_per_window"])
    op = run_leg(a, "op", {})
    n = a.batch * a.k
    out = [f"# Gradient accumulation: wall time per {n} sprites (batch {a.batch}, latent {a.latent}, k = {a.k})", "",
           f"{a.rounds} rounds, the three legs alternating, each leg a fresh process; per leg {a.warmup} windows of warm-up, then {a.windows} windows timed one by "
           "one (host clock around a device synchronise, the pipelined optimizer's tail of the previous window included).", "",
           f"| leg | updates per {n} sprites | median ms per round | median of all | min | max | sprites/s (median) |", "|---|---|---|---|---|---|---|"]
    for name, _ in legs:
        allw = [t for r in ms[name] for t in r]
        med = statistics.median(allw)
        out.append(f"| {name} | {a.k if name == 'plain' else 1} | {' / '.join(f'{statistics.median(r):.3f}' for r in ms[name])} | {med:.3f} | {min(allw):.3f} | "
                   f"{max(allw):.3f} | {1e3 * n / med:.0f} |")
    out += ["", "## The passes alone (HIP events around each launch, 10 warm-up launches, 50 timed, one process)", "",
            "| pass | range | elements | median us | min | max | GB/s (median) |", "|---|---|---|---|---|---|---|"]
    for r in op["rows"]:
        out.append(f"| {r['pass']} | {r['range']} | {r['elems']} | {r['us_median']:.1f} | {r['us_min']:.1f} | {r['us_max']:.1f} | {r['GBps_median']:.0f} |")
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
