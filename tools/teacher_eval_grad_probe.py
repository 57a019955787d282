#!/usr/bin/env python
"""Three routes to `recon.grad` through a frozen LunarMoETeacher at batch 64, feature_dim 128 (dropout_rate 0 in all three, so that the
BatchNorm mode is the only difference), timed with device events and alternated inside one process; one JSON line.

  i    train mode: lo_teacher_forward_keep + lo_teacher_full_backward_dx (the only route before eval_input_grad existed)
  ii   eval mode, parameters live: lo_teacher_forward_keep_eval + lo_teacher_eval_backward with a flat gradient
  iii  eval mode, teacher.requires_grad_(False): the same with flat_grads = NULL (no parameter gradient computed)

  python tools/teacher_eval_grad_probe.py [--routes i,ii,iii] [--reps 7] [--warmup 2] [--batch 64]

Launch counts: one route per process under the profiler, e.g.
  rocprofv3 --kernel-trace --stats -d OUT -o iii -- python3 tools/teacher_eval_grad_probe.py --routes iii --reps 1 --warmup 0
then tools/rocpd_extract.py stats.  Results: profiles/teacher_eval_grad_ab.md.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lunaris_orion_amd.teacher import LunarMoETeacher  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--routes", default="i,ii,iii")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    routes = a.routes.split(",")
    torch.manual_seed(1)
    # the closed-form state and sprites of the tests: trained-looking running statistics instead of a fresh module's (0, 1)
    from oracle import teacher_ref as T
    from oracle import vae_ref as R
    t = LunarMoETeacher(feature_dim=128, dropout_rate=0.0, eval_input_grad=True)
    t.load_state_dict(T.closed_form_teacher_state())
    t = t.to("cuda")
    x = R.normalise_sprites(R.closed_form_sprites(a.batch)).cuda()
    finite = {}

    def step(route):
        t.train(route == "i")
        # i and iii: a frozen reward model (the train-mode path computes the parameter gradients regardless); ii: parameters live
        t.requires_grad_(route == "ii")
        xg = x.clone().requires_grad_()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        q = t(xg)["quality_scores"]
        e1.record()
        (-0.5 * q.mean()).backward()
        e2.record()
        torch.cuda.synchronize()
        assert xg.grad is not None
        finite[route] = finite.get(route, True) and bool(torch.isfinite(xg.grad).all())
        t.zero_grad(set_to_none=True)
        return e0.elapsed_time(e1), e1.elapsed_time(e2)

    for _ in range(a.warmup):
        for r in routes:
            step(r)
    ms = {r: [] for r in routes}
    for _ in range(a.reps):
        for r in routes:                            # alternated: drift of the clocks hits every route alike
            ms[r].append(step(r))
    res = {"batch": a.batch, "feature_dim": 128, "reps": a.reps, "unit": "ms"}
    for r in routes:
        tot = [f + b for f, b in ms[r]]
        res[r] = {"forward_median": round(statistics.median(f for f, _ in ms[r]), 3), "backward_median": round(statistics.median(b for _, b in ms[r]), 3),
                  "total_median": round(statistics.median(tot), 3), "total_min": round(min(tot), 3), "total_max": round(max(tot), 3)}
    res["finite"] = finite
    res["max_mem_GB"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
