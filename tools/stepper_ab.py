#!/usr/bin/env python
"""Bitwise A/B of the steppers' host side: SHA-256 of the raw bytes of what every step of every scenario leaves behind.

Run it once in each of two trees (it imports the package of the tree it lies in and, through tests/stepper_scenarios.py, uses only
names both have), each in a process of its own, then compare:

    python tools/stepper_ab.py --out a.json          # in tree A
    python tools/stepper_ab.py --out b.json          # in tree B
    python tools/stepper_ab.py --compare a.json b.json

The scenario table is the one of tests/test_stepper_trace_gpu.py (batch 2, latent 64; teacher feature_dim 128, 4 experts, dropout 0.1 on
a fixed stream; closed-form state, sprites and eps from oracle/).  After every `step()` call: recon, the JSON text of `metrics()`,
`flat_grads()` unless an accumulation window is open, the VAE's flat buffer and AdamW moments, the weight EMA where one is kept, and
for the hybrid stepper `t_grads` and the teacher's flat buffer."""
import argparse
import hashlib
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def scenario_digests(sc, out):
    import torch
    from tests import stepper_scenarios as S

    def after_call(i, st, teacher, recon, window_open):
        tag = f"{sc['name']}/{i}"
        met = st.metrics()
        st.synchronize_parameters()
        torch.cuda.synchronize()
        out[f"{tag}/recon"] = digest(recon)
        out[f"{tag}/metrics"] = json.dumps(met, sort_keys=True)
        if not window_open:
            out[f"{tag}/flat_grads"] = digest(st.flat_grads())
        out[f"{tag}/vae_flat"] = digest(st.vae.flat_parameters())
        out[f"{tag}/exp_avg"] = digest(st.exp_avg)
        out[f"{tag}/exp_avg_sq"] = digest(st.exp_avg_sq)
        if getattr(st, "ema", None) is not None:
            out[f"{tag}/ema"] = digest(st.ema)
        if teacher is not None:
            out[f"{tag}/t_grads"] = digest(st.t_grads)
            out[f"{tag}/teacher_flat"] = digest(teacher._flat)

    S.run_scenario(sc, after_call)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="write the digests here as JSON (they are printed either way)")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two digest files; exit 1 if any entry differs")
    args = ap.parse_args()
    if args.compare:
        a, b = (json.load(open(p)) for p in args.compare)
        diff = sorted(k for k in a.keys() | b.keys() if a.get(k) != b.get(k))
        for k in diff:
            print(f"DIFFERS {k}: {a.get(k)} | {b.get(k)}")
        print(f"{len(a)} / {len(b)} entries, {len(diff)} differ")
        sys.exit(1 if diff else 0)
    warnings.simplefilter("ignore", UserWarning)
    from tests import stepper_scenarios as S
    out = {}
    for sc in S.SCENARIOS:
        scenario_digests(sc, out)
    for k in sorted(out):
        print(out[k] if len(out[k]) <= 64 else out[k][:200], k)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=0, sort_keys=True)


if __name__ == "__main__":
    main()
