#!/usr/bin/env python
"""Bitwise A/B of the teacher's host side: SHA-256 of the raw bytes of everything the module's routes and the hybrid step produce.

Run it once in each of two trees (it imports the package of the tree it lies in and uses only names both have), then compare:

    python tools/teacher_host_ab.py --out a.json          # in tree A
    python tools/teacher_host_ab.py --out b.json          # in tree B
    python tools/teacher_host_ab.py --compare a.json b.json

Batch 2, latent 256, feature_dim 128, dropout 0.1 on a fixed stream; closed-form state, sprites and eps from oracle/."""
import argparse
import hashlib
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, L, DROP_SEED = 2, 256, 0x5EEDD209C0FFEE11


def digest(t):
    if t is None:
        return "none"
    if not hasattr(t, "detach"):
        return repr(t)
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def module_scenarios(out):
    import torch
    from lunaris_orion_amd.teacher import LunarMoETeacher
    from oracle import teacher_ref as T
    from oracle import vae_ref as R
    state = T.closed_form_teacher_state()
    images = R.normalise_sprites(R.closed_form_sprites(B)).cuda()
    # name: (train mode, x requires grad, frozen parameters, constructor arguments)
    scenarios = {
        "heads": (True, False, False, {}),
        "train_dx": (True, True, False, {}),
        "eval_dx_live": (False, True, False, {"eval_input_grad": True}),
        "eval_dx_frozen": (False, True, True, {"eval_input_grad": True}),
        "eval_odd_row": (False, False, False, {"full_backward": True}),
    }
    for name, (train, x_rg, frozen, kw) in scenarios.items():
        m = LunarMoETeacher(num_experts=4, feature_dim=128, dropout_rate=0.1, **kw)
        m.load_state_dict(state)
        m = m.to("cuda").train(train)
        if frozen:
            m.requires_grad_(False)
        m.set_dropout_stream(DROP_SEED, exact_next=True)
        x = images.clone().requires_grad_(x_rg)
        o = m.forward(x)
        (0.5 * -torch.mean(o["quality_scores"]) + o["expert_weights"].square().sum()).backward()
        torch.cuda.synchronize()
        for k, v in o.items():
            out[f"{name}/out/{k}"] = digest(v)
        out[f"{name}/x.grad"] = digest(x.grad)
        for k, p in m.named_parameters():
            out[f"{name}/grad/{k}"] = digest(p.grad)
        for k, v in m.state_dict().items():
            if "running" in k or "num_batches" in k:
                out[f"{name}/state/{k}"] = digest(v)
    # the coefficient form after a plain train-mode forward
    m = LunarMoETeacher(num_experts=4, feature_dim=128, dropout_rate=0.1)
    m.load_state_dict(state)
    m = m.to("cuda").train()
    m.set_dropout_stream(DROP_SEED, exact_next=True)
    with torch.no_grad():
        o = m.forward(images)
    out["coef_form/flat"] = digest(m.full_backward(images, o["expert_weights"], 0.5))


def stepper_scenarios(out):
    import torch
    from lunaris_orion_amd.teacher import LunarMoETeacher
    from lunaris_orion_amd.trainer import HybridStepper
    from lunaris_orion_amd.vae import LunarisCoreVAE
    from oracle import teacher_ref as T
    from oracle import vae_ref as R
    images = R.normalise_sprites(R.closed_form_sprites(B)).cuda()
    for full in (False, True):
        for weight in (0.0, 0.05):
            tag = f"step/{'full' if full else 'heads'}/w{weight}"
            vae = LunarisCoreVAE(latent_dim=L)
            vae.load_state_dict(R.closed_form_params(L))
            vae = vae.to("cuda")
            t = LunarMoETeacher(num_experts=4, feature_dim=128, dropout_rate=0.1)
            t.load_state_dict(T.closed_form_teacher_state())
            t = t.to("cuda").train()
            t.set_dropout_stream(0x5EED0F8)
            st = HybridStepper(vae, t, lr=1e-4, teacher_lr=1e-4, teacher_full_backward=full, reward_grad_weight=weight)
            for s in range(2):
                recon, mu, logvar = st.step(images, s, R.closed_form_eps(B, L, salt=s).cuda())
                met = st.metrics()
                torch.cuda.synchronize()
                out[f"{tag}/{s}/recon"] = digest(recon)
                out[f"{tag}/{s}/metrics"] = json.dumps(met, sort_keys=True)
                out[f"{tag}/{s}/t_grads"] = digest(st.t_grads)
                out[f"{tag}/{s}/vae_flat"] = digest(vae.flat_parameters())
                out[f"{tag}/{s}/teacher_flat"] = digest(t._flat)


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
    out = {}
    module_scenarios(out)
    stepper_scenarios(out)
    for k in sorted(out):
        print(out[k] if len(out[k]) <= 64 else out[k][:200], k)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=0, sort_keys=True)


if __name__ == "__main__":
    main()
