"""Reference composition for LunarisCoreVAE(attention=True): oracle.vae_ref's own pieces (`_conv_gn_mish`, `res_block`, `vae_losses`,
`vae_objective`, `clip_coef`, `adamw_step`) with `R.self_attention_2d` -- pinned to the reference's class by tests/golden/selfattn2d.npz
-- inserted where the model has its two sites: on the encoder's stage-4 output before the flatten, and on decoder.fc's output before
up1.  TEST INFRASTRUCTURE ONLY (plain PyTorch fp32 on the CPU).

Fixture weights: `R.closed_form_params(L)` plus `R.closed_form_tensor("<site>.<name>", shape)` for the six conv tensors of a site and
gamma = 0.5 at both.  `saturated=True` multiplies the query and key WEIGHTS by 4: energies of a few hundred, a near one-hot softmax,
`exp` overflowing fp32 without the max subtraction.
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import vae_ref as R

SITES = ("encoder.attn", "decoder.attn")
# a site's tensors in state_dict order: the module's own parameter first, then its three 1x1 convs
SITE_SHAPES = OrderedDict([("gamma", (1,)), ("query_conv.weight", (64, 512, 1, 1)), ("query_conv.bias", (64,)),
                           ("key_conv.weight", (64, 512, 1, 1)), ("key_conv.bias", (64,)),
                           ("value_conv.weight", (512, 512, 1, 1)), ("value_conv.bias", (512,))])
ATTN_EXTRA_ELEMS = 2 * sum(int(torch.Size(s).numel()) for s in SITE_SHAPES.values())      # 656 642


def attention_param_shapes(latent_dim):
    """The 86 parameter tensors of LunarisCoreVAE(attention=True) in state_dict order."""
    out = OrderedDict()
    for k, shp in R.param_shapes(latent_dim).items():
        for site, first_after in zip(SITES, ("encoder.fc_mu.weight", "decoder.up1.0.weight")):
            if k == first_after:
                for n, s in SITE_SHAPES.items():
                    out[f"{site}.{n}"] = s
        out[k] = shp
    return out


def attention_params(latent_dim, gamma=0.5, saturated=False):
    P72 = R.closed_form_params(latent_dim)
    out = OrderedDict()
    for k, shp in attention_param_shapes(latent_dim).items():
        if k in P72:
            out[k] = P72[k]
        elif k.endswith(".gamma"):
            out[k] = torch.full((1,), float(gamma))
        else:
            t = R.closed_form_tensor(k, shp)
            if saturated and k.endswith(("query_conv.weight", "key_conv.weight")):
                t = t * 4.0
            out[k] = t
    return out


def site_attention(x, P, site):
    g = lambda n: P[f"{site}.{n}"]
    return R.self_attention_2d(x, g("query_conv.weight"), g("query_conv.bias"), g("key_conv.weight"), g("key_conv.bias"),
                               g("value_conv.weight"), g("value_conv.bias"), g("gamma"))


def encoder_forward(x, P):
    skips = []
    h = x
    for i, (name, _cin, _cout) in enumerate(R.ENC_STAGES):
        p = f"encoder.{name}"
        h = R._conv_gn_mish(h, P, p + ".0", p + ".1", 2)
        h = R.res_block(h, P, p + ".3")
        if i < 3:
            skips.append(h)
    h = site_attention(h, P, SITES[0])
    flat = h.flatten(1)
    mu = F.linear(flat, P["encoder.fc_mu.weight"], P["encoder.fc_mu.bias"])
    logvar = F.linear(flat, P["encoder.fc_logvar.weight"], P["encoder.fc_logvar.bias"])
    return mu, logvar, skips


def decoder_forward(z, skips, P):
    B = z.shape[0]
    h = F.linear(z, P["decoder.fc.weight"], P["decoder.fc.bias"]).view(B, 512, 8, 8)
    h = site_attention(h, P, SITES[1])
    for i, (name, _cin, _cout) in enumerate(R.DEC_STAGES):
        p = f"decoder.{name}"
        h = R._conv_gn_mish(h, P, p + ".0", p + ".1", 2, transposed=True)
        need = 3 - i
        if i < 3 and len(skips) >= need:
            h = h + skips[need - 1]
    return torch.tanh(F.conv2d(h, P["decoder.final_conv.weight"], P["decoder.final_conv.bias"], padding=1))


def vae_forward(x, eps, P):
    mu, logvar, skips = encoder_forward(x, P)
    z = mu + eps * torch.exp(0.5 * logvar)
    return decoder_forward(z, skips, P), mu, logvar


class AttnOracleTrainer(R.OracleTrainer):
    """R.OracleTrainer.step with the composition's forward: same losses, objective, clip, AdamW and scheduler."""

    def step(self, x, eps, mean_advantage=0.0, do_update=True):
        for p in self.P.values():
            p.grad = None
        recon, mu, logvar = vae_forward(x, eps, self.P)
        recon_loss, kl_loss = R.vae_losses(recon, x, mu, logvar)
        vae_loss, pg_loss = R.vae_objective(recon_loss, kl_loss, self.recon_weight, self.kl_weight, mean_advantage, self.accum)
        vae_loss.backward()
        grads = [p.grad for p in self.P.values()]
        total, coef = R.clip_coef(grads, self.max_grad_norm)
        out = dict(recon=recon.detach(), mu=mu.detach(), logvar=logvar.detach(), recon_loss=float(recon_loss.detach()),
                   kl_loss=float(kl_loss.detach()), vae_loss=float(vae_loss.detach()), pg_loss=float(pg_loss.detach()),
                   grad_norm=float(total), lr=self.lr(), grads=OrderedDict((k, p.grad.detach().clone()) for k, p in self.P.items()))
        if do_update:
            lr = self.lr()
            self.opt_steps += 1
            with torch.no_grad():
                for k, p in self.P.items():
                    R.adamw_step(p, p.grad * coef, self.m[k], self.v[k], self.opt_steps, lr, weight_decay=self.weight_decay)
        return out


_STEP_CACHE = {}


def reference_step(L, B, gamma=0.5):
    """One composition step (no update) at the fixture weights, computed once per (L, B, gamma) and shared; callers must not modify it."""
    key = (L, B, float(gamma))
    if key not in _STEP_CACHE:
        x = R.normalise_sprites(R.closed_form_sprites(B))
        eps = R.closed_form_eps(B, L)
        _STEP_CACHE[key] = AttnOracleTrainer(attention_params(L, gamma)).step(x, eps, 0.0, do_update=False)
    return _STEP_CACHE[key]
