"""Opt-in bottleneck self-attention, the parts that need no GPU: the module surface (86 state_dict keys), the native plan's parameter
table with LO_VAE_ATTN, the refusals (fp8 operands, unknown flag bits, data parallel) and the CLI flag."""
import ctypes as C
import os
import sys

import pytest
import torch

from tests import attention_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO_VAE_FP8_FWD, LO_VAE_ATTN = 1, 2


def _lib():
    from lunaris_orion_amd import _lib
    return _lib


def test_attention_model_has_the_86_tensors_in_order_and_gamma_zero():
    from lunaris_orion_amd.vae import LunarisCoreVAE, SelfAttention2d
    m = LunarisCoreVAE(256, attention=True)
    want = A.attention_param_shapes(256)
    sd = m.state_dict()
    assert len(sd) == 86 and list(sd.keys()) == list(want.keys())
    assert [k for k, _ in m.named_parameters()] == list(want.keys())
    for k, shp in want.items():
        assert tuple(sd[k].shape) == shp, k
    assert sum(p.numel() for p in m.parameters()) == 36468869 == 35812227 + A.ATTN_EXTRA_ELEMS and A.ATTN_EXTRA_ELEMS == 656642
    assert isinstance(m.encoder.attn, SelfAttention2d) and isinstance(m.decoder.attn, SelfAttention2d)
    assert float(sd["encoder.attn.gamma"]) == 0.0 and float(sd["decoder.attn.gamma"]) == 0.0
    new = [k for k in sd if ".attn." in k]
    assert len(new) == 14 and set(new) == {f"{s}.{n}" for s in A.SITES for n in A.SITE_SHAPES}
    # the sites sit after down4 / before fc_mu and after fc / before up1
    keys = list(sd.keys())
    assert keys[keys.index("encoder.attn.gamma") - 1].startswith("encoder.down4.") and keys[keys.index("encoder.attn.value_conv.bias") + 1] == "encoder.fc_mu.weight"
    assert keys[keys.index("decoder.attn.gamma") - 1] == "decoder.fc.bias" and keys[keys.index("decoder.attn.value_conv.bias") + 1] == "decoder.up1.0.weight"
    # the fixture parameter set loads strictly
    m.load_state_dict(A.attention_params(256), strict=True)
    assert float(m.decoder.attn.gamma) == 0.5


def test_default_model_is_unchanged():
    from lunaris_orion_amd.vae import LunarisCoreVAE
    from oracle import vae_ref as R
    torch.manual_seed(3)
    m = LunarisCoreVAE(256)
    assert not m.attention and m._engine_flags() == 0
    assert list(m.state_dict().keys()) == list(R.param_shapes(256).keys()) and len(m.state_dict()) == 72
    assert sum(p.numel() for p in m.parameters()) == 35812227
    assert not hasattr(m.encoder, "attn") and not hasattr(m.decoder, "attn")
    # the attention model draws its 72 shared tensors from the same generator positions up to the first site
    torch.manual_seed(3)
    ma = LunarisCoreVAE(256, attention=True)
    assert torch.equal(m.state_dict()["encoder.down4.3.conv2.0.weight"], ma.state_dict()["encoder.down4.3.conv2.0.weight"])


def _table(h):
    lib = _lib().lib
    n = lib.lo_vae_num_params(h)
    return [(lib.lo_vae_param_offset(h, i), lib.lo_vae_param_numel(h, i)) for i in range(n)], lib.lo_vae_flat_elems(h)


@pytest.mark.parametrize("L", [256, 512])
def test_plan_parameter_table_with_attention(L):
    lib = _lib().lib
    h = C.c_void_p()
    assert lib.lo_vae_create_ex(8, L, LO_VAE_ATTN, C.byref(h)) == 0, lib.lo_last_error()
    try:
        table, flat = _table(h)
    finally:
        lib.lo_vae_destroy(h)
    shapes = A.attention_param_shapes(L)
    names = list(shapes.keys())
    assert len(table) == 86
    for (off, numel), (k, shp) in zip(table, shapes.items()):
        assert numel == torch.Size(shp).numel(), k
        assert off % 64 == 0, k
    assert sum(n for _, n in table) == (35812227 if L == 256 else sum(torch.Size(s).numel() for s in shapes.values()) - A.ATTN_EXTRA_ELEMS) + A.ATTN_EXTRA_ELEMS
    spans = sorted(table)
    for (o0, n0), (o1, _n1) in zip(spans, spans[1:]):
        assert o0 + n0 <= o1, "parameter ranges overlap"
    assert spans[-1][0] + spans[-1][1] <= flat
    off = {k: t[0] for k, t in zip(names, table)}
    for n in A.SITE_SHAPES:
        assert off[f"encoder.attn.{n}"] < off["encoder.fc_mu.weight"] and off[f"encoder.attn.{n}"] > off["encoder.down4.3.conv2.1.bias"]
        assert off[f"decoder.attn.{n}"] > off["decoder.fc.bias"] and off[f"decoder.attn.{n}"] < off["decoder.up1.0.weight"]
    # the [2L, 32768] head matrix and the adjacent head biases are kept
    assert off["encoder.fc_logvar.weight"] == off["encoder.fc_mu.weight"] + L * 32768
    assert off["encoder.fc_logvar.bias"] == off["encoder.fc_mu.bias"] + L
    # a site's three weights are one [640][512] matrix and its three biases one [640] vector
    for s in A.SITES:
        assert off[f"{s}.key_conv.weight"] == off[f"{s}.query_conv.weight"] + 64 * 512
        assert off[f"{s}.value_conv.weight"] == off[f"{s}.key_conv.weight"] + 64 * 512
        assert off[f"{s}.key_conv.bias"] == off[f"{s}.query_conv.bias"] + 64 and off[f"{s}.value_conv.bias"] == off[f"{s}.key_conv.bias"] + 64


@pytest.mark.parametrize("L", [256, 512])
def test_flags_zero_is_the_plain_plan(L):
    lib = _lib().lib
    h0, h1 = C.c_void_p(), C.c_void_p()
    assert lib.lo_vae_create(8, L, C.byref(h0)) == 0 and lib.lo_vae_create_ex(8, L, 0, C.byref(h1)) == 0
    try:
        assert _table(h0) == _table(h1) and len(_table(h0)[0]) == 72
        assert lib.lo_vae_workspace_bytes(h0) == lib.lo_vae_workspace_bytes(h1)
    finally:
        lib.lo_vae_destroy(h0)
        lib.lo_vae_destroy(h1)


def test_refused_flag_combinations_say_why():
    lib = _lib().lib
    h = C.c_void_p()
    assert lib.lo_vae_create_ex(8, 256, LO_VAE_ATTN | LO_VAE_FP8_FWD, C.byref(h)) == -1
    assert b"LO_VAE_FP8_FWD" in lib.lo_last_error() and not h.value
    assert lib.lo_vae_create_ex(8, 256, LO_VAE_ATTN | 4, C.byref(h)) == -1
    assert b"unknown flag bits" in lib.lo_last_error() and not h.value
    from lunaris_orion_amd.vae import LunarisCoreVAE
    with pytest.raises(ValueError, match="fp8"):
        LunarisCoreVAE(256, mfma_precision="fp8", attention=True)


def test_debug_tensor_names_need_the_flag():
    lib = _lib().lib
    h = C.c_void_p()
    assert lib.lo_vae_create_ex(2, 64, 0, C.byref(h)) == 0
    off, dims, eb = C.c_size_t(), (C.c_int * 4)(), C.c_int()
    try:
        assert lib.lo_vae_debug_tensor_ex(h, 11, 0, 0, C.byref(off), dims, C.byref(eb)) != 0 and b"LO_VAE_ATTN" in lib.lo_last_error()
    finally:
        lib.lo_vae_destroy(h)
    assert lib.lo_vae_create_ex(2, 64, LO_VAE_ATTN, C.byref(h)) == 0
    try:
        seen = set()
        for which in range(11, 23):
            assert lib.lo_vae_debug_tensor_ex(h, which, 0, 0, C.byref(off), dims, C.byref(eb)) == 0
            assert list(dims) == [2, 8, 8, 640 if which in (11, 12, 19, 20) else 512] and eb.value == 2
            assert off.value + 2 * 2 * 64 * dims[3] <= lib.lo_vae_workspace_bytes(h)
            seen.add(off.value)
        assert len(seen) == 12
    finally:
        lib.lo_vae_destroy(h)


def test_data_parallel_with_attention_is_not_implemented(monkeypatch):
    from lunaris_orion_amd import _lib as lib, trainer
    from lunaris_orion_amd.vae import LunarisCoreVAE
    monkeypatch.setattr(lib, "require_gpu", lambda: None)

    class Sync:
        world = 2

        def __call__(self, flat):
            pass

    with pytest.raises(NotImplementedError, match="attention"):
        trainer.VAEStepper(LunarisCoreVAE(64, attention=True), grad_sync=Sync())
    with pytest.raises(NotImplementedError, match="attention"):
        trainer.HybridStepper(LunarisCoreVAE(64, attention=True), None, grad_sync=Sync())


def test_cli_flag_parses_and_defaults_to_off():
    sys.path.insert(0, ROOT)
    import train_hybrid
    p = train_hybrid.build_parser()
    assert p.parse_args(["--data_dir", "x"]).vae_attention is False
    assert p.parse_args(["--data_dir", "x", "--vae_attention"]).vae_attention is True


def test_reference_composition_moves_the_outputs():
    """gamma = 0.5 against gamma = 0 on the oracle: the shift is at least 10x the GPU tests' 5e-3 output tolerance, so a kernel that
    ignored the attention could not pass them; and the saturated fixture really needs the max subtraction."""
    from oracle import vae_ref as R
    L, B = 64, 2
    x = R.normalise_sprites(R.closed_form_sprites(B))
    eps = R.closed_form_eps(B, L)
    with torch.no_grad():
        r1, mu1, _ = A.vae_forward(x, eps, A.attention_params(L, 0.5))
        r0, mu0, _ = A.vae_forward(x, eps, A.attention_params(L, 0.0))
        p72 = R.closed_form_params(L)
        rp, mup, _ = R.vae_forward(x, eps, p72)
        assert torch.equal(r0, rp) and torch.equal(mu0, mup)          # gamma = 0 is the plain model
        assert (mu1 - mu0).abs().max().item() >= 0.05 and (r1 - r0).abs().max().item() >= 0.05
        Ps = A.attention_params(L, 0.5, saturated=True)
        h = x
        for name, _ci, _co in R.ENC_STAGES:
            h = R.res_block(R._conv_gn_mish(h, Ps, f"encoder.{name}.0", f"encoder.{name}.1", 2), Ps, f"encoder.{name}.3")
        q = torch.nn.functional.conv2d(h, Ps["encoder.attn.query_conv.weight"], Ps["encoder.attn.query_conv.bias"]).flatten(2)
        k = torch.nn.functional.conv2d(h, Ps["encoder.attn.key_conv.weight"], Ps["encoder.attn.key_conv.bias"]).flatten(2)
        e = torch.bmm(q.transpose(1, 2), k)
        assert e.abs().max().item() > 89.0                              # exp overflows fp32 above 88.7
