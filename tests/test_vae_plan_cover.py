"""The in-situ batch sizes cover the plan: every way the VAE step launches a layer at batch 1..128 is launched at a batch size
tests/test_vae_insitu_gpu.py checks layer by layer.

The kernel, tile, split and fusion of every conv, GroupNorm-backward and weight-gradient launch are functions of the batch size (the
choosers of lo_conv_select.hip, lo_norm.hip, lo_wgrad.hip switch on workgroup counts, tiles per sample, K steps per split).
lo_vae_layer_plan_ex names them without a device, from the same helper calls the executor makes, and the executor refuses a launch
whose own choice differs from it.  Here the query runs for batch 1..128 in both operand modes with default knobs, planning for the
256 compute units of an MI355X, and each layer's answer is reduced to two keys:
  the layer's SIGNATURE   the whole answer -- every launch of the layer together, so that a kernel is also seen beside each neighbour it
                          hands rows to -- except for the weight gradient's counts, which grow with the batch: splits launched and slabs
                          provided become two flags, splits == 1 and splits < slabs (the "no empty split" rule dropped a split: slabs exist
                          that nobody writes); K units per split and K units (32 B / 42 on enc1.1: kept raw, every batch would be its own
                          signature) are left out.  The K-split counts of the convs stay;
  the WEIGHT GRADIENT's   its own fields with those two flags and a third, the last split is shorter than the others -- what a different
                          unit count changes in the kernel.  Per launch, not joint: crossed with the layer signature it asks for 24
                          batch sizes instead of 16 and shows no kernel a new case.
In the fp8 mode the forward fields count, and the first key alone.

INSITU_BATCHES is the list tests/test_vae_insitu_gpu.py imports.  The tests: every (layer, mode, signature) of 1..128 occurs at a listed
batch; no listed batch can go (each holds a signature no other listed batch has), so the list is not longer than the cover needs.
"""
import ctypes as C
import functools

LATENT = 64
CUS = 256                 # MI355X, SPX: what a handle made without a device is told to plan for
BATCHES = range(1, 129)
MODES = {"fp16": 0, "fp8": 1}          # lo_vae_create_ex flags
LAYERS = [(f"enc{s}.{k}", 0, s, k) for s in range(4) for k in range(3)] + [(f"dec{s}", 1, s, 0) for s in range(4)]
FIELDS = 40               # LO_VAE_PLAN_FIELDS

# default knobs, run in-process by tests/test_vae_insitu_gpu.py; what each batch adds is in that module's docstring
INSITU_BATCHES = {
    "fp16": (1, 2, 5, 7, 9, 10, 16, 32, 40, 45, 46, 56, 64, 65, 96, 128),
    "fp8": (2, 32, 64, 128),
}

_CONV_KERNELS = {0: "-", 1: "igemm", 2: "igemm-splitK", 3: "igemm-e4m3", 4: "conv3x3_pp", 5: "convt4_patch", 6: "convs2d_patch"}
_GNB_FORMS = {-1: "in-dgrad-epilogue", 0: "slab+one-pass", 1: "apply-only", 2: "one-pass", 3: "reduce+apply"}
_WG_KERNELS = {-1: "first-conv", 0: "wgrad3x3_mt", 1: "wgrad_s2_mt", 2: "wgrad_tn"}


@functools.lru_cache(maxsize=None)
def layer_plans(B, mode):
    """{layer name: the FIELDS ints of lo_vae_layer_plan_ex} at batch B, default knobs"""
    from lunaris_orion_amd import _lib
    h = C.c_void_p()
    _lib.check(_lib.lib.lo_vae_create_ex(B, LATENT, MODES[mode], C.byref(h)), "lo_vae_create_ex")
    try:
        rc = _lib.lib.lo_vae_plan_assume_cus(h, CUS)
        assert rc in (0, -3), rc       # -3: the process has a device, the handle plans for that one
        out = {}
        for name, dec, s, k in LAYERS:
            info = (C.c_int * FIELDS)()
            _lib.check(_lib.lib.lo_vae_layer_plan_ex(h, dec, s, k, info, FIELDS), "lo_vae_layer_plan_ex")
            out[name] = tuple(info)
        return out
    finally:
        _lib.lib.lo_vae_destroy(h)


def signature(info, mode):
    if mode == "fp8":
        return tuple(info[:18])
    return tuple(info[:34]) + (int(info[34] == 1), int(info[34] < info[35]), info[37], info[38])


def wgrad_signature(info):
    splits, slabs, per, units = info[34], info[35], info[36], info[39]
    return tuple(info[31:34]) + (int(splits == 1), int(splits < slabs), int(per > 0 and units % per != 0), info[37], info[38])


def keys(name, info, mode):
    out = [(name, "layer", signature(info, mode))]
    if mode == "fp16":
        out.append((name, "weight gradient", wgrad_signature(info)))
    return out


def describe(info):
    """one line that names the kernels and tiles of a layer's launches (the raw answer, counts included)"""
    def conv(f):
        if f[0] == 0:
            return "-"
        tile = f"{f[4]}x{f[5]}x{f[2]}" if f[0] == 4 else (f"{f[1]}x{f[2]}x{f[3]}" if f[0] in (1, 2, 3) else "")
        return f"{_CONV_KERNELS[f[0]]} {tile} rows {f[6]} nt {f[7]}" + (f" K/{f[8]}" if f[8] else "")
    fwd = conv(info[9:18]) if info[9] else (conv(info[0:9]) if info[0] else f"first-conv rows {info[6]}")
    dg = conv(info[18:27]) + (" +gn-apply" if info[27] else "")
    gnb = f"{_GNB_FORMS[info[28]]} P1 {info[29]} P2 {info[30]}"
    wg = _WG_KERNELS[info[31]] if info[31] < 0 else (f"{_WG_KERNELS[info[31]]} tw {info[32]} convt {info[33]} splits {info[34]}/{info[35]} x {info[36]} "
                                                     f"of {info[39]} direct {info[37]} reduce {info[38]}")
    return f"fwd[{fwd}] dgrad[{dg}] gnb[{gnb}] wgrad[{wg}]"


def uncovered(listed):
    """[(layer, mode, first batch of 1..128 with the key, description, key)] for every key no batch of listed[mode] has"""
    out = []
    for mode in MODES:
        have = {k for B in listed[mode] for name, *_ in LAYERS for k in keys(name, layer_plans(B, mode)[name], mode)}
        seen = set()
        for B in BATCHES:
            for name, *_ in LAYERS:
                info = layer_plans(B, mode)[name]
                for key in keys(name, info, mode):
                    if key not in have and key not in seen:
                        seen.add(key)
                        out.append((name, mode, B, describe(info), key[1:]))
    return out


def test_query_refuses_a_short_buffer_and_a_handle_with_no_such_layer():
    from lunaris_orion_amd import _lib
    h = C.c_void_p()
    _lib.check(_lib.lib.lo_vae_create(8, LATENT, C.byref(h)))
    info = (C.c_int * FIELDS)()
    assert _lib.lib.lo_vae_layer_plan_ex(h, 0, 0, 1, info, FIELDS - 1) == -1
    assert _lib.lib.lo_vae_layer_plan_ex(h, 1, 0, 1, info, FIELDS) == -1
    assert _lib.lib.lo_vae_layer_plan_ex(h, 0, 3, 2, info, FIELDS) == 0
    _lib.lib.lo_vae_destroy(h)


def test_query_agrees_with_the_four_field_plan():
    """lo_vae_layer_plan's e4m3 flag, row count and split counts are the same decisions"""
    from lunaris_orion_amd import _lib
    for mode in MODES:
        for B in (2, 32, 64):
            h = C.c_void_p()
            _lib.check(_lib.lib.lo_vae_create_ex(B, LATENT, MODES[mode], C.byref(h)))
            for name, dec, s, k in LAYERS:
                i4 = (C.c_int * 4)()
                _lib.check(_lib.lib.lo_vae_layer_plan(h, dec, s, k, i4))
                info = layer_plans(B, mode)[name]
                assert (info[9] != 0) == bool(i4[0]), (mode, B, name)
                if not info[8]:
                    assert (info[15] if i4[0] else info[6]) == i4[1], (mode, B, name)
                # a planned split-K data gradient runs only where a producing layer's GroupNorm backward takes its slabs
                assert info[8] == i4[2] and info[26] in (0, i4[3]), (mode, B, name, tuple(i4), info)
            _lib.lib.lo_vae_destroy(h)


def test_every_signature_of_batch_1_to_128_occurs_at_an_insitu_batch():
    missing = uncovered(INSITU_BATCHES)
    assert not missing, "\n".join(f"{m} {n} first at batch {b}: {d}  signature {s}" for n, m, b, d, s in missing)


def test_no_insitu_batch_is_redundant():
    for mode, listed in INSITU_BATCHES.items():
        for b in listed:
            rest = dict(INSITU_BATCHES)
            rest[mode] = tuple(x for x in listed if x != b)
            assert uncovered(rest), f"{mode}: batch {b} covers nothing the other listed batches do not"
