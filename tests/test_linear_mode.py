"""CPU test of the one mode behind lo_vae_set_linear_factored (csrc/lo_vae.h: LoLinearMode and its predicates): what each mode
reports back, which numbers and batches are refused, and the two mode-3 queries.  lo_vae_create plans on the host: no device."""
import ctypes as C

import pytest


@pytest.fixture()
def engines():
    from lunaris_orion_amd import _lib
    made = []

    def make(B, L):
        h = C.c_void_p()
        _lib.check(_lib.lib.lo_vae_create(B, L, C.byref(h)), "lo_vae_create")
        made.append(h)
        return h
    yield make
    for h in made:
        _lib.lib.lo_vae_destroy(h)


def test_linear_mode_round_trip_limits_and_mode3_queries(engines):
    from lunaris_orion_amd import _lib
    lib = _lib.lib
    h = engines(8, 64)
    # the flat buffer lacks the two matrices after a step in modes 1 and 3 only (mode 2 writes the averaged matrices out itself)
    for mode, reported in ((0, 0), (1, 1), (2, 0), (3, 3)):
        assert lib.lo_vae_set_linear_factored(h, mode) == 0, mode
        assert lib.lo_vae_linear_factored(h) == reported, mode
    for bad in (-1, 4):
        assert lib.lo_vae_set_linear_factored(h, bad) == -1 and b"mode must be" in lib.lo_last_error()
        assert lib.lo_vae_linear_factored(h) == 3              # a refused call changes nothing
    # batch 129 is above the rank the factored passes are built for: only "off" is accepted
    big = engines(129, 64)
    for mode in (1, 2, 3):
        assert lib.lo_vae_set_linear_factored(big, mode) == -1 and b"129" in lib.lo_last_error()
        assert lib.lo_vae_linear_factored(big) == 0
    assert lib.lo_vae_set_linear_factored(big, 0) == 0
    # Gram scratch of the gathered norm: two [world Bp]^2 fp32 matrices while world * Bp <= 512 (Bp = 32 at batch 8), else 0
    Bp = 32
    for world in (1, 2, 8, 16, 17, 64):
        want = 2 * (world * Bp) ** 2 * 4 if world * Bp <= 512 else 0
        assert lib.lo_vae_gathered_scratch_bytes(h, world) == want, world
    # lo_vae_gathered_early_norm belongs to mode 3: the state error (-3) comes before anything is read or launched
    buf = (C.c_float * 4)()
    p = C.addressof(buf)
    for mode in (0, 1, 2):
        assert lib.lo_vae_set_linear_factored(h, mode) == 0
        assert lib.lo_vae_gathered_early_norm(h, p, 1, p, p, p, None) == -3, mode
        assert b"mode 3" in lib.lo_last_error()
