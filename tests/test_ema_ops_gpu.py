"""`lo_ema_update`, the weight-EMA pass, through the C ABI: e <- e + (p - e)(1 - decay).

Every comparison is bitwise.  The kernel rounds subtract, multiply and add to fp32 one by one (no fma contraction), which is exactly what
numpy does with float32 arrays, so the expectation is `e + (p - e) * np.float32(omd)` and no tolerance is involved.  Buffers come from
tests/guarded.py: the exact element count with 1 MiB of guard band on each side, so a 16-byte access past an odd `n` shows.

Sizes: 1 and 3 (scalar tail only), 4 (one vector), 5 (vector + tail), 1023, 4 * 256 * 4 * 2 + 5 (two workgroups' worth of one unrolled
iteration, + tail: the unroll boundary), 1 048 583 (the 256-workgroup grid takes a second pass; odd tail)."""
import numpy as np
import pytest
import torch

from tests.guarded import check_guards, gin
from tests.hip_helpers import L as _L, sync

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 1023, 4 * 256 * 4 * 2 + 5, 1_048_583]


def _data(n, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)


def _expected(e, p, omd):
    out = e + (p - e) * np.float32(omd)
    assert out.dtype == np.float32
    return out


def _update(e_d, p_d, n, omd, gate=None, e_off=0):
    lib = _L()
    lib.check(lib.lib.lo_ema_update(e_d.data_ptr() + 4 * e_off, p_d.data_ptr() + 4 * e_off, n, omd, lib.ptr(gate), lib.stream_ptr()),
              "lo_ema_update")


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("decay", [0.5, 0.999])
@pytest.mark.parametrize("n", SIZES)
def test_ema_update_equals_numpy_float32(n, decay):
    e, p = _data(n, seed=n)
    omd = 1.0 - decay                                    # the host's double; ctypes rounds it to fp32 like np.float32()
    e_d, p_d = gin(torch.from_numpy(e)), gin(torch.from_numpy(p))
    _update(e_d, p_d, n, omd)
    sync()
    check_guards(e_d, p_d)
    assert np.array_equal(_bits(e_d), _expected(e, p, omd).view(np.uint32))
    assert np.array_equal(_bits(p_d), p.view(np.uint32))           # p is only read


@pytest.mark.parametrize("n", [5, 8197])
def test_gate_zero_leaves_every_bit_and_gate_one_is_the_plain_update(n):
    e, p = _data(n, seed=7)
    omd = 1.0 - 0.9
    for flag, want in ((0.0, e), (1.0, _expected(e, p, omd))):
        e_d, p_d = gin(torch.from_numpy(e)), gin(torch.from_numpy(p))
        gate = gin(torch.tensor([float("nan"), 0.25, flag], dtype=torch.float32))     # norm, clip coefficient, finite flag
        _update(e_d, p_d, n, omd, gate)
        sync()
        check_guards(e_d, p_d, gate)
        assert np.array_equal(_bits(e_d), want.view(np.uint32)), f"gate[2] = {flag}"


@pytest.mark.parametrize("n,m", [(8197, 64), (1_048_583, 64 * 5000)])
def test_two_launches_over_sub_ranges_equal_one_launch(n, m):
    e, p = _data(n, seed=3)
    omd = 1.0 - 0.999
    one, two, p_d = gin(torch.from_numpy(e)), gin(torch.from_numpy(e)), gin(torch.from_numpy(p))
    _update(one, p_d, n, omd)
    _update(two, p_d, m, omd)
    _update(two, p_d, n - m, omd, e_off=m)
    sync()
    check_guards(one, two, p_d)
    assert torch.equal(one.view(torch.int32), two.view(torch.int32))
    assert np.array_equal(_bits(one), _expected(e, p, omd).view(np.uint32))


def test_an_average_equal_to_the_parameters_stays_on_them():
    _, p = _data(8197, seed=5)
    e_d, p_d = gin(torch.from_numpy(p)), gin(torch.from_numpy(p))
    for _ in range(3):
        _update(e_d, p_d, p.size, 1.0 - 0.5)
    sync()
    check_guards(e_d, p_d)
    assert np.array_equal(_bits(e_d), p.view(np.uint32))


def test_bad_arguments_launch_nothing():
    lib = _L()
    e_d, p_d = gin(torch.zeros(8)), gin(torch.ones(8))
    st = lib.stream_ptr()
    assert lib.lib.lo_ema_update(e_d.data_ptr(), p_d.data_ptr(), 0, 0.1, None, st) == -1           # n = 0
    assert lib.lib.lo_ema_update(e_d.data_ptr() + 4, p_d.data_ptr(), 4, 0.1, None, st) == -1       # not 16-byte aligned
    assert lib.lib.lo_ema_update(e_d.data_ptr(), e_d.data_ptr() + 16, 8, 0.1, None, st) == -1      # overlap
    assert lib.lib.lo_ema_update(e_d.data_ptr(), p_d.data_ptr(), 8, 1.5, None, st) == -1           # 1 - decay outside [0, 1]
    sync()
    assert torch.equal(e_d, torch.zeros(8, device="cuda"))
