"""`lo_teacher_debug_tensor`: the read-only query for where a teacher forward leaves its tensors (include/lunaris_hip.h has the table).
Plan level: no GPU, nothing is launched.  tests/test_teacher_insitu_gpu.py reads the tensors it names."""
import ctypes as C

import pytest

SPACE1_FE = [(0, 0, 32), (1, 0, 32), (1, 1, 32), (1, 2, 32), (2, 0, 192), (3, 0, 192), (4, 0, 128), (5, 0, 128)]     # (kind, l, channels)


def _lib():
    from lunaris_orion_amd import _lib
    return _lib.lib


def _q(lib, h, space, which, e=0, l=0):
    off, dims, eb = C.c_size_t(), (C.c_int * 4)(), C.c_int()
    rc = lib.lo_teacher_debug_tensor(h, space, which, e, l, C.byref(off), dims, C.byref(eb))
    return rc, off.value, list(dims), eb.value


def _handle(lib, B, F):
    h = C.c_void_p()
    assert lib.lo_teacher_create_ex(B, 4, F, 64, 0, C.byref(h)) == 0, lib.lo_last_error()
    return h


@pytest.mark.parametrize("B,F", [(3, 128), (1, 256)])
def test_every_kind_lies_inside_its_buffer_and_overlaps_no_other(B, F):
    lib = _lib()
    h = _handle(lib, B, F)
    try:
        spans = []

        def ok(space, which, e, l, want_dims, want_eb):
            rc, off, dims, eb = _q(lib, h, space, which, e, l)
            assert rc == 0, (space, which, e, l, lib.lo_last_error())
            assert dims == want_dims and eb == want_eb, (space, which, e, l, dims, eb)
            n = dims[0] * dims[1] * dims[2] * dims[3] * eb
            assert off % 256 == 0 and off + n <= (lib.lo_teacher_full_backward_bytes(h) if space else lib.lo_teacher_workspace_bytes(h))
            spans.append((space, off, off + n, (which, e, l)))

        for which, l, ch in SPACE1_FE:
            ok(1, which, 0, l, [B, 128, 128, ch], 2)
        for e in range(4):
            for l in range(3):
                ok(1, 6, e, l, [B, 128, 128, F], 2)
                for which in (7, 8, 12, 13):
                    ok(1, which, e, l, [B, 128, 128, F], 2)
                ok(1, 9, e, l, [B, 128, 128, 3 * F], 2)
                ok(1, 10, e, l, [B, 8, 128, F], 2)
                ok(1, 11, e, l, [B, 8, 128, F], 2)
                ok(1, 15, e, l, [1, 1, F, 2], 4)
                ok(1, 16, e, l, [1, 1, F, 2], 4)
                for which in (14, 17, 18):
                    if F != 128 and l == 0:
                        ok(1, which, e, l, [B, 128, 128, F] if which == 14 else [1, 1, F, 2], 2 if which == 14 else 4)
                    else:
                        rc = _q(lib, h, 1, which, e, l)[0]
                        assert rc != 0 and b"shortcut" in lib.lo_last_error()
        for l, ch in ((3, 32), (4, 64), (5, 64), (6, 64), (7, 128)):
            ok(1, 19, 0, l, [1, 1, ch, 2], 4)
        ok(1, 20, 0, 0, [1, 1, 32, 2], 4)
        want0 = {0: [B, 128, 128, 32], 1: [B, 128, 128, 192], 2: [B, 128, 128, 128], 3: [B, 128, 128, F], 4: [B, 128, 128, F],
                 5: [B, 128, 128, F], 6: [B, 8, 128, F], 7: [B, 128, 128, F], 8: [B, 128, 128, F], 9: [1, 1, F, 2], 10: [B, 1, F, 2],
                 11: [1, 1, 192, 2], 12: [1, 1, 128, 192], 13: [1, 1, 1, 128]}
        for which, dims in want0.items():
            ok(0, which, 0, 0, dims, 4 if which in (9, 10, 11, 13) else 2)
        # the heads' inputs (lo_teacher_heads_saved) are tensors of the same workspace
        offs, elems = (C.c_size_t * 3)(), (C.c_size_t * 3)()
        assert lib.lo_teacher_heads_saved(h, offs, elems) == 0
        for i in range(3):
            spans.append((0, offs[i], offs[i] + 4 * elems[i], ("saved", i, 0)))
        for space in (0, 1):
            s = sorted(x for x in spans if x[0] == space)
            for a, b in zip(s, s[1:]):
                assert a[2] <= b[1], (a, b)
    finally:
        lib.lo_teacher_destroy(h)


def test_what_it_refuses_and_why():
    lib = _lib()
    h = _handle(lib, 2, 128)
    try:
        for args, word in (((2, 0, 0, 0), b"unknown space"), ((-1, 0, 0, 0), b"unknown space"),
                           ((0, 14, 0, 0), b"unknown tensor kind 14"), ((0, -1, 0, 0), b"unknown tensor kind -1"),
                           ((0, 5, 1, 0), b"e = l = 0"), ((0, 5, 0, 2), b"e = l = 0"),
                           ((1, 21, 0, 0), b"unknown tensor kind 21"), ((1, -1, 0, 0), b"unknown tensor kind -1"),
                           ((1, 7, 4, 0), b"out of range"), ((1, 7, -1, 0), b"out of range"), ((1, 13, 0, 3), b"out of range"),
                           ((1, 6, 0, -1), b"out of range"), ((1, 1, 0, 3), b"depthwise branch"), ((1, 1, 1, 0), b"depthwise branch"),
                           ((1, 19, 0, 2), b"(mean, rstd) table"), ((1, 19, 0, 8), b"(mean, rstd) table"),
                           ((1, 0, 0, 1), b"e = l = 0"), ((1, 20, 1, 0), b"e = l = 0")):
            rc = _q(lib, h, *args)[0]
            assert rc != 0 and word in lib.lo_last_error(), (args, lib.lo_last_error())
        off, dims, eb = C.c_size_t(), (C.c_int * 4)(), C.c_int()
        assert lib.lo_teacher_debug_tensor(None, 1, 0, 0, 0, C.byref(off), dims, C.byref(eb)) != 0
        assert lib.lo_teacher_debug_tensor(h, 1, 0, 0, 0, None, dims, C.byref(eb)) != 0 and b"null" in lib.lo_last_error()
    finally:
        lib.lo_teacher_destroy(h)


def test_shared_set_plan_refuses_the_per_block_kinds(monkeypatch):
    """LO_T_BWD_SHARED=1: one tensor set, refilled in front of every block's backward -- a per-block name would be a lie for 11 of 12."""
    lib = _lib()
    monkeypatch.setenv("LO_T_BWD_SHARED", "1")
    h = _handle(lib, 2, 128)
    try:
        for which in range(7, 19):
            rc = _q(lib, h, 1, which, 3, 2)[0]
            assert rc != 0 and b"LO_T_BWD_SHARED" in lib.lo_last_error(), which
        assert _q(lib, h, 1, 6, 3, 2)[0] == 0 and _q(lib, h, 1, 5)[0] == 0 and _q(lib, h, 1, 19, 0, 7)[0] == 0
    finally:
        lib.lo_teacher_destroy(h)
