"""Real gradient accumulation (``--accumulate_gradients``, ``VAEStepper(accumulate_gradients=True)``), the parts that need no GPU:
the flag, the ABI entry behind the mode (header, binding, library) and the host bookkeeping of a window.  The reference steps on the
last micro-batch of k alone (train_hybrid.py:841-842, 907); the mode is this project's own and off by default."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_exists_and_defaults_to_off():
    import train_hybrid
    p = train_hybrid.build_parser()
    assert p.parse_args(["--data_dir", "x"]).accumulate_gradients is False
    assert p.parse_args(["--data_dir", "x", "--accumulate_gradients"]).accumulate_gradients is True
    help_text = next(a.help for a in p._actions if a.dest == "accumulate_gradients")
    assert "checkpoint" in help_text          # a partial window is not part of a checkpoint: said where the user reads it


def test_entry_points_are_declared_bound_and_exported():
    from lunaris_orion_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lunaris_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+lo_grad_accumulate\s*\(\s*float\s*\*\s*acc,\s*const\s+float\s*\*\s*g,\s*size_t\s+n,\s*float\s+scale,\s*int\s+first,"
                     r"\s*void\s*\*\s*stream\s*\)", header)
    for name in ("lo_grad_accumulate", "lo_vae_set_gathered_sum"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    res, args = _lib.SIGNATURES["lo_grad_accumulate"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.c_void_p]
    # the reference lines the entry replaces are cited where every other entry cites its own
    full = open(os.path.join(ROOT, "include", "lunaris_hip.h")).read()
    comment = full[:full.index("int lo_grad_accumulate(")].rsplit("/*", 1)[1]
    assert "train_hybrid.py:841-842" in comment and "895-896" in comment and "907" in comment


def test_bad_arguments_are_refused_before_any_launch():
    from lunaris_orion_amd import _lib
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    assert _lib.lib.lo_grad_accumulate(None, a, 4, 1.0, 1, None) == -1
    assert _lib.lib.lo_grad_accumulate(a, a + 16, 0, 1.0, 1, None) == -1                 # n >= 1
    assert _lib.lib.lo_grad_accumulate(a + 2, a + 64, 4, 1.0, 1, None) == -1             # 4-byte alignment
    assert _lib.lib.lo_grad_accumulate(a, a + 8, 4, 1.0, 0, None) == -1 and b"overlap" in _lib.lib.lo_last_error()


def test_steppers_take_the_argument_and_default_to_off():
    from lunaris_orion_amd.trainer import HybridStepper, VAEStepper
    assert inspect.signature(VAEStepper.__init__).parameters["accumulate_gradients"].default is False
    assert "kw" in inspect.signature(HybridStepper.__init__).parameters       # forwarded to VAEStepper


def test_window_positions():
    from lunaris_orion_amd.trainer import AccumulationWindow
    w = AccumulationWindow(3)
    got = [w.advance(b) for b in range(7)]
    assert got == [(True, False, 0), (False, False, 1), (False, True, 2), (True, False, 0), (False, False, 1), (False, True, 2),
                   (True, False, 0)]
    assert w.open
    # k = 1: every call is a whole window
    w1 = AccumulationWindow(1)
    assert [w1.advance(b) for b in range(3)] == [(True, True, 0)] * 3 and not w1.open
    assert AccumulationWindow(0).k == 1


def test_window_restarts_at_a_multiple_of_k_after_an_incomplete_one():
    from lunaris_orion_amd.trainer import AccumulationWindow
    w = AccumulationWindow(3)
    assert w.advance(0) == (True, False, 0) and w.advance(1) == (False, False, 1)      # the epoch ends here: 2 of 3
    assert w.advance(0) == (True, False, 0)                                            # next epoch: a clean window, slot 0 again
    assert w.advance(1) == (False, False, 1) and w.advance(2) == (False, True, 2) and not w.open
    # one call of a window, then the restart
    assert w.advance(3) == (True, False, 0) and w.open
    assert w.advance(0) == (True, False, 0)


def test_window_that_starts_in_the_middle_is_short_and_ends_at_the_reference_step():
    from lunaris_orion_amd.trainer import AccumulationWindow
    w = AccumulationWindow(4)
    assert w.advance(2) == (True, False, 0)            # nothing open: a window starts where the run starts
    assert w.advance(3) == (False, True, 1) and not w.open
    assert w.advance(4) == (True, False, 0)


def test_window_never_hands_out_a_slot_beyond_k():
    from lunaris_orion_amd.trainer import AccumulationWindow
    w = AccumulationWindow(2)
    assert w.advance(0) == (True, False, 0)
    assert w.advance(2 + 0) == (True, False, 0)        # a multiple of k restarts
    w = AccumulationWindow(3)
    w.advance(0), w.advance(1)
    assert w.advance(1) == (False, False, 2)           # a repeated index still fills a slot ...
    with pytest.raises(ValueError):
        w.advance(1)                                   # ... but never one beyond the k blocks the buffers hold
    assert not w.open
