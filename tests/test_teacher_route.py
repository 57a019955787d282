"""`teacher.teacher_route`: which backward a `LunarMoETeacher.forward` call takes, as a table.  No GPU, no tensors."""
import inspect

import pytest

from lunaris_orion_amd.teacher import TeacherRoute, _TeacherFunction, teacher_route

# (training, eval_input_grad, all_parameters_live, x_requires_grad) -> (backward, want_dx, live_set, warn)
TABLE = {
    # train mode: eval_input_grad plays no part; an input that requires grad pulls in the whole path
    (True, False, False, False): ("heads", False, "heads", False),
    (True, False, False, True): ("train_full", True, "path", False),
    (True, False, True, False): ("train_full", False, "path", False),
    (True, False, True, True): ("train_full", True, "path", False),
    (True, True, False, False): ("heads", False, "heads", False),
    (True, True, False, True): ("train_full", True, "path", False),
    (True, True, True, False): ("train_full", False, "path", False),
    (True, True, True, True): ("train_full", True, "path", False),
    # eval mode, default: always the heads-only backward; the input gets no gradient and the call warns.  With full_backward=True the
    # trunk parameters are in the live set and receive zeros (the odd row, kept as it is)
    (False, False, False, False): ("heads", False, "heads", False),
    (False, False, False, True): ("heads", False, "heads", True),
    (False, False, True, False): ("heads", False, "path", False),
    (False, False, True, True): ("heads", False, "path", True),
    # eval mode with eval_input_grad: the train-mode rule with the frozen-BatchNorm backward
    (False, True, False, False): ("heads", False, "heads", False),
    (False, True, False, True): ("eval_full", True, "path", False),
    (False, True, True, False): ("eval_full", False, "path", False),
    (False, True, True, True): ("eval_full", True, "path", False),
}


@pytest.mark.parametrize("flags", sorted(TABLE), ids=lambda f: "".join("TF"[not b] for b in f))
def test_route_table(flags):
    route = teacher_route(*flags)
    assert isinstance(route, TeacherRoute) and route._fields == ("backward", "want_dx", "live_set", "warn")
    assert tuple(route) == TABLE[flags]
    assert all(type(v) is t for v, t in zip(route, (str, bool, str, bool)))


def test_table_covers_every_combination():
    assert len(TABLE) == 16


def test_autograd_node_takes_its_route_from_its_arguments():
    src = inspect.getsource(_TeacherFunction)
    for flag in (".training", "eval_input_grad", "all_parameters_live"):
        assert flag not in src, f"_TeacherFunction reads {flag}: the route is decided once, in LunarMoETeacher.forward"
