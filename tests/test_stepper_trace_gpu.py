"""Launch-order pin of `VAEStepper.step` / `HybridStepper.step`: for every scenario of tests/stepper_scenarios.py the ordered list
of library calls three optimizer steps make -- names, integer and float arguments, which buffer every pointer points into, the stream
-- and the hand-overs to the exchange stand-in equal tests/golden/stepper_trace.json exactly.  The golden file was recorded with the
steppers as they were before their host side was refactored (`python -m tests.stepper_scenarios --record FILE` in that tree), so the
test pins what a step launches, not how `trainer.py` is written."""
import functools
import json
import os

import pytest

from tests import stepper_scenarios as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stepper_trace.json")


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_the_scenario_table_and_nothing_else():
    assert list(_golden()) == [sc["name"] for sc in S.SCENARIOS]


@pytest.mark.parametrize("name", [sc["name"] for sc in S.SCENARIOS])
def test_a_step_makes_the_recorded_calls_in_the_recorded_order(name):
    sc = S.BY_NAME[name]
    got = S.run_scenario(sc)
    calls = S.STEPS * int(sc["kw"].get("gradient_accumulation_steps", 1))
    assert len(got) >= calls, f"{name}: {len(got)} recorded calls in {calls} step() calls: the tracer saw nothing"
    want = _golden()[name]
    at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (f"{name}: {len(got)} events against {len(want)} recorded; the first difference is event {at}: "
                         f"{got[at] if at < len(got) else None} against {want[at] if at < len(want) else None} "
                         f"(behind {got[at - 1] if at else None})")


@pytest.mark.parametrize("hybrid", [False, True], ids=["vae", "hybrid"])
def test_deleting_a_stepper_frees_its_buffers_at_once(hybrid):
    """No reference cycle runs through a stepper: `del st; torch.cuda.empty_cache()` (bench.py between its legs, the A/B tools)
    releases the flat gradient buffer, the moments and the EMA by reference count, without waiting for a pass of the cyclic
    collector -- which is switched off here."""
    import gc
    import weakref

    from lunaris_orion_amd.trainer import HybridStepper, VAEStepper
    gc.collect()
    gc.disable()
    try:
        if hybrid:
            st = HybridStepper(S._vae(), S._teacher(), lr=1e-4, teacher_lr=1e-4)
        else:
            st = VAEStepper(S._vae(), lr=1e-4, ema_decay=0.9, gradient_accumulation_steps=2, accumulate_gradients=True)
        for i in range(2):
            st.step(S._inputs(i)[0], i, S._inputs(i)[1])
        st.metrics()
        refs = [weakref.ref(t) for t in (st, st.grads, st.exp_avg, st.exp_avg_sq)]
        del st
        assert all(r() is None for r in refs), "a stepper, or one of its buffers, outlives `del st`: a reference cycle holds it"
    finally:
        gc.enable()
