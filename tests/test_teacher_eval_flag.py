"""`LunarMoETeacher(eval_input_grad=...)`: an opt-in keyword after the existing ones; it changes neither the reference's positional
signature nor the state_dict (no GPU needed: the module is a parameter container until its first forward)."""
import inspect

from oracle import teacher_ref as T


def test_eval_input_grad_is_an_opt_in_keyword_that_leaves_the_module_surface_alone():
    from lunaris_orion_amd.teacher import LunarMoETeacher
    params = list(inspect.signature(LunarMoETeacher.__init__).parameters.values())[1:]
    names = [p.name for p in params]
    # the reference's positional arguments (lunar_evaluator.py:279-281), then this build's keywords, the new one last
    assert names[:8] == ["num_experts", "feature_dim", "dropout_rate", "rel_pos_size", "use_checkpointing", "expert_layers", "intermediate_dim",
                         "embedding_dim"]
    assert names[8:] == ["mfma_precision", "full_backward", "eval_input_grad"]
    assert params[-1].default is False
    off, on = LunarMoETeacher(), LunarMoETeacher(eval_input_grad=True)
    assert off.eval_input_grad is False and on.eval_input_grad is True
    assert LunarMoETeacher(4, 128, 0.1, 8, True, 3, 256, 64).eval_input_grad is False
    assert list(off.state_dict().keys()) == list(on.state_dict().keys()) == list(T.closed_form_teacher_state().keys())
    assert [k for k, _ in off.named_parameters()] == [k for k, _ in on.named_parameters()]
