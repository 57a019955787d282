"""Scenario table and call tracer behind the steppers' launch-order pin (tests/test_stepper_trace_gpu.py) and their bitwise A/B
(tools/stepper_ab.py).  TEST INFRASTRUCTURE ONLY.  It uses the steppers' public surface alone -- constructor arguments, the public
flags and buffers, `step()` -- so that one table runs unchanged on two trees whose `trainer.py` differ.

Every scenario runs `STEPS` optimizer steps at the smallest shapes the engines accept (batch 2, latent 64; the teacher at
feature_dim 128 with 4 experts), on closed-form parameters, sprites and noise from oracle/.

`Tracer` swaps `_lib.lib` for a proxy while `step()` runs (every module reaches the library as `_lib.lib.NAME`) and writes down, in
order, every call that enqueues work or changes what the next one does: the entries of `_lib.SIGNATURES` whose last argument is the
stream, and the `lo_vae_set_*` setters.  Pure queries (the `*_grad_range` family, `*_scratch_bytes`, `lo_vae_factor_block`,
`lo_vae_linear_factored`, `lo_vae_gradnorm_presummed`, ...) take no stream and are left out.  Per call: the name; integers as they
are; floats as the hex of their float32 value; pointers as `null`, `NAME+byte offset` inside one of the stepper's public buffers,
the flat parameter buffers and the engines' workspaces, or `ptr`; the stream as `current` or `other`.  The one-GPU exchange stand-in
(`_OneGpuRanks`) and the plain callable add their own events, with element ranges of the flat gradient buffer, to the same list.
"""
import contextlib
import ctypes as C
import functools
import os
import struct

import torch

from oracle import vae_ref as R

L, B, STEPS, WORLD = 64, 2, 3, 2
DROP_SEED = 0x5EEDD209C0FFEE11
KNOBS = ("LO_LINEAR_FACTORED", "LO_EARLY_NORM")
# what the steppers promise to keep by name: pointers into these are written as NAME+offset
PUBLIC_BUFFERS = ("grads", "exp_avg", "exp_avg_sq", "scratch", "losses", "ema", "t_grads", "t_m", "t_v", "t_scratch", "reward_state",
                  "reward_out")


def _elem_range(t, base):
    """[first, end) of `t` in elements of `base` if it is a slice of it, else its size alone."""
    off = t.data_ptr() - base.data_ptr()
    if t.dtype == base.dtype and 0 <= off and off + t.numel() * t.element_size() <= base.numel() * base.element_size():
        return [off // base.element_size(), off // base.element_size() + t.numel()]
    return ["numel", t.numel()]


class _Traced:
    """`trace` = (event list, flat gradient buffer) while a Tracer listens, else None."""
    trace = None

    def _note(self, what, *tensors):
        if self.trace is not None:
            events, base = self.trace
            events.append([what] + [_elem_range(t, base) for t in tensors])


class _OneGpuRanks(_Traced):
    """Stand-in for FlatGradSync on one GPU, everything on the current stream.  Without a gathered buffer it only collects the
    factor block a rank hands over; with one it plays the exchange of that rank: the hooks get the concatenated blocks of all ranks.
    The other gradient ranges stay this rank's own (the tests compare two runs of the same rank).  In the factored modes no plain
    range comes with a norm request or a `then` hook: `begin` asserts that."""
    supports_then = True

    def __init__(self, world, gathered=None):
        self.world, self.gathered, self.block = world, gathered, None

    def begin(self, g, then=None, pre=None, sumsq_scratch=None):
        self._note("begin", g)
        if pre is not None:
            pre()
        assert sumsq_scratch is None and then is None
        return True

    def begin_factored(self, pieces, factors, materialize, then=None, pre=None):
        self._note("begin_factored", factors, *pieces)
        if pre is not None:
            pre()                                   # the factor block is final behind this
        if self.gathered is None:
            self.block = factors.clone()
            return False
        materialize(self.gathered, self.world)
        if then is not None:
            then()
        return True

    def finish(self):
        self._note("finish")

    def average_small(self, t):
        pass


class _OneGpuRanksMode0(_OneGpuRanks):
    """The stand-in for the scenario whose Linear gradients travel like the rest (mode 0 of lo_vae_set_linear_factored): there the
    first range is handed over with `sumsq_scratch`, and its sum of squares is taken behind the (absent) exchange as
    FlatGradSync takes it.  Only that scenario uses it; every other one keeps `_OneGpuRanks` and its assert."""

    def begin(self, g, then=None, pre=None, sumsq_scratch=None):
        self._note("begin", g)
        if pre is not None:
            pre()
        if sumsq_scratch is not None:
            from lunaris_orion_amd import _lib
            _lib.check(_lib.lib.lo_gradnorm_early_range(g.data_ptr(), 0, g.numel(), sumsq_scratch, _lib.stream_ptr()), "lo_gradnorm_early_range")
        if then is not None:
            then()
        return True


class _PlainSync(_Traced):
    """`grad_sync` as a plain callable (no `begin`): it is handed the whole buffer behind the backward and averages nothing."""

    def __call__(self, g):
        self._note("call", g)


# ---- the tracer ------------------------------------------------------------------------------------------------------------------
def _arg_kinds():
    """name -> one letter per argument (i integer, f float, p pointer, s stream) for every library call that is written down."""
    from lunaris_orion_amd import _lib
    ints = (C.c_int, C.c_size_t, C.c_uint64, C.c_uint, C.c_longlong)
    out = {}
    for name, (_res, args) in _lib.SIGNATURES.items():
        setter = name.startswith("lo_vae_set_")
        if not setter and not (len(args) >= 2 and args[-1] is C.c_void_p):
            continue
        kinds = ["f" if a is C.c_float else "i" if a in ints else "p" for a in args]
        if not setter:
            kinds[-1] = "s"
        out[name] = "".join(kinds)
    return out


class _LibProxy:
    def __init__(self, real, tracer):
        self.__dict__["_real"], self.__dict__["_tracer"] = real, tracer

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        kinds = self._tracer.kinds.get(name)
        if kinds is not None:
            real_fn, record = fn, self._tracer.record

            def fn(*args):
                record(name, kinds, args)
                return real_fn(*args)
        self.__dict__[name] = fn
        return fn


class Tracer:
    def __init__(self, stepper, teacher=None):
        self.stepper, self.teacher, self.events, self.kinds = stepper, teacher, [], _arg_kinds()

    def _regions(self):
        st = self.stepper
        out = [(n, getattr(st, n, None)) for n in PUBLIC_BUFFERS]
        out.append(("vae.flat", st.vae._flat))
        out += [("vae.ws[%s]" % ",".join(str(k) for k in key), eng.ws) for key, eng in st.vae._engines.items()]
        if self.teacher is not None:
            out.append(("teacher.flat", self.teacher._flat))
            out += [("teacher.ws[%s]" % key, eng.ws) for key, eng in self.teacher._engines.items()]
        return [(n, t.data_ptr(), t.numel() * t.element_size()) for n, t in out if torch.is_tensor(t)]

    def record(self, name, kinds, args):
        regions, ev = None, [name]
        for k, a in zip(kinds, args):
            a = getattr(a, "value", a)
            if k == "i":
                ev.append(int(a))
            elif k == "f":
                ev.append("f32:" + struct.pack(">f", float(a)).hex())
            elif k == "s":
                ev.append("current" if int(a or 0) == torch.cuda.current_stream().cuda_stream else "other")
            elif not a:
                ev.append("null")
            elif not isinstance(a, int):
                ev.append("ptr")
            else:
                regions = regions or self._regions()
                ev.append(next((f"{n}+{a - p}" for n, p, size in regions if p <= a < p + size), "ptr"))
        self.events.append(ev)

    @contextlib.contextmanager
    def listening(self):
        from lunaris_orion_amd import _lib
        real, sync = _lib.lib, self.stepper.grad_sync
        _lib.lib = _LibProxy(real, self)
        if isinstance(sync, _Traced):
            sync.trace = (self.events, self.stepper.grads)
        try:
            yield self
        finally:
            _lib.lib = real
            if isinstance(sync, _Traced):
                sync.trace = None


# ---- the scenarios ---------------------------------------------------------------------------------------------------------------
def _sc(name, hybrid=False, env=None, sync=None, attrs=None, attention=False, **kw):
    return dict(name=name, hybrid=hybrid, env=env or {}, sync=sync, attrs=attrs or {}, attention=attention, kw=kw)


_MATERIALISED = {"LO_LINEAR_FACTORED": "0"}
_WINDOW = dict(gradient_accumulation_steps=2, accumulate_gradients=True)
SCENARIOS = [
    _sc("vae/default"),
    _sc("vae/materialised", env=_MATERIALISED),
    _sc("vae/materialised_late_norm", env={"LO_LINEAR_FACTORED": "0", "LO_EARLY_NORM": "0"}),
    _sc("vae/pipelined", pipeline_optimizer=True),
    _sc("vae/last_of_2_only", gradient_accumulation_steps=2),
    _sc("vae/window_of_2_factored", **_WINDOW),
    _sc("vae/window_of_2_materialised", env=_MATERIALISED, **_WINDOW),
    _sc("vae/ema", ema_decay=0.9, ema_every=2, ema_warmup=True),
    _sc("vae/plain_callable", sync="callable"),
    _sc("vae/dp_mode2", sync="ranks", dp_factored_adamw=False),
    _sc("vae/dp_mode3", sync="ranks", dp_factored_adamw=True),
    _sc("vae/dp_two_phase", sync="ranks", attrs={"dp_three_phase": False}),
    _sc("vae/dp_mode0", sync="ranks_mode0", env=_MATERIALISED),
    _sc("vae/dp_exchange_taken_away", sync="ranks", attrs={"grad_sync": None}),     # bench.py does, for its rank-local leg
    _sc("vae/attention", attention=True),
]
for _win_name, _win in (("", {}), ("window_of_2/", _WINDOW)):
    for _full in (False, True):
        for _w in (0.0, 0.05):
            SCENARIOS.append(_sc(f"hybrid/{_win_name}{'full' if _full else 'heads'}/w{_w}", hybrid=True, teacher_full_backward=_full,
                                 reward_grad_weight=_w, **_win))
SCENARIOS.append(_sc("hybrid/no_dead_teacher_call", hybrid=True, run_dead_teacher_call=False))
BY_NAME = {sc["name"]: sc for sc in SCENARIOS}


@contextlib.contextmanager
def _knobs(env):
    """The two A/B knobs of the steppers as the scenario states them (unset unless stated), for construction AND the steps."""
    before = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in before.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _vae_state(attention):
    if attention:
        from tests import attention_ref as A
        return A.attention_params(L, gamma=0.5)
    return R.closed_form_params(L)


@functools.lru_cache(maxsize=None)
def _inputs(i):
    return R.normalise_sprites(R.closed_form_sprites(B, salt=i)).cuda(), R.closed_form_eps(B, L, salt=i).cuda()


def _vae(attention=False):
    from lunaris_orion_amd.vae import LunarisCoreVAE
    m = LunarisCoreVAE(L, attention=True) if attention else LunarisCoreVAE(L)
    m.load_state_dict(_vae_state(attention), strict=True)
    return m.to("cuda")


@functools.lru_cache(maxsize=None)
def _gathered_blocks():
    """What the all-gather of `WORLD` ranks delivers: each rank's factor block from a step of its own, rank-major.  Never modified."""
    from lunaris_orion_amd.trainer import VAEStepper
    blocks = []
    with _knobs({}):
        for r in range(WORLD):
            col = _OneGpuRanks(WORLD)
            VAEStepper(_vae(), lr=0.0, weight_decay=0.0, max_grad_norm=1e9, grad_sync=col, dp_factored_adamw=False).step(_inputs(r)[0], 0, _inputs(r)[1])
            torch.cuda.synchronize()
            blocks.append(col.block)
    return torch.cat(blocks)


def _teacher():
    from lunaris_orion_amd.teacher import LunarMoETeacher
    from oracle import teacher_ref as T
    t = LunarMoETeacher(num_experts=4, feature_dim=128, dropout_rate=0.1)
    t.load_state_dict(T.closed_form_teacher_state())
    t = t.to("cuda").train()
    t.set_dropout_stream(DROP_SEED)
    return t


def run_scenario(sc, after_call=None):
    """Builds the scenario's stepper and runs its `STEPS` optimizer steps (k calls each under accumulation k); returns the events the
    tracer wrote down during the `step()` calls.  `after_call(i, stepper, teacher, recon, window_open)` runs behind every call,
    outside the tracer."""
    from lunaris_orion_amd.trainer import HybridStepper, VAEStepper
    torch.manual_seed(0)            # the model derives the seed argument of lo_vae_forward from torch's (unused: eps is given)
    gathered = _gathered_blocks().clone() if sc["sync"] in ("ranks", "ranks_mode0") else None
    with _knobs(sc["env"]):
        kw = dict(sc["kw"])
        if sc["sync"] in ("ranks", "ranks_mode0"):
            kw["grad_sync"] = (_OneGpuRanks if sc["sync"] == "ranks" else _OneGpuRanksMode0)(WORLD, gathered)
        elif sc["sync"] == "callable":
            kw["grad_sync"] = _PlainSync()
        vae, teacher = _vae(sc["attention"]), None
        if sc["hybrid"]:
            teacher = _teacher()
            st = HybridStepper(vae, teacher, lr=1e-4, teacher_lr=1e-4, **kw)
        else:
            st = VAEStepper(vae, lr=1e-4, **kw)
        for k, v in sc["attrs"].items():
            setattr(st, k, v)
        k = int(kw.get("gradient_accumulation_steps", 1))
        tracer = Tracer(st, teacher)
        for i in range(STEPS * k):
            x, eps = _inputs(i)
            with tracer.listening():
                recon = st.step(x, i, eps)[0]
            if after_call is not None:
                after_call(i, st, teacher, recon, bool(kw.get("accumulate_gradients")) and (i + 1) % k != 0)
        st.synchronize_parameters()
        torch.cuda.synchronize()
    return tracer.events


def main():
    """python -m tests.stepper_scenarios --record FILE: the traces of every scenario as the golden file holds them."""
    import argparse
    import json
    import time
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--record", required=True)
    args = ap.parse_args()
    out = {}
    for sc in SCENARIOS:
        t0 = time.perf_counter()
        out[sc["name"]] = run_scenario(sc)
        print(f"{sc['name']}: {len(out[sc['name']])} events, {time.perf_counter() - t0:.1f} s", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
    with open(args.record, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in out.items()) + "\n}\n")


if __name__ == "__main__":
    main()
