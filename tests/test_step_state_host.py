"""CPU: the single-sequence step's tail state has one owner per layer -- the Intern ensemble forwards exactly the names
step_state.py exports, and every setter of a tail, the step's eight and the multi-sequence passes' seven, still refuses a missing decoder
under its own name through the one entry check they share."""
import ctypes

STEP_SETTERS = ("logits_penalty", "sampler", "logits_mask", "logit_bias", "top_logprobs", "count_penalty", "dry_penalty", "xtc")
BATCH_SETTERS = ("batch_tail", "batch_top_logprobs", "batch_logits_edits", "batch_count_penalty", "batch_dry_penalty", "batch_xtc", "prompt_logprobs")


class StubTower:
    """A language model that has the step-tail surface, private state beside it, and records what it is asked."""

    def __init__(self, surface):
        self.calls = []
        self._tail, self._xtc = ("private",), ("private",)
        self._values = {n: object() for n in surface}

    def set_step_tail(self, *args, **kwargs):
        self.calls.append(("set_step_tail", args, kwargs))

    def reset_step_counts(self, *args, **kwargs):
        self.calls.append(("reset_step_counts", args, kwargs))

    def _set_tail_dry(self, dry):
        raise AssertionError("private")

    def __getattr__(self, name):   # the surface's properties
        if name != "_values" and name in self._values:
            return self._values[name]
        raise AttributeError(name)


def test_ensemble_forwards_exactly_the_exported_surface():
    from proxy_inference_engine_amd.models.intern.ensemble import Model as Ensemble, ModelArgs
    from proxy_inference_engine_amd.models.llama.step_state import STEP_TAIL_SURFACE, StepTailState
    # the tuple is the mixin's public surface, name for name
    assert len(set(STEP_TAIL_SURFACE)) == len(STEP_TAIL_SURFACE)
    assert set(STEP_TAIL_SURFACE) == {n for n in vars(StepTailState) if not n.startswith("_")}
    assert {"step_xtc_record", "step_tail_dry"} <= set(STEP_TAIL_SURFACE)
    tower = StubTower(STEP_TAIL_SURFACE)
    ens = Ensemble(ModelArgs(), tower)
    ens.set_step_tail(("top_k", 0.8, 0.0, 5), 1.3, xtc=(0.5, 0.1, ()))
    ens.reset_step_counts(7, generated_ids=[1, 2])
    assert tower.calls == [("set_step_tail", (("top_k", 0.8, 0.0, 5), 1.3), {"xtc": (0.5, 0.1, ())}), ("reset_step_counts", (7,), {"generated_ids": [1, 2]})]
    for name in STEP_TAIL_SURFACE:
        if name not in ("set_step_tail", "reset_step_counts"):
            assert getattr(ens, name) is tower._values[name], name
    # nothing else of the step's tail state comes through
    for name in ("_tail", "_xtc", "_set_tail_dry", "_step_tail_plain", "_init_step_state", "calls", "step_tail_xtc"):
        assert not hasattr(ens, name), name


def test_every_tail_setter_refuses_a_null_decoder_under_its_own_name():
    from proxy_inference_engine_amd import _ffi
    lib = _ffi.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)   # a host stand-in, never dereferenced: every call is refused first
    assert len(STEP_SETTERS) == 8 and len(BATCH_SETTERS) == 7
    for short in STEP_SETTERS + BATCH_SETTERS:
        name = "pie_decoder_set_" + short
        fn = getattr(lib, name)
        args = [p if t is ctypes.c_void_p else (1.5 if t is ctypes.c_double else 1) for t in fn.argtypes[1:]]
        assert fn(None, *args) == -1, name                      # PIE_E_ARG
        assert lib.pie_last_error() == (name + ": null decoder").encode(), (name, lib.pie_last_error())
