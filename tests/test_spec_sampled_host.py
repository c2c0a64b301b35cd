"""No GPU: speculative decoding under a configured tail -- the reference's accept rule, SpeculativeParams(configured_tail=),
check_speculative_tail's refusals, and the engine's routing over a stub model whose "draws" are a fixed text."""
from pathlib import Path

import pytest
import torch

from tests import spec_sampled_reference as sref
from tests import speculative_reference as ref
from tests.test_speculative_host import PROMPT_LEN, TEXT, StubModel


# ------------------------------------------------------------------ the rule, by hand
def test_reference_accept_rule_and_stream():
    V = 100
    assert sref.accept([5, 6, 7, 8], [5, 6, 7], V) == (3, [5, 6, 7, 8])
    assert sref.accept([5, 6, 7, 8], [5, 9, 7], V) == (1, [5, 6, -1, -1])
    assert sref.accept([5, 6, 7, 8], [4, 6, 7], V) == (0, [5, -1, -1, -1])
    assert sref.accept([5, 6, 7, 8], [5, 6, 9], V) == (2, [5, 6, 7, -1])
    # an id outside [0, V) is never accepted, even where the row's token could not equal it anyway
    assert sref.accept([5, 6, 7, 8], [-1, 6, 7], V) == (0, [5, -1, -1, -1])
    assert sref.accept([5, 6, 7, 8], [5, V, 7], V) == (1, [5, 6, -1, -1])
    assert sref.accept([5, 6], [5], 5) == (0, [5, -1])              # the draft equals the token, but 5 is no id of a 5-token vocabulary
    with pytest.raises(ValueError):
        sref.accept([5, 6, 7], [5], V)
    # row r draws at c + r; afterwards out_n positions are consumed, whatever was drawn behind the accepted run
    assert sref.stream_positions(40, 4) == [40, 41, 42, 43]
    assert sref.counter_after(40, 0) == (41, 0) and sref.counter_after(40, 3) == (44, 0)
    # token j of a generation is draw j of the seed: a pass that accepts 2 of 7 and the step behind it use positions c .. c + 3
    c, used = 10, []
    for n_acc in (2, 0, 7):
        used += sref.stream_positions(c, 8)[:n_acc + 1]
        c = sref.counter_after(c, n_acc)[0]
    assert used == list(range(10, 10 + 3 + 1 + 8))


def test_reference_row_window():
    before, fed, draft = list(range(100, 110)), 7, [1, 2, 3]
    assert sref.row_window(before, fed, draft, 10, 0, 4) == [107, 108, 109, 7]            # row 0: the step's own window
    assert sref.row_window(before, fed, draft, 10, 2, 4) == [109, 7, 1, 2]                # row 2 sees the drafts before it, not its own
    assert sref.row_window(before, fed, draft, 10, 3, 60) == before + [7, 1, 2, 3]        # a window longer than the sequence starts at 0
    assert sref.row_window(before, fed, draft, 10, 3, 1) == [3]
    assert sref.recorded_ids(before, fed, [1, 2, -1, -1], 10) == before + [7, 1, 2]


# ------------------------------------------------------------------ SpeculativeParams(configured_tail=)
def test_params_validation_and_default():
    from proxy_inference_engine_amd import SpeculativeParams
    assert SpeculativeParams().configured_tail is False
    assert SpeculativeParams() == SpeculativeParams(num_draft=7, ngram_max=3, ngram_min=1, min_draft=5, configured_tail=False)
    assert SpeculativeParams(configured_tail=True).configured_tail is True
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="configured_tail"):
            SpeculativeParams(configured_tail=bad)
    with pytest.raises(ValueError, match="SpeculativeParams"):
        SpeculativeParams(num_draft=32, configured_tail=True)


# ------------------------------------------------------------------ check_speculative_tail
class TailStub(StubModel):
    """StubModel with the configured-tail interface: the "drawn" token after a sequence of length n is text[n], whatever is configured."""

    def __init__(self, text):
        super().__init__(text)
        self.fed_ids = torch.zeros(4096, dtype=torch.int32)
        self.tails = []

    def set_step_tail(self, **kw):
        self.tails.append(kw)

    def spec_step_tail(self, draft_ids, cache, then_draft=None):
        out = StubModel.spec_step(self, draft_ids, cache, then_draft)
        self.calls[-1] = ("tail_pass", self.calls[-1][1])
        return out


def plan_args(**kw):
    from proxy_inference_engine_amd.samplers import make_sampler
    args = dict(sampler=make_sampler(temp=0.7, top_p=0.9), processors=[], structuring_engine=None, pixel_values=None, kv_bits=None, max_kv_size=None,
                prompt_logprobs=None)
    args.update(kw)
    return args


def test_check_speculative_tail_plans_and_refusals_by_name():
    from proxy_inference_engine_amd.engine.inference_engine import check_speculative_tail
    from proxy_inference_engine_amd.logits_processors import (count_penalty_logits_processor, dry_logits_processor, make_logit_bias, make_token_mask,
                                                              repetition_penalty_logits_processor)
    from proxy_inference_engine_amd.samplers import make_sampler
    m = TailStub(TEXT)
    plan = check_speculative_tail(m, *plan_args().values())
    assert plan["sampler"][0] == "top_p" and plan["repetition_penalty"] == 1.0 and plan["mask"] is None and plan["bias"] is None
    pen, bias = repetition_penalty_logits_processor(1.3, 20), make_logit_bias({3: 1.5, 9: -2.0})
    plan = check_speculative_tail(m, *plan_args(sampler=make_sampler(temp=0), processors=[pen, bias]).values())
    assert plan["sampler"] is None and (plan["repetition_penalty"], plan["context_size"]) == (1.3, 20) and plan["bias"] is bias
    plan = check_speculative_tail(m, *plan_args(sampler=make_sampler(temp=1.0, top_k=4, xtc_probability=0.5, xtc_threshold=0.1)).values())
    assert plan["sampler"][0] == "top_k" and plan["xtc"][:2] == (0.5, 0.1)

    class Pool:
        dtype = torch.int8

    cases = [(dict(structuring_engine=object()), "structuring engine"), (dict(pixel_values=torch.zeros(1)), "pixel_values"), (dict(kv_bits=8), "kv_bits"),
             (dict(max_kv_size=64), "max_kv_size"), (dict(prompt_logprobs=2), "prompt_logprobs"),
             (dict(processors=[make_token_mask(torch.ones(64, dtype=torch.bool))]), "token mask"),
             (dict(processors=[count_penalty_logits_processor(0.5, 0.0)]), "frequency / presence"),
             (dict(processors=[dry_logits_processor(0.8, 1.75, 2, 64, ())]), "DRY"),
             (dict(processors=[lambda t, x: x]), "outside the fused tail plan"), (dict(processors=[bias, pen]), "outside the fused tail plan"),
             (dict(processors=[repetition_penalty_logits_processor(1.3, 0)]), "outside the fused tail plan"),
             (dict(sampler=lambda x: x), "outside the fused tail plan")]
    for kw, name in cases:
        with pytest.raises(ValueError, match=name):
            check_speculative_tail(m, *plan_args(**kw).values())
    tp_model, i8_model = TailStub(TEXT), TailStub(TEXT)
    tp_model.tp, i8_model._page_pool = object(), Pool()
    with pytest.raises(ValueError, match="tensor-parallel"):
        check_speculative_tail(tp_model, *plan_args().values())
    with pytest.raises(ValueError, match="int8 KV pages"):
        check_speculative_tail(i8_model, *plan_args().values())
    with pytest.raises(ValueError, match="spec_step_tail"):
        check_speculative_tail(StubModel(TEXT), *plan_args().values())


# ------------------------------------------------------------------ the engine's routing
def tail_engine(**request):
    from proxy_inference_engine_amd import InferenceEngine
    eng = InferenceEngine(model=TailStub(TEXT))
    eng.prepare_engine(TEXT[:PROMPT_LEN], **request)
    return eng


@pytest.mark.parametrize("request_kw,want_tail", [
    (dict(temp=0.7, top_p=0.9), dict(sampler=("top_p", 0.7, 0.9, 0), repetition_penalty=1.0)),
    (dict(temp=0, repetition_penalty=1.3, context_size=20), dict(sampler=None, repetition_penalty=1.3, context_size=20)),
    (dict(temp=1.0, top_k=4, logit_bias={3: 1.5}, xtc_probability=0.5, xtc_threshold=0.1), dict(sampler=("top_k", 1.0, 0.0, 4), repetition_penalty=1.0)),
])
def test_engine_routes_passes_through_the_tail_entry(request_kw, want_tail):
    from proxy_inference_engine_amd import SpeculativeParams
    sp = SpeculativeParams(configured_tail=True)
    n_tokens = 60
    want_tokens, schedule = ref.simulate(TEXT[:PROMPT_LEN], lambda s: TEXT[len(s)], n_tokens, 7, 3, 1, 5)
    eng = tail_engine(**request_kw)
    gen = eng.generate_step(TEXT[:PROMPT_LEN], speculative=sp)
    got, yields = [], 0
    while len(got) < n_tokens:
        tokens, rows = next(gen)
        assert tokens.dtype == torch.int32 and rows.shape == (tokens.numel(), rows.shape[1])
        got += tokens.tolist()
        yields += 1
    assert got == want_tokens[:len(got)]
    done = schedule[:yields - 1]
    passes = [e for e in done if e[0] == "pass"]
    model = eng.model
    # every pass went through spec_step_tail, every step through the ordinary step; spec_step was never called
    assert model.calls[1:] == [("tail_pass", e[1]) if e[0] == "pass" else ("step", 1) for e in done]
    assert eng.spec_stats == {"passes": len(passes), "steps": len(done) - len(passes), "drafted": sum(e[1] for e in passes),
                              "accepted": sum(e[2] for e in passes)}
    # prompt_cache.update received the ids whose rows the cache holds
    assert eng.prompt_cache.computed_ids == TEXT[:eng.prompt_cache.cache[0].offset]
    # the tail was configured once, with the plan's parts, and never reset to the greedy one
    assert len(model.tails) == 1
    tail = model.tails[0]
    for key, val in want_tail.items():
        got_val = tail[key]
        assert (tuple(got_val) if isinstance(val, tuple) else got_val) == val, (key, got_val)
    assert ("xtc" in tail) == ("xtc_probability" in request_kw)
    assert (tail["logit_bias"] is not None) == ("logit_bias" in request_kw)


def test_greedy_request_without_processors_takes_the_greedy_path():
    from proxy_inference_engine_amd import SpeculativeParams
    eng = tail_engine(temp=0)
    gen = eng.generate_step(TEXT[:PROMPT_LEN], speculative=SpeculativeParams(configured_tail=True))
    got = []
    while len(got) < 30:
        got += next(gen)[0].tolist()
    assert got == TEXT[PROMPT_LEN:PROMPT_LEN + len(got)]
    assert eng.spec_stats["passes"] >= 1 and all(c[0] in ("step", "pass") for c in eng.model.calls)
    assert eng.model.tails == [{}]                                           # set_step_tail(): the documented greedy tail


def test_default_params_still_refuse_and_tail_refusals_reach_the_engine():
    from proxy_inference_engine_amd import SpeculativeParams
    eng = tail_engine(temp=0.7)
    with pytest.raises(ValueError, match="non-greedy sampler"):
        next(eng.generate_step(TEXT[:PROMPT_LEN], speculative=SpeculativeParams()))
    eng = tail_engine(temp=0, repetition_penalty=1.3)
    with pytest.raises(ValueError, match="logits processors"):
        next(eng.generate_step(TEXT[:PROMPT_LEN], speculative=SpeculativeParams()))
    sp = SpeculativeParams(configured_tail=True)
    eng = tail_engine(temp=0.7, frequency_penalty=0.5)
    with pytest.raises(ValueError, match="frequency / presence"):
        next(eng.generate_step(TEXT[:PROMPT_LEN], speculative=sp))
    eng = tail_engine(temp=0.7, dry_multiplier=0.8)
    with pytest.raises(ValueError, match="DRY"):
        next(eng.generate_step(TEXT[:PROMPT_LEN], speculative=sp))
    eng = tail_engine(temp=0.7)
    for kw, name in ((dict(kv_bits=8), "kv_bits"), (dict(prompt_logprobs=2), "prompt_logprobs")):
        with pytest.raises(ValueError, match=name):
            next(eng.generate_step(TEXT[:PROMPT_LEN], speculative=sp, **kw))
    assert eng.model.calls == []                                             # refused before any model call


def test_new_symbols_are_exported():
    from proxy_inference_engine_amd import _ffi, hip_ops
    from proxy_inference_engine_amd.engine import inference_engine
    from proxy_inference_engine_amd.models.llama import Model
    assert callable(inference_engine.check_speculative_tail)
    for name in ("spec_verify_sampled", "spec_verify_sampled_workspace"):
        assert callable(getattr(hip_ops, name))
    assert callable(Model.spec_step_tail)
    names = ("pie_spec_verify_sampled", "pie_spec_verify_sampled_workspace_bytes", "pie_decoder_spec_step_tail", "pie_decoder_spec_tail_workspace_bytes")
    header = (Path(__file__).resolve().parent.parent / "include" / "pie_hip.h").read_text()
    for name in names:
        assert name in _ffi.EXPORTS and name + "(" in header
