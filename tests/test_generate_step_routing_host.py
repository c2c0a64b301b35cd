"""No GPU: which calls one InferenceEngine.generate_step step makes, in which order and with which arguments -- the fused tail plan's
Model.set_step_tail kwargs per request feature, the repair of Model.fed_ids over a reused prefix, and the host-orchestrated branches
with and without processors, for text and for pixel_values.  The model is a stub that logs every call the engine makes on it; the
assertions are the whole logs."""
import numpy as np
import pytest
import torch

from proxy_inference_engine_amd import InferenceEngine, hip_ops
from proxy_inference_engine_amd.cache import ReusableKVCache
from proxy_inference_engine_amd.logits_processors import TokenAutomaton
from proxy_inference_engine_amd.samplers import greedy

V = 64
PROMPT = [3, 9, 27, 17, 51, 25, 11, 33, 35, 41, 59, 49]
L = len(PROMPT)


def token_at(offset: int) -> int:
    """The stub's choice behind `offset` cached positions."""
    return (5 * offset + 3) % V


T = [token_at(L + i) for i in range(4)]   # the tokens a request over PROMPT yields: 63, 4, 9, 14


class Cache(ReusableKVCache):
    """A KV cache that holds nothing but its offset (PromptCache.reuse_cache asserts the type)."""

    def reuse(self, new_prompt_length, common_prefix_length):
        self.offset = common_prefix_length


class FedIds:
    """Model.fed_ids as far as the engine touches it: its size, and writes into a slice of it, which are logged."""

    def __init__(self, log, n):
        self.log, self.n = log, n

    def numel(self):
        return self.n

    def __setitem__(self, sl, src):
        self.log.append(("fed_ids", sl.start, sl.stop, torch.as_tensor(src).tolist()))

    def __getitem__(self, sl):
        fed = self

        class View:
            def copy_(self, src):
                fed[sl] = src
        return View()


class PlainStub:
    """Model as generate_step's plain loop uses it, without a configurable tail.  A model call's log entry is (name, ids passed: how many
    or None, rows fed, the prompt cache's computed_ids at that moment: how many) -- the last says on which side of the call
    prompt_cache.update ran."""
    device, tp, _page_pool = "cpu", None, None
    step_top_logprobs = ("the step's ids", "the step's vals")

    def __init__(self, fed=4096):
        self.log, self.recorded = [], lambda: 0
        self.fed_ids = FedIds(self.log, fed)
        self.logprobs = torch.zeros(V)

    def make_cache(self):
        return [Cache()]

    def _fed(self, name, ids, rows, cache):
        self.log.append((name, None if ids is None else int(ids.numel()), rows, self.recorded()))
        cache[0].offset += rows
        tok = token_at(cache[0].offset)
        lp = torch.full((V,), -30.0)
        lp[tok] = -0.25
        return torch.tensor([tok], dtype=torch.int32), lp

    def step(self, ids, cache):
        tok, lp = self._fed("step", ids, 1 if ids is None else int(ids.numel()), cache)
        return tok, lp, lp

    def __call__(self, ids, cache=None):
        assert ids.dim() == 2 and ids.shape[0] == 1
        return self._fed("call", ids, ids.shape[1], cache)[1].expand(1, ids.shape[1], V)


class TextStub(PlainStub):
    """PlainStub with Model's configured tail: set_step_tail's kwargs are logged as they come (tensors as lists)."""

    def set_step_tail(self, **kw):
        self.log.append(("set_step_tail", {k: v.tolist() if isinstance(v, torch.Tensor) else v for k, v in kw.items()}))

    def reset_step_automaton(self):
        self.log.append(("reset_step_automaton",))


class VlmStub(TextStub):
    """The VLM ensemble's surface: get_input_embeddings, step_embeds and the text tower as `language_model`."""

    def __init__(self, fed=4096):
        super().__init__(fed)
        outer = self

        class Tower:
            logprobs = outer.logprobs

            def __call__(self, ids, cache=None, inputs_embeds=None):
                return outer._fed("language_model", ids, inputs_embeds.shape[1], cache)[1].expand(1, inputs_embeds.shape[1], V)
        self.language_model = Tower()

    def get_input_embeddings(self, ids, pixel_values):
        assert ids.dim() == 2 and pixel_values is PIXELS
        self.log.append(("get_input_embeddings", int(ids.numel())))
        return torch.zeros(1, ids.shape[1], 4)

    def step_embeds(self, embeds, cache, ids=None):
        tok, lp = self._fed("step_embeds", ids, embeds.shape[1], cache)
        return tok, lp, lp


PIXELS = torch.zeros(1, 3, 2, 2)


def make_engine(model, **request):
    eng = InferenceEngine(model=model)
    model.recorded = lambda: len(eng.prompt_cache.computed_ids)
    eng.prepare_engine(PROMPT, **request)
    return eng


def run(eng, prompt, steps, **kw):
    """`steps` steps of generate_step: [(token, logprobs)], and the prompt cache's computed_ids after each."""
    gen = eng.generate_step(prompt, **kw)
    out, seen = [], []
    for _ in range(steps):
        out.append(next(gen))
        seen.append(list(eng.prompt_cache.computed_ids))
    gen.close()
    return out, seen


def tokens_of(out):
    return [[int(t) for t in tok.reshape(-1).tolist()] for tok, _ in out]


def tail(**kw):
    """A set_step_tail log entry: the kwargs every fused step passes, then the request's own."""
    return ("set_step_tail", {**dict(sampler=None, repetition_penalty=1.0, context_size=60, token_mask=None, logit_bias=None), **kw})


# ------------------------------------------------------------------ the fused plan: set_step_tail's kwargs per feature
AUTOMATON = TokenAutomaton.from_token_table(np.zeros((1, V), dtype=np.int32))
MASK = torch.zeros(V, dtype=torch.bool)
MASK[[1, 4, 9, 63]] = True
MASK_WORDS = [2 + 16 + 512, -2 ** 31]   # ids 1, 4, 9 in word 0; id 63 is bit 31 of word 1, an int32's sign
TOP_K = ("top_k", 0.8, 0.0, 5)

FUSED = {
    "greedy": (dict(temp=0), {}, {}),
    "sampler": (dict(temp=0.8, top_k=5), {}, dict(sampler=TOP_K)),
    "penalty": (dict(temp=0.8, top_k=5, repetition_penalty=1.3, context_size=20), {}, dict(sampler=TOP_K, repetition_penalty=1.3, context_size=20)),
    "static mask": (dict(temp=0, token_mask=MASK), {}, dict(token_mask=MASK_WORDS)),
    "bias": (dict(temp=0, logit_bias={3: 1.5, 9: -2.0}), {}, dict(logit_bias=((3, 9), (1.5, -2.0)))),
    "dry": (dict(temp=0, dry_multiplier=0.8, dry_base=1.5, dry_allowed_length=3, dry_range=16, dry_sequence_breakers=[7]), {},
            dict(dry=(0.8, 1.5, 3, 16, (7,)))),
    "xtc": (dict(temp=1.0, top_k=4, xtc_probability=0.5, xtc_threshold=0.1, xtc_special_tokens=[2]), {},
            dict(sampler=("top_k", 1.0, 0.0, 4), xtc=(0.5, 0.1, (2,)))),
    "top_logprobs": (dict(temp=0), dict(top_logprobs=3), dict(top_logprobs=3)),
    "everything": (dict(temp=0.8, top_k=5, token_mask=MASK, repetition_penalty=1.3, context_size=20, logit_bias={3: 1.5}, dry_multiplier=0.8, dry_range=16),
                   dict(top_logprobs=0),
                   dict(sampler=TOP_K, repetition_penalty=1.3, context_size=20, token_mask=MASK_WORDS, logit_bias=((3,), (1.5,)), top_logprobs=0,
                        dry=(0.8, 1.75, 2, 16, ()))),
}


@pytest.mark.parametrize("case", list(FUSED))
def test_fused_plan_configures_the_tail_then_steps(case):
    request, step_kw, want = FUSED[case]
    eng = make_engine(TextStub(), **request)
    out, seen = run(eng, PROMPT, 4, **step_kw)
    t = tail(**want)
    # the prompt's ids are passed, a fed-back step passes nothing whatever the sampler; the ids are recorded after the model call
    assert eng.model.log == [t, ("step", L, L, 0), t, ("step", None, 1, L), t, ("step", None, 1, L + 1), t, ("step", None, 1, L + 2)]
    assert tokens_of(out) == [[T[0]], [T[1]], [T[2]], [T[3]]]
    assert all(tok.dtype == torch.int32 and tok.shape == (1,) and lp.shape == (V,) for tok, lp in out)
    assert seen == [PROMPT, PROMPT + T[:1], PROMPT + T[:2], PROMPT + T[:3]]
    assert eng.top_record is (TextStub.step_top_logprobs if "top_logprobs" in step_kw else None)


def test_fused_plan_counts_start_on_the_first_call_only():
    eng = make_engine(TextStub(), temp=0, frequency_penalty=0.5, presence_penalty=0.25)
    _, seen = run(eng, PROMPT, 3)
    first = tail(frequency_penalty=0.5, presence_penalty=0.25, count_start=L)
    later = tail(frequency_penalty=0.5, presence_penalty=0.25, count_start=None)
    assert eng.model.log == [first, ("step", L, L, 0), later, ("step", None, 1, L), later, ("step", None, 1, L + 1)]
    assert seen == [PROMPT, PROMPT + T[:1], PROMPT + T[:2]]


def test_fused_plan_resets_the_automaton_on_the_first_call_only():
    eng = make_engine(TextStub(), temp=0, token_automaton=AUTOMATON)
    _, seen = run(eng, PROMPT, 3)
    t = tail(token_automaton=AUTOMATON)
    assert eng.model.log == [t, ("reset_step_automaton",), ("step", L, L, 0), t, ("step", None, 1, L), t, ("step", None, 1, L + 1)]
    assert eng.model.log[0][1]["token_automaton"] is AUTOMATON
    assert seen == [PROMPT, PROMPT + T[:1], PROMPT + T[:2]]


def test_fused_plan_mask_fn_records_the_ids_before_the_model_call():
    calls = []

    def mask_fn(tokens):
        calls.append(list(tokens))
        return [len(tokens)]   # one allowed id, another one every step

    eng = make_engine(TextStub(), temp=0, token_mask=mask_fn)
    _, seen = run(eng, PROMPT, 3)
    # the mask sees this row's input, so the ids are in computed_ids when the model runs: new words every step
    assert eng.model.log == [tail(token_mask=[1 << L, 0]), ("step", L, L, L),
                             tail(token_mask=[1 << (L + 1), 0]), ("step", None, 1, L + 1),
                             tail(token_mask=[1 << (L + 2), 0]), ("step", None, 1, L + 2)]
    assert calls == seen == [PROMPT, PROMPT + T[:1], PROMPT + T[:2]]   # (recorded once: not again behind the call)


def test_fused_plan_with_pixel_values_steps_on_the_embeddings_with_the_ids():
    eng = make_engine(VlmStub(), temp=0)
    out, seen = run(eng, PROMPT, 3, pixel_values=PIXELS)
    t = tail()
    assert eng.model.log == [t, ("get_input_embeddings", L), ("step_embeds", L, L, 0), t, ("step", None, 1, L), t, ("step", None, 1, L + 1)]
    assert tokens_of(out) == [[T[0]], [T[1]], [T[2]]] and seen == [PROMPT, PROMPT + T[:1], PROMPT + T[:2]]


@pytest.mark.parametrize("request_kw,window,want", [
    (dict(repetition_penalty=1.3, context_size=4), 4, dict(repetition_penalty=1.3, context_size=4)),
    (dict(repetition_penalty=1.3, context_size=4, dry_multiplier=0.8, dry_range=6), 6,
     dict(repetition_penalty=1.3, context_size=4, dry=(0.8, 1.75, 2, 6, ()))),
    (dict(dry_multiplier=0.8, dry_range=3), 3, dict(dry=(0.8, 1.75, 2, 3, ()))),
    (dict(repetition_penalty=1.3, context_size=40), L + 2, dict(repetition_penalty=1.3, context_size=40)),   # a window past the prefix: all of it
    (dict(logit_bias={3: 1.5}), 0, dict(logit_bias=((3,), (1.5,)))),                                         # no tail reads the fed ids: no repair
])
def test_fused_plan_repairs_fed_ids_over_a_reused_prefix(request_kw, window, want):
    eng = make_engine(TextStub(), temp=0)
    run(eng, PROMPT, 3)                                   # a greedy request: the cache holds PROMPT + T[:2], recorded by no penalty
    prefix = PROMPT + T[:2]
    assert eng.prompt_cache.computed_ids == prefix and eng.prompt_cache.cache[0].offset == L + 2
    follow_up = prefix + [7, 8]
    eng.prepare_engine(follow_up, temp=0.8, top_k=5, **request_kw)
    del eng.model.log[:]
    out, seen = run(eng, follow_up, 3)
    t = tail(sampler=TOP_K, **want)
    repair = [("fed_ids", L + 2 - window, L + 2, prefix[-window:])] if window else []
    assert eng.model.log == repair + [t, ("step", 2, 2, L + 2), t, ("step", None, 1, L + 4), t, ("step", None, 1, L + 5)]   # first call only
    nxt = [token_at(L + 4 + i) for i in range(3)]
    assert tokens_of(out) == [[n] for n in nxt] and seen == [follow_up, follow_up + nxt[:1], follow_up + nxt[:2]]


def test_fused_plan_refused_when_the_ids_run_past_fed_ids():
    """A greedy request the plan would take, on a model whose id history ends before the prompt does: the host tail's plain step."""
    eng = make_engine(TextStub(fed=L - 1), temp=0)
    out, seen = run(eng, PROMPT, 3)
    assert eng.model.log == [("set_step_tail", {}), ("step", L, L, 0), ("set_step_tail", {}), ("step", None, 1, L), ("set_step_tail", {}), ("step", None, 1, L + 1)]
    assert tokens_of(out) == [[T[0]], [T[1]], [T[2]]] and seen == [PROMPT, PROMPT + T[:1], PROMPT + T[:2]]


# ------------------------------------------------------------------ the host-orchestrated branches
class Stochastic:
    """A sampler the fused plan does not know (no `is_greedy`, no `hip_spec`): int64 [1], like torch's own argmax."""

    def __init__(self, log):
        self.log = log

    def __call__(self, logprobs):
        self.log.append(("sampler", tuple(logprobs.shape)))
        return logprobs.argmax(dim=-1)


def host_engine(model, monkeypatch, stochastic, foreign):
    """A request outside the fused plan on every count the case does not vary: a tensor-parallel model."""
    model.tp = object()
    eng = make_engine(model, temp=0)
    log = model.log
    if stochastic:
        eng.samplers["root"] = Stochastic(log)
    else:
        assert eng.samplers["root"] is greedy
    if foreign:
        def proc(tokens, logits):
            log.append(("processor", len(tokens), tuple(logits.shape)))
            return logits
        eng.logits_processors["root"] = [proc]

    def logprobs_argmax(last):   # the op's contract on the host: (token int32 [1], logprobs fp32 [V])
        log.append(("logprobs_argmax", tuple(last.shape)))
        lp = torch.log_softmax(last.reshape(-1).float(), dim=0)
        return lp.argmax().to(torch.int32).reshape(1), lp
    monkeypatch.setattr(hip_ops, "logprobs_argmax", logprobs_argmax)
    return eng


RESET = ("set_step_tail", {})
DRAW = ("sampler", (1, V))
ARGMAX = ("logprobs_argmax", (1, V))


@pytest.mark.parametrize("stochastic", [False, True])
def test_host_tail_text_without_processors(monkeypatch, stochastic):
    eng = host_engine(TextStub(), monkeypatch, stochastic, foreign=False)
    out, seen = run(eng, PROMPT, 3)
    draw = [DRAW] if stochastic else []
    fed = 1 if stochastic else None   # only a greedy step finds its input on the device
    assert eng.model.log == [RESET, ("step", L, L, 0)] + draw + [RESET, ("step", fed, 1, L)] + draw + [RESET, ("step", fed, 1, L + 1)] + draw
    assert tokens_of(out) == [[T[0]], [T[1]], [T[2]]] and seen == [PROMPT, PROMPT + T[:1], PROMPT + T[:2]]
    assert all(tok.dtype == torch.int32 and tok.shape == (1,) and lp.shape == (V,) for tok, lp in out)


@pytest.mark.parametrize("stochastic", [False, True])
def test_host_tail_text_with_a_foreign_processor(monkeypatch, stochastic):
    eng = host_engine(TextStub(), monkeypatch, stochastic, foreign=True)
    out, seen = run(eng, PROMPT, 3)
    draw = [DRAW] if stochastic else []
    assert eng.model.log == ([RESET, ("call", L, L, 0), ("processor", L, (1, V)), ARGMAX] + draw
                             + [RESET, ("call", 1, 1, L), ("processor", L + 1, (1, V)), ARGMAX] + draw
                             + [RESET, ("call", 1, 1, L + 1), ("processor", L + 2, (1, V)), ARGMAX] + draw)
    assert tokens_of(out) == [[T[0]], [T[1]], [T[2]]] and seen == [PROMPT, PROMPT + T[:1], PROMPT + T[:2]]
    # the sampler's own result as it is, else the op's int32 token
    assert all(tok.dtype == (torch.int64 if stochastic else torch.int32) and tok.shape == (1,) and lp.shape == (V,) for tok, lp in out)


@pytest.mark.parametrize("stochastic", [False, True])
def test_host_tail_pixel_values_without_processors(monkeypatch, stochastic):
    eng = host_engine(VlmStub(), monkeypatch, stochastic, foreign=False)
    out, seen = run(eng, PROMPT, 3, pixel_values=PIXELS)
    draw = [DRAW] if stochastic else []
    fed = 1 if stochastic else None
    # the prompt alone goes through the embeddings, and step_embeds gets no ids; the later steps are the text steps
    assert eng.model.log == ([RESET, ("get_input_embeddings", L), ("step_embeds", None, L, 0)] + draw
                             + [RESET, ("step", fed, 1, L)] + draw + [RESET, ("step", fed, 1, L + 1)] + draw)
    assert tokens_of(out) == [[T[0]], [T[1]], [T[2]]] and seen == [PROMPT, PROMPT + T[:1], PROMPT + T[:2]]
    assert all(tok.dtype == torch.int32 and tok.shape == (1,) and lp.shape == (V,) for tok, lp in out)


@pytest.mark.parametrize("stochastic", [False, True])
def test_host_tail_pixel_values_with_a_foreign_processor(monkeypatch, stochastic):
    eng = host_engine(VlmStub(), monkeypatch, stochastic, foreign=True)
    out, seen = run(eng, PROMPT, 3, pixel_values=PIXELS)
    draw = [DRAW] if stochastic else []
    assert eng.model.log == ([RESET, ("get_input_embeddings", L), ("language_model", None, L, 0), ("processor", L, (1, V)), ARGMAX] + draw
                             + [RESET, ("call", 1, 1, L), ("processor", L + 1, (1, V)), ARGMAX] + draw
                             + [RESET, ("call", 1, 1, L + 1), ("processor", L + 2, (1, V)), ARGMAX] + draw)
    assert tokens_of(out) == [[T[0]], [T[1]], [T[2]]] and seen == [PROMPT, PROMPT + T[:1], PROMPT + T[:2]]
    assert all(tok.dtype == (torch.int64 if stochastic else torch.int32) and tok.shape == (1,) and lp.shape == (V,) for tok, lp in out)


def test_host_tail_on_a_model_without_a_configurable_tail():
    eng = make_engine(PlainStub(), temp=0)
    out, seen = run(eng, PROMPT, 3)
    assert eng.model.log == [("step", L, L, 0), ("step", None, 1, L), ("step", None, 1, L + 1)]
    assert tokens_of(out) == [[T[0]], [T[1]], [T[2]]] and seen == [PROMPT, PROMPT + T[:1], PROMPT + T[:2]]


def test_host_tail_top_logprobs_record_is_allocated_once(monkeypatch):
    """The host-orchestrated branches write the step's top-n record with the op: one record [n + 1] per step, one workspace per generation."""
    eng = host_engine(TextStub(), monkeypatch, stochastic=False, foreign=False)
    made, outs = [], []

    def workspace(device, rows, vocab, n):
        made.append((rows, vocab, n))
        return torch.empty(1, dtype=torch.int64)

    def top_logprobs(logprobs, n, tokens=None, count=None, workspace=None, out=None):
        assert logprobs.shape == (1, V) and tokens.dtype == torch.int32 and tokens.shape == (1,) and workspace is not None
        ids, vals = out
        outs.append(ids)
        ids[0, 0], vals[0, 0] = tokens[0], logprobs[0, int(tokens[0])]
        return ids, vals
    monkeypatch.setattr(hip_ops, "top_logprobs_workspace", workspace)
    monkeypatch.setattr(hip_ops, "top_logprobs", top_logprobs)
    gen = eng.generate_step(PROMPT, top_logprobs=2)
    for i in range(3):
        next(gen)
        ids, vals = eng.top_record
        assert ids.shape == vals.shape == (3,) and ids.dtype == torch.int32 and vals.dtype == torch.float32
        assert int(ids[0]) == T[i] and float(vals[0]) == -0.25
    gen.close()
    assert made == [(1, V, 2)] and all(o.data_ptr() == outs[0].data_ptr() and o.shape == (1, 3) for o in outs)


# ------------------------------------------------------------------ one sampler-branch rule for both engines
def test_make_sampler_and_sampling_params_select_the_same_branch():
    from proxy_inference_engine_amd.engine.batch_engine import SamplingParams
    from proxy_inference_engine_amd.samplers import make_sampler
    table = [
        (dict(temp=0), None),
        (dict(temp=0, top_p=0.9, top_k=5), None),                                        # greedy whatever else is set
        (dict(temp=0.7, top_p=0.9, min_p=0.1, top_k=5), ("top_p", 0.7, 0.9, 0)),           # top-p first
        (dict(temp=0.7, top_p=1.0, min_p=0.1, min_tokens_to_keep=2, top_k=5), ("min_p", 0.7, 0.1, 2)),   # top_p == 1 is no top-p
        (dict(temp=0.7, top_p=0.0, min_p=0.1), ("min_p", 0.7, 0.1, 1)),
        (dict(temp=0.8, top_p=1.0, top_k=5), ("top_k", 0.8, 0.0, 5)),
        (dict(temp=1.5, top_p=1.0, top_k=0), ("categorical", 1.5, 0.0, 0)),
        (dict(temp=1.5, top_p=1.0), ("categorical", 1.5, 0.0, 0)),
    ]
    for kw, want in table:
        sampler = make_sampler(**kw)
        assert (None if getattr(sampler, "is_greedy", False) else sampler.hip_spec) == want, kw
        assert SamplingParams(**kw).hip_spec() == want, kw
