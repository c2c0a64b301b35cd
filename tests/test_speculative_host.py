"""No GPU: greedy speculative decoding's host half -- the reference drafter on hand-written cases, the engine loop over a
stub model (a table of next tokens behind Model's speculative interface), and the exported symbols."""
from pathlib import Path

import pytest
import torch

from tests import speculative_reference as ref


# ------------------------------------------------------------------ the reference drafter, by hand
@pytest.mark.parametrize("ids,nmax,nmin,k,want", [
    ([1, 2, 3, 4, 5], 3, 1, 4, []),                                  # no id occurs twice: no match
    ([7, 7], 3, 2, 4, []),                                           # len <= ngram_min
    ([7], 1, 1, 4, []),
    ([5, 1, 9, 5, 2, 8, 5], 1, 1, 2, [2, 8]),                        # the most recent of several matches (p = 3, not p = 0)
    ([1, 2, 3, 9, 3, 8, 1, 2, 3], 3, 1, 2, [9, 3]),                  # n = 3 at p = 0 beats the more recent n = 1 match at p = 4
    ([4, 6, 4, 6], 3, 1, 5, [4, 6, 4, 6, 4]),                        # a period-2 tail extends to k
    ([9, 1, 2, 3, 1, 2, 3], 3, 1, 7, [1, 2, 3, 1, 2, 3, 1]),         # a period-3 tail drafts k ids, not 3
    ([3, 5, 5], 2, 1, 3, [5, 5, 5]),                                 # a match ending at len - 1: the copy starts on the last id
    ([1, 2, 1, 2, 7], 8, 3, 3, []),                                  # matches only below ngram_min
])
def test_reference_drafter_by_hand(ids, nmax, nmin, k, want):
    assert ref.ngram_draft(ids, nmax, nmin, k) == want


def test_reference_accept_rule():
    assert ref.accept([5, 6, 7, 8], [5, 6, 7]) == (3, [5, 6, 7, 8])
    assert ref.accept([5, 6, 7, 8], [5, 9, 7]) == (1, [5, 6, -1, -1])
    assert ref.accept([5, 6, 7, 8], [-1, 6, 7]) == (0, [5, -1, -1, -1])


# ------------------------------------------------------------------ the engine loop over a stub model
V = 64


class StubCache:
    def __init__(self):
        self.offset = 0


class StubModel:
    """Greedy decoding of a fixed text: the token after a sequence of length n is text[n].  Model's speculative interface, host only."""
    device, tp, _page_pool, spec_min_rows = "cpu", None, None, 6

    def __init__(self, text):
        self.text, self.seq, self.last, self.calls = [int(t) for t in text], [], None, []
        self._rec, self._draft = None, []

    def make_cache(self):
        return [StubCache()]

    def next_token(self, seq):
        return self.text[len(seq)]

    def _rows(self, tokens):
        lp = torch.full((len(tokens), V), -30.0)
        for r, t in enumerate(tokens):
            lp[r, t] = -0.25
        return lp

    def step(self, ids, cache):
        fed = [self.last] if ids is None else [int(t) for t in ids.tolist()]
        self.calls.append(("step", len(fed)))
        self.seq += fed
        cache[0].offset += len(fed)
        self.last = self.next_token(self.seq)
        lp = self._rows([self.last])[0]
        return torch.tensor([self.last], dtype=torch.int32), lp, lp

    def draft(self, ngram_max, ngram_min, k):
        self._draft = ref.ngram_draft(self.seq + [self.last], ngram_max, ngram_min, k)
        self._rec = ([self.last], len(self._draft))

    @property
    def spec_draft(self):
        return torch.tensor(self._draft + [0] * (31 - len(self._draft)), dtype=torch.int32)

    @property
    def spec_tokens(self):
        return torch.tensor(self._rec[0] + [-1] * (32 - len(self._rec[0])), dtype=torch.int32)

    def spec_read(self):
        return self._rec

    def spec_step(self, draft_ids, cache, then_draft=None):
        draft = [int(t) for t in draft_ids.tolist()]
        self.calls.append(("pass", len(draft)))
        greedy, s = [], self.seq + [self.last]
        for i in range(len(draft) + 1):
            greedy.append(self.next_token(s))
            if i == len(draft) or draft[i] != greedy[-1]:
                break
            s = s + [draft[i]]
        self.seq = self.seq + [self.last] + greedy[:-1]
        cache[0].offset += len(greedy)
        self.last = greedy[-1]
        self._draft = ref.ngram_draft(self.seq + [self.last], *then_draft) if then_draft else []
        self._rec = (greedy, len(self._draft))
        return torch.tensor(greedy, dtype=torch.int32), len(greedy), self._rows(greedy)


BLOCK = [11, 12, 13, 14, 15, 16, 17, 18, 19, 20]
# a text whose continuation repeats the prompt (full accepts), departs from it (partial rejects) and turns novel (plain steps)
TEXT = BLOCK + [1, 2] + BLOCK + [3] + BLOCK[:4] + [40, 41, 42, 43, 44, 45, 46, 47] + BLOCK + BLOCK[:6] + [50, 51, 52] + BLOCK + list(range(21, 40))
PROMPT_LEN = 13


def make_engine(stop=()):
    from proxy_inference_engine_amd import InferenceEngine
    eng = InferenceEngine(model=StubModel(TEXT), stop_tokens=stop)
    eng.prepare_engine(TEXT[:PROMPT_LEN], temp=0)
    return eng


def test_engine_loop_follows_the_simulated_schedule():
    from proxy_inference_engine_amd import SpeculativeParams
    sp = SpeculativeParams(num_draft=7, ngram_max=3, ngram_min=1, min_draft=5)
    n_tokens = 60
    want_tokens, schedule = ref.simulate(TEXT[:PROMPT_LEN], lambda s: TEXT[len(s)], n_tokens, 7, 3, 1, 5)
    kinds = {("full" if e[2] == e[1] else "partial") if e[0] == "pass" else "step" for e in schedule}
    assert kinds == {"full", "partial", "step"}, schedule          # the text exercises every branch
    eng = make_engine()
    got, yields = [], 0
    gen = eng.generate_step(TEXT[:PROMPT_LEN], speculative=sp)
    while len(got) < n_tokens:
        tokens, rows = next(gen)
        assert tokens.dtype == torch.int32 and rows.shape == (tokens.numel(), V)
        assert rows.argmax(dim=1).tolist() == tokens.tolist()      # row r belongs to token r
        got += tokens.tolist()
        yields += 1
    assert got == want_tokens[:len(got)] == TEXT[PROMPT_LEN:PROMPT_LEN + len(got)]
    done = schedule[:yields - 1]                                   # the first yield is the prompt's step
    passes = [e for e in done if e[0] == "pass"]
    assert eng.spec_stats == {"passes": len(passes), "steps": len(done) - len(passes), "drafted": sum(e[1] for e in passes),
                              "accepted": sum(e[2] for e in passes)}
    assert eng.model.calls[1:] == [("pass", e[1]) if e[0] == "pass" else ("step", 1) for e in done]
    # the prompt cache holds the ids whose rows the cache holds: the text up to the cache's offset
    assert eng.prompt_cache.computed_ids == TEXT[:eng.prompt_cache.cache[0].offset]


def test_fallback_to_steps_below_min_draft():
    from proxy_inference_engine_amd import SpeculativeParams
    eng = make_engine()
    gen = eng.generate_step(TEXT[:PROMPT_LEN], speculative=SpeculativeParams(num_draft=4, min_draft=4))   # 5 rows: below the many-row pass
    got = [t for _ in range(20) for t in next(gen)[0].tolist()]
    assert got == TEXT[PROMPT_LEN:PROMPT_LEN + 20]
    assert eng.spec_stats == {"passes": 0, "steps": 19, "drafted": 0, "accepted": 0}
    assert all(c[0] == "step" for c in eng.model.calls)


def test_generate_stops_inside_an_accepted_run():
    from proxy_inference_engine_amd import SpeculativeParams
    sp = SpeculativeParams()
    _, schedule = ref.simulate(TEXT[:PROMPT_LEN], lambda s: TEXT[len(s)], 12, 7, 3, 1, 5)
    assert schedule[0][0] == "pass" and schedule[0][2] >= 3          # the first pass accepts a run: tokens 1 .. of the continuation
    stop = TEXT[PROMPT_LEN + 3]                                      # inside that run
    assert stop not in TEXT[PROMPT_LEN:PROMPT_LEN + 3]
    eng = make_engine(stop=(stop,))
    gen = eng.generate(TEXT[:PROMPT_LEN], speculative=sp)
    out = []
    try:
        while True:
            out.append(next(gen)[0])
    except StopIteration as e:
        assert e.value == "stop"
    assert out == TEXT[PROMPT_LEN:PROMPT_LEN + 3]
    # max_completion_tokens inside a run: exactly that many tokens, reason "length"
    eng = make_engine()
    gen = eng.generate(TEXT[:PROMPT_LEN], speculative=sp, max_completion_tokens=4)
    out = []
    try:
        while True:
            out.append(next(gen)[0])
    except StopIteration as e:
        assert e.value == "length"
    assert out == TEXT[PROMPT_LEN:PROMPT_LEN + 4]
    # without `speculative` the same request is the plain loop
    eng = make_engine()
    plain = [t for t, _ in eng.generate(TEXT[:PROMPT_LEN], max_completion_tokens=4)]
    assert plain == out and not hasattr(eng, "spec_stats")


def test_every_refusal_by_name():
    from proxy_inference_engine_amd import SpeculativeParams
    from proxy_inference_engine_amd.engine.inference_engine import check_speculative

    class Greedy:
        is_greedy = True

    class Pool:
        dtype = torch.int8

    m = StubModel(TEXT)
    check_speculative(m, Greedy(), [], None, None, None, None)      # nothing to refuse
    cases = [(dict(sampler=object()), "non-greedy sampler"), (dict(processors=[lambda t, x: x]), "logits processors"),
             (dict(structuring_engine=object()), "structuring engine"), (dict(pixel_values=torch.zeros(1)), "pixel_values"),
             (dict(kv_bits=8), "kv_bits"), (dict(max_kv_size=64), "max_kv_size")]
    for kw, name in cases:
        args = dict(sampler=Greedy(), processors=[], structuring_engine=None, pixel_values=None, kv_bits=None, max_kv_size=None)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            check_speculative(m, *args.values())
    tp_model, i8_model = StubModel(TEXT), StubModel(TEXT)
    tp_model.tp, i8_model._page_pool = object(), Pool()
    with pytest.raises(ValueError, match="tensor-parallel"):
        check_speculative(tp_model, Greedy(), [], None, None, None, None)
    with pytest.raises(ValueError, match="int8 KV pages"):
        check_speculative(i8_model, Greedy(), [], None, None, None, None)
    # through the engine: a sampling request and a request with a processor
    eng = make_engine()
    eng.prepare_engine(TEXT[:PROMPT_LEN], temp=0.7)
    with pytest.raises(ValueError, match="non-greedy sampler"):
        next(eng.generate_step(TEXT[:PROMPT_LEN], speculative=SpeculativeParams()))
    eng.prepare_engine(TEXT[:PROMPT_LEN], temp=0, repetition_penalty=1.3)
    with pytest.raises(ValueError, match="logits processors"):
        next(eng.generate_step(TEXT[:PROMPT_LEN], speculative=SpeculativeParams()))
    with pytest.raises(ValueError, match="prompt_logprobs"):
        next(make_engine().generate_step(TEXT[:PROMPT_LEN], speculative=SpeculativeParams(), prompt_logprobs=2))
    for bad in (dict(num_draft=0), dict(num_draft=32), dict(min_draft=8), dict(ngram_min=0), dict(ngram_max=9), dict(ngram_min=4, ngram_max=3)):
        with pytest.raises(ValueError, match="SpeculativeParams"):
            SpeculativeParams(**bad)


def test_new_symbols_are_exported():
    import proxy_inference_engine_amd as pkg
    from proxy_inference_engine_amd import _ffi, engine, hip_ops
    from proxy_inference_engine_amd.models.llama import Model
    assert pkg.SpeculativeParams is engine.SpeculativeParams and "SpeculativeParams" in pkg.__all__ and "SpeculativeParams" in engine.__all__
    assert pkg.SpeculativeParams() == pkg.SpeculativeParams(num_draft=7, ngram_max=3, ngram_min=1, min_draft=5)
    for name in ("ngram_draft", "spec_verify", "ngram_draft_workspace", "spec_verify_workspace"):
        assert callable(getattr(hip_ops, name))
    for name in ("spec_step", "draft", "spec_read"):
        assert callable(getattr(Model, name))
    for name in ("pie_ngram_draft", "pie_spec_verify", "pie_decoder_spec_step", "pie_decoder_spec_workspace_bytes"):
        assert name in _ffi.EXPORTS
    header = (Path(__file__).resolve().parent.parent / "include" / "pie_hip.h").read_text()
    for name in ("pie_ngram_draft(", "pie_spec_verify(", "pie_decoder_spec_step(", "pie_decoder_spec_workspace_bytes("):
        assert name in header
