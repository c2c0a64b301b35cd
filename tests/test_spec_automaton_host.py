"""Host side of grammar-constrained speculative decoding: TokenAutomaton.forced() against a brute-force loop, the reference
drafter's properties (tests/spec_automaton_reference.py restates pie_token_dfa_draft's rule), SpeculativeParams(grammar=) and
check_speculative_grammar.  No GPU."""
import numpy as np
import pytest
import torch

from proxy_inference_engine_amd.logits_processors import TokenAutomaton, make_logit_bias, make_repetition_penalty, make_token_automaton, make_token_mask
from tests import spec_automaton_reference as ref
from tests.test_token_automaton_host import CHOICES, vocabulary


def random_automaton(rng, V: int, S: int, C: int, density: float) -> TokenAutomaton | None:
    cls = rng.integers(0, C, size=V).astype(np.int32)
    trans = np.where(rng.random((S, C)) < density, rng.integers(0, S, size=(S, C)), -1).astype(np.int32)
    try:
        return TokenAutomaton(cls, trans, 0)
    except ValueError:  # a reachable state that allows nothing
        return None


def poisoned_tables(a: TokenAutomaton) -> list[np.ndarray]:
    """Forced tables that lie: ids at and beyond V, a wrong next state, next = S, every state 'forced', and a negative id."""
    good, S, V = a.forced(), a.n_states, a.vocab_size
    out = []
    for ids, nxt in ((V, 0), (V + 5, 0), (None, None), (None, S), (0, 0), (-3, 0)):
        t = good.copy()
        if ids is not None:
            t[:, 0] = ids
        if nxt is None:
            t[:, 1] = np.where(t[:, 1] >= 0, (t[:, 1] + 1) % S, 0)   # a wrong next state everywhere
        else:
            t[:, 1] = nxt
        out.append(t)
    return out


def test_forced_equals_the_brute_force_loop():
    rng = np.random.default_rng(23)
    seen_forced = made = 0
    for V, S, C, density in [(65, 1, 1, 1.0), (64, 1, 3, 0.5), (40, 7, 1, 1.0), (97, 12, 9, 0.2), (97, 12, 40, 0.05), (300, 30, 120, 0.02), (33, 5, 33, 0.1)]:
        for _ in range(30):
            a = random_automaton(rng, V, S, C, density)
            if a is None:
                continue
            made += 1
            got = a.forced()
            assert got.dtype == np.int32 and got.shape == (S, 2) and np.array_equal(got, ref.forced_brute(a)), (V, S, C)
            assert a.forced() is got                                     # cached on the object
            seen_forced += int((got[:, 0] >= 0).sum())
    assert made > 60 and seen_forced > 20, "the random automata force nothing: the comparison tests nothing"
    # a class of two ids that is the only allowed class is not forced; a class of one id is
    two = TokenAutomaton(np.array([0, 1, 1, 2], dtype=np.int32), np.array([[-1, 0, -1], [-1, -1, 1]], dtype=np.int32), 0)
    assert two.forced().tolist() == [[-1, -1], [3, 1]]
    # an allowed class no id maps to does not count
    ghost = TokenAutomaton(np.array([0, 0, 2], dtype=np.int32), np.array([[-1, 0, 0]], dtype=np.int32), 0)
    assert ghost.forced().tolist() == [[2, 0]]


def test_forced_of_from_choices():
    toks, eos = vocabulary(1)
    a = TokenAutomaton.from_choices(CHOICES, toks, eos)
    assert np.array_equal(a.forced(), ref.forced_brute(a))
    sink = a.n_states - 1
    assert a.forced()[sink].tolist() == [eos[0], sink]                  # one EOS id: the sink is forced
    assert a.forced()[a.start].tolist() == [-1, -1]
    b = TokenAutomaton.from_choices(CHOICES, toks, [eos[0], eos[0] + 1])
    assert np.array_equal(b.forced(), ref.forced_brute(b)) and b.forced()[b.n_states - 1].tolist() == [-1, -1]   # two: it is not


def chain(V=97, L=33):
    run = [int(t) for t in (np.arange(L) * 7 + 3) % V]
    cls, trans = ref.chain_automaton(V, run, branch_ids=list(range(0, V, 2)))
    return TokenAutomaton(cls, trans, 0), run


def test_reference_drafter_properties():
    rng = np.random.default_rng(5)
    checked = 0
    for V, S, C, density in [(65, 6, 5, 0.5), (64, 9, 20, 0.15), (97, 12, 40, 0.08)]:
        for _ in range(40):
            a = random_automaton(rng, V, S, C, density)
            if a is None:
                continue
            rec, arena = ref.record_of(a, cls_off=3)
            for k in (1, 7, 31):
                for s0 in range(S):
                    cand = rng.integers(-1, V + 1, size=31).tolist()
                    for table in [a.forced()] + poisoned_tables(a):
                        ids, n = ref.dfa_draft(rec, s0, arena, table, V, cand, int(rng.integers(0, 32)), k)
                        assert n == len(ids) <= k
                        s = s0                                             # every id is allowed along the walk, whatever the table holds
                        for t in ids:
                            assert 0 <= s < S and 0 <= t < V and a.allowed(s)[t], (V, S, C, s0, ids)
                            s = a.step(s, t)
                        checked += n
    assert checked > 1000
    # the grammar allows all of the candidate and forces nothing: the output is the candidate
    free = TokenAutomaton(np.zeros(50, dtype=np.int32), np.array([[0]], dtype=np.int32), 0)
    rec, arena = ref.record_of(free)
    cand = list(range(31))
    assert ref.dfa_draft(rec, 0, arena, free.forced(), 50, cand, 31, 31) == (cand, 31)
    assert ref.dfa_draft(rec, 0, arena, free.forced(), 50, cand, 9, 5) == (cand[:5], 5)
    # a forced cycle longer than k is cut at k; nothing looked up: the grammar alone drafts its run
    a, run = chain()
    rec, arena = ref.record_of(a)
    assert ref.dfa_draft(rec, 1, arena, a.forced(), 97, [], 0, 7) == (run[:7], 7)
    assert ref.dfa_draft(rec, a.n_states - 1, arena, a.forced(), 97, [], 0, 31) == ([run[-1]] * 31, 31)
    # a candidate that agrees with the run stays live and goes on behind it; one that differs is replaced and dropped
    assert ref.dfa_draft(rec, 0, arena, a.forced(), 97, [4] + run[:3], 4, 6) == ([4] + run[:5], 6)
    assert ref.dfa_draft(rec, 0, arena, a.forced(), 97, [5, 1, 2], 3, 6) == ([], 0)          # id 5 is odd: the branch forbids it
    # a left automaton, or an unarmed record, passes the candidate through
    assert ref.dfa_draft(rec, -1, arena, a.forced(), 97, [5, 1, 2], 3, 2) == ([5, 1], 2)
    assert ref.dfa_draft((0, 0, 0, 0), 0, arena, a.forced(), 97, list(range(40)), 1000, 31) == (list(range(31)), 31)   # the count is clamped
    # the walk is the advance op iterated
    assert ref.dfa_walk(rec, 0, arena, 97, [4] + run[:2] + [run[2] + 1, 4]) == [0, 1, 2, 3, -1, -1]
    assert ref.dfa_walk((0, 0, 0, 0), 5, arena, 97, [1, 2]) == [5, 5, 5]


def test_speculative_params_grammar():
    from proxy_inference_engine_amd.engine.inference_engine import SpeculativeParams
    assert SpeculativeParams().grammar is False and SpeculativeParams(grammar=True).grammar is True
    assert list(SpeculativeParams.__dataclass_fields__)[-1] == "grammar"
    with pytest.raises(ValueError, match="grammar is a bool"):
        SpeculativeParams(grammar=1)

    class Drafter:
        step = set_step_tail = history = logprobs = None
    with pytest.raises(ValueError, match="grammar is not available with a draft model"):
        SpeculativeParams(grammar=True, draft_model=Drafter())


def test_check_speculative_grammar():
    from proxy_inference_engine_amd import samplers
    from proxy_inference_engine_amd.engine import inference_engine as ie
    toks, eos = vocabulary(6)
    a = TokenAutomaton.from_choices(CHOICES, toks, eos)
    greedy, top_p = samplers.make_sampler(temp=0), samplers.make_sampler(temp=0.8, top_p=0.9)
    auto, pen, bias = make_token_automaton(a), make_repetition_penalty(1.3, 20), make_logit_bias({5: 1.0})

    class Stub:   # what the checks read of a model
        tp = None
        spec_step = spec_step_tail = spec_step_grammar = set_step_tail = None
    none = (None, None, None, None)
    plan = ie.check_speculative_grammar(Stub(), greedy, [auto, pen], *none)
    assert plan["automaton"] is auto and plan["repetition_penalty"] == 1.3 and plan["sampler"] is None
    assert ie.check_speculative_grammar(Stub(), top_p, [auto, pen, bias], *none)["sampler"] is not None
    assert ie.check_speculative_grammar(Stub(), greedy, [auto], *none)["automaton"] is auto      # the automaton alone is enough
    eng = ie.InferenceEngine.__new__(ie.InferenceEngine)
    eng.structuring_engine = None
    mask = make_token_mask(torch.ones(a.vocab_size, dtype=torch.bool))
    for procs, name in (([mask, pen], "a token mask"), ([mask, auto], "a token mask"),
                        (eng.make_processors(token_automaton=a, frequency_penalty=0.5), "frequency / presence penalties"),
                        (eng.make_processors(token_automaton=a, dry_multiplier=0.8), "a DRY penalty")):
        with pytest.raises(ValueError, match=name):
            ie.check_speculative_grammar(Stub(), greedy, procs, *none)
    with pytest.raises(ValueError, match="no token automaton"):
        ie.check_speculative_grammar(Stub(), greedy, [pen], *none)
    for env, name in (((object(), None, None, None), "a structuring engine"), ((None, object(), None, None), "pixel_values"),
                      ((None, None, 4, None), "kv_bits"), ((None, None, None, 64), "max_kv_size")):
        with pytest.raises(ValueError, match=name):
            ie.check_speculative_grammar(Stub(), greedy, [auto], *env)

    class Old:    # a model without the pass
        tp = None
        set_step_tail = None
    with pytest.raises(ValueError, match="no spec_step_grammar"):
        ie.check_speculative_grammar(Old(), greedy, [auto], *none)
    # the existing checks keep refusing an automaton
    with pytest.raises(ValueError, match="a token automaton"):
        ie.check_speculative_tail(Stub(), greedy, [auto, pen], *none)
    with pytest.raises(ValueError, match="a token automaton"):
        ie.check_speculative(Stub(), greedy, [auto], None, None, None, None)
    # which check a request goes through
    sp = ie.SpeculativeParams
    route = lambda s, procs, sampler=greedy: ie._speculative_request_plan(Stub(), None, s, {"root": sampler}, {"root": procs}, *none)
    assert route(sp(grammar=True), [auto, pen])["automaton"] is auto
    with pytest.raises(ValueError, match="a token automaton"):
        route(sp(configured_tail=True), [auto, pen])
    with pytest.raises(ValueError, match="a token automaton"):
        route(sp(), [auto])
    assert "automaton" not in route(sp(grammar=True), [pen])                  # without an automaton: configured_tail=True's path
    assert route(sp(grammar=True), [pen]) == route(sp(configured_tail=True), [pen])
    assert route(sp(grammar=True), []) is None                                # and a greedy request without processors the greedy path
