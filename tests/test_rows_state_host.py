"""No GPU: the two host-side owners of the multi-sequence passes' per-row tail state -- the model's per-rows_cap buffer
cache and the engine's seating object, the latter driven directly with a recording fake of the model's write_* methods (no engine loop)."""
from collections import Counter
from types import SimpleNamespace

import pytest
import torch

from proxy_inference_engine_amd.engine.batch_engine import SamplingParams, _RowSeats, same_occupant
from proxy_inference_engine_amd.models.llama.rows_state import RowsCapCache


# ------------------------------------------------------------------ 1. the rows_cap cache
def counting_cache():
    made = []

    def make(rows_cap):
        made.append(rows_cap)
        return {"table": torch.zeros((rows_cap, 4), dtype=torch.int64), "ws": torch.zeros(8 * rows_cap, dtype=torch.int64)}
    return RowsCapCache(make), made


def test_a_sixth_rows_cap_evicts_the_least_recently_used():
    cache, made = counting_cache()
    first = {r: cache.get(r) for r in (1, 2, 3, 4)}
    cache.get(5)                                    # evicts 1, the oldest
    assert made == [1, 2, 3, 4, 5]
    assert cache.get(2) is first[2]                 # 2 is now the most recent: order 3, 4, 5, 2
    cache.get(6)                                    # the sixth distinct rows_cap evicts 3 -- not 2, the most recent of the first four
    assert made == [1, 2, 3, 4, 5, 6]
    assert cache.get(2) is first[2] and cache.get(4) is first[4] and made == [1, 2, 3, 4, 5, 6]
    assert cache.get(3) is not first[3] and made[-1] == 3     # 3 was evicted and is made again (which evicts 5, the oldest by now)
    assert cache.get(1) is not first[1] and made[-1] == 1


def test_get_returns_the_same_object_and_makes_it_the_most_recent():
    cache, made = counting_cache()
    a = cache.get(7)
    assert cache.get(7) is a and made == [7]
    for r in (8, 9, 10):
        cache.get(r)
    assert cache.get(7) is a                        # moved to the most recent position: the next three evict 8, 9, 10 and leave it
    for r in (11, 12, 13):
        cache.get(r)
    assert cache.get(7) is a and made == [7, 8, 9, 10, 11, 12, 13]
    assert cache.get(8) is not None and made[-1] == 8


def test_set_clear_set_keeps_the_tensors():
    cache, _ = counting_cache()
    armed = cache.get(3)                            # set
    ptrs = {k: t.data_ptr() for k, t in armed.items()}
    armed = None                                    # clear: the model forgets what is armed, the cache keeps the buffers
    again = cache.get(3)                            # set
    assert {k: t.data_ptr() for k, t in again.items()} == ptrs


# ------------------------------------------------------------------ 2. the occupancy rule
@pytest.mark.parametrize("have,want,same", [(None, None, True), ((2, 5), (2, 5), True), ((2, 5), (2, 6), True), ((2, 5), (2, 7), False), ((2, 5), (2, 4), False),
                                            ((2, 5), (3, 6), False), (None, (2, 0), False), ((2, 5), None, False)])
def test_same_occupant(have, want, same):
    assert same_occupant(have, want) is same


# ------------------------------------------------------------------ 3. the seating object
class Recorder:
    """What _RowSeats calls on a model, as a list of (method, arguments)."""

    def __init__(self, V=70):
        self.args, self.calls = SimpleNamespace(vocab_size=V), []

    def __getattr__(self, name):
        if not name.startswith(("set_batch_", "write_batch_", "clear_batch_")):
            raise AttributeError(name)

        def call(*a, **kw):
            self.calls.append((name, a, kw))
            if name == "set_batch_top_logprobs":
                self.top = {"ids": torch.zeros((a[0], a[1] + 1), dtype=torch.int32), "vals": torch.zeros((a[0], a[1] + 1)), "count": torch.zeros(a[0], dtype=torch.int32)}
                return self.top
        return call

    def take(self, name=None):
        out, self.calls = [c for c in self.calls if name is None or c[0] == name], []
        return out


def active(*pairs):
    return [SimpleNamespace(request=r, generated=list(g)) for r, g in pairs]


PROMPTS = [[1, 2, 3], [4, 5], [6, 7, 8, 9]]
PARAMS = [SamplingParams(temp=0.7, top_k=4, repetition_penalty=1.2), SamplingParams(temp=0.9), SamplingParams()]
SEEDS = [11, 22, 33]
CNTS = [(0.5, 0.0), None, (0.0, 1.5)]


def test_a_request_that_keeps_its_row_is_not_rewritten():
    m = Recorder()
    with _RowSeats(m, 4, PROMPTS, tails=(PARAMS, SEEDS), cnts=CNTS) as seats:
        seats.seat([0, 2], active())                                   # both arrive: written
        first = m.take()
        assert [c[1][0] for c in first if c[0] == "write_batch_tail"][-1] == [0, 1]
        seats.seat([0, 2], active((0, [40]), (2, [41])))               # one token further on, same rows
        seats.seat([0, 2], active((0, [40, 42]), (2, [41, 43])))
        assert [(c[0], c[1][0]) for c in m.take()] == [("write_batch_count_penalty", []), ("write_batch_tail", [])] * 2
        seats.seat([0, 2], active((0, [40, 42, 44, 45]), (2, [41, 43, 46])))   # request 0 two tokens further on is not the row's own progress
        assert [(c[0], c[1][0]) for c in m.take()] == [("write_batch_count_penalty", [0]), ("write_batch_tail", [0])]


def test_a_request_that_moves_is_rewritten_there_and_its_old_row_is_neutral():
    m = Recorder()
    with _RowSeats(m, 4, PROMPTS, tails=(PARAMS, SEEDS), cnts=CNTS) as seats:
        seats.seat([1, 0], active((1, [50])))                          # request 0 arrives in row 1
        m.take()
        gen = [40, 41, 40, 40]
        seats.seat([0, None], active((0, gen)))                        # request 1 left: request 0 moves to row 0, a filling prompt takes row 1
        (_, (rows, recs, gens), _), = m.take("write_batch_count_penalty")
        assert rows == [0, 1] and recs == [(0.5, 0.0, len(PROMPTS[0])), None] and gens[1] is None     # the row it left: a zero record
        assert Counter(gens[0]) == Counter({40: 3, 41: 1})             # the counts the model builds: the multiplicities of its generated ids


def test_a_moved_requests_sampler_record_counts_the_tokens_it_has_drawn():
    m = Recorder()
    with _RowSeats(m, 4, PROMPTS, tails=(PARAMS, SEEDS)) as seats:
        seats.seat([1, 0], active((1, [50])))
        m.take()
        gen = [40, 41, 40, 40]
        seats.seat([0, None], active((0, gen)))
        (_, (rows, recs, fed), _), = m.take()
        assert rows == [0, 1]
        assert bytes(recs[0]) == bytes(PARAMS[0].record(len(gen), SEEDS[0]))       # calls = the tokens drawn
        assert fed[0] == PROMPTS[0] + gen[:-1]                         # the ring: what it has been fed (the last id is this pass's input)
        assert bytes(recs[1]) == bytes(SamplingParams().record()) and fed[1] is None    # the row it left: greedy, the ring left alone


def test_a_filling_prompt_is_neutral_in_every_kind():
    m = Recorder()
    mask = torch.zeros(70, dtype=torch.bool)
    mask[::2] = True
    edits = [SamplingParams(token_mask=mask, logit_bias={3: 1.5}).edits(70)] * 3
    with _RowSeats(m, 4, PROMPTS, tails=(PARAMS, SEEDS), edits=edits, cnts=CNTS, tops=[3, 3, 3]) as seats:
        seats.seat([0, 2], active())                                   # two requests hold rows 0 and 1 ...
        assert m.top["count"].tolist() == [3, 3, -1, -1]
        m.take()
        seats.seat([None, None], active())                             # ... which two prompts that are still filling take over
        calls = {c[0] + ":" + "/".join(sorted(c[2])): c for c in m.take()}
        assert m.top["count"].tolist() == [-1, -1, -1, -1]
        assert calls["write_batch_edits:masks"][1] == ([0, 1],) and calls["write_batch_edits:masks"][2] == {"masks": [None, None]}
        assert calls["write_batch_edits:biases"][1] == ([0, 1],) and calls["write_batch_edits:biases"][2] == {"biases": [None, None]}
        assert calls["write_batch_count_penalty:"][1] == ([0, 1], [None, None], [None, None])          # zero records
        rows, recs, fed = calls["write_batch_tail:"][1]
        assert rows == [0, 1] and fed == [None, None] and all(bytes(r) == bytes(SamplingParams().record()) for r in recs)   # greedy


def test_a_callable_mask_is_evaluated_every_pass_and_uploaded_when_it_differs():
    seen = []

    def grammar(tokens):
        seen.append(list(tokens))
        return [0, 1] if len(tokens) < 5 else [2, 3]                   # the allowed ids change once the request has been fed five

    m = Recorder()
    edits = [SamplingParams(token_mask=grammar).edits(70), (None, None), (None, None)]
    with _RowSeats(m, 4, PROMPTS, edits=edits) as seats:
        m.take()
        seats.seat([0, 1], active())
        assert [c[1][0] for c in m.take("write_batch_edits")] == [[0]]         # row 0: its words; row 1 (a request without edits) was never armed
        seats.seat([0, 1], active((0, [9]), (1, [9])))
        assert m.take() == []                                                   # evaluated, the same words: nothing goes up
        seats.seat([0, 1], active((0, [9, 9]), (1, [9, 9])))
        (_, (rows,), kw), = m.take()
        assert rows == [0] and list(kw) == ["masks"] and kw["masks"][0].tolist()[0] == 0b1100
        assert seen == [PROMPTS[0], PROMPTS[0] + [9], PROMPTS[0] + [9, 9]]


@pytest.mark.parametrize("raises", [False, True])
def test_leaving_clears_every_kind_that_was_armed(raises):
    m = Recorder()
    edits = [SamplingParams(logit_bias={3: 1.5}).edits(70)] * 3
    try:
        with _RowSeats(m, 4, PROMPTS, tails=(PARAMS, SEEDS), edits=edits, tops=[0, 2, 1]):
            armed = m.take()
            if raises:
                raise KeyError("the body failed")
    except KeyError:
        assert raises
    assert [c[0] for c in armed] == ["set_batch_tail", "write_batch_tail", "set_batch_edits", "write_batch_edits", "set_batch_top_logprobs"]
    assert armed[2][1:] == ((4,), {"masks": False, "bias_cap": 1}) and armed[4][1] == (4, 2) and m.top["count"].tolist() == [-1] * 4
    assert [c[0] for c in m.take()] == ["clear_batch_tail", "clear_batch_edits", "clear_batch_top_logprobs"]      # not the count penalty: never armed
    m = Recorder()
    with _RowSeats(m, 4, PROMPTS) as seats:                            # nothing asked for: nothing armed, written or cleared
        seats.seat([0, None], active())
        assert seats.lone_step(0) and seats.records(2) == [None, None]
    assert m.calls == []
