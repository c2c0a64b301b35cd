"""Batched speculation under per-request tails on the CPU: the rules of tests/spec_batch_tail_reference.py against
hand-made cases, and BatchedEngine(speculative=SpeculativeParams(batch_tail=True)) on a stub model that carries spec_step_batch_tail.
The stub's next token is a function of the sequence alone, and it keeps what the device would keep per seat -- the record's `calls` and
the ring of fed ids -- moving them as the passes would: every pass first checks that seat s holds exactly its occupant's stream position
and fed ids, so a seat the host rewrote wrongly, or failed to move, fails the pass that reads it."""
import types

import numpy as np
import pytest

from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine, SamplingParams, _RowSeats
from proxy_inference_engine_amd.engine.inference_engine import SpeculativeParams
from tests import spec_batch_reference as sb
from tests import spec_batch_tail_reference as tr
from tests.test_spec_batch_host import SpecStub, alone, cyclic, repeating

SP = SpeculativeParams(num_draft=7, ngram_max=3, ngram_min=1, min_draft=5, batch_tail=True)
V = 64


# ------------------------------------------------------------------ the rules
def test_window_below_the_context_and_at_position_zero():
    ring = np.full(tr.RING, -9)
    ring[:5] = [10, 11, 12, 13, 14]                                      # positions 0..4
    fed = [20, 21, 22]
    assert tr.window(ring, fed, 5, 0, 3) == [13, 14, 20]
    assert tr.window(ring, fed, 5, 2, 3) == [20, 21, 22]                 # the drafts before the row, and its own input
    assert tr.window(ring, fed, 5, 2, 60) == [10, 11, 12, 13, 14, 20, 21, 22]
    assert tr.window(ring, fed, 0, 0, 60) == [20]                        # pos0 = 0: nothing comes from the ring
    assert tr.window(ring, fed, 0, 2, 2) == [21, 22]
    assert tr.window(ring, fed, 5, 1, 0) == [21] and tr.window(ring, fed, 5, 1, 5000) == tr.window(ring, fed, 5, 1, 1024)   # the clamps


def test_window_where_the_segment_wraps_onto_positions_it_still_reads():
    """pos0 = 1020, context 1024: the ring's slot of position 1020 + j still holds position j - 4, which row 0's window reads (j >= 4)
    and which no row may have overwritten; a row's own segment never comes from the ring."""
    ring = np.arange(1000, 1000 + tr.RING)                               # slot q holds 1000 + q: positions 0 .. 1019 in slots 0 .. 1019, ...
    ring[1020:] = [-1, -2, -3, -4]                                       # ... and slots 1020 .. 1023 hold what position -4 .. -1 never wrote
    fed = [1, 2, 3, 4, 5, 6, 7, 8]
    w0 = tr.window(ring, fed, 1020, 0, 1024)
    assert len(w0) == 1021 and w0[:1020] == list(range(1000, 2020)) and w0[-1] == 1
    w7 = tr.window(ring, fed, 1020, 7, 1024)                             # positions 4 .. 1027: slots 4 .. 1019, then the segment's 8 ids
    assert len(w7) == 1024 and w7[:1016] == list(range(1004, 2020)) and w7[1016:] == fed
    w5 = tr.window(ring, fed, 1020, 5, 1024)                             # positions 2 .. 1025: slot 0 / 1 (positions 1024 / 1025) are fed[4] / fed[5], not the ring's
    assert w5[:1018] == list(range(1002, 2020)) and w5[1018:] == fed[:6]


def test_accept_per_segment():
    toks = [4, 10, 11, 12, 13, 20, 21, 30]
    seg_first = [0, 1, 5, 7, 7, 8]
    drafts = [[-1] * 7, [10, 11, 99, 13, 0, 0, 0], [20, 0, 0, 0, 0, 0, 0], [1] * 7, [V, 0, 0, 0, 0, 0, 0]]
    assert tr.accept_rows(toks, seg_first, drafts, V) == [(1, [4]), (3, [10, 11, 12]), (2, [20, 21]), (0, []), (1, [30])]
    assert tr.accept_rows([3, V + 3], [0, 2], [[3]], V) == [(2, [3, V + 3])]    # a ROW's token is whatever it is; only drafts are range-checked
    assert tr.accept_rows([3, 5], [0, 2], [[V + 3]], V) == [(1, [3])] and tr.accept_rows([3, 5], [0, 2], [[-1]], V) == [(1, [3])]
    assert [n for n, _ in tr.accept_rows(toks, seg_first, drafts, V)] == [n for n, _ in sb.accept_segments(toks, seg_first, drafts)]


def test_commit_moves_calls_and_exactly_n_ring_slots():
    rings = np.full((3, tr.RING), -7)
    fed = [5, 6, 7, 8, 9, 1, 2]                                          # segments of 4, 1 and 2 rows
    got, calls = tr.commit(rings, [10, 20, 30], [True, False, True], fed, [0, 4, 5, 7], [1022, 0, 7], [3, 1, 2])
    assert calls == [13, 20, 32]                                         # a greedy seat's record is not written
    want = np.full((3, tr.RING), -7)
    want[0, [1022, 1023, 0]] = [5, 6, 7]                                 # positions 1022, 1023, 1024: the third wraps
    want[1, 0] = 9
    want[2, [7, 8]] = [1, 2]
    assert np.array_equal(got, want) and (rings == -7).all()             # the input is left unchanged
    got, calls = tr.commit(rings, [1], [True], [3], [0, 0], [5], [0])    # an idle slot
    assert calls == [1] and (got == -7).all()


# ------------------------------------------------------------------ the engine on a stub that keeps the seats' device state
class TailSpecStub(SpecStub):
    def __init__(self, next_token=cyclic):
        super().__init__(next_token)
        self.args = types.SimpleNamespace(vocab_size=V)
        self.prompts = []
        self.armed = False
        self.table, self.rings = {}, {}     # seat -> [draws, calls, penalised]; seat -> the ids the ring has been given, by position
        self.tail_writes = []               # the rows of every write_batch_tail that wrote any
        self.bias_rows = {}

    # ---- the per-row state the engine arms
    def set_batch_tail(self, rows_cap):
        self.armed, self.table, self.rings = True, {}, {}

    def clear_batch_tail(self):
        self.armed = False

    def write_batch_tail(self, rows, records, fed=None):
        assert self.armed
        if rows:
            self.tail_writes.append(list(rows))
        for i, (s, rec) in enumerate(zip(rows, records)):
            self.table[s] = [rec.mode != -1, int(rec.calls), rec.penalty != 1.0]
            if fed is not None and fed[i] is not None:
                self.rings[s] = [int(t) for t in fed[i]]

    def set_batch_edits(self, rows_cap, masks=True, bias_cap=0):
        assert not masks and bias_cap >= 1

    def write_batch_edits(self, rows, masks=None, biases=None):
        assert masks is None
        self.bias_rows.update(zip(rows, biases))

    def clear_batch_edits(self):
        pass

    def set_batch_xtc(self, rows_cap):
        pass

    def write_batch_xtc(self, rows, records):
        pass

    def clear_batch_xtc(self):
        pass

    # ---- what every pass checks of a decode seat, and how it moves the seat
    def _seat_is_whole(self, s, cache, token):
        seq = cache[0].page_manager
        hist = self._hist(seq)
        mine = [p for p in self.prompts if (hist + [token])[:len(p)] == p]
        assert len(mine) == 1
        draws, calls, penalised = self.table[s]
        assert draws, "seat %d holds a greedy record" % s
        assert calls == len(hist) + 1 - len(mine[0]), "seat %d: stream position %d, but its request has drawn %d tokens" % (s, calls, len(hist) + 1 - len(mine[0]))
        if penalised:
            assert self.rings[s] == hist, "seat %d's ring is not what its request has been fed" % s

    def _rows_drew(self, decode_ids, n_prompts=0):
        """Behind a plain pass: every output row that draws moves its stream by one; a decode row's ring takes the row's input (a prompt
        row's seat was written with its whole prompt when it was seated, the prompt pass's own input included)."""
        for s in range(len(decode_ids) + n_prompts):
            if s in self.table:
                self.table[s][1] += int(self.table[s][0])
            if s < len(decode_ids) and self.rings.get(s) is not None:
                self.rings[s] = self.rings[s] + [decode_ids[s]]

    def step_batch(self, tokens, caches):
        if self.armed:
            for s, (c, t) in enumerate(zip(caches, tokens.tolist())):
                self._seat_is_whole(s, c, t)
        out = super().step_batch(tokens, caches)
        if self.armed:
            self._rows_drew(tokens.tolist())
        return out

    def prefill_batch(self, prompts, caches):
        out = super().prefill_batch(prompts, caches)
        if self.armed:
            self._rows_drew([], len(prompts))
        return out

    def step_mixed(self, tokens, decode_caches, prompts, prompt_caches):
        toks = tokens.tolist() if decode_caches else []
        if self.armed:
            for s, (c, t) in enumerate(zip(decode_caches, toks)):
                self._seat_is_whole(s, c, t)
        out = super().step_mixed(tokens, decode_caches, prompts, prompt_caches)
        if self.armed:
            self._rows_drew(toks, len(prompts))
        return out

    def spec_step_batch_tail(self, tokens, caches, drafts, counts, seq_ids=None, seq_len=None, then_draft=None):
        assert self.armed, "spec_step_batch_tail needs set_batch_tail armed"
        toks_in = tokens.tolist()
        for s, (c, t) in enumerate(zip(caches, toks_in)):
            self._seat_is_whole(s, c, t)
        n, toks, nxt = SpecStub.spec_step_batch(self, tokens, caches, drafts, counts, seq_ids, seq_len, then_draft)
        self.calls["spec_step_batch"] -= 1
        self.calls["spec_step_batch_tail"] += 1
        for s in range(len(caches)):                                     # the commit launch: calls by n, the ring by the n ids fed for good
            self.table[s][1] += n[s]
            if self.rings.get(s) is not None:
                self.rings[s] = self.rings[s] + [toks_in[s]] + toks[s][:n[s] - 1]
        return n, toks, nxt


def sampled(i):
    return SamplingParams(temp=0.8, top_p=0.9, seed=100 + i, repetition_penalty=1.1 if i % 2 == 0 else 1.0, logit_bias={3: 0.5} if i % 3 == 0 else None)


def run_tail(prompts, new, sampling, **kw):
    model = TailSpecStub()
    model.prompts = [list(p) for p in prompts]
    assert not any(a != b and a[:len(b)] == b for a in model.prompts for b in model.prompts)
    eng = BatchedEngine(model, speculative=SP, num_pages=64, **kw)
    out = eng.generate(prompts, new, sampling=sampling)
    assert eng.pool.get_num_free_pages() == eng.pool.size()
    return out, eng, model


@pytest.mark.parametrize("kw", [dict(max_batch=8), dict(max_batch=2), dict(max_batch=3), dict(max_batch=4, mixed=False), dict(max_batch=4, prefill_chunk=8)])
@pytest.mark.parametrize("seed", [1, 2, 11])
def test_seats_stay_whole_through_passes_steps_and_prompt_rows(kw, seed):
    """Requests retire and are replaced mid-generation (seats change occupants), passes carry prompt rows beside decode rows, and plain
    steps run between speculative passes: before every pass every decode seat holds its occupant's stream position and fed ids."""
    prompts = repeating(seed, 6)
    new = 40
    got, eng, model = run_tail(prompts, new, [sampled(i) for i in range(len(prompts))], **kw)
    assert got == [alone(cyclic, p, new) for p in prompts]
    assert model.calls["spec_step_batch_tail"] == eng.spec_stats["passes"] >= 1 and model.calls["spec_step_batch"] == 0
    assert eng.spec_stats["steps"] >= 1 and eng.spec_stats["accepted"] > 0
    assert any(n_ > 1 for _, n in model.passes for n_ in n)             # some pass moved a seat by more than one
    if kw["max_batch"] < len(prompts) and kw.get("mixed", True):
        assert model.calls["step_mixed"] >= 1                             # passes that carried prompt rows beside the seats
    want, schedule = sb.simulate_batch(prompts, cyclic, new, kw["max_batch"], (), SP.num_draft, SP.ngram_max, SP.ngram_min, SP.min_draft)
    if "prefill_chunk" not in kw and kw.get("mixed", True):
        assert want == got and eng.spec_stats == sb.stats_of(schedule)    # the schedule is the greedy engine's: the tail changes no pass's shape


def test_a_kept_seat_is_not_rewritten():
    prompts = [[1, 2, 3, 0] * 4]
    got, eng, model = run_tail(prompts, 40, sampled(0), max_batch=1)
    assert got == [alone(cyclic, prompts[0], 40)] and eng.spec_stats["passes"] >= 2 and eng.spec_stats["accepted"] > 0
    assert model.tail_writes == [[0], [0]]                                # arming, then the request's one seating: the passes moved the seat themselves


def test_row_seats_moved():
    seats = _RowSeats(None, 4, [[1], [2], [3]], tails=([SamplingParams()] * 3, [0] * 3))
    seats.slots = [(0, 3), None, (2, 9)]
    seats.moved([4, 1, 1])
    assert seats.slots == [(0, 7), None, (2, 10)]


def test_the_tail_entry_is_chosen_exactly_when_sampling_is_given():
    prompts = repeating(1, 3)
    for sampling, tail in ((None, False), (SamplingParams(), True), ([SamplingParams(), SamplingParams(temp=1.0, top_k=1), SamplingParams(), SamplingParams()], True),
                           (SamplingParams(logit_bias={1: 0.25}), True)):
        model = TailSpecStub()
        model.prompts = [list(p) for p in prompts]
        checked = model._seat_is_whole
        model._seat_is_whole = lambda s, c, t: None if not model.table[s][0] else checked(s, c, t)   # (greedy seats hold no stream)
        eng = BatchedEngine(model, speculative=SP, num_pages=64, max_batch=4)
        assert eng.generate(prompts, 30, sampling=sampling) == [alone(cyclic, p, 30) for p in prompts]
        assert eng.spec_stats["passes"] >= 1
        assert (model.calls["spec_step_batch_tail"], model.calls["spec_step_batch"]) == ((eng.spec_stats["passes"], 0) if tail else (0, eng.spec_stats["passes"]))
        assert model.armed is False                                       # cleared on the way out


def test_refusals_by_name():
    eng = BatchedEngine(TailSpecStub(), num_pages=16, max_batch=2, speculative=SP)
    prompts = [[1, 2, 3], [4, 5]]
    from proxy_inference_engine_amd.logits_processors import TokenAutomaton
    auto = object.__new__(TokenAutomaton)
    for gen, name in ((dict(sampling=SamplingParams(token_mask=[1, 2])), "a token mask"), (dict(sampling=SamplingParams(token_automaton=auto)), "a token automaton"),
                      (dict(sampling=[SamplingParams(), SamplingParams(frequency_penalty=0.5)]), "frequency / presence"),
                      (dict(sampling=SamplingParams(presence_penalty=0.5)), "frequency / presence"), (dict(sampling=SamplingParams(dry_multiplier=0.8)), "DRY"),
                      (dict(logprobs=True), "`logprobs`"), (dict(top_logprobs=2), "`top_logprobs`"), (dict(prompt_logprobs=0), "`prompt_logprobs`")):
        with pytest.raises(ValueError, match=name):
            eng.generate(prompts, 4, **gen)
    assert eng.model.calls["spec_step_batch_tail"] == 0 and eng.model.tail_writes == []       # nothing was armed, nothing ran
    for kw, name in ((dict(configured_tail=True), "configured_tail"), (dict(grammar=True), "grammar"), (dict(num_draft=8, min_draft=5), "num_draft > 7")):
        with pytest.raises(ValueError, match=name):
            BatchedEngine(TailSpecStub(), speculative=SpeculativeParams(batch_tail=True, **kw))
    with pytest.raises(ValueError, match="batch_tail is a bool"):
        SpeculativeParams(batch_tail=1)


def test_inference_engine_refuses_batch_tail_by_name():
    from proxy_inference_engine_amd.engine import inference_engine as ie
    with pytest.raises(ValueError, match="batch_tail"):
        ie._check_generate_args(None, None, None, None, None, None, None, None, SP)
    ie._check_generate_args(None, None, None, None, None, None, None, None, SpeculativeParams())   # without it: as before


def test_without_batch_tail_nothing_new_is_admitted():
    eng = BatchedEngine(TailSpecStub(), num_pages=16, max_batch=2, speculative=SpeculativeParams(num_draft=7, min_draft=5))
    prompts = [[1, 2, 3], [4, 5]]
    for sampling in (SamplingParams(temp=0.7), SamplingParams(top_k=4, temp=1.0), SamplingParams(repetition_penalty=1.1), SamplingParams(logit_bias={1: 1.0}),
                     SamplingParams(temp=1.0, xtc_probability=0.5, xtc_threshold=0.1), [SamplingParams(), SamplingParams(seed=3, temp=0.5)]):
        with pytest.raises(ValueError, match="batched speculation is greedy and raw -- not available with a request whose `sampling` is not plain"):
            eng.generate(prompts, 4, sampling=sampling)
    assert eng.generate(prompts, 4, sampling=SamplingParams()) == [alone(cyclic, p, 4) for p in prompts]
    assert eng.model.calls["spec_step_batch_tail"] == 0
