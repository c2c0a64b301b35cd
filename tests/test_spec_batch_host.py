"""Batched speculation's host logic on the CPU: the rules of tests/spec_batch_reference.py against the engine's own helpers,
and BatchedEngine(speculative=...) on a stub model whose next token is a fixed function of the sequence -- so what a request generates can
never depend on HOW its tokens were verified.  The stub keeps the real page pool, checks on every speculative pass that the seat's ids on
the "device" are the sequence it holds, and drafts with speculative_reference.ngram_draft."""
from unittest import mock

import numpy as np
import pytest
import torch

from proxy_inference_engine_amd.engine import batch_engine
from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine, SamplingParams
from proxy_inference_engine_amd.engine.inference_engine import SpeculativeParams
from tests import spec_batch_reference as sb
from tests import speculative_reference as ref
from tests.test_batch_engine_host import StubModel

PERIOD = 17


def cyclic(hist) -> int:
    """A model that settles into short cycles -- the next token is a function of the last two -- and leaves them at every PERIOD-th
    length, where no look-up can know the token: drafts are right for a while, then wrong at a place the period decides."""
    L = len(hist)
    if L % PERIOD == 0:
        return 5 + (L // PERIOD) % 3
    return (3 * int(hist[-1]) + (int(hist[-2]) if L > 1 else 0) + 1) % 5


def alone(next_token, prompt, max_new, stop=()):
    hist, out = list(prompt), []
    for _ in range(max_new):
        out.append(next_token(hist))
        if out[-1] in stop:
            break
        hist.append(out[-1])
    return out


class SpecStub(StubModel):
    def __init__(self, next_token=cyclic):
        super().__init__()
        self.next_token = next_token
        self.passes = []          # (m, n) of every speculative pass

    def _feed(self, cache, ids):
        seq = cache[0].page_manager
        hist = self._hist(seq) if seq.offset else seq.__dict__.setdefault("_hist", [])
        seq.reserve(len(ids))
        hist.extend(int(t) for t in ids)
        seq.advance(len(ids))
        self.by_first_page.setdefault(seq.pages[0], hist)
        return self.next_token(hist)

    def draft_rows(self, seq_ids, seq_len, ngram_max, ngram_min, k, out):
        for s in range(seq_ids.shape[0]):
            d = ref.ngram_draft(seq_ids[s, :int(seq_len[s])].tolist(), ngram_max, ngram_min, k)
            out[1][s] = len(d)
            if d:
                out[0][s, :k] = torch.tensor(d, dtype=torch.int32)
        return out

    def spec_step_batch(self, tokens, caches, drafts, counts, seq_ids=None, seq_len=None, then_draft=None):
        self.calls["spec_step_batch"] += 1
        B = len(caches)
        assert tokens.numel() == B == len(counts) and len({id(c[0].page_manager) for c in caches}) == B
        assert all(0 <= m <= 7 for m in counts) and B + sum(counts) <= 256 and any(counts)
        n, toks = [], []
        for s, (c, t, m) in enumerate(zip(caches, tokens.tolist(), counts)):
            seq = c[0].page_manager
            # the seat holds this very sequence, the fed token last
            assert seq_ids[s, :int(seq_len[s])].tolist() == self._hist(seq) + [t], "seat %d holds another sequence's ids" % s
            seq.reserve(1 + m)                                          # the pass writes every row; the pages stay with the sequence
            greedy = [self._feed(c, [t])]
            for i in range(m):
                if int(drafts[s, i]) != greedy[-1]:
                    break
                greedy.append(self._feed(c, [int(drafts[s, i])]))
            L = int(seq_len[s])
            seq_ids[s, L:L + len(greedy)] = torch.tensor(greedy, dtype=torch.int32)
            seq_len[s] = L + len(greedy)
            n.append(len(greedy)), toks.append(greedy)
        self.passes.append((list(counts), n))
        nxt = None
        if then_draft is not None:
            ngram_max, ngram_min, k, drafts_out = then_draft
            cnt = torch.zeros(B, dtype=torch.int32)
            self.draft_rows(seq_ids[:B], seq_len[:B], ngram_max, ngram_min, k, out=(drafts_out[:B], cnt))
            nxt = cnt.tolist()
        return n, toks, nxt


def repeating(seed, n):
    """n prompts that repeat a short base of the cyclic model's alphabet a few times, plus one that repeats nothing."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        base = rng.integers(0, 5, int(rng.integers(2, 6))).tolist()
        out.append(base * int(rng.integers(2, 5)) + rng.integers(0, 5, int(rng.integers(0, 3))).tolist())
    return out + [list(range(100, 100 + int(rng.integers(3, 9))))]


def run_engine(prompts, new, sp, next_token=cyclic, **kw):
    model = SpecStub(next_token)
    eng = BatchedEngine(model, speculative=sp, **kw)
    out = eng.generate(prompts, new)
    assert eng.pool.get_num_free_pages() == eng.pool.size()             # every page came back, the rejected rows' included
    return out, eng, model


# ------------------------------------------------------------------ the rules
def test_form_rows_is_what_the_model_uploads():
    seg_first, row_seq, row_ctx = sb.form_rows([5, 60, 252], [0, 3, 7])
    assert seg_first == [0, 1, 5, 13]
    assert row_seq == [0] + [1] * 4 + [2] * 8
    assert row_ctx == [6] + [61, 62, 63, 64] + list(range(253, 261))
    assert sb.form_rows([9], [0]) == ([0, 1], [0], [10])


@pytest.mark.parametrize("counts,room,min_draft,want", [
    ([7, 4, 5, 0], [50, 50, 50, 50], 5, [7, 0, 5, 0]),                  # below min_draft: no drafts
    ([7, 7, 7], [50, 3, 0], 5, [7, 3, 0]),                              # never past len(prompt) + max_new_tokens
    ([9, 31], [50, 50], 1, [7, 7]),                                     # at most 7
    ([7] * 40, [50] * 40, 5, [5] * 24 + [6] * 16),                      # 40 + 280 rows -> 256: the largest first, the lowest row among equals
    ([7] * 33 + [0], [50] * 34, 5, [6] * 9 + [7] * 24 + [0]),
])
def test_clamps(counts, room, min_draft, want):
    assert sb.clamp_drafts(counts, room, min_draft) == want
    assert batch_engine.spec_plan(counts, room, min_draft) == want
    assert len(want) + sum(want) <= 256


def test_acceptance_per_segment_and_the_cut():
    greedy = [4, 10, 11, 12, 13, 20, 21]                                # rows 0 | 1-4 | 5-6, and an idle slot
    drafts = [[-1] * 7, [10, 11, 99, 13, 0, 0, 0], [20, 0, 0, 0, 0, 0, 0], [1] * 7]
    assert sb.accept_segments(greedy, [0, 1, 5, 7, 7], drafts) == [(1, [4]), (3, [10, 11, 12]), (2, [20, 21]), (0, [])]
    for gen, run, stop, new, want in (([1], [2, 3, 4], {9}, 10, ([1, 2, 3, 4], False)), ([1], [2, 9, 4], {9}, 10, ([1, 2, 9], True)),
                                      ([1, 2], [3, 4, 5], {9}, 4, ([1, 2, 3, 4], True)), ([1, 2, 3], [9], {9}, 4, ([1, 2, 3, 9], True))):
        assert sb.cut_run(gen, run, stop, new) == want
        mine = list(gen)
        assert batch_engine.cut_run(mine, run, stop, new) == want[1] and mine == want[0]


# ------------------------------------------------------------------ the engine on the stub
SP = SpeculativeParams(num_draft=7, ngram_max=3, ngram_min=1, min_draft=5)


@pytest.mark.parametrize("kw", [dict(max_batch=8), dict(max_batch=2), dict(max_batch=3, share_prefix=True), dict(max_batch=4, mixed=False),
                                dict(max_batch=4, prefill_chunk=8)])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_speculation_changes_no_token(kw, seed):
    prompts = repeating(seed, 5)
    if kw.get("share_prefix"):
        prompts = [list(range(30, 30 + 70)) + p for p in prompts]     # more than a page in common
    new = 40
    want = [alone(cyclic, p, new) for p in prompts]
    plain = BatchedEngine(SpecStub(), num_pages=64, **kw).generate(prompts, new)
    got, eng, model = run_engine(prompts, new, SP, num_pages=64, **kw)
    assert got == plain == want
    assert model.calls["spec_step_batch"] == eng.spec_stats["passes"] >= 1
    assert eng.spec_stats["drafted"] == sum(sum(m) for m, _ in model.passes)
    assert eng.spec_stats["accepted"] == sum(sum(n) - len(n) for _, n in model.passes)


@pytest.mark.parametrize("max_batch", [2, 3, 8])
def test_the_schedule_is_the_simulated_one(max_batch):
    """Drafts that are right, wrong at position 0 and wrong in the middle; rows with and without drafts in one pass; iterations without
    any; requests that retire and are replaced mid-generation, so that seats change; max_batch below the number of prompts."""
    prompts = repeating(11, 6)
    new = [30, 48][max_batch > 2]
    want, schedule = sb.simulate_batch(prompts, cyclic, new, max_batch, (), SP.num_draft, SP.ngram_max, SP.ngram_min, SP.min_draft)
    assert want == [alone(cyclic, p, new) for p in prompts]
    passes = [e for e in schedule if e[0] == "pass"]
    rows = [(m, n) for e in passes for m, n in zip(e[2], e[3])]
    assert any(m and n == m + 1 for m, n in rows) and any(m and n == 1 for m, n in rows) and any(m and 1 < n < m + 1 for m, n in rows)
    assert any(0 in e[2] and max(e[2]) > 0 for e in passes) and any(e[0] == "step" for e in schedule)
    got, eng, model = run_engine(prompts, new, SP, num_pages=64, max_batch=max_batch)
    assert got == want
    assert model.passes == [(e[2], e[3]) for e in passes]
    assert eng.spec_stats == sb.stats_of(schedule)


def test_a_run_is_cut_at_a_stop_token_and_at_max_new_tokens():
    cuts = []
    real = batch_engine.cut_run

    def logged(generated, tokens, stop_tokens, max_new_tokens):
        before = len(generated)
        ended = real(generated, tokens, stop_tokens, max_new_tokens)
        if len(generated) - before < len(tokens):
            cuts.append("stop" if generated[-1] in stop_tokens else "length")
        return ended

    def copy5(hist):                                                    # a model that repeats with period 5: every draft is right
        return int(hist[-5])

    for model, prompts, stop, new in ((cyclic, repeating(5, 4), (2,), 40), (cyclic, repeating(5, 4), (), 23),
                                      (copy5, [[1, 2, 3, 9, 4] * 3, [5, 6, 7, 8, 0] * 2, [3, 9, 4, 1, 2] * 4], (9,), 30)):
        want = [alone(model, p, new, stop) for p in prompts]
        with mock.patch.object(batch_engine, "cut_run", logged):
            got, eng, _ = run_engine(prompts, new, SP, model, num_pages=64, max_batch=3, stop_tokens=stop)
        assert got == want
        sim, schedule = sb.simulate_batch(prompts, model, new, 3, stop, SP.num_draft, SP.ngram_max, SP.ngram_min, SP.min_draft)
        assert sim == want and eng.spec_stats == sb.stats_of(schedule)
    assert "stop" in cuts and "length" in cuts                          # tokens behind either cut were dropped somewhere


def test_a_wrong_model_of_the_drafts_still_generates_the_same_tokens():
    """The hash model of tests/test_batch_engine_host.py: nearly every draft is wrong at position 0."""
    from tests.test_batch_engine_host import next_token
    prompts = [[1, 2, 3] * 6, [4, 5] * 9 + [4], [9, 8, 7, 6] * 4]
    got, eng, model = run_engine(prompts, 25, SpeculativeParams(num_draft=4, min_draft=2), next_token, num_pages=32, max_batch=3)
    assert got == [alone(next_token, p, 25) for p in prompts]
    assert eng.spec_stats["passes"] >= 1 and eng.spec_stats["accepted"] <= eng.spec_stats["drafted"] // 2


def test_without_speculative_nothing_of_it_runs():
    model = SpecStub()
    eng = BatchedEngine(model, num_pages=64, max_batch=3)
    prompts = repeating(1, 3)
    assert eng.generate(prompts, 20) == [alone(cyclic, p, 20) for p in prompts]
    assert model.calls["spec_step_batch"] == 0 and eng.spec_stats == {"passes": 0, "steps": 0, "drafted": 0, "accepted": 0}


# ------------------------------------------------------------------ refusals, by name
def test_refusals_by_name():
    class Tp(SpecStub):
        tp = object()

    for kw, name in ((dict(sampler=lambda lp: lp.argmax(dim=-1)), "sampler"), (dict(kv_dtype=torch.int8), "int8"),
                     (dict(speculative=SpeculativeParams(num_draft=8, min_draft=5)), "num_draft > 7"),
                     (dict(speculative=SpeculativeParams(draft_model=StubModelWithSteps())), "draft_model"),
                     (dict(speculative=SpeculativeParams(grammar=True)), "grammar"),
                     (dict(speculative=SpeculativeParams(configured_tail=True)), "configured_tail")):
        with pytest.raises(ValueError, match=name):
            BatchedEngine(SpecStub(), **{"speculative": SP, **kw})
    with pytest.raises(ValueError, match="tensor-parallel"):
        BatchedEngine(Tp(), speculative=SP)
    eng = BatchedEngine(SpecStub(), num_pages=16, max_batch=2, speculative=SP)
    prompts = [[1, 2, 3], [4, 5]]
    for gen, name in ((dict(sampling=SamplingParams(temp=0.7)), "not plain"), (dict(sampling=[SamplingParams(), SamplingParams(repetition_penalty=1.1)]), "not plain"),
                      (dict(sampling=SamplingParams(logit_bias={1: 1.0})), "not plain"), (dict(logprobs=True), "`logprobs`"),
                      (dict(top_logprobs=2), "`top_logprobs`"), (dict(prompt_logprobs=0), "`prompt_logprobs`")):
        with pytest.raises(ValueError, match=name):
            eng.generate(prompts, 4, **gen)
    assert eng.generate(prompts, 4, sampling=SamplingParams()) == [alone(cyclic, p, 4) for p in prompts]   # a plain SamplingParams is admitted


class StubModelWithSteps(SpecStub):
    """What SpeculativeParams takes for a built draft model."""
    history = logprobs = None

    def set_step_tail(self, **kw):
        pass
