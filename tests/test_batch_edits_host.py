"""Per-request token masks and logit biases without a device: SamplingParams' two fields and their validation, and
BatchedEngine's bookkeeping of whose mask and bias table sits in which row of a pass -- on the stub model of
tests/test_batch_engine_host.py, extended by the edits' surface: every pass checks each output row's words and table against the request
that sits in the row and against what that request has been fed."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from proxy_inference_engine_amd.engine import BatchedEngine, SamplingParams
from proxy_inference_engine_amd.hip_ops import pack_token_mask
from proxy_inference_engine_amd.logits_processors import packed_token_mask
from tests.test_batch_engine_host import StubModel, V, requests


# ------------------------------------------------------------------ SamplingParams
def test_defaults_change_nothing():
    sp = SamplingParams()
    assert sp.token_mask is None and sp.logit_bias is None and sp.plain and sp.tailless
    assert sp.edits(V) == (None, None)


def test_plain_with_the_new_fields():
    mask = torch.ones(V, dtype=torch.bool)
    assert not SamplingParams(token_mask=mask).plain and SamplingParams(token_mask=mask).tailless
    assert not SamplingParams(logit_bias={3: 1.0}).plain and SamplingParams(logit_bias={3: 1.0}).tailless
    assert not SamplingParams(token_mask=lambda toks: [1]).plain
    assert not SamplingParams(temp=0.7, logit_bias={3: 1.0}).tailless
    assert SamplingParams(token_mask=mask).record().mode == -1            # the record knows nothing of the edits: pie_row_tail is unchanged


def test_edits_come_out_as_the_processors_carry_them():
    words = pack_token_mask([1, 5, 40], V)
    proc, bias = SamplingParams(token_mask=words, logit_bias={7: 0.5, 9: -2.0}).edits(V)
    assert torch.equal(proc.mask, words) and proc.mask_fn is None and bias == ((7, 9), (0.5, -2.0))
    fn = lambda toks: [len(toks) % V]
    proc, bias = SamplingParams(token_mask=fn).edits(V)
    assert proc.mask is None and proc.mask_fn is fn and bias is None
    proc, _ = SamplingParams(token_mask=torch.arange(V) % 3 == 0).edits(V)
    assert torch.equal(proc.mask, pack_token_mask(torch.arange(V) % 3 == 0, V))


@pytest.mark.parametrize("kw", [
    dict(logit_bias={}), dict(logit_bias={i: 0.1 for i in range(1025)}),                  # 1..1024 entries
    dict(logit_bias={3: float("inf")}), dict(logit_bias={3: float("nan")}),               # finite values
    dict(logit_bias={-1: 1.0}), dict(logit_bias={2 ** 31: 1.0}),                          # int32 ids
    dict(logit_bias={3: 1.0, "3": 2.0}),                                                  # no duplicate ids
    dict(token_mask=torch.ones(V - 3, dtype=torch.bool)),                                 # a bool mask of another vocabulary's length
    dict(token_mask=torch.zeros(V, dtype=torch.bool)),                                    # nothing allowed
    dict(token_mask=torch.zeros((V + 31) // 32, dtype=torch.int32)),
    dict(token_mask=torch.ones(2, dtype=torch.int32)),                                    # too few packed words
    dict(token_mask=[1, 2, 3]), dict(token_mask=torch.ones(V)),                           # neither words, a bool mask nor a callable
])
def test_bad_edits_are_refused_before_anything_runs(kw):
    with pytest.raises(ValueError):
        SamplingParams(**kw).edits(V)
    model = EditStub([[1, 2, 3]], [SamplingParams(**kw)], 0)
    eng = BatchedEngine(model, num_pages=8, max_batch=2)
    with pytest.raises(ValueError):
        eng.generate([[1, 2, 3]], 4, sampling=SamplingParams(**kw))
    assert not model.calls and model.sets == 0                                           # no pass ran, nothing was armed


# ------------------------------------------------------------------ the engine's bookkeeping
class EditStub(StubModel):
    """StubModel + the batch edits' surface.  Every pass checks each output row's mask words and bias table against the request that sits in
    the row: a static mask's words, a callable's words for exactly the ids the row has been fed (this pass's included), the request's bias
    table, and nothing armed for a prompt still filling or the shared prefix's own pass."""

    def __init__(self, prompts, params, mark, tail=False):
        super().__init__()
        self.args = SimpleNamespace(vocab_size=V)
        self.prompts, self.params, self.mark = prompts, params, mark
        self.W = (V + 31) // 32
        self.be = None
        self.sets = self.checked = self.mask_rows = self.bias_rows = 0
        self.tail_armed, self.has_tail = False, tail

    # ---- the batch tail's surface, as far as the engine touches it
    def set_batch_tail(self, rows_cap):
        assert self.has_tail
        self.tail_armed = True

    def write_batch_tail(self, rows, records, fed=None):
        assert self.tail_armed

    def clear_batch_tail(self):
        self.tail_armed = False

    # ---- the batch edits' surface
    def set_batch_edits(self, rows_cap, masks=True, bias_cap=0):
        assert rows_cap >= 1 and (masks or bias_cap) and 0 <= bias_cap <= 1024
        self.sets += 1
        rng = np.random.default_rng(5)
        self.be = {"masks": rng.integers(-2 ** 31, 2 ** 31, (rows_cap, self.W)).astype(np.int32) if masks else None,   # stale rows of an earlier use
                   "mask_on": np.ones(rows_cap, np.int32) if masks else None,
                   "bias": [((1,), (9.0,))] * rows_cap if bias_cap else None, "cap": bias_cap}

    def write_batch_edits(self, rows, masks=None, biases=None):
        assert self.be is not None and rows and len(set(rows)) == len(rows)
        if masks is not None:
            assert self.be["masks"] is not None and len(masks) == len(rows)
            for r, m in zip(rows, masks):
                self.be["mask_on"][r] = int(m is not None)
                if m is not None:
                    self.be["masks"][r] = packed_token_mask(m, V).numpy()
                    self.mask_rows += 1
        if biases is not None:
            assert self.be["bias"] is not None and len(biases) == len(rows)
            for r, b in zip(rows, biases):
                assert b is None or 1 <= len(b[0]) == len(b[1]) <= self.be["cap"]
                self.be["bias"][r] = b
                self.bias_rows += b is not None

    def clear_batch_edits(self):
        self.be = None

    def _row(self, s, cache, ids):
        if self.be is None:
            return
        seq = cache[0].page_manager
        hist = (list(self._hist(seq)) if seq.offset else []) + [int(t) for t in ids]
        on = 0 if self.be["masks"] is None else int(self.be["mask_on"][s])
        bias = None if self.be["bias"] is None else self.be["bias"][s]
        r = hist[self.mark] if len(hist) > self.mark else None            # the request: its index is the id behind the shared prefix
        if r is None or len(hist) < len(self.prompts[r]):                  # the shared prefix's own pass, a prompt still filling: disarmed
            assert on == 0 and bias is None, s
            return
        sp = self.params[r]
        assert hist[:len(self.prompts[r])] == self.prompts[r]
        proc, want_bias = sp.edits(V)
        assert bias == want_bias, (s, r)
        if proc is None:
            assert on == 0, (s, r)
        else:
            want = proc.mask if proc.mask_fn is None else packed_token_mask(proc.mask_fn(hist), V)
            assert on == 1 and np.array_equal(self.be["masks"][s], packed_token_mask(want, V).numpy()), (s, r, len(hist))
        self.checked += 1

    def step_batch(self, tokens, caches):
        for s, (c, t) in enumerate(zip(caches, tokens.tolist())):
            self._row(s, c, [t])
        return super().step_batch(tokens, caches)

    def prefill_batch(self, prompts, caches):
        for s, (c, p) in enumerate(zip(caches, prompts)):
            self._row(s, c, p)
        return super().prefill_batch(prompts, caches)

    def step_mixed(self, tokens, decode_caches, prompts, prompt_caches):
        for s, (c, t) in enumerate(zip(decode_caches, tokens.tolist() if decode_caches else [])):
            self._row(s, c, [t])
        for j, (c, p) in enumerate(zip(prompt_caches, prompts)):
            self._row(len(decode_caches) + j, c, p)
        return super().step_mixed(tokens, decode_caches, prompts, prompt_caches)


def grammar(tokens):
    """Depends on everything the request was fed: its length and its last id."""
    grammar.args.append(list(tokens))
    return [(int(tokens[-1]) + 1) % V, (len(tokens) * 7) % V]


grammar.args = []


def mixed_params(n, tail):
    kinds = [SamplingParams(token_mask=torch.arange(V) % 3 == 0), SamplingParams(token_mask=grammar), SamplingParams(logit_bias={11: 100.0}),
             SamplingParams(), SamplingParams(token_mask=pack_token_mask(range(5, 60), V), logit_bias={i: -1.0 for i in range(40)},
                                              **(dict(temp=0.8, top_k=5, seed=4) if tail else {}))]
    return [kinds[i % len(kinds)] for i in range(n)]


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("kw", [dict(), dict(mixed=False), dict(batch_prefill=False), dict(prefill_chunk=16), dict(prefill_chunk=4), dict(kv_dtype=torch.int8),
                                dict(share_prefix=True)])
@pytest.mark.parametrize("slots,pages", [(1, 8), (3, 16), (4, 30)])
def test_engine_seats_every_requests_edits_in_its_row(kw, slots, pages, tail):
    prefix = list(range(100, 100 + 70)) if kw.get("share_prefix") else []
    prompts = [prefix + [i] + p for i, p in enumerate(requests(5, 9, lo=1, hi=90))]     # a distinct id behind the prefix: requests are told apart
    params = mixed_params(len(prompts), tail)
    model = EditStub(prompts, params, len(prefix), tail)
    grammar.args.clear()
    eng = BatchedEngine(model, num_pages=pages + 2, max_batch=slots, stop_tokens={3, 77}, **kw)
    out = eng.generate(prompts, 7, sampling=params)
    assert model.be is None and not model.tail_armed and model.sets == 1                 # armed once, cleared on the way out
    assert model.checked >= sum(len(o) for i, o in enumerate(out) if not params[i].plain)   # every token of an edited request came from a checked row
    plain = BatchedEngine(StubModel(), num_pages=pages + 2, max_batch=slots, stop_tokens={3, 77}, **kw).generate(prompts, 7)
    assert out == plain                                                                   # (the stub's tokens do not depend on the edits)
    # the callable received, for every token of its requests, the prompt plus everything generated before that token -- and nothing else
    want = [prompts[i] + out[i][:j] for i in range(len(prompts)) if params[i].token_mask is grammar for j in range(len(out[i]))]
    assert sorted(map(tuple, set(map(tuple, grammar.args)))) == sorted(map(tuple, want))


def test_rows_are_rewritten_only_when_their_occupant_changes():
    prompts = [[0, 5, 9], [1, 8, 2, 4]]
    params = [SamplingParams(token_mask=torch.arange(V) % 2 == 0, logit_bias={4: 2.0}), SamplingParams(logit_bias={6: -3.0, 8: 1.0})]
    model = EditStub(prompts, params, 0)
    writes = []
    inner = model.write_batch_edits
    model.write_batch_edits = lambda rows, masks=None, biases=None: (writes.append((list(rows), masks is not None, biases is not None)), inner(rows, masks, biases))[1]
    out = BatchedEngine(model, num_pages=8, max_batch=2).generate(prompts, 6, sampling=params)
    assert [len(o) for o in out] == [6, 6]
    # the arming write that disarms every row, then one mask write and one bias write for the two rows the prompts take: the decode passes write nothing
    assert writes == [([0, 1], True, True), ([0, 1], True, False), ([0, 1], False, True)]
    assert model.calls["step_batch"] == 5 and model.checked == 12


def test_a_lone_edited_prompt_is_a_batch_of_one():
    prompts = [[0, 5, 9], [1, 8, 2, 4]]
    params = [SamplingParams(logit_bias={4: 2.0}), SamplingParams()]
    model = EditStub(prompts, params, 0)
    BatchedEngine(model, num_pages=8, max_batch=1).generate(prompts, 3, sampling=params)
    assert model.calls["prefill_batch"] == 1 and model.calls["step"] == 1                 # the plain request keeps the single-sequence prompt pass
    assert model.sets == 1 and not model.tail_armed                                       # and a request with only edits arms no batch tail
