"""-m gpu: per-row token automata in the multi-sequence passes against the same passes with every row's mask written by
the host (pinned by tests/test_gpu_batch_edits.py): an armed row derives its mask from its state on the device and advances
the state by the token it drew; an unarmed row keeps the host's mask, or none.  Every comparison is exact on storage bits."""
import numpy as np
import pytest
import torch

from tests._util import to_bits
from tests.test_gpu_batch_edits import make_model, tiny  # noqa: F401  (tiny: the fixture)
from tests.test_gpu_batch_tail import dev_ids, f32_bits, prefilled, repeating_prompts
from tests.test_gpu_step_automaton import random_automaton

pytestmark = pytest.mark.gpu


class Row:
    """One output row on the host: an automaton and its state, or a fixed mask, or nothing."""

    def __init__(self, automaton=None, state=None, mask=None):
        self.a, self.mask = automaton, mask
        self.s = None if automaton is None else (automaton.start if state is None else state)

    def allowed(self):
        """bool [V] the coming pass masks the row with, or None: unmasked."""
        if self.a is None:
            return self.mask
        return self.a.allowed(self.s) if 0 <= self.s < self.a.n_states else None

    def took(self, tok: int) -> None:
        if self.a is not None:
            self.s = self.a.step(self.s, tok)


def five_kinds(V, n):
    """A | B, of another S and C | a host mask | nothing | A again at another state | B at another state | nothing."""
    A, B = random_automaton(V, 6, 9, seed=21), random_automaton(V, 4, 5, seed=22, start=1)
    mask = np.random.default_rng(23).random(V) < 0.4
    return A, B, [Row(A), Row(B), Row(mask=mask), Row(), Row(A, 3), Row(B, 2), Row()][:n]


def host_masks(model, rows):
    model.write_batch_edits(list(range(len(rows))), masks=[None if r.allowed() is None else torch.from_numpy(r.allowed()) for r in rows])


def arm(model, rows, tables_words):
    """The automaton rows into armed records; the fixed mask by the host, once."""
    bd = model.set_batch_automata(len(rows), tables_words)
    model.write_batch_automata(list(range(len(rows))), [r.a for r in rows], [r.s for r in rows])
    model.write_batch_edits(list(range(len(rows))), masks=[None if r.a is not None or r.mask is None else torch.from_numpy(r.mask) for r in rows])
    return bd


def states_of(bd, rows):
    got = bd["states"].tolist()
    return [got[i] for i, r in enumerate(rows) if r.a is not None]


def assert_rows(got, want, what):
    (nxt, lp, lg), (wn, wlp, wlg) = got, want
    assert nxt.tolist() == wn, what
    for i in range(len(wn)):
        assert np.array_equal(to_bits(lg[i]), wlg[i]), (what, i, "logits")
        assert np.array_equal(f32_bits(lp[i]), wlp[i]), (what, i, "logprobs")


def snapshot(out):
    nxt, lp, lg = out
    return nxt.tolist(), [f32_bits(lp[i]) for i in range(nxt.numel())], [to_bits(lg[i]).copy() for i in range(nxt.numel())]


# ------------------------------------------------------------------ 1. the batched step
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("B", [5, 7])              # the fused few-sequence form; the general form
def test_step_batch_with_automata_equals_host_written_masks(tiny, B, graph):
    g, cfg, model = tiny
    V, steps = cfg["vocab_size"], 6
    prompts = repeating_prompts(V, [9, 60, 30, 12, 7, 21, 33][:B], 3)
    model.clear_batch_tail(), model.clear_batch_edits()
    model.enable_paged_kv(num_pages=48)
    A, Bm, rows = five_kinds(V, B)
    # run 1: every row's mask written by the host before every pass
    caches, first = prefilled(model, prompts)
    want, feed = [], dev_ids(first)
    try:
        model.set_batch_edits(B, masks=True)
        for st in range(steps):
            host_masks(model, rows)
            out = model.step_batch(feed, caches, graph=graph)
            want.append(snapshot(out))
            for r, t in zip(rows, want[-1][0]):
                assert r.allowed() is None or r.allowed()[t]
                r.took(t)
            feed = out[0].clone()
    finally:
        model.clear_batch_edits()
    final = [r.s for r in rows if r.a is not None]
    # run 2: fresh caches, the automata on the device
    caches, first_a = prefilled(model, prompts)
    assert first_a == first
    _, _, rows = five_kinds(V, B)
    try:
        model.set_batch_edits(B, masks=True)
        bd = arm(model, rows, A.words().size + Bm.words().size)
        assert len(bd["uploaded"]) == 2 and bd["used"] == A.words().size + Bm.words().size     # every distinct object once
        replays, feed = model.batch_graph_replays(), dev_ids(first)
        for st in range(steps):
            out = model.step_batch(feed, caches, graph=graph)
            assert_rows(out, want[st], (B, graph, st))
            feed = out[0].clone()
        assert states_of(bd, rows) == final
        assert model.batch_graph_replays() - replays == (steps - 2 if graph else 0)            # eager, capture, then replays only
        assert model._batch_edits["mask_on"].tolist()[:5] == [1, 1, 1, 0, 1]
    finally:
        model.clear_batch_automata()
        model.clear_batch_edits()
    assert model._batch_dfa is None and model._batch_edits is None


# ------------------------------------------------------------------ 2. the launch table
@pytest.mark.parametrize("B", [3, 7])
def test_launches_are_two_more_than_masks_only(golden_dir, B):
    g, cfg, model = make_model(golden_dir)
    V = cfg["vocab_size"]
    model.enable_paged_kv(num_pages=64)
    prompts = repeating_prompts(V, [5 + 2 * i for i in range(B)], 9)
    A = random_automaton(V, 6, 9, seed=24)

    def count():
        caches, first = prefilled(model, prompts)
        feed = dev_ids(first)
        for _ in range(3):                         # eager, capture, replay
            feed = model.step_batch(feed, caches)[0].clone()
        for c in caches:
            c[0].page_manager.release()
        return model.batch_graph_launches()

    plain = count()
    for tailed in (False, True):
        try:
            if tailed:
                model.set_batch_tail(B)
            model.set_batch_edits(B, masks=True)
            masks_only = count()
            model.set_batch_automata(B, A.words().size)
            assert count() == masks_only + 2, (B, tailed)                      # armed or not: the two ops run over every row
            model.write_batch_automata([0], [A])
            assert count() == masks_only + 2, (B, tailed)
            model.clear_batch_automata()
            assert count() == masks_only, (B, tailed)
        finally:
            model.clear_batch_automata(), model.clear_batch_edits(), model.clear_batch_tail()
    assert count() == plain
    # set_batch_automata arms the edits' mask part where none is set, and takes it away again
    model.set_batch_automata(B, A.words().size)
    assert model._batch_edits is not None and model._batch_edits["masks"] is not None
    model.clear_batch_automata()
    assert model._batch_edits is None and count() == plain


# ------------------------------------------------------------------ 3. the prompt passes
def test_prompt_passes_with_automata(tiny):
    g, cfg, model = tiny
    V = cfg["vocab_size"]
    ps = repeating_prompts(V, [20, 11, 9, 20, 14], 5)
    model.clear_batch_tail(), model.clear_batch_edits()
    model.enable_paged_kv(num_pages=64)
    fresh = lambda n: [model.make_cache() for _ in range(n)]
    A, Bm, _ = five_kinds(V, 5)
    words = A.words().size + Bm.words().size
    try:
        model.set_batch_edits(5, masks=True)
        # prefill_batch: five prompts, the five kinds
        _, _, rows = five_kinds(V, 5)
        host_masks(model, rows)
        want_pf = snapshot(model.prefill_batch(ps, fresh(5)))
        for r, t in zip(rows, want_pf[0]):
            r.took(t)
        want_states = [r.s for r in rows if r.a is not None]
        _, _, rows = five_kinds(V, 5)
        bd = arm(model, rows, words)
        assert_rows(model.prefill_batch(ps, fresh(5)), want_pf, "prefill_batch")
        assert states_of(bd, rows) == want_states
        model.clear_batch_automata()
        # step_mixed: three decoding rows (A at a state, the host mask, nothing) and two prompts (A and B from their start states)
        def mixed_rows():
            _, _, r = five_kinds(V, 5)
            return [r[4], r[2], r[3], r[0], r[1]]
        rows = mixed_rows()
        dcs, dtoks = prefilled(model, ps[:3])
        host_masks(model, rows)
        want_mx = snapshot(model.step_mixed(dev_ids(dtoks), dcs, ps[3:], fresh(2)))
        for r, t in zip(rows, want_mx[0]):
            r.took(t)
        want_states = [r.s for r in rows if r.a is not None]
        rows = mixed_rows()
        dcs, dtoks2 = prefilled(model, ps[:3])
        assert dtoks2 == dtoks
        bd = arm(model, rows, words)
        assert_rows(model.step_mixed(dev_ids(dtoks), dcs, ps[3:], fresh(2)), want_mx, "step_mixed")
        assert states_of(bd, rows) == want_states
    finally:
        model.clear_batch_automata()
        model.clear_batch_edits()


# ------------------------------------------------------------------ 4. refusals
def test_refusals(tiny):
    from proxy_inference_engine_amd import _ffi
    g, cfg, model = tiny
    lib, V = _ffi.load(), cfg["vocab_size"]
    model.clear_batch_tail(), model.clear_batch_edits()
    model.enable_paged_kv(num_pages=16)
    A = random_automaton(V, 6, 9, seed=25)
    rec, st, tab = torch.zeros((2, 4), dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"), torch.from_numpy(A.words()).cuda()
    call = lambda *a: lib.pie_decoder_set_batch_token_dfa(model._dec, *a)
    # without the edits' mask part: refused by name
    assert call(2, _ffi.p(rec), _ffi.p(st), _ffi.p(tab), tab.numel()) == -5 and b"pie_decoder_set_batch_logits_edits" in lib.pie_last_error()
    model.set_batch_edits(2, masks=False, bias_cap=4)
    assert call(2, _ffi.p(rec), _ffi.p(st), _ffi.p(tab), tab.numel()) == -5
    try:
        model.set_batch_edits(2, masks=True)
        assert call(2, None, _ffi.p(st), _ffi.p(tab), tab.numel()) == -1 and call(2, _ffi.p(rec), None, _ffi.p(tab), tab.numel()) == -1
        assert call(2, _ffi.p(rec), _ffi.p(st), None, tab.numel()) == -1
        assert call(-1, _ffi.p(rec), _ffi.p(st), _ffi.p(tab), tab.numel()) == -2 and call(2, _ffi.p(rec), _ffi.p(st), _ffi.p(tab), 0) == -2
        import ctypes as C
        assert call(2, C.c_void_p(rec.data_ptr() + 2), _ffi.p(st), _ffi.p(tab), tab.numel()) == -3
        assert call(2, _ffi.p(rec), _ffi.p(st), _ffi.p(tab), tab.numel()) == 0
        # more output rows than rows_cap, and the mask part gone: each before any launch
        prompts = repeating_prompts(V, [9, 20, 30], 3)
        caches, first = prefilled(model, prompts)
        model.set_batch_edits(3, masks=True)
        with pytest.raises(ValueError, match="batch token automata"):
            model.step_batch(dev_ids(first), caches, graph=False)
        model.set_batch_edits(3, masks=False, bias_cap=4)
        with pytest.raises(RuntimeError, match="mask part"):
            model.step_batch(dev_ids(first[:2]), caches[:2], graph=False)
        assert call(0, None, None, None, 0) == 0
        nxt, _, _ = model.step_batch(dev_ids(first), caches, graph=False)
        assert nxt.shape == (3,)
        # the host family's own checks
        with pytest.raises(RuntimeError):
            model.write_batch_automata([0], [A])
        with pytest.raises(RuntimeError):
            model.upload_automaton(A)
        with pytest.raises(ValueError):
            model.set_batch_automata(0, 10)
        model.set_batch_automata(3, A.words().size)
        assert model.upload_automaton(A) == (0, V) and model.upload_automaton(A) == (0, V)
        with pytest.raises(ValueError, match="arena"):
            model.upload_automaton(random_automaton(V, 6, 9, seed=26))
        with pytest.raises(ValueError, match="vocabulary"):
            model.upload_automaton(random_automaton(V - 1, 3, 4, seed=27))
        with pytest.raises(ValueError):
            model.write_batch_automata([0, 1], [A])
    finally:
        model.clear_batch_automata()
        model.clear_batch_edits()


# ------------------------------------------------------------------ 5. BatchedEngine.generate
def test_engine_generates_under_automata_as_under_the_callable_host_mask(tiny):
    """Four requests through two rows, their prompts fed in chunks: the rows change occupants and a prompt that is still filling holds
    a row.  Every request under token_automaton equals the same request under the callable host mask of the same automaton, in tokens
    and in the maps of the processed log-probabilities; no callable runs for the automaton's requests, and the buffers are cleared."""
    from proxy_inference_engine_amd.engine import BatchedEngine, SamplingParams
    g, cfg, model = tiny
    V, new = cfg["vocab_size"], 7
    model.clear_batch_tail(), model.clear_batch_edits()
    prompts = repeating_prompts(V, [12, 37, 5, 22], 11)
    A, B = random_automaton(V, 6, 9, seed=28), random_automaton(V, 4, 5, seed=29, start=1)
    autos = [A, B, A, B]
    calls = []

    def walker(i):
        def fn(tokens):
            calls.append(i)
            return torch.from_numpy(autos[i].allowed(autos[i].walk(list(tokens)[len(prompts[i]):])))
        return fn

    mixed = [dict(), dict(temp=0.8, top_k=5, seed=21), dict(repetition_penalty=1.3, repetition_context_size=8), dict(logit_bias={int(prompts[3][0]): 3.0}, temp=0.7, seed=5)]
    by_auto = [SamplingParams(token_automaton=autos[i], **kw) for i, kw in enumerate(mixed)]
    by_mask = [SamplingParams(token_mask=walker(i), **kw) for i, kw in enumerate(mixed)]
    kw = dict(num_pages=48, max_batch=2, prefill_chunk=6)
    want, want_maps = BatchedEngine(model, **kw).generate(prompts, new, sampling=by_mask, logprobs=True, top_logprobs=4)
    assert len(calls) >= 4 * new
    calls.clear()
    out, maps = BatchedEngine(model, **kw).generate(prompts, new, sampling=by_auto, logprobs=True, top_logprobs=4)
    assert not calls
    assert out == want and maps == want_maps
    for i, o in enumerate(out):
        assert len(o) == new and autos[i].walk(o) >= 0, i        # every request stayed inside its grammar
    assert model._batch_dfa is None and model._batch_edits is None and model._batch_tail is None
    assert BatchedEngine(model, **kw).generate(prompts, new, sampling=by_auto) == out
    # a lone request is a batch of one: its first token is chosen under the start state's mask
    lone = BatchedEngine(model, num_pages=48, max_batch=2).generate(prompts[:1], 3, sampling=SamplingParams(token_automaton=A))
    assert A.walk(lone[0]) >= 0 and A.allowed(A.start)[lone[0][0]]
    with pytest.raises(ValueError, match="exclusive"):
        BatchedEngine(model, **kw).generate(prompts[:1], 2, sampling=SamplingParams(token_automaton=A, token_mask=[1]))
    assert model._batch_dfa is None and model._batch_edits is None
