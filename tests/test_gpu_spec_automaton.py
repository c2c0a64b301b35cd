"""-m gpu: grammar-constrained speculative decoding -- the walk and the grammar-aware drafter against their Python
restatements (exact), the decoder's pass under a token automaton against every row alone (exact) with the plain automaton steps behind
it, the refusals by name, the untouched plain path and the engine end to end.

The pass tests use a chain automaton: one branching state that allows the even ids, then 33 states of one id each -- a forced run --
and a last state that loops.  A draft made of the run is accepted in full under any sampler and with any weights."""
import json

import numpy as np
import pytest
import torch

from proxy_inference_engine_amd.logits_processors import TokenAutomaton
from tests import spec_automaton_reference as ref
from tests._util import codes_dev, to_dev
from tests.test_gpu_spec_sampled import draw_at, position, set_position
from tests.test_gpu_speculative import bits_of, dev_ids, fresh_cache, load_tiny
from tests.test_spec_automaton_host import poisoned_tables, random_automaton

pytestmark = pytest.mark.gpu
SENT = -77
NAME = "tiny_llama_w4_bf16"
RUN_LEN, FURTHER, C0 = 33, 12, 11
BIAS = ([5, 17, 300, 17], [4.0, -3.0, 2.5, 9.0])
TAILS = {
    "greedy": dict(),
    "top_p+penalty+bias": dict(sampler=("top_p", 0.8, 0.9, 0), repetition_penalty=1.3, context_size=20, logit_bias=BIAS),
}


def chain(V: int):
    """(automaton, run): state 0 allows the even ids, state 1 + i only run[i], the last state run[-1] for ever."""
    run = [int(t) for t in (np.arange(RUN_LEN) * 7 + 3) % V]
    cls, trans = ref.chain_automaton(V, run, branch_ids=list(range(0, V, 2)))
    return TokenAutomaton(cls, trans, 0), run


def records(rec) -> torch.Tensor:
    from proxy_inference_engine_amd import hip_ops
    return hip_ops.token_dfa_records([rec], "cuda")


# ------------------------------------------------------------------ 1. the ops against the reference, exact
@pytest.mark.parametrize("V", [65, 64])
def test_walk_and_draft_equal_the_reference(V):
    """V = 65 and 64: the mask word's edge.  Per automaton (the chain, two random ones at another arena offset): every forced table --
    the true one and the poisoned ones --, k = 1 and 31, candidate counts 0, 1, 31 and 1000 (clamped on the device), candidate ids that
    include -1 and V, start states -1 and S (left: the candidate passes through) and inside; the outputs have canaries behind them."""
    from proxy_inference_engine_amd import hip_ops
    rng = np.random.default_rng(V)
    automata = [chain(V)[0]]
    for _ in range(5000):                                                   # random automata that force something
        a = random_automaton(rng, V, 6, 40, 0.06)
        if a is not None and (a.forced()[:, 0] >= 0).sum() >= 2:
            automata.append(a)
        if len(automata) == 3:
            break
    assert len(automata) == 3
    drafted = cut = 0
    for ai, a in enumerate(automata):
        S = a.n_states
        rec, arena = ref.record_of(a, cls_off=5 * ai)
        rec_dev, tables = records(rec), dev_ids(arena)
        zero_rec = records(None)
        for table in [a.forced()] + poisoned_tables(a):
            forced = torch.from_numpy(table.copy()).cuda()
            for k in (1, 31):
                for count in (0, 1, 31, 1000):
                    for s0 in (-1, S, 0, S - 1, int(rng.integers(0, S))):
                        cand = rng.integers(-1, V + 1, size=31)
                        cand[int(rng.integers(0, 31))] = -1
                        cand[int(rng.integers(0, 31))] = V
                        if count == 31 and 0 <= s0 < S:                     # a candidate the grammar follows for a while
                            s = s0
                            for i in range(int(rng.integers(1, 12))):
                                ok = np.flatnonzero(a.allowed(s))
                                if ok.size == 0:                            # (a state the start does not reach may allow nothing)
                                    break
                                cand[i] = int(rng.choice(ok))
                                s = a.step(s, cand[i])
                                if not 0 <= s < S:
                                    break
                        what = (V, ai, k, count, s0, cand.tolist())
                        want_ids, want_n = ref.dfa_draft(rec, s0, arena, table, V, cand, count, k)
                        state, cand_dev, count_dev = dev_ids([s0]), dev_ids(cand), dev_ids([count])
                        out = (torch.full((k + 3,), SENT, dtype=torch.int32, device="cuda"), torch.full((1,), SENT, dtype=torch.int32, device="cuda"))
                        ids, n = hip_ops.token_dfa_draft(rec_dev, state, tables, forced, V, cand_dev, count_dev, k, out=out)
                        got = out[0].tolist()
                        assert int(n.item()) == want_n and got[:want_n] == want_ids, what
                        assert all(t == SENT for t in got[want_n:]), what                  # nothing behind the count, nothing behind out_ids[k]
                        assert state.tolist() == [s0] and cand_dev.tolist() == cand.tolist(), what
                        drafted += want_n
                        cut += int(0 < want_n < min(count, 31, k))
                        # in place: the candidate's own words
                        hip_ops.token_dfa_draft(rec_dev, state, tables, forced, V, cand_dev, count_dev, k, out=(cand_dev, count_dev))
                        assert count_dev.tolist() == [want_n] and cand_dev.tolist() == want_ids + cand.tolist()[want_n:], what
            # an all-zero record: unarmed, the candidate passes through (the true table only needs one visit)
        cand = rng.integers(0, V, size=31)
        for table in [a.forced()]:
            forced = torch.from_numpy(table.copy()).cuda()
            ids, n = hip_ops.token_dfa_draft(zero_rec, dev_ids([0]), tables, forced, V, dev_ids(cand), dev_ids([9]), 31)
            assert int(n.item()) == 9 and ids[:9].tolist() == cand[:9].tolist() and ids[9:].eq(-1).all()
        # the walk
        for n_tok in (1, 7, 31):
            for s0 in (-1, S, 0, S - 1):
                toks = rng.integers(-1, V + 1, size=n_tok)
                if 0 <= s0 < S:
                    s = s0
                    for i in range(min(n_tok, int(rng.integers(1, 9)))):
                        if not a.allowed(s).any():
                            break
                        toks[i] = int(rng.choice(np.flatnonzero(a.allowed(s))))
                        s = a.step(s, toks[i])
                        if not 0 <= s < S:
                            break
                out = torch.full((n_tok + 4,), SENT, dtype=torch.int32, device="cuda")
                state = dev_ids([s0])
                got = hip_ops.token_dfa_walk(rec_dev, state, tables, V, dev_ids(toks), out=out)
                want = ref.dfa_walk(rec, s0, arena, V, toks)
                assert got.tolist() == want and want == [s0] + [a.walk(toks[:i + 1], s0) for i in range(n_tok)], (V, ai, n_tok, s0)
                assert out[n_tok + 1:].eq(SENT).all() and state.tolist() == [s0]
                assert hip_ops.token_dfa_walk(zero_rec, state, tables, V, dev_ids(toks)).tolist() == [s0] * (n_tok + 1)
    assert drafted > 500 and cut > 5, "the cases draft or cut nothing: the comparison tests nothing"


def test_walk_and_draft_check_arguments():
    from proxy_inference_engine_amd import _ffi, hip_ops
    a = chain(65)[0]
    rec, arena = ref.record_of(a)
    rec_dev, tables, state, forced = records(rec), dev_ids(arena), dev_ids([0]), hip_ops.token_dfa_forced(a, "cuda")
    cand, count = dev_ids([0] * 31), dev_ids([3])
    for k in (0, 32):
        with pytest.raises(ValueError, match="token_dfa_draft"):
            hip_ops.token_dfa_draft(rec_dev, state, tables, forced, 65, cand, count, k)
    with pytest.raises(ValueError, match="forced"):
        hip_ops.token_dfa_draft(rec_dev, state, tables, forced.reshape(-1), 65, cand, count, 3)
    with pytest.raises(ValueError, match="token_dfa_walk"):
        hip_ops.token_dfa_walk(rec_dev, state, tables, 65, dev_ids([0] * 32))
    lib, out = _ffi.load(), torch.full((40,), SENT, dtype=torch.int32, device="cuda")
    P = _ffi.p
    assert lib.pie_token_dfa_walk(P(rec_dev), P(state), P(tables), tables.numel(), 65, P(cand), 0, P(out), _ffi.stream()) == -2
    assert lib.pie_token_dfa_walk(P(rec_dev), P(state), P(tables), tables.numel(), 65, None, 3, P(out), _ffi.stream()) == -1
    assert lib.pie_token_dfa_draft(P(rec_dev), P(state), P(tables), tables.numel(), P(forced), 0, 65, P(cand), P(count), 3, P(out), P(out[35:]), _ffi.stream()) == -2
    assert lib.pie_token_dfa_draft(P(rec_dev), P(state), P(tables), tables.numel(), None, 5, 65, P(cand), P(count), 3, P(out), P(out[35:]), _ffi.stream()) == -1
    assert lib.pie_token_dfa_draft(P(rec_dev), P(state), P(tables), tables.numel(), P(forced[:, 1:]), 5, 65, P(cand), P(count), 3, P(out), P(out[35:]),
                                   _ffi.stream()) == -3
    torch.cuda.synchronize()
    assert out.eq(SENT).all()                                              # each before any launch


# ------------------------------------------------------------------ 2. the decoder's pass
def own_row(model, A, row: torch.Tensor, state: int, c: int, tail):
    """(token, log-probabilities) of one processed row alone: masked with A.allowed(state), then the argmax, or hip_ops.sample at stream
    position c."""
    from proxy_inference_engine_amd import hip_ops
    V = row.numel()
    words = hip_ops.pack_token_mask(torch.from_numpy(A.allowed(state)), V).cuda()
    tok, lp = hip_ops.logprobs_argmax_masked(row.clone().contiguous(), words)
    if tail.get("sampler") is None:
        return int(tok.item()), lp
    return draw_at(lp, c, tail["sampler"]), lp


def start_pass(model, A, prompt, tail, kind="contiguous", state=None):
    """A fresh cache behind the prompt's own step under the tail and the automaton: (cache, the token behind the prompt, c)."""
    cache = fresh_cache(model, kind)
    model.set_step_tail(token_automaton=A, **tail)
    model.reset_step_automaton()
    set_position(C0)
    tok, _, _ = model.step(dev_ids(prompt), cache)
    if state is not None:
        model.reset_step_automaton(state)
    return cache, int(tok.item()), position()[0]


def check_rows(model, A, draft, s0, c, tail, n, what):
    """Every row of the last pass -- yielded or not -- is its own row alone in the state the drafts before it lead to, at c + r."""
    rows = len(draft) + 1
    states = [s0] + [A.walk(draft[:i + 1], s0) for i in range(len(draft))]
    block, lps = model.spec_logits(rows).clone(), model._spec_state()["logprobs"][:rows].clone()
    here = position()
    for r in range(rows):
        tok, lp = own_row(model, A, block[r], states[r], c + r, tail)
        assert torch.equal(lp.view(torch.int32), lps[r].view(torch.int32)), f"{what} row {r}"
        if r < n:
            assert int(model.spec_tokens[r].item()) == tok, f"{what} row {r}"
            assert A.allowed(states[r])[tok], f"{what} row {r}"
    set_position(here[0])
    return states


def plain_steps_after(model, A, cache, emitted, what):
    """Plain automaton steps behind a pass emit only allowed ids, and the device state is the walk of everything emitted."""
    state_dev = model.step_tail_automaton[1]
    s = A.walk(emitted)
    assert state_dev.tolist() == [s], what
    for k in range(FURTHER):
        tok, _, _ = model.step(None, cache)
        t = int(tok.item())
        assert A.allowed(s)[t], f"{what} step {k}"
        s = A.step(s, t)
        assert state_dev.tolist() == [s], f"{what} step {k}"


@pytest.mark.parametrize("tail_name", list(TAILS))
@pytest.mark.parametrize("kind", ["contiguous", "pages"])
def test_spec_step_grammar_on_the_chain(golden_dir, kind, tail_name):
    cfg, dt, orc, model = load_tiny(golden_dir, NAME)
    V, tail = cfg["vocab_size"], TAILS[tail_name]
    draws = tail.get("sampler") is not None
    A, run = chain(V)
    prompt = [int(t) for t in np.random.default_rng(60).integers(0, V, 60)]
    try:
        # a forced draft, m = 5 and m = 31: accepted in full, whatever the weights and the sampler
        for m in (5, 31):
            what = f"{kind} {tail_name} m={m}"
            cache, t0, c = start_pass(model, A, prompt, tail, kind)
            assert t0 % 2 == 0 and model.step_tail_automaton[1].tolist() == [1], what
            tokens, n, lps = model.spec_step_grammar(dev_ids(run[:m]), cache)
            assert n == m + 1 and tokens.tolist() == run[:m + 1], what
            assert model.step_tail_automaton[1].tolist() == [A.walk(run[:m + 1], 1)] == [m + 2], what
            assert position() == [c + n if draws else C0, 0], what                          # the counter ends at c + out_n
            assert all(c_.offset == len(prompt) + n for c_ in cache) and lps.shape == (n, V), what
            check_rows(model, A, run[:m], 1, c, tail, n, what)
            seq = prompt + [t0] + run[:m + 1]
            assert model.history[len(prompt):len(seq)].tolist() == seq[len(prompt):], what
            plain_steps_after(model, A, cache, [t0] + run[:m + 1], what)
        # the pass from the branching state: row 0 is drawn among the even ids.  First with a draft whose id 0 is allowed and (almost
        # surely) wrong, then with row 0's own token in front of the run: accepted in full
        m = 7
        cache, _, c = start_pass(model, A, prompt, tail, kind, state=0)
        guess = [2] + run[:m - 1]
        tokens, n, _ = model.spec_step_grammar(dev_ids(guess), cache)
        first = int(tokens[0].item())
        assert first % 2 == 0 and n == (m + 1 if first == 2 else 1)
        check_rows(model, A, guess, 0, c, tail, n, f"{kind} {tail_name} branch guess")
        cache, _, c = start_pass(model, A, prompt, tail, kind, state=0)
        draft = [first] + run[:m - 1]
        tokens, n, _ = model.spec_step_grammar(dev_ids(draft), cache)
        what = f"{kind} {tail_name} branch"
        assert n == m + 1 and tokens.tolist() == draft + [run[m - 1]], what
        assert position() == [c + n if draws else C0, 0], what
        check_rows(model, A, draft, 0, c, tail, n, what)
        plain_steps_after(model, A, cache, tokens.tolist(), what)
        # a draft whose id 2 the grammar forbids: cut there, and token 2 is the grammar's
        cache, t0, c = start_pass(model, A, prompt, tail, kind)
        bad = run[:m]
        bad[2] = (run[2] + 1) % V
        assert not A.allowed(A.walk(run[:2], 1))[bad[2]]
        tokens, n, _ = model.spec_step_grammar(dev_ids(bad), cache)
        what = f"{kind} {tail_name} forbidden"
        assert n == 3 and tokens.tolist() == run[:3] and model.spec_tokens[3:m + 1].eq(-1).all(), what
        assert position() == [c + n if draws else C0, 0], what
        states = check_rows(model, A, bad, 1, c, tail, n, what)
        assert states[3:] == [-1] * (m - 2)                                                  # the rows behind it ran unmasked, and were not accepted
        assert all(c_.offset == len(prompt) + n for c_ in cache), what
        plain_steps_after(model, A, cache, [t0] + run[:3], what)
        # draft ids outside the vocabulary are never accepted
        cache, t0, c = start_pass(model, A, prompt, tail, kind)
        tokens, n, _ = model.spec_step_grammar(dev_ids([run[0], V, -1, 0, 0]), cache)
        assert n == 2 and tokens.tolist() == run[:2]
        plain_steps_after(model, A, cache, [t0] + run[:2], f"{kind} {tail_name} outside")
    finally:
        model.set_step_tail()


def test_then_draft_hands_the_grammar_the_next_draft(golden_dir):
    """draft(grammar=True) and then_draft with the grammar on: the forced run is drafted with nothing looked up, in one read-back."""
    cfg, dt, orc, model = load_tiny(golden_dir, NAME)
    V = cfg["vocab_size"]
    A, run = chain(V)
    prompt = [int(t) for t in np.random.default_rng(61).integers(0, V, 40)]
    try:
        cache, t0, _ = start_pass(model, A, prompt, {})
        model.draft(3, 1, 7, grammar=True)
        tokens, count = model.spec_read()
        assert tokens == [t0] and count == 7 and model.spec_read_draft() == run[:7]
        _, n, _ = model.spec_step_grammar(model.spec_draft[:count], cache, then_draft=(3, 1, 9, True))
        tokens, count = model.spec_read()
        assert n == 8 and tokens == run[:8] and count == 9 and model.spec_read_draft() == run[8:17]
        model.set_step_tail()
        with pytest.raises(ValueError, match="token_automaton"):
            model.draft(3, 1, 7, grammar=True)
    finally:
        model.set_step_tail()


# ------------------------------------------------------------------ 3. the refusals, by name
def test_grammar_entry_refusals_by_name(golden_dir):
    from proxy_inference_engine_amd import _ffi, hip_ops
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    cfg, dt, orc, model = load_tiny(golden_dir, NAME)
    V = cfg["vocab_size"]
    A, run = chain(V)
    prompt, draft = dev_ids(np.random.default_rng(5).integers(0, V, 20)), dev_ids(run[:7])
    lib, st = _ffi.load(), model._spec_state()
    rec = st["rec"]
    error = lambda: lib.pie_last_error().decode()                          # noqa: E731
    try:
        cache, _, _ = start_pass(model, A, prompt.tolist(), {})
        tokens, n, _ = model.spec_step_grammar(draft, cache)                # (makes the workspace)
        assert n == 8

        def raw_call(n_draft=7, entry="pie_decoder_spec_step_dfa", ws="grammar_ws", lp=st["logprobs"]):
            return getattr(lib, entry)(model._dec, _ffi.p(draft), n_draft, _ffi.p(rec[1:]), _ffi.p(rec[0:]), _ffi.p(lp), _ffi.p(st[ws]), None, 0, None, _ffi.stream())

        refused = ((dict(top_logprobs=3), "top_logprobs", "a top-logprobs record"), (dict(frequency_penalty=0.5, count_start=20), "frequency / presence", "frequency / presence counts"),
                   (dict(dry=(0.8, 1.75, 2, 64, ())), "DRY", "a DRY penalty"))
        for kw, name, c_name in refused:
            model.set_step_tail(token_automaton=A, **kw)
            with pytest.raises(ValueError, match=name):
                model.spec_step_grammar(draft, cache)
            assert raw_call() == -5 and c_name in error(), kw              # PIE_E_STATE from the library too, before any launch
        # a host mask (exclusive with the automaton), and no automaton at all
        model.set_step_tail(token_mask=hip_ops.pack_token_mask(torch.ones(V, dtype=torch.bool), V))
        with pytest.raises(ValueError, match="a token mask"):
            model.spec_step_grammar(draft, cache)
        assert raw_call() == -5 and "a token mask" in error()
        model.set_step_tail(sampler=("top_k", 0.8, 0.0, 5))
        with pytest.raises(ValueError, match="spec_step_tail"):
            model.spec_step_grammar(draft, cache)
        assert raw_call() == -5 and "pie_decoder_spec_step_tail" in error()
        # the automaton set: the tail's pass still refuses it, and the prompt scoring is refused here
        model.set_step_tail(token_automaton=A, sampler=("top_k", 0.8, 0.0, 5))
        with pytest.raises(ValueError, match="a token automaton"):
            model.spec_step_tail(draft, cache)
        assert raw_call(entry="pie_decoder_spec_step_tail") == -5 and "a token automaton" in error()
        bufs = model.set_prompt_logprobs(8, 3, 16)
        bufs["count"].fill_(-1)
        assert raw_call() == -5 and "prompt scoring" in error()
        model.clear_prompt_logprobs()
        assert raw_call(lp=None) == -1                                      # logprobs_rows is required
        assert raw_call(4) == -2 and raw_call(32) == -2 and raw_call(0) == -2
        for m in (4, 32):
            with pytest.raises(ValueError, match="rows"):
                model.spec_step_grammar(dev_ids([1] * m), cache)
        assert int(lib.pie_decoder_spec_dfa_workspace_bytes(model._dec, 1)) == 0 and int(lib.pie_decoder_spec_dfa_workspace_bytes(model._dec, 33)) == 0
        assert int(lib.pie_decoder_spec_dfa_workspace_bytes(model._dec, 8)) > int(lib.pie_decoder_spec_tail_workspace_bytes(model._dec, 8))
        torch.cuda.synchronize()
        assert all(c_.offset == 20 + n for c_ in cache)                     # each before any launch
        model.reset_step_automaton(A.walk(run[:8], 1))                      # (switched off and on again above: back to where the first pass left it)
        tokens, n2, _ = model.spec_step_grammar(dev_ids(run[8:15]), cache)  # and after all that the pass still runs
        assert n2 == 8 and tokens.tolist() == run[8:16]
    finally:
        model.set_step_tail()
        model.clear_prompt_logprobs()
    # int8 pages
    g = np.load(golden_dir / f"{NAME}.npz")
    w = {k[2:]: g[k] for k in g.files if k.startswith("w:")}
    paged = Model(ModelArgs(**cfg), {k: (codes_dev(v) if v.dtype == np.uint32 else to_dev(v, "bfloat16")) for k, v in w.items()})
    paged.enable_paged_kv(num_pages=8, max_blocks=2, kv_dtype=torch.int8)
    cache = paged.make_cache()
    paged.step(dev_ids(g["prompt"][:4]), cache)
    with pytest.raises(ValueError, match="int8 KV pages"):
        paged.spec_step_grammar(draft, cache)
    ws = torch.zeros(64, dtype=torch.int64, device="cuda")
    out = torch.zeros(40, dtype=torch.int32, device="cuda")
    assert lib.pie_decoder_spec_step_dfa(paged._dec, _ffi.p(draft), 7, _ffi.p(out[1:]), _ffi.p(out), _ffi.p(st["logprobs"]), _ffi.p(ws), None, 0, None, _ffi.stream()) == -5
    assert "int8 KV pages" in error()


# ------------------------------------------------------------------ 4. the engine, and the untouched plain path
def engine_for(model, prompt, **request):
    from proxy_inference_engine_amd import InferenceEngine
    eng = InferenceEngine(model=model)
    eng.prompt_cache.cache = fresh_cache(model, "contiguous")
    eng.prepare_engine(prompt, **request)
    return eng


@pytest.mark.parametrize("request_kw", [dict(temp=0), dict(temp=0.8, top_p=0.9)], ids=["greedy", "temp0.8"])
def test_engine_speculates_the_forced_run(golden_dir, request_kw):
    from proxy_inference_engine_amd import SpeculativeParams
    cfg, dt, orc, model = load_tiny(golden_dir, NAME)
    V = cfg["vocab_size"]
    A, run = chain(V)
    rec, arena = ref.record_of(A)
    assert ref.dfa_draft(rec, 1, arena, A.forced(), V, [], 0, 7) == (run[:7], 7)            # behind the branch every draft is a forced run of >= 5
    prompt = np.random.default_rng(62).integers(0, V, 24)
    sp = SpeculativeParams(grammar=True, num_draft=7, min_draft=5)
    n_tokens = 44                                                                           # beyond the run: the last state loops
    try:
        eng = engine_for(model, prompt, token_automaton=A, **request_kw)
        set_position(0)
        out = [t for t, _ in eng.generate(torch.from_numpy(prompt), speculative=sp, max_completion_tokens=n_tokens)]
        assert len(out) == n_tokens and out[0] % 2 == 0
        assert out[1:] == (run + [run[-1]] * n_tokens)[:n_tokens - 1]                       # behind the branching token: the chain's ids
        assert A.walk(out) >= 0
        stats = eng.spec_stats
        assert stats["passes"] >= 5 and stats["steps"] == 0 and stats["accepted"] == stats["drafted"] == stats["forced"] == 7 * stats["passes"], stats
        assert model.step_tail_automaton[0] is A
        # the same request under configured_tail=True alone is still refused
        eng = engine_for(model, prompt, token_automaton=A, **request_kw)
        with pytest.raises(ValueError, match="a token automaton"):
            next(eng.generate_step(torch.from_numpy(prompt), speculative=SpeculativeParams(configured_tail=True)))
        # and the plain automaton loop emits the same ids (greedy: the same branching token too)
        eng = engine_for(model, prompt, token_automaton=A, **request_kw)
        set_position(0)
        plain = [t for t, _ in eng.generate(torch.from_numpy(prompt), max_completion_tokens=n_tokens)]
        assert plain[1:] == out[1:] and plain[0] == out[0]
    finally:
        model.set_step_tail()


def test_plain_generation_is_the_same_before_and_after_a_grammar_speculative_one(golden_dir):
    from proxy_inference_engine_amd import SpeculativeParams
    cfg, dt, orc, model = load_tiny(golden_dir, NAME)
    V = cfg["vocab_size"]
    A, run = chain(V)
    prompt = np.random.default_rng(63).integers(0, V, 24)

    def plain():
        eng = engine_for(model, prompt, temp=0)
        gen = eng.generate_step(torch.from_numpy(prompt))
        toks, bits = [], []
        for _ in range(24):
            t, lp = next(gen)
            toks.append(int(t.item())), bits.append(bits_of(lp))
        return toks, np.stack(bits), model.graph_launches()

    try:
        toks0, bits0, launches0 = plain()
        eng = engine_for(model, prompt, temp=0, token_automaton=A)
        spec = [t for t, _ in eng.generate(torch.from_numpy(prompt), speculative=SpeculativeParams(grammar=True), max_completion_tokens=24)]
        assert eng.spec_stats["passes"] >= 1 and spec[1:] == run[:23]
        toks1, bits1, launches1 = plain()
    finally:
        model.set_step_tail()
    assert launches0 > 0 and launches1 == launches0                        # the captured step's kernel count
    assert toks1 == toks0 and np.array_equal(bits0, bits1)
