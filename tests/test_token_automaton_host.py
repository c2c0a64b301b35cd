"""CPU: TokenAutomaton (logits_processors/token_automaton.py) -- its vectorised constructors against a brute-force per-token
byte walk, class compression, the EOS and dead-state rules, every constructor refusal, the consistency of walk / step / allowed, the
processor's torch body, the fused plan's routing, SamplingParams' validation, and the new entry points' refusals before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from proxy_inference_engine_amd.logits_processors import TokenAutomaton, make_logit_bias, make_repetition_penalty, make_token_automaton, make_token_mask
from tests import token_automaton_reference as ref


# ------------------------------------------------------------------ a synthetic vocabulary and two small grammars
def vocabulary(seed: int = 0):
    """256 single bytes, 250 random 2..5-byte strings over an alphabet the grammars below use, 3 special tokens (the first is EOS)."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"0123456789+-yesnomaybx", dtype=np.uint8)
    toks = [bytes([i]) for i in range(256)]
    toks += [bytes(rng.choice(alphabet, size=int(rng.integers(2, 6))).tolist()) for _ in range(250)]
    toks += [None, None, None]
    return toks, [256 + 250]


def number_dfa():
    """[+-]?[0-9]+ : 0 start, 1 behind a sign, 2 inside the digits (accepting), 3 a trap that 'x' leads to from anywhere and nothing leaves."""
    bt = np.full((4, 256), -1, dtype=np.int32)
    bt[0, ord("+")] = bt[0, ord("-")] = 1
    for d in b"0123456789":
        bt[0, d] = bt[1, d] = bt[2, d] = 2
    bt[:, ord("x")] = 3
    return bt, [2]


CHOICES = [b"yes", b"no", b"maybe"]


def test_from_byte_dfa_equals_the_brute_force_walk():
    toks, eos = vocabulary()
    bt, acc = number_dfa()
    a = TokenAutomaton.from_byte_dfa(bt, acc, toks, eos)
    want = ref.byte_walk_table(bt, acc, toks, eos)
    assert a.vocab_size == len(toks) and a.n_states == bt.shape[0] + 1 and a.start == 0
    assert np.array_equal(a.trans[:, a.cls], want)          # class compression reproduces the [S, V] table exactly
    assert a.n_classes == np.unique(want, axis=1).shape[1] < 16
    multi = [t for t in range(256, 506) if want[0, t] >= 0]
    assert multi, "no multi-byte token is a prefix of a number: the vocabulary tests nothing"
    # dead-state pruning: 'x' leads to the trap from everywhere, so neither it nor a token holding it is allowed anywhere
    assert (want[:, ord("x")] == -1).all() and all((want[:4, t] == -1).all() for t in range(256, 506) if b"x" in toks[t])
    # the EOS rule: allowed in the accepting state only, into the absorbing state, where nothing but EOS goes on
    S = bt.shape[0]
    assert want[2, eos[0]] == S and (want[[0, 1, 3], eos[0]] == -1).all()
    assert a.allowed(S).nonzero()[0].tolist() == eos and a.step(S, eos[0]) == S
    # the other special tokens are allowed nowhere
    assert (want[:, 507:] == -1).all()


def test_from_choices_equals_the_brute_force_walk():
    toks, eos = vocabulary(1)
    a = TokenAutomaton.from_choices(CHOICES, toks, eos)
    # the trie the constructor builds, by hand: one node per distinct prefix, in insertion order
    nodes, acc = {b"": 0}, []
    for c in CHOICES:
        for i in range(1, len(c) + 1):
            nodes.setdefault(c[:i], len(nodes))
        acc.append(nodes[c])
    bt = np.full((len(nodes), 256), -1, dtype=np.int32)
    for pre, n in nodes.items():
        if pre:
            bt[nodes[pre[:-1]], pre[-1]] = n
    want = ref.byte_walk_table(bt, acc, toks, eos)
    assert np.array_equal(a.trans[:, a.cls], want)
    # every accepted token sequence spells a choice
    for c in CHOICES:
        s = a.walk(list(c))
        assert a.allowed(s).nonzero()[0].tolist() == eos, c
    assert set(a.allowed(a.start).nonzero()[0].tolist()) >= {ord("y"), ord("n"), ord("m")}
    assert not a.allowed(a.start)[ord("e")]


def test_from_token_table_compresses_by_distinct_columns():
    rng = np.random.default_rng(3)
    cols = np.array([[1, -1, 2], [-1, -1, 0], [2, 0, -1], [0, 1, 1]], dtype=np.int32).T   # [S = 3, 4 distinct columns]
    pick = rng.integers(0, 4, size=97)
    table = cols[:, pick]
    a = TokenAutomaton.from_token_table(table, start=1)
    assert a.n_classes == len(set(pick.tolist())) and a.start == 1 and a.cls.dtype == np.int32 and a.trans.dtype == np.int32
    assert np.array_equal(a.trans[:, a.cls], table)
    w = a.words()
    assert w.dtype == np.int32 and w.size == 97 + 3 * a.n_classes
    assert np.array_equal(w[:97], a.cls) and np.array_equal(w[97:].reshape(3, -1), a.trans)


def test_walk_step_allowed_agree():
    toks, eos = vocabulary(2)
    bt, acc = number_dfa()
    a = TokenAutomaton.from_byte_dfa(bt, acc, toks, eos)
    rng = np.random.default_rng(4)
    for _ in range(50):
        s, seq = a.start, []
        for _ in range(8):
            ok = a.allowed(s)
            assert ok.any()
            for t in rng.integers(0, a.vocab_size, size=16):   # allowed(s)[t] <=> step(s, t) >= 0
                assert (a.step(s, int(t)) >= 0) == bool(ok[t])
            t = int(rng.choice(ok.nonzero()[0]))
            seq.append(t)
            s = a.step(s, t)
            assert 0 <= s < a.n_states and a.walk(seq) == s and a.walk(torch.tensor(seq)) == s
        assert a.walk(seq[4:], a.walk(seq[:4])) == s
    bad = int((~a.allowed(a.start)).nonzero()[0][0])
    assert a.step(a.start, bad) == -1 and a.step(a.start, -1) == -1 and a.step(a.start, a.vocab_size) == -1
    # a state outside [0, S) stays what it is and constrains nothing
    assert a.step(-1, 5) == -1 and a.step(a.n_states, 5) == a.n_states and a.walk([bad, 5, 6]) == -1
    assert a.allowed(-1).all() and a.allowed(a.n_states).all()


def test_constructor_refusals():
    cls, trans = np.array([0, 1, 0], dtype=np.int32), np.array([[1, 0], [0, -1]], dtype=np.int32)
    TokenAutomaton(cls, trans)
    TokenAutomaton(cls.tolist(), trans.tolist(), 1)   # lists of ints are taken
    for bad_cls, bad_trans, start, what in (
            (cls.astype(np.int64), trans, 0, "cls must be int32"), (cls, trans.astype(np.float32), 0, "trans must be int32"),
            (cls[None], trans, 0, "cls must be a non-empty 1-d"), (cls, trans[0], 0, "trans must be a non-empty 2-d"),
            (cls[:0], trans, 0, "cls must be a non-empty"),
            (np.array([0, 2, 0], dtype=np.int32), trans, 0, r"class outside \[0, 2\)"), (np.array([0, -1, 0], dtype=np.int32), trans, 0, "class outside"),
            (cls, np.array([[1, 0], [2, -1]], dtype=np.int32), 0, r"state outside \[-1, 2\)"), (cls, np.array([[1, 0], [0, -2]], dtype=np.int32), 0, "state outside"),
            (cls, trans, 2, "start"), (cls, trans, -1, "start"), (cls, trans, 0.5, "start"),
            (cls, np.array([[1, 0], [-1, -1]], dtype=np.int32), 0, "state 1 is reachable from start and allows no token")):
        with pytest.raises(ValueError, match=what):
            TokenAutomaton(bad_cls, bad_trans, start)
    # an unreachable state may allow nothing; a class no id maps to allows nothing
    TokenAutomaton(cls, np.array([[0, 0], [-1, -1]], dtype=np.int32))
    with pytest.raises(ValueError, match="state 1 is reachable"):
        TokenAutomaton(np.array([0, 0, 0], dtype=np.int32), np.array([[1, 0], [-1, 0]], dtype=np.int32))
    toks, eos = vocabulary()
    bt, acc = number_dfa()
    with pytest.raises(ValueError, match="allows no token"):   # an accepting state without an EOS id, and nothing leaves it
        TokenAutomaton.from_choices([b"no"], toks, [])
    for args, what in (((bt[:, :255], acc, toks, eos), "256"), ((bt, [4], toks, eos), "accepting"), ((bt, acc, toks, [len(toks)]), "EOS"),
                       ((np.where(bt == 3, 9, bt), acc, toks, eos), "state outside"), ((bt, acc, toks, eos, 4), "start")):
        with pytest.raises(ValueError, match=what):
            TokenAutomaton.from_byte_dfa(*args)
    with pytest.raises(ValueError, match="choice"):
        TokenAutomaton.from_choices([b"a", b""], toks, eos)
    with pytest.raises(ValueError, match="from_token_table"):
        TokenAutomaton.from_token_table(np.zeros((2, 3), dtype=np.float32))
    a = TokenAutomaton(cls, trans)
    a.check_vocab(3)
    with pytest.raises(ValueError, match="vocabulary of 3"):
        a.check_vocab(4)


def test_processor_body_is_the_mask_of_the_walk():
    toks, eos = vocabulary(5)
    a = TokenAutomaton.from_choices(CHOICES, toks, eos)
    proc = make_token_automaton(a)
    assert proc.automaton is a
    prompt, V = [7, 8, 9, 10], a.vocab_size
    gen = list(b"may")
    for k in range(len(gen) + 1):
        logits = torch.randn(1, V)
        before = logits.clone()
        out = proc(prompt + gen[:k], logits)
        ok = torch.from_numpy(a.allowed(a.walk(gen[:k])))
        assert torch.equal(out[0][ok], before[0][ok]) and bool(torch.isinf(out[0][~ok]).all()) and bool((out[0][~ok] < 0).all()), k
    # a new request: the walk starts behind the new prompt
    proc.reset(2)
    out = proc([1, 2, ord("n")], torch.zeros(1, V))
    assert torch.equal(torch.isfinite(out[0]), torch.from_numpy(a.allowed(a.walk([ord("n")]))))
    with pytest.raises(ValueError, match="vocabulary"):
        proc(prompt, torch.zeros(1, V + 1))
    with pytest.raises(ValueError):
        make_token_automaton(object())


def test_fused_tail_plan_routes_the_automaton():
    from proxy_inference_engine_amd import samplers
    from proxy_inference_engine_amd.engine.inference_engine import InferenceEngine, check_speculative, check_speculative_tail, fused_tail_plan
    toks, eos = vocabulary(6)
    a = TokenAutomaton.from_choices(CHOICES, toks, eos)
    greedy = samplers.make_sampler(temp=0)
    auto, pen, bias = make_token_automaton(a), make_repetition_penalty(1.3, 20), make_logit_bias({5: 1.0})
    plan = fused_tail_plan([auto, pen, bias], greedy)
    assert plan["automaton"] is auto and plan["mask"] is None and plan["repetition_penalty"] == 1.3 and plan["bias"] is bias
    assert "automaton" not in fused_tail_plan([pen, bias], greedy)          # a request without one gets the plan it always got
    assert fused_tail_plan([pen, auto], greedy) is None                       # the mask's position: in front of the penalty
    assert fused_tail_plan([auto, auto], greedy) is None
    assert fused_tail_plan([auto], greedy, structuring_engine=object()) is None and fused_tail_plan([auto], greedy, tensor_parallel=True) is None
    mask = make_token_mask(torch.ones(a.vocab_size, dtype=torch.bool))
    for procs in ([mask, auto], [auto, mask]):
        with pytest.raises(ValueError, match="exclusive"):
            fused_tail_plan(procs, greedy)

    class Stub:   # what the checks read of a model
        tp = None
        spec_step = spec_step_tail = set_step_tail = None
    with pytest.raises(ValueError, match="a token automaton"):
        check_speculative(Stub(), greedy, [auto], None, None, None, None)
    with pytest.raises(ValueError, match="a token automaton"):
        check_speculative_tail(Stub(), greedy, [auto, pen], None, None, None, None)
    eng = InferenceEngine.__new__(InferenceEngine)
    eng.structuring_engine = None
    procs = eng.make_processors(token_automaton=a, repetition_penalty=1.2, logit_bias={3: 0.5})
    assert procs[0].automaton is a and len(procs) == 3 and fused_tail_plan(procs, greedy)["automaton"] is procs[0]
    with pytest.raises(ValueError, match="exclusive"):
        eng.make_processors(token_automaton=a, token_mask=torch.ones(a.vocab_size, dtype=torch.bool))


def test_sampling_params_validation():
    from proxy_inference_engine_amd.engine.batch_engine import SamplingParams
    toks, eos = vocabulary(7)
    a = TokenAutomaton.from_choices(CHOICES, toks, eos)
    sp = SamplingParams(token_automaton=a)
    assert not sp.plain and sp.tailless and sp.automaton(a.vocab_size) is a
    assert SamplingParams().plain and SamplingParams().automaton(a.vocab_size) is None
    with pytest.raises(ValueError, match="vocabulary"):
        sp.automaton(a.vocab_size + 1)
    with pytest.raises(ValueError, match="exclusive"):
        SamplingParams(token_automaton=a, token_mask=[1, 2]).automaton(a.vocab_size)
    with pytest.raises(ValueError, match="TokenAutomaton"):
        SamplingParams(token_automaton=lambda t: [1]).automaton(a.vocab_size)


def test_entry_points_refuse_before_any_launch_without_gpu():
    """pie_token_dfa_mask / _advance and the two setters: NULL pointers, shapes and alignment are refused with the neighbouring ops' codes
    before anything reaches HIP, so this runs without a device."""
    from proxy_inference_engine_amd import _ffi, hip_ops
    lib = _ffi.load()
    buf = ctypes.create_string_buffer(8192)
    base = (ctypes.addressof(buf) + 255) & ~255
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 2)   # aligned / misaligned stand-ins, never dereferenced
    ARG, SHAPE, ALIGN = -1, -2, -3

    def refused(fn, args, code):
        rc = getattr(lib, fn)(*args)
        err = lib.pie_last_error()
        assert rc == code and err.split(b":")[0] == fn.encode(), (fn, args, rc, err)

    ok = [p, p, p, 64, 2, 65, p, 3, p, None]   # records, states, tables, tables_len, rows, V, masks, mask_words, mask_on, stream
    for i, v, code in ((0, None, ARG), (1, None, ARG), (2, None, ARG), (6, None, ARG), (7, 2, SHAPE), (4, 0, SHAPE), (4, 65536, SHAPE), (5, 0, SHAPE),
                       (3, 0, SHAPE), (0, odd, ALIGN), (1, odd, ALIGN), (2, odd, ALIGN), (6, odd, ALIGN), (8, odd, ALIGN)):
        refused("pie_token_dfa_mask", ok[:i] + [v] + ok[i + 1:], code)
    ok = [p, p, p, 64, 2, 65, p, None]         # records, states, tables, tables_len, rows, V, tokens, stream
    for i, v, code in ((0, None, ARG), (1, None, ARG), (2, None, ARG), (6, None, ARG), (4, 0, SHAPE), (5, -1, SHAPE), (3, -4, SHAPE),
                       (0, odd, ALIGN), (1, odd, ALIGN), (2, odd, ALIGN), (6, odd, ALIGN)):
        refused("pie_token_dfa_advance", ok[:i] + [v] + ok[i + 1:], code)
    refused("pie_decoder_set_token_dfa", [None, p, p, p, 64, p, 3], ARG)
    refused("pie_decoder_set_batch_token_dfa", [None, 2, p, p, p, 64], ARG)
    assert ctypes.sizeof(_ffi.pie_row_dfa) == 16 and hip_ops.DFA_WORDS == 4
    recs = hip_ops.token_dfa_records([None, (3, 68, 2, 5)])
    assert recs.dtype == torch.int32 and recs.tolist() == [[0, 0, 0, 0], [3, 68, 2, 5]]
    for bad in ([], [(1, 2, 3)], [(1, 2, 3, 2 ** 31)]):
        with pytest.raises(ValueError):
            hip_ops.token_dfa_records(bad)
