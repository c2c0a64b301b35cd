"""-m gpu: pie_token_dfa_mask and pie_token_dfa_advance (csrc/token_dfa.hpp), bit-exact against their numpy definitions
(tests/token_automaton_reference.py) -- armed rows, rows whose state has left the automaton, unarmed rows that keep a host-written mask,
records that overrun the arena, class ids out of range, both mask_on forms, and canary words behind the rows."""
import numpy as np
import pytest
import torch

from tests import token_automaton_reference as ref

pytestmark = pytest.mark.gpu
FILL = np.uint32(0xA5A5A5A5)     # what the mask words hold before the launch
CANARY = np.uint32(0x5EEDC0DE)


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a, dtype=np.int32)).cuda()


def random_tables(rng, V: int, S: int, C: int, bad_classes: bool = False) -> np.ndarray:
    """cls [V] then trans [S, C], about a third of the transitions disallowed; bad_classes: some ids carry the classes C and -1."""
    cls = rng.integers(0, C, size=V).astype(np.int32)
    if bad_classes:
        cls[rng.random(V) < 0.2] = C
        cls[rng.random(V) < 0.1] = -1
    trans = rng.integers(0, S, size=(S, C)).astype(np.int32)
    trans[rng.random((S, C)) < 0.35] = -1
    return np.concatenate([cls, trans.reshape(-1)])


def arena_and_rows(rng, V: int, S: int, C: int, rows: int, left_state: int):
    """An arena of two automata behind 5 words of padding, and `rows` (record, state) pairs: an armed row; an armed row that has left the
    automaton (state `left_state`); an unarmed row; a row whose record overruns the arena; an armed row over class ids out of range."""
    good, bad = random_tables(rng, V, S, C), random_tables(rng, V, S, C, bad_classes=True)
    tables = np.concatenate([np.full(5, -7, np.int32), good, bad])
    at_good, at_bad = 5, 5 + good.size
    recs = [(at_good, at_good + V, S, C), (at_good, at_good + V, S, C), (0, 0, 0, 0), (at_bad, at_bad + V + 1, S, C), (at_bad, at_bad + V, S, C)]
    states = [int(rng.integers(0, S)), left_state, 3, 0, S - 1]
    if rows == 1:
        recs, states = recs[:1], states[:1]
    assert ref.armed(recs[0], V, tables.size) and (rows == 1 or (not ref.armed(recs[3], V, tables.size) and ref.armed(recs[4], V, tables.size)))
    return tables, recs, states


@pytest.mark.parametrize("with_mask_on", [True, False])
@pytest.mark.parametrize("V", [33, 65, 512, 1000, 128256])
def test_mask_op(V, with_mask_on):
    from proxy_inference_engine_amd import _ffi, hip_ops
    lib = _ffi.load()
    rng = np.random.default_rng(V)
    n = (V + 31) // 32
    for S, C in ((1, 1), (1, 2), (7, 2), (7, 300), (1, 300), (7, 1)):
        for rows, left in ((1, -1), (5, -1), (5, S)):
            tables, recs, states = arena_and_rows(rng, V, S, C, rows, left)
            for mask_words in (n, n + 1):   # the rows back to back with one canary behind the last; a canary word behind every row
                host = np.full((rows, mask_words), FILL, np.uint32)
                if mask_words > n:
                    host[:, n:] = CANARY
                if rows == 5:
                    host[2, :n] = ref.pack(rng.random(V) < 0.5)   # the unarmed row's host-written mask
                on = np.array([7, 7, 1, 7, 7][:rows], np.int32) if with_mask_on else None
                want, want_on = ref.dfa_mask(recs, states, tables, V, host, on)
                flat = dev(np.concatenate([host.reshape(-1), [CANARY]]).astype(np.uint32))
                d_rec, d_st, d_tab = hip_ops.token_dfa_records(recs, "cuda"), dev(np.array(states)), dev(tables)
                d_on = dev(on) if with_mask_on else None
                _ffi.check(lib.pie_token_dfa_mask(_ffi.p(d_rec), _ffi.p(d_st), _ffi.p(d_tab), tables.size, rows, V, _ffi.p(flat), mask_words, _ffi.p(d_on), _ffi.stream()))
                got = flat.cpu().numpy().view(np.uint32)
                what = (V, S, C, rows, left, mask_words)
                assert got[-1] == CANARY, what
                assert np.array_equal(got[:-1].reshape(rows, mask_words), want), what
                if with_mask_on:
                    assert d_on.cpu().numpy().tolist() == want_on.tolist(), what
                assert d_st.cpu().numpy().tolist() == states, what   # the mask op moves no state
                # what the reference says, spelled out: bits at or beyond V are zero, the left row is unmasked or untouched, the two unarmed rows keep their words
                if V % 32:
                    assert int(want[0, n - 1]) >> (V % 32) == 0, what
                if rows == 5:
                    assert np.array_equal(want[2], host[2]) and np.array_equal(want[3], host[3]), what
                    if with_mask_on:
                        assert want_on.tolist() == [1, 0, 1, 7, 1] and np.array_equal(want[1], host[1]), what
                    else:
                        assert np.array_equal(want[1, :n], ref.pack(np.ones(V, bool))), what


def test_mask_op_through_hip_ops():
    from proxy_inference_engine_amd import hip_ops
    V, S, C = 1000, 7, 300
    rng = np.random.default_rng(9)
    tables, recs, states = arena_and_rows(rng, V, S, C, 5, -1)
    n = (V + 31) // 32
    host = np.full((5, n), FILL, np.uint32)
    masks, on = dev(host).view(5, n), dev(np.zeros(5))
    d_rec, d_st, d_tab = hip_ops.token_dfa_records(recs, "cuda"), dev(np.array(states)), dev(tables)
    out = hip_ops.token_dfa_mask(d_rec, d_st, d_tab, V, masks, on)
    want, want_on = ref.dfa_mask(recs, states, tables, V, host, np.zeros(5, np.int32))
    assert out is masks and np.array_equal(masks.cpu().numpy().view(np.uint32), want) and on.cpu().numpy().tolist() == want_on.tolist()
    # row 0's words are the packed mask the host class computes from the same tables
    from proxy_inference_engine_amd.logits_processors import TokenAutomaton
    a = TokenAutomaton.__new__(TokenAutomaton)
    a.cls, a.trans, a.start = tables[5:5 + V], tables[5 + V:5 + V + S * C].reshape(S, C), 0
    assert np.array_equal(want[0], ref.pack(a.allowed(states[0])))
    with pytest.raises(ValueError):
        hip_ops.token_dfa_mask(d_rec, d_st, d_tab, V, masks[:, :n - 1].contiguous(), on)   # too few words: refused before the launch
    with pytest.raises(ValueError):
        hip_ops.token_dfa_mask(d_rec, d_st[:4], d_tab, V, masks, on)


@pytest.mark.parametrize("V,S,C", [(65, 7, 2), (1000, 7, 300), (128256, 7, 300), (33, 1, 1)])
def test_advance_op(V, S, C):
    """Every branch of the rule: an allowed token, a disallowed one, tokens -1 and V, a class out of range, states -1 and S (stay), an
    unarmed row and a record that overruns the arena (both untouched)."""
    from proxy_inference_engine_amd import hip_ops
    rng = np.random.default_rng(V + S)
    good, bad = random_tables(rng, V, S, C), random_tables(rng, V, S, C, bad_classes=True)
    good[V:] = np.where(np.arange(S * C) % 2 == 0, np.abs(good[V:]) % S, -1)   # even classes allowed, odd ones not (C == 1: all allowed)
    tables = np.concatenate([np.full(3, 99, np.int32), good, bad])
    g, b = 3, 3 + good.size
    cls = good[:V]
    t_ok = int(np.flatnonzero(cls % 2 == 0)[0])
    t_no = int(np.flatnonzero(cls % 2 == 1)[0]) if C > 1 else -1
    t_badcls = int(np.flatnonzero((bad[:V] < 0) | (bad[:V] >= C))[0])
    t_goodcls = int(np.flatnonzero((bad[:V] >= 0) & (bad[:V] < C))[0])
    armed, badrec = (g, g + V, S, C), (b, b + V, S, C)
    rows = [(armed, S - 1, t_ok), (armed, 0, t_no), (armed, 0, -1), (armed, S - 1, V), (badrec, 0, t_badcls), (badrec, S - 1, t_goodcls), (armed, -1, t_ok),
            (armed, S, t_ok), ((0, 0, 0, 0), 12345, t_ok), ((b, b + V + 1, S, C), 0, t_ok), ((g, g + V, S, -C), 0, t_ok), ((-1, g + V, S, C), 0, t_ok)]
    recs, states, tokens = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    want = ref.dfa_advance(recs, states, tables, V, tokens)
    assert want[0] == good[V + (S - 1) * C + cls[t_ok]] >= 0 and want[1:5].tolist() == [-1] * 4 and want[6:].tolist() == [-1, S, 12345, 0, 0, 0]
    d_st = dev(np.array(states))
    out = hip_ops.token_dfa_advance(hip_ops.token_dfa_records(recs, "cuda"), d_st, dev(tables), V, dev(np.array(tokens)))
    assert out is d_st and d_st.cpu().numpy().tolist() == want.tolist()
    # one row, and more rows than one wave
    many = 150
    recs, states, tokens = [armed] * many, rng.integers(-1, S + 1, size=many).tolist(), rng.integers(-1, V + 1, size=many).tolist()
    d_st = dev(np.array(states))
    hip_ops.token_dfa_advance(hip_ops.token_dfa_records(recs, "cuda"), d_st, dev(tables), V, dev(np.array(tokens)))
    assert d_st.cpu().numpy().tolist() == ref.dfa_advance(recs, states, tables, V, tokens).tolist()
    d_st = dev(np.array(states[:1]))
    hip_ops.token_dfa_advance(hip_ops.token_dfa_records(recs[:1], "cuda"), d_st, dev(tables), V, dev(np.array(tokens[:1])))
    assert d_st.cpu().numpy().tolist() == ref.dfa_advance(recs[:1], states[:1], tables, V, tokens[:1]).tolist()
