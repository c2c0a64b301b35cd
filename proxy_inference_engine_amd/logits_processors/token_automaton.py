"""A grammar as a token-level DFA compressed by token classes: what a structuring engine compiles a regex, a choice list or
a JSON schema to ahead of time, so that the decode step derives its own token mask from a state on the device and advances the state by
the token it drew (csrc/token_dfa.hpp) -- no read-back, no Python `mask_fn`, no upload per token.

An automaton over a vocabulary of V ids has S states and C token classes:
    cls   int32 [V]     token id -> class in [0, C)
    trans int32 [S, C]  the next state in [0, S), or -1: the token is not allowed in this state
    start               the start state
Token t is allowed in state s iff trans[s, cls[t]] >= 0.  On the device an automaton is V + S * C consecutive int32 words (cls, then
trans) inside a caller-owned arena (`words()`).  Nothing here needs a tokenizer at run time: `from_byte_dfa` takes the vocabulary's byte
strings once, on the host.  This class is the host definition: `allowed`, `step` and `walk` are what the device ops compute."""
from __future__ import annotations

from collections.abc import Callable, Sequence

import numpy as np
import torch


def _table(x, name: str, ndim: int) -> np.ndarray:
    """An int32 array of `ndim` dimensions; arrays and tensors of another dtype are refused, not converted."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        if x.dtype != np.int32:
            raise ValueError(f"TokenAutomaton: {name} must be int32, got {x.dtype}")
        a = x
    else:
        try:
            a = np.asarray(x)
        except Exception as e:  # ragged lists
            raise ValueError(f"TokenAutomaton: {name} is not an array: {e}") from None
        if a.dtype.kind not in "iu":
            raise ValueError(f"TokenAutomaton: {name} must be int32, got {a.dtype}")
        a = a.astype(np.int32)
    if a.ndim != ndim or a.size == 0:
        raise ValueError(f"TokenAutomaton: {name} must be a non-empty {ndim}-d array, got shape {a.shape}")
    return np.ascontiguousarray(a)


class TokenAutomaton:
    def __init__(self, cls, trans, start: int = 0):
        cls, trans = _table(cls, "cls", 1), _table(trans, "trans", 2)
        S, C = trans.shape
        if cls.min() < 0 or cls.max() >= C:
            raise ValueError(f"TokenAutomaton: cls holds a class outside [0, {C})")
        if trans.min() < -1 or trans.max() >= S:
            raise ValueError(f"TokenAutomaton: trans holds a state outside [-1, {S})")
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or not 0 <= int(start) < S:
            raise ValueError(f"TokenAutomaton: start must be a state in [0, {S}), got {start!r}")
        self.cls, self.trans, self.start = cls, trans, int(start)
        self._forced = None
        self.cls.setflags(write=False)
        self.trans.setflags(write=False)
        # every state reachable from start allows some token: the device never sees an all-zero mask (a class no id maps to allows nothing)
        used = np.zeros(C, dtype=bool)
        used[cls] = True
        live = np.where(used[None, :], trans, -1)
        seen = np.zeros(S, dtype=bool)
        seen[self.start] = True
        todo = [self.start]
        while todo:
            s = todo.pop()
            nxt = live[s][live[s] >= 0]
            if nxt.size == 0:
                raise ValueError(f"TokenAutomaton: state {s} is reachable from start and allows no token")
            for n in np.unique(nxt):
                if not seen[n]:
                    seen[n] = True
                    todo.append(int(n))

    # ---------------------------------------------------------------- shapes
    @property
    def vocab_size(self) -> int:
        return int(self.cls.shape[0])

    @property
    def n_states(self) -> int:
        return int(self.trans.shape[0])

    @property
    def n_classes(self) -> int:
        return int(self.trans.shape[1])

    def check_vocab(self, vocab_size: int) -> None:
        """ValueError when the automaton was compiled for another vocabulary than the model's."""
        if self.vocab_size != int(vocab_size):
            raise ValueError(f"token automaton: compiled for a vocabulary of {self.vocab_size}, the model's is {int(vocab_size)}")

    def words(self) -> np.ndarray:
        """int32 [V + S * C]: cls, then trans row by row -- the device layout."""
        return np.concatenate([self.cls, self.trans.reshape(-1)])

    def forced(self) -> np.ndarray:
        """int32 [S, 2]: row s = (t, trans[s, cls[t]]) when exactly one id t in [0, V) is allowed in state s -- the masked distribution is
        a point mass there, and a grammar-aware drafter drafts t without a model -- else (-1, -1).  From the ids per class
        and the allowed classes per state; computed once."""
        if self._forced is None:
            S, C = self.trans.shape
            per = np.bincount(self.cls, minlength=C).astype(np.int64)        # ids per class
            live = (self.trans >= 0) & (per[None, :] > 0)                    # the allowed classes that hold an id
            one = (live * per[None, :]).sum(axis=1) == 1                     # exactly one allowed id: one live class, of one id
            c = np.argmax(live, axis=1)
            first = np.full(C, -1, dtype=np.int64)
            first[self.cls[::-1]] = np.arange(self.vocab_size - 1, -1, -1)   # a class's lowest id (the last write wins)
            out = np.full((S, 2), -1, dtype=np.int32)
            out[one, 0] = first[c[one]]
            out[one, 1] = self.trans[one, c[one]]
            out.setflags(write=False)
            self._forced = out
        return self._forced

    # ---------------------------------------------------------------- the host definition of the two device ops
    def allowed(self, state: int) -> np.ndarray:
        """bool [V].  A state outside [0, S) -- the automaton has been left -- constrains nothing."""
        if not 0 <= int(state) < self.n_states:
            return np.ones(self.vocab_size, dtype=bool)
        return self.trans[int(state)][self.cls] >= 0

    def step(self, state: int, token: int) -> int:
        """The state after `token`: -1 for a token that is not allowed or not an id; a state outside [0, S) stays what it is."""
        state, token = int(state), int(token)
        if not 0 <= state < self.n_states:
            return state
        if not 0 <= token < self.vocab_size:
            return -1
        return int(self.trans[state, self.cls[token]])

    def walk(self, tokens, state: int | None = None) -> int:
        state = self.start if state is None else int(state)
        if isinstance(tokens, torch.Tensor):
            tokens = tokens.reshape(-1).tolist()
        for t in tokens:
            state = self.step(state, t)
        return state

    # ---------------------------------------------------------------- constructors
    @classmethod
    def from_token_table(cls, next_state, start: int = 0) -> "TokenAutomaton":
        """next_state [S, V], -1 for disallowed: the classes are its distinct columns."""
        table = np.asarray(next_state)
        if table.ndim != 2 or table.size == 0 or table.dtype.kind not in "iu":
            raise ValueError("TokenAutomaton.from_token_table: next_state is a non-empty integer [S, V] table")
        uniq, inverse = np.unique(table, axis=1, return_inverse=True)
        return cls(np.asarray(inverse).reshape(-1).astype(np.int32), uniq.astype(np.int32), start)

    @classmethod
    def from_byte_dfa(cls, byte_trans, accepting, token_bytes: Sequence, eos_ids, start: int = 0) -> "TokenAutomaton":
        """A byte-level DFA lifted to the vocabulary.  byte_trans [Sb, 256] (-1: a dead byte), accepting: the accepting byte states,
        token_bytes[t]: the token's bytes, or None for a special token (disallowed everywhere unless it is an EOS id; so is a token of no
        bytes, which would move nothing).  Every token is walked through its bytes from every state at once.  A transition into a byte
        state from which no accepting state is reachable is disallowed.  In an accepting state the eos_ids are allowed and lead to one
        extra absorbing state (Sb), in which only the eos_ids are allowed; nowhere else is an EOS id allowed, whatever bytes it has."""
        bt = np.asarray(byte_trans)
        if bt.ndim != 2 or bt.shape[1] != 256 or bt.shape[0] == 0 or bt.dtype.kind not in "iu":
            raise ValueError("TokenAutomaton.from_byte_dfa: byte_trans is an integer [Sb, 256] table")
        bt = bt.astype(np.int64)
        Sb, V = bt.shape[0], len(token_bytes)
        if bt.min() < -1 or bt.max() >= Sb:
            raise ValueError(f"TokenAutomaton.from_byte_dfa: byte_trans holds a state outside [-1, {Sb})")
        acc = np.zeros(Sb, dtype=bool)
        acc_ids = np.asarray(list(accepting), dtype=np.int64).reshape(-1)
        if acc_ids.size and (acc_ids.min() < 0 or acc_ids.max() >= Sb):
            raise ValueError(f"TokenAutomaton.from_byte_dfa: an accepting state outside [0, {Sb})")
        acc[acc_ids] = True
        eos = np.asarray(list(eos_ids), dtype=np.int64).reshape(-1)
        if V == 0 or (eos.size and (eos.min() < 0 or eos.max() >= V)):
            raise ValueError(f"TokenAutomaton.from_byte_dfa: an EOS id outside the vocabulary of {V}")
        if not 0 <= int(start) < Sb:
            raise ValueError(f"TokenAutomaton.from_byte_dfa: start must be a byte state in [0, {Sb})")
        # the byte states from which an accepting state is reachable: a fixed point over the edges, backwards
        live = acc.copy()
        while True:
            grown = live | (np.where(bt >= 0, live[np.maximum(bt, 0)], False)).any(axis=1)
            if (grown == live).all():
                break
            live = grown
        # the vocabulary as a padded byte matrix
        lens = np.fromiter((0 if b is None else len(b) for b in token_bytes), dtype=np.int64, count=V)
        L = int(lens.max()) if V else 0
        mat = np.zeros((V, max(L, 1)), dtype=np.int64)
        flat = np.frombuffer(b"".join(b for b in token_bytes if b), dtype=np.uint8)
        col = np.arange(max(L, 1))[None, :]
        mat[col < lens[:, None]] = flat  # row-major: each token's bytes in order
        cur = np.broadcast_to(np.arange(Sb, dtype=np.int64)[:, None], (Sb, V)).copy()
        for j in range(L):  # one gather per byte position
            has = lens > j
            nxt = np.where(cur >= 0, bt[np.maximum(cur, 0), mat[None, :, j]], -1)
            cur = np.where(has[None, :], nxt, cur)
        cur[:, lens == 0] = -1
        cur = np.where((cur >= 0) & live[np.maximum(cur, 0)], cur, -1)
        table = np.full((Sb + 1, V), -1, dtype=np.int32)
        table[:Sb] = cur
        if eos.size:
            table[:, eos] = -1
            table[np.ix_(np.flatnonzero(acc), eos)] = Sb
            table[Sb, eos] = Sb
        return cls.from_token_table(table, int(start))

    @classmethod
    def from_choices(cls, choices: Sequence[bytes], token_bytes: Sequence, eos_ids) -> "TokenAutomaton":
        """Exactly one of `choices` (non-empty byte strings), then EOS: a trie DFA over the choices, lifted by from_byte_dfa."""
        choices = [bytes(c) for c in choices]
        if not choices or any(len(c) == 0 for c in choices):
            raise ValueError("TokenAutomaton.from_choices: at least one choice, none of them empty")
        rows, accepting = [np.full(256, -1, dtype=np.int64)], set()
        for c in choices:
            s = 0
            for b in c:
                if rows[s][b] < 0:
                    rows[s][b] = len(rows)
                    rows.append(np.full(256, -1, dtype=np.int64))
                s = int(rows[s][b])
            accepting.add(s)
        return cls.from_byte_dfa(np.stack(rows), sorted(accepting), token_bytes, eos_ids, 0)


def make_token_automaton(automaton: TokenAutomaton) -> Callable:
    """The automaton as a logits processor.  Its torch body is the host definition: it walks tokens[n0:] -- the ids generated so far, n0
    being the length seen at its first call (the prompt's, since processors receive every id the model was fed, the current row's
    included) -- and masks with `allowed`.  It carries `.automaton`: where the engine can, the state lives on the device inside the
    decode step (Model.set_step_tail(token_automaton=)) and this body is never called."""
    if not isinstance(automaton, TokenAutomaton):
        raise ValueError("make_token_automaton takes a TokenAutomaton")
    seen = {"n0": None}

    def token_automaton_processor(tokens, logits: torch.Tensor) -> torch.Tensor:
        automaton.check_vocab(logits.shape[-1])
        n = len(tokens)
        if seen["n0"] is None:
            seen["n0"] = n
        ok = automaton.allowed(automaton.walk(tokens[seen["n0"]:]))
        return logits.masked_fill_(~torch.from_numpy(ok).to(logits.device), float("-inf"))

    def reset(n0: int | None = None) -> None:
        """A new request: the walk starts behind `n0` ids (None: behind whatever the next call sees)."""
        seen["n0"] = None if n0 is None else int(n0)

    token_automaton_processor.automaton, token_automaton_processor.reset = automaton, reset
    return token_automaton_processor
