"""Pure Python definitions of the automaton along a draft (include/pie_hip.h: pie_token_dfa_walk, pie_token_dfa_draft), on
the device layout -- a record (cls_off, trans_off, n_states, n_classes) over an arena of int32 words, both untrusted -- and a brute-force
forced table: what the kernels, TokenAutomaton.forced() and the engine's drafts are checked against."""
import numpy as np

from tests.token_automaton_reference import armed

MAX_DRAFT = 31


def record_of(a, cls_off: int = 0):
    """(record, arena) of a TokenAutomaton laid out at word cls_off of an arena of its own."""
    words = a.words()
    arena = np.concatenate([np.full(cls_off, -7, dtype=np.int32), words])
    return (cls_off, cls_off + a.vocab_size, a.n_states, a.n_classes), arena


def next_state(rec, tables, V: int, s: int, t: int) -> int:
    """pie_token_dfa_advance's rule for an armed record and a state inside [0, S)."""
    cls_off, trans_off, S, C = (int(v) for v in rec)
    if not 0 <= int(t) < V:
        return -1
    c = int(tables[cls_off + int(t)])
    return int(tables[trans_off + s * C + c]) if 0 <= c < C else -1


def dfa_walk(rec, s0: int, tables, V: int, tokens) -> list[int]:
    """out[0] = s0, out[i + 1] = the advance op's result for out[i] and tokens[i]."""
    out, s = [int(s0)], int(s0)
    on = armed(rec, V, tables.size)
    for t in tokens:
        if on and 0 <= s < int(rec[2]):
            s = next_state(rec, tables, V, s, t)
        out.append(s)
    return out


def dfa_draft(rec, s0: int, tables, forced, V: int, cand, cand_count: int, k: int):
    """The grammar-aware drafter's rule -> (ids, count).  forced: int32 [forced_states, 2], a hint that is re-derived from the tables."""
    cc = min(max(int(cand_count), 0), MAX_DRAFT)
    cand = [int(t) for t in cand[:cc]]
    S = int(rec[2])
    if not armed(rec, V, tables.size) or not 0 <= int(s0) < S:
        return cand[:min(cc, k)], min(cc, k)
    forced = np.asarray(forced).reshape(-1, 2)
    s, j, live, out = int(s0), 0, True, []
    while len(out) < k:
        f, fn = (int(forced[s, 0]), int(forced[s, 1])) if s < forced.shape[0] else (-1, -1)
        if 0 <= f < V and fn >= 0 and next_state(rec, tables, V, s, f) == fn:
            t, nxt = f, fn
            if live and j < cc and cand[j] == t:
                j += 1
            else:
                live = False
        elif live and j < cc and next_state(rec, tables, V, s, cand[j]) >= 0:
            t, nxt = cand[j], next_state(rec, tables, V, s, cand[j])
            j += 1
        else:
            break
        out.append(t)
        s = nxt
        if not 0 <= s < S:
            break
    return out, len(out)


def forced_brute(a) -> np.ndarray:
    """TokenAutomaton.forced() by a loop over allowed(s)."""
    out = np.full((a.n_states, 2), -1, dtype=np.int32)
    for s in range(a.n_states):
        ids = np.flatnonzero(a.allowed(s))
        if ids.size == 1:
            out[s] = (int(ids[0]), a.step(s, int(ids[0])))
    return out


def chain_automaton(V: int, run, branch_ids, tail_id: int | None = None):
    """(cls, trans) of the tests' chain: state 0 allows `branch_ids` (each leads to state 1), then state 1 + i allows run[i] alone and
    leads on; the last state allows tail_id (default run[-1]) and loops.  One class per distinct id of the run, one for the branch's ids
    (where they are not the run's), one for everything else."""
    run = [int(t) for t in run]
    tail_id = run[-1] if tail_id is None else int(tail_id)
    special = sorted(set(run) | {tail_id})
    cls = np.zeros(V, dtype=np.int32)                       # class 0: everything else
    branch_only = [t for t in branch_ids if t not in special]
    cls[branch_only] = 1
    for n, t in enumerate(special):
        cls[t] = 2 + n
    S, C = len(run) + 2, 2 + len(special)
    trans = np.full((S, C), -1, dtype=np.int32)
    trans[0, 1] = 1
    for t in branch_ids:
        if t in special:
            trans[0, cls[t]] = 1
    for i, t in enumerate(run):
        trans[1 + i, cls[t]] = 2 + i
    trans[S - 1, cls[tail_id]] = S - 1
    return cls, trans
