"""Pure numpy / Python definitions of the token automaton's two device ops (include/pie_hip.h: pie_token_dfa_mask, pie_token_dfa_advance;
DESIGN.md 22) and a brute-force per-token byte walk: what the kernels and TokenAutomaton's vectorised constructors are checked against."""
import numpy as np


def armed(rec, V: int, tables_len: int) -> bool:
    """rec = (cls_off, trans_off, n_states, n_classes), untrusted: both of its ranges lie inside the arena."""
    cls_off, trans_off, S, C = (int(v) for v in rec)
    return S > 0 and C > 0 and cls_off >= 0 and trans_off >= 0 and cls_off + V <= tables_len and trans_off + S * C <= tables_len


def allowed_bits(rec, state: int, tables: np.ndarray, V: int) -> np.ndarray:
    """bool [V] of an armed row in a state inside [0, S): an id whose class lies outside [0, C) is disallowed."""
    cls_off, trans_off, S, C = (int(v) for v in rec)
    cls = tables[cls_off:cls_off + V].astype(np.int64)
    ok = (cls >= 0) & (cls < C)
    row = tables[trans_off + state * C:trans_off + (state + 1) * C]
    out = np.zeros(V, dtype=bool)
    out[ok] = row[cls[ok]] >= 0
    return out


def pack(bits: np.ndarray) -> np.ndarray:
    """bool [V] -> uint32 [ceil(V / 32)], token i = bit i & 31 of word i >> 5, the bits at or beyond V zero."""
    V = bits.size
    return np.packbits(np.pad(bits, (0, -V % 32)), bitorder="little").view("<u4").astype(np.uint32)


def dfa_mask(records, states, tables, V: int, masks: np.ndarray, mask_on):
    """The mask op on host arrays: masks uint32 [rows, mask_words] and mask_on (int32 [rows] or None) are the buffers as they stood
    before the launch; returns what they hold after it."""
    masks = masks.copy()
    mask_on = None if mask_on is None else mask_on.copy()
    n = (V + 31) // 32
    for r, (rec, s) in enumerate(zip(records, states)):
        if not armed(rec, V, tables.size):
            continue  # nothing of the row is written
        S = int(rec[2])
        if 0 <= int(s) < S:
            masks[r, :n] = pack(allowed_bits(rec, int(s), tables, V))
            if mask_on is not None:
                mask_on[r] = 1
        elif mask_on is not None:
            mask_on[r] = 0  # left or finished: unmasked, the words stay
        else:
            masks[r, :n] = pack(np.ones(V, dtype=bool))
    return masks, mask_on


def dfa_advance(records, states, tables, V: int, tokens) -> np.ndarray:
    """The advance op on host arrays: the states after it."""
    states = np.array(states, dtype=np.int32)
    for r, (rec, t) in enumerate(zip(records, tokens)):
        if not armed(rec, V, tables.size):
            continue
        cls_off, trans_off, S, C = (int(v) for v in rec)
        s = int(states[r])
        if not 0 <= s < S:
            continue  # stays what it is
        nxt = -1
        if 0 <= int(t) < V:
            c = int(tables[cls_off + int(t)])
            if 0 <= c < C:
                nxt = int(tables[trans_off + s * C + c])
        states[r] = nxt
    return states


def byte_walk_table(byte_trans, accepting, token_bytes, eos_ids, start: int = 0) -> np.ndarray:
    """TokenAutomaton.from_byte_dfa's [Sb + 1, V] next-state table by brute force: one Python walk per (state, token)."""
    bt = np.asarray(byte_trans)
    Sb, V = bt.shape[0], len(token_bytes)
    acc, eos = set(int(a) for a in accepting), set(int(e) for e in eos_ids)
    live = set(acc)  # the states from which an accepting state is reachable
    grew = True
    while grew:
        grew = False
        for s in range(Sb):
            if s not in live and any(int(n) in live for n in bt[s] if n >= 0):
                live.add(s)
                grew = True
    table = np.full((Sb + 1, V), -1, dtype=np.int32)
    for s in range(Sb):
        for t, b in enumerate(token_bytes):
            if t in eos:
                table[s, t] = Sb if s in acc else -1
                continue
            if not b:  # a special token, or one of no bytes
                continue
            cur = s
            for byte in b:
                cur = int(bt[cur, byte])
                if cur < 0:
                    break
            if cur >= 0 and cur in live:
                table[s, t] = cur
    for t in eos:
        table[Sb, t] = Sb
    return table
