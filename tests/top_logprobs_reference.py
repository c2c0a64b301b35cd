"""The contract of pie_top_logprobs (include/pie_hip.h) restated in numpy -- TEST INFRASTRUCTURE, shared by
tests/test_top_logprobs_host.py (CPU) and tests/test_gpu_top_logprobs.py (-m gpu).

Ids are ranked by (okey(lp[id]) descending, id ascending), okey being csrc/sampler.hpp's order-preserving 32-bit key of a float: float
order, except that +0.0 ranks above -0.0 and a NaN has the place its bits give it.  A stable argsort of the negated keys IS that order."""
from __future__ import annotations

import numpy as np

from tests import sampler_rows as sr

N_MAX = 20
SENTINEL_ID, SENTINEL_BITS = -7, 0x42F60000     # (123.0f) what the tests preset records with


def okey(lp: np.ndarray) -> np.ndarray:
    """uint32 [V]: larger float <-> larger key (sign bit set: all bits flipped; clear: the sign bit set)."""
    b = np.ascontiguousarray(lp, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def reference(lp: np.ndarray, n: int, token=None, count=None):
    """One row's record: (ids int32 [n + 1], value bits uint32 [n + 1]), or None for a negative count (the row is left alone)."""
    lp = np.ascontiguousarray(lp, np.float32).reshape(-1)
    V = lp.shape[0]
    c = n if count is None else int(count)
    if c < 0:
        return None
    m = min(c, n, V)
    order = np.argsort(-okey(lp).astype(np.int64), kind="stable")[:m]
    ids = np.full(n + 1, -1, np.int32)
    bits = np.full(n + 1, np.float32(-np.inf).view(np.uint32), np.uint32)
    ids[1:1 + m] = order
    bits[1:1 + m] = lp.view(np.uint32)[order]
    if token is not None and 0 <= int(token) < V:       # an id outside the row is never indexed: (-1, -inf)
        ids[0], bits[0] = int(token), lp.view(np.uint32)[int(token)]
    return ids, bits


def brute_force(lp: np.ndarray, m: int) -> list:
    """The first m ids of sorted((-key, id)), in plain Python."""
    key = okey(lp).tolist()
    return [i for _, i in sorted((-k, i) for i, k in enumerate(key))[:m]]


def to_map(ids: np.ndarray, bits: np.ndarray, top_k: int) -> list:
    """The engines' logprobs map of one record as its (id, value) items IN ORDER: the best top_k pairs, then the chosen token when absent."""
    vals = np.ascontiguousarray(bits, np.uint32).view(np.float32)
    out = {int(i): float(v) for i, v in zip(ids[1:1 + top_k], vals[1:1 + top_k]) if i >= 0}
    if int(ids[0]) not in out:
        out[int(ids[0])] = float(vals[0])
    return list(out.items())


def specials_row(V: int, seed: int = 0) -> np.ndarray:
    """+0.0, -0.0, +inf and a positive NaN among negative values: NaN (0x7FC00000) ranks first, then +inf, +0.0, -0.0."""
    rng = np.random.default_rng(seed + 31)
    lp = (-1.0 - rng.random(V) * 5.0).astype(np.float32)
    at = rng.choice(V, size=min(4, V), replace=False)
    vals = np.array([0x80000000, 0x00000000, 0x7FC00000, 0x7F800000], np.uint32).view(np.float32)   # -0.0, +0.0, NaN, +inf at random ids
    lp[at] = vals[:len(at)]
    return lp


def boundary_tie_row(V: int, seed: int = 0):
    """wide_tie(V) with 8 of its 20 `above` ids moved to the row's minimum: 12 ids lie above the 40-id tie class, so with n = 20 the
    20th place falls inside the class and its 8 lowest ids must win.  -> (lp, the 12 ids above, the class)."""
    row = sr.wide_tie(V, seed)
    lp = row.lp.copy()
    above = row.notes["above"]
    lp[above[:8]] = lp.min()
    return lp, above[8:], row.notes["tie"]


def family_rows(V: int, seed: int = 0) -> list:
    """(name, lp) of every sampler_rows family at V, the specials row and, where wide_tie exists, the boundary-tie row."""
    rows = [(r.name, r.lp) for r in sr.families(V, seed)] + [("specials", specials_row(V, seed))]
    if V >= 64:
        rows.append(("boundary_tie", boundary_tie_row(V, seed)[0]))
    return rows
