"""The reference and the data recipes of the prompt-attention tests (k_prefill_attn, csrc/prefill_attn.hpp): tests/test_prefill_attn_host.py
checks them without a device, tests/test_gpu_prefill_attn.py runs the same inputs through the three op-level entries.

All three mask forms of the kernel are intervals: query row r attends keys [lo[r], hi[r]) of its kv head --
  causal    lo = 0,                     hi = off + r + 1   (models/base.py:18-53)
  window    lo = max(off + r - W, 0),   hi = off + r + 1   (create_causal_mask(L, off, window_size=W): W + 1 keys once the window is full)
  segments  lo / hi = the bounds of the row's segment      (the block mask of vision.py:160-167)
so one float64 function is the reference of all of them, and one data recipe (edge_needle_case) makes the two keys on either side of
both ends of every row's interval carry the row's softmax: a key wrongly admitted or dropped at an edge moves the row far beyond the
tolerance (test_prefill_attn_host.py asserts that for every case below, which is what makes the device test a test of the edges).
"""
import zlib
from typing import NamedTuple

import numpy as np

from oracle import pie_oracle as po
from tests._util import EPS, POISON


# ------------------------------------------------------------------ reference
def attn_intervals_f64(q, k, v, scale, lo, hi, rep):
    """Float64 scores, softmax and P.V: q [Hq, L, D]; k, v [Hkv, cap, D]; query row r of head h attends keys [lo[r], hi[r]) of kv head
    h // rep.  -> float64 [Hq, L, D]; the caller rounds to the dtype once."""
    Hq, L, D = q.shape
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    assert lo.shape == hi.shape == (L,) and (lo >= 0).all() and (hi > lo).all() and hi.max() <= k.shape[1]
    n = int(hi.max())
    t = np.arange(n)[None]
    mask = (t >= lo[:, None]) & (t < hi[:, None])                       # [L, n]
    out = np.empty((Hq, L, D), np.float64)
    for h in range(Hq):
        kg, vg = k[h // rep, :n].astype(np.float64), v[h // rep, :n].astype(np.float64)
        s = np.where(mask, (q[h].astype(np.float64) * float(scale)) @ kg.T, -np.inf)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[h] = (p @ vg) / p.sum(axis=1, keepdims=True)
    return out


def beyond_tolerance(got, want, dt):
    """Elementwise: |got - want| beyond the bound of tests/_util.assert_dot_close, 2 eps max(|want|, max|want| / 128)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) > 2.0 * EPS[dt] * np.maximum(np.abs(want), np.abs(want).max() / 128.0)


# ------------------------------------------------------------------ intervals
def causal_bounds(L, off):
    r = np.arange(L, dtype=np.int64)
    return np.zeros(L, np.int64), off + r + 1


def window_bounds(L, off, W):
    r = np.arange(L, dtype=np.int64)
    return np.maximum(off + r - W, 0), off + r + 1


def segment_bounds(cu):
    """hip_ops.segment_bounds on the host: cu_seqlens [0, ..., N] -> (lo, hi) [N]."""
    cu = np.asarray(cu, np.int64)
    lens = np.diff(cu)
    return np.repeat(cu[:-1], lens), np.repeat(cu[1:], lens)


MUTATIONS = ("hi+1", "hi-1", "lo-1", "lo+1")


def mutate_bounds(lo, hi, which, T):
    """One edge of every row's interval moved by one key, clipped so that the interval stays non-empty and inside the T valid keys."""
    lo, hi = lo.copy(), hi.copy()
    if which == "hi+1":
        hi = np.minimum(hi + 1, T)
    elif which == "hi-1":
        hi = np.maximum(hi - 1, lo + 1)
    elif which == "lo-1":
        lo = np.maximum(lo - 1, 0)
    elif which == "lo+1":
        lo = np.minimum(lo + 1, hi - 1)
    else:
        raise ValueError(which)
    return lo, hi


# ------------------------------------------------------------------ data
def _poison(rng, k, v, T):
    """Rows T .. cap - 1: K = +-1e4, V = -+1e4 (the sign recipe of tests/_util.kv_history)."""
    Hkv, cap, D = k.shape
    if cap > T:
        sign = np.sign(rng.standard_normal((Hkv, cap - T, D), dtype=np.float32))
        k[:, T:], v[:, T:] = POISON * sign, -POISON * sign


def edge_needle_case(rng, Hkv, rep, L, off, D, dt, lo, hi, cap):
    """q [Hkv * rep, L, D], k / v [Hkv, cap, D] (fp32, representable in dt) with T = off + L valid keys.  K and V are N(0, 1); every
    query row is 0.3 N(0, 1) plus, for each existing key t of {hi[r] - 1, hi[r], lo[r], lo[r] - 1}, the term (s / scale) k_t / |k_t|^2
    with s = ln T + 3: the row scores ~s on the two keys just inside and the two just outside its own interval and ~N(0, 1) elsewhere.
    The inside pair dominates the softmax; an outside key admitted by mistake would take about a third of the weight, an inside key
    dropped by mistake removes about half.  As r runs the edges sweep every residue modulo 32 and 64."""
    T, scale = off + L, D ** -0.5
    assert cap >= T and hi.max() <= T
    k = rng.standard_normal((Hkv, cap, D), dtype=np.float32)
    v = rng.standard_normal((Hkv, cap, D), dtype=np.float32)
    _poison(rng, k, v, T)
    k, v = po.round_T(k, dt), po.round_T(v, dt)
    q = 0.3 * rng.standard_normal((Hkv * rep, L, D))
    s = np.log(T) + 3.0
    for r in range(L):
        for t in sorted({int(hi[r]) - 1, int(hi[r]), int(lo[r]), int(lo[r]) - 1}):
            if 0 <= t < T:
                for g in range(Hkv):
                    kt = k[g, t].astype(np.float64)
                    q[g * rep:(g + 1) * rep, r] += (s / scale) * kt / float(kt @ kt)
    return po.round_T(q.astype(np.float32), dt), k, v


STAIR_DELTA = 0.25          # natural-log units of score per key: 8 per 32-key block


def staircase_case(rng, Hkv, rep, L, off, D, dt, cap, descending):
    """K[t] = 0.1 noise + sign (delta t / (scale |u|^2)) u with a +-1 vector u, every query 0.3 noise + u: the score moves by ~delta per key
    (by a per-row factor 1 + O(0.3 / sqrt(D))), 8 natural-log units per 32-key block.  Ascending, the running maximum moves in every key
    block, so l_run and every oacc[dt] are rescaled in every block; descending, the maximum sits at the row's first key and the later
    terms fall towards zero (e^-58 at 231 keys)."""
    T, scale = off + L, D ** -0.5
    u = np.sign(rng.standard_normal(D)).astype(np.float32)
    step = STAIR_DELTA / (scale * D) * (-1.0 if descending else 1.0)
    k = 0.1 * rng.standard_normal((Hkv, cap, D), dtype=np.float32) + (step * np.arange(cap, dtype=np.float32))[None, :, None] * u
    v = rng.standard_normal((Hkv, cap, D), dtype=np.float32)
    _poison(rng, k, v, T)
    q = 0.3 * rng.standard_normal((Hkv * rep, L, D), dtype=np.float32) + u
    return po.round_T(q, dt), po.round_T(k, dt), po.round_T(v, dt)


# ------------------------------------------------------------------ case tables
class Case(NamedTuple):
    family: str             # "causal" | "window" | "segments"
    data: str               # "needle" | "stair_up" | "stair_down"
    dt: str
    D: int
    Hkv: int
    rep: int
    L: int
    off: int = 0
    W: int = 0              # window family
    cu: tuple = ()          # segments family: cu_seqlens
    knob: int = 0           # prefill_qt: 1 / 2 query tiles per workgroup (2 takes effect for rep <= 4 and L > 32); 0 = the launcher's own rule
    draw: int = 0           # which draw of the data: the needles' scores on each other's keys are ~N(0, s^2 / D), so about one (head, edge)
                            # in a thousand draws an outside key too weak to be noticed -- the sensitivity check then asks for another draw


def case_id(c: Case) -> str:
    tag = {"causal": f"L{c.L}-off{c.off}", "window": f"L{c.L}-off{c.off}-W{c.W}", "segments": f"N{c.L}-{len(c.cu) - 1}seg"}[c.family]
    return f"{c.family}-{c.data}-{c.dt}-D{c.D}-{c.Hkv}x{c.rep}-{tag}-qt{c.knob}" + (f"-draw{c.draw}" if c.draw else "")


_DTS = ("bfloat16", "float16")


def _causal_cases():
    """Every ratio 1..8 x both head dims x both dtypes once (32 cases) with L >= 2, L and off drawn by a seeded sweep in which every value
    occurs, Hkv and the knob alternating; plus, with two query tiles per workgroup (rep <= 4), the L next to a tile boundary: 65 and 96
    (the last workgroup's second tile is wholly padding), 97 (one live row in it), 129 (the same one tile pair later), until the two-tile
    form has met every (rep <= 4, D, dtype); plus L = 1 at an offset (one live row, 31 rows of padding), which the device test sends to
    pie_sdpa_prefill itself: hip_ops.scaled_dot_product_attention gives one query row to the decode attention."""
    rng = np.random.default_rng(20250)
    Ls, offs = (31, 32, 33, 64, 65, 96, 97, 129), (0, 19, 31, 32, 100)
    combos = [(rep, D, dt) for rep in range(1, 9) for D in (64, 128) for dt in _DTS]
    li, oi = rng.permutation(len(combos)) % len(Ls), rng.permutation(len(combos)) % len(offs)
    out = [Case("causal", "needle", dt, D, 1 + (i + rep) % 2, rep, Ls[li[i]], offs[oi[i]], knob=1 + (i // 2 + rep) % 2)
           for i, (rep, D, dt) in enumerate(combos)]
    edge = [(65, 1, 64, "bfloat16", 0), (65, 4, 128, "float16", 31), (96, 2, 128, "bfloat16", 32), (96, 3, 64, "float16", 0),
            (97, 4, 64, "bfloat16", 19), (97, 1, 128, "float16", 100), (97, 3, 128, "bfloat16", 0), (129, 2, 64, "float16", 31),
            (129, 4, 128, "bfloat16", 100), (64, 4, 64, "float16", 32), (33, 2, 128, "float16", 0), (65, 1, 128, "bfloat16", 19),
            (96, 2, 64, "bfloat16", 100), (97, 3, 128, "float16", 32)]
    out += [Case("causal", "needle", dt, D, 1 + i % 2, rep, L, off, knob=2) for i, (L, rep, D, dt, off) in enumerate(edge)]
    one = [(2, 64, "float16", 19), (4, 128, "float16", 31), (5, 64, "bfloat16", 100), (6, 128, "float16", 32), (1, 128, "bfloat16", 19),
           (8, 64, "bfloat16", 100)]
    out += [Case("causal", "needle", dt, D, 1 + i % 2, rep, 1, off, knob=1 + i % 2) for i, (rep, D, dt, off) in enumerate(one)]
    return out


def _window_cases():
    """Every (W, L) pair under both knob values; rep / D / dtype / off cycle so that the two-tile form (knob 2, rep <= 4) meets every
    (rep, D, dtype) of {1, 3, 4} x {64, 128} x {bf16, f16}.  W = 1000 clips nothing (the causal mask through the windowed form)."""
    combos = [(rep, D, dt) for rep in (1, 3, 4) for D in (64, 128) for dt in _DTS]
    out, i = [], 0
    for W in (5, 33, 40, 64, 1000):
        for L in (37, 97, 150, 200):
            rep, D, dt = combos[i % len(combos)]
            out.append(Case("window", "needle", dt, D, 1 + i % 2, rep, L, (0, 70)[(i + i // 4) % 2], W, knob=2))
            rep1, D1, dt1 = (8, (64, 128)[i % 2], _DTS[(i // 2) % 2]) if i % 3 == 0 else combos[(i + 5) % len(combos)]
            out.append(Case("window", "needle", dt1, D1, 1 + (i + 1) % 2, rep1, L, (0, 70)[(i + 1 + i // 4) % 2], W, knob=1,
                            draw=int((W, L) == (33, 200))))          # (the first draw left one row's lower edge unnoticed)
            i += 1
    return out


# segments: ragged lists with 1-row and 4-row segments and segments that straddle the 32- and 64-row tiles (tests/test_gpu_vision.py's, with
# needle data); then the two-tile form, which segment_attn_launch_d picks by ceil(N / 64) * H >= 512 and which reads no knob: H = 64 and
# N = 449 is the smallest N that satisfies it at 64 heads (8 workgroups per head, the last with one live row and a wholly padding
# second tile), N = 512 fills every tile
_RAGGED_A = (0, 40, 44, 108, 109, 300)
_RAGGED_B = (0, 16, 48, 112, 176, 180, 436, 500)
_TWO_TILE_449 = (0, 1, 5, 70, 200, 330, 449)
_TWO_TILE_512 = (0, 60, 64, 65, 200, 383, 512)
SEGMENT_TWO_TILE_RULE = 512   # ceil(N / 64) * H at and above which segment_attn_launch_d runs two query tiles per workgroup


def _segment_cases():
    out = [Case("segments", "needle", dt, D, H, 1, cu[-1], cu=cu) for dt in _DTS for H, D, cu in ((3, 128, _RAGGED_A), (4, 64, _RAGGED_B))]
    out += [Case("segments", "needle", dt, D, 64, 1, cu[-1], cu=cu, draw=draw)          # (draw 1: the first left one head's segment end unnoticed)
            for dt, D, cu, draw in (("bfloat16", 64, _TWO_TILE_449, 1), ("float16", 64, _TWO_TILE_512, 0), ("float16", 128, _TWO_TILE_449, 0),
                                    ("bfloat16", 128, _TWO_TILE_512, 0))]
    return out


def _staircase_cases():
    """Ascending and descending, causal and windowed (W = 40: a window longer than a key block), both head dims, rep 4 under both knob
    values, L = 200 at offset 31 (8 key blocks); the dtypes alternate."""
    out, i = [], 0
    for family, W in (("causal", 0), ("window", 40)):
        for data in ("stair_up", "stair_down"):
            for D in (64, 128):
                for knob in (1, 2):
                    out.append(Case(family, data, _DTS[(i // 2 + i) % 2], D, 2, 4, 200, 31, W, knob=knob))
                    i += 1
    return out


CAUSAL_CASES = _causal_cases()
WINDOW_CASES = _window_cases()
SEGMENT_CASES = _segment_cases()
STAIRCASE_CASES = _staircase_cases()
CASES = CAUSAL_CASES + WINDOW_CASES + SEGMENT_CASES          # the edge-needle cases: the sensitivity check covers every one of them


def two_tiles(c: Case) -> bool:
    """Whether the launcher runs the case with two 32-row query tiles per workgroup (prefill_attn_launch_d / segment_attn_launch_d)."""
    if c.family == "segments":
        return c.L > 32 and -(-c.L // 64) * c.Hkv >= SEGMENT_TWO_TILE_RULE
    return c.rep <= 4 and c.L > 32 and (c.knob == 2 if c.knob else -(-c.L // 64) * c.Hkv >= 256)


def case_bounds(c: Case):
    if c.family == "causal":
        return causal_bounds(c.L, c.off)
    if c.family == "window":
        return window_bounds(c.L, c.off, c.W)
    return segment_bounds(c.cu)


def case_data(c: Case):
    """(q [Hq, L, D], k, v [Hkv, cap, D], lo, hi, want [Hq, L, D]) of one case: fp32 arrays representable in c.dt, the float64 reference
    rounded once.  Deterministic in the case (seeded by its id) and read-only."""
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    lo, hi = case_bounds(c)
    T = c.off + c.L
    cap = T if c.family == "segments" else T + 40          # pie_sdpa_segments takes no capacity: k, v are [H, N, D]
    if c.data == "needle":
        q, k, v = edge_needle_case(rng, c.Hkv, c.rep, c.L, c.off, c.D, c.dt, lo, hi, cap)
    else:
        q, k, v = staircase_case(rng, c.Hkv, c.rep, c.L, c.off, c.D, c.dt, cap, c.data == "stair_down")
    want = po.round_T(attn_intervals_f64(q, k, v, c.D ** -0.5, lo, hi, c.rep).astype(np.float32), c.dt)
    for a in (q, k, v, lo, hi, want):
        a.setflags(write=False)
    return q, k, v, lo, hi, want
