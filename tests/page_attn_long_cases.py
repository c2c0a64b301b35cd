"""The long-context cases of the paged verify and chunk attention kernels, shared by tests/test_gpu_page_attn_long_context.py
(the kernels against float64) and tests/test_page_attn_long_context_data.py (the data against its own float64 reference with one thing wrong).

Verify: four slots in one launch on Hkv = 2 -- 8 rows whose first context is 8193 (the longest row attends 8200 positions: 129 pages, 32 splits
of 257, so no split edge is page-aligned and every split walks 5 pages), 2 rows at 70, 1 row at 4097, an idle slot.  Chunk: LONG_PAIRS.
Both come from the short tests' builders (attn_case, i8_case, chunk_case) in their long mode."""
import functools

import numpy as np

from oracle import pie_oracle as po
from tests._util import EPS, middle_page, sdpa_f64

BF, F16 = "bfloat16", "float16"
LONG_CELLS = [(4, 128, BF), (4, 64, F16), (8, 128, F16), (5, 64, BF)]   # (rep, D, dtype): 32, 32, 64 and 40 columns in the 8-row segment
LONG_FIRST, LONG_ROWS = (8193, 70, 4097), (8, 2, 1)
LONG_HKV, LONG_BLOCKS, LONG_PAGES, LONG_SPLITS = 2, 129, 200, 32
LONG_PAIRS = [(40, 8193), (33, 8159), (70, 4097), (1, 64)]             # (rows, cached): the second pair's rows cross 8192, a page edge


# The worst row's differing share of chunk_fp32 (below) against float64 over both data sets of a cell, measured on the CPU: the fp32 arithmetic's
# own share where the kernel's exceeds the short cases' 0.03 (tests/test_gpu_page_attn_long_context.py allows twice this; the kernel: 0.0449)
CHUNK_FP32_SHARE = {(4, 64, F16): 0.0547}


def i8_page_bytes(hkv, D):
    """pie_page_i8_bytes restated (page_pool.cpp: K and V codes, 2 Hkv fp16 scales, rounded up to 256), so that the CPU checks of the data
    do not ask the library under test; tests/test_gpu_page_attn_long_context.py asserts the two agree."""
    return (2 * 64 * hkv * D + 4 * hkv + 255) // 256 * 256


def _seed(rep, D, dt):
    return D * 100 + rep * 10 + len(dt) + 29000


@functools.lru_cache(maxsize=None)
def long_attn_case(rep, D, dt):
    """(attn_case's tuple, its details) of the 16-bit long verify case."""
    from tests.test_gpu_spec_batch import attn_case
    details = []
    case = attn_case(np.random.default_rng(_seed(rep, D, dt)), D, rep, dt, LONG_FIRST, LONG_SPLITS, seg_rows=LONG_ROWS, hkv=LONG_HKV, max_blocks=LONG_BLOCKS,
                     n_pages=LONG_PAGES, long=True, details=details)
    return case, details


@functools.lru_cache(maxsize=None)
def long_i8_case(rep, D, dt):
    from tests.test_gpu_spec_batch_i8 import i8_case
    details = []
    case = i8_case(np.random.default_rng(_seed(rep, D, dt)), D, rep, dt, LONG_FIRST, seg_rows=LONG_ROWS, hkv=LONG_HKV, max_blocks=LONG_BLOCKS, n_pages=LONG_PAGES,
                   splits=LONG_SPLITS, details=details, page_bytes=i8_page_bytes(LONG_HKV, D))
    return case, details


@functools.lru_cache(maxsize=None)
def long_chunk_case(rep, D, dt, salt=0):
    from tests.test_gpu_prefill_attn_i8 import chunk_case
    details = []
    case = chunk_case(np.random.default_rng(_seed(rep, D, dt) + salt), D, rep, dt, LONG_PAIRS, long=True, details=details, page_bytes=i8_page_bytes(LONG_HKV, D))
    return case, details


def chunk_fp32(q, k8, v8, ksc, vsc, P, scale, dt):
    """k_prefill_attn_i8's arithmetic restated in fp32 on the CPU for one chunk (never the kernel itself): q [M, Hq, D] in T, codes
    [Hkv, P + M, D], scales [pages, Hkv] -> [M, Hq, D] in fp32 before the closing rounding.  Per 32-key image, in key order: the score =
    fp32(K codes . q) * (scale * log2e * k_scale[page]); base-2 online softmax with fp32 maxima, sums and rescaling; the value operand
    p * (v_scale[page] / v_scale[first page]) split into hi + lo halves of T (f16: subnormals kept, as the matrix units read them);
    O += V codes . (hi + lo) in fp32; the closing division by l / v_scale[first page]."""
    f = np.float32
    M, Hq, D = q.shape
    hkv = k8.shape[0]
    rep, out = Hq // hkv, np.empty((M, Hq, D), np.float32)
    sl2 = f(f(scale) * f(1.4426950408889634))
    t_row = np.repeat(P + np.arange(M), rep)                            # the last key a (row, head) attends
    for g in range(hkv):
        Q = q[:, g * rep:(g + 1) * rep].reshape(M * rep, D).astype(f)
        m, l, o = np.full(M * rep, -3.0e38, f), np.zeros(M * rep, f), np.zeros((M * rep, D), f)
        inv_vref = f(1.0) / vsc[0, g].astype(f)
        for tb in range(0, P + M, 32):
            n = min(32, P + M - tb)
            ksl, vs = f(sl2 * ksc[tb // 64, g].astype(f)), f(vsc[tb // 64, g].astype(f) * inv_vref)
            sc = (Q @ k8[g, tb:tb + n].astype(f).T) * ksl
            seen = (tb + np.arange(n))[None] <= t_row[:, None]
            sc = np.where(seen, sc, f(-3.0e38))
            on = seen.any(axis=1)                                       # an image behind a wave's last row is skipped
            m_new = np.where(on, np.maximum(m, sc.max(axis=1)), m)
            alpha = np.exp2(m - m_new, dtype=f)
            l, o, m = l * alpha, o * alpha[:, None], m_new
            p = np.where(seen, np.exp2(sc - m[:, None], dtype=f), f(0))
            l = l + p.sum(axis=1, dtype=f)
            va = p * vs
            hi = po.round_T(va, dt)
            lo = po.round_T(va - hi, dt)
            vcodes = v8[g, tb:tb + n].astype(f)
            o = o + hi @ vcodes + lo @ vcodes
        out[:, g * rep:(g + 1) * rep] = (o / (l * inv_vref)[:, None]).reshape(M, rep, D)
    return out


def chunk_fp32_share(rep, D, dt, salt=0):
    """The worst row's share of elements whose T rounding differs between chunk_fp32 and the float64 reference, over the long chunk case."""
    (q, slab, tables, chunks, want), details = long_chunk_case(rep, D, dt, salt)
    worst = 0.0
    for (first, M, P, s), (k, v, _, _, marks, (k8, v8, ksc, vsc)) in zip(chunks, details):
        got = po.round_T(chunk_fp32(q[first:first + M], k8, v8, ksc, vsc, P, 1.0 / np.sqrt(D), dt), dt)
        ref = po.round_T(want[first:first + M], dt)
        worst = max(worst, float((got != ref).reshape(M, -1).mean(axis=1).max()))
    return worst


def clear():
    for f in (long_attn_case, long_i8_case, long_chunk_case):
        f.cache_clear()


# ---------------------------------------------------------------------------- the float64 reference with one thing wrong
def moved(got, want, dt):
    """Whether any element of a row [Hq, D] (or of each row of a stack [n, Hq, D]) lies beyond assert_dot_close's element bound around
    the T-rounded reference, or is not finite."""
    want = po.round_T(np.asarray(want, np.float32), dt).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        got = po.round_T(np.asarray(got).astype(np.float32), dt).astype(np.float64)
        tol = 2.0 * EPS[dt] * np.maximum(np.abs(want), np.abs(want).max() / 128.0)
        bad = ~np.isfinite(got) | (np.abs(got - want) > tol)
    return bad.reshape(bad.shape[:-2] + (-1,)).any(axis=-1)


def without_each(q, k, v, scale, ctx, rows):
    """[len(rows), Hq, D]: the float64 attention of one query row q [Hq, D] over positions 0 .. ctx - 1 with one of `rows` left out, each in turn."""
    Hq, hkv = q.shape[0], k.shape[0]
    rep, rows = Hq // hkv, np.asarray(rows, np.int64)
    out = np.empty((len(rows), Hq, q.shape[1]), np.float64)
    for g in range(hkv):
        kg, vg = k[g, :ctx].astype(np.float64), v[g, :ctx].astype(np.float64)
        s = (q[g * rep:(g + 1) * rep].astype(np.float64) * scale) @ kg.T
        p = np.exp(s - s.max(axis=1, keepdims=True))
        acc, l = p @ vg, p.sum(axis=1)
        pm = p[:, rows].T                                               # [n, rep]
        out[:, g * rep:(g + 1) * rep] = (acc[None] - pm[:, :, None] * vg[rows][:, None, :]) / (l[None] - pm)[:, :, None]
    return out


def attend(q, k, v, scale, ctx, drop=None):
    """sdpa_f64 of one query row q [Hq, D] over positions 0 .. ctx - 1, without the positions drop = (lo, hi)."""
    if drop is not None:
        lo, hi = drop[0], min(drop[1], ctx)
        if lo < hi:
            k, v, ctx = np.delete(k, np.s_[lo:hi], 1), np.delete(v, np.s_[lo:hi], 1), ctx - (hi - lo)
    with np.errstate(invalid="ignore", over="ignore"):
        return sdpa_f64(q[:, None], k, v, scale, ctx)[:, 0]


def split_of(T, splits):
    """(lo, hi): the positions of the middle split of attn_split(T, splits)."""
    chunk = max(-(-T // splits), 32)
    lo = (-(-T // chunk) // 2) * chunk
    return lo, min(T, lo + chunk)


def page_of(T, splits):
    lo = 64 * middle_page(T, splits)
    return lo, min(T, lo + 64)


def other_scale(k8, v8, ksc, vsc, page, T):
    """(k, v) of a segment's codes with `page` read under the scales of the page before it."""
    use = np.repeat(np.arange(len(ksc)), 64)[:T]
    use[64 * page:64 * page + 64] = page - 1
    k = po.kv_i8_dequantize(k8[:, :T].transpose(1, 0, 2), ksc[use]).transpose(1, 0, 2)
    v = po.kv_i8_dequantize(v8[:, :T].transpose(1, 0, 2), vsc[use]).transpose(1, 0, 2)
    return k, v
