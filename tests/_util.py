"""Shared helpers for the parity tests."""
import numpy as np
import torch

from oracle import pie_oracle as po

TORCH_DT = {"bfloat16": torch.bfloat16, "float16": torch.float16}


def ulp_key(bits: np.ndarray) -> np.ndarray:
    """Maps 16-bit float storage bits to integers whose difference is the distance in ulps."""
    s = bits.astype(np.int32)
    return np.where(s & 0x8000, -(s & 0x7FFF), s & 0x7FFF)


def assert_bits_close(got_bits, want_bits, max_ulp=1, max_frac=0.02, what=""):
    """Results are 16-bit floats: both sides accumulate in fp32 in different orders, so an element may land on
    the neighbouring representable value.  Bound: every element within `max_ulp`, at most `max_frac` of them off."""
    got_bits, want_bits = np.asarray(got_bits).reshape(-1), np.asarray(want_bits).reshape(-1)
    assert got_bits.shape == want_bits.shape, (got_bits.shape, want_bits.shape)
    d = np.abs(ulp_key(got_bits) - ulp_key(want_bits))
    frac = float((d > 0).mean())
    assert d.max() <= max_ulp, f"{what}: max ulp distance {d.max()} > {max_ulp} (mismatch fraction {frac:.4f})"
    allowed = max(int(np.ceil(max_frac * d.size)), 1)          # tiny outputs: one neighbouring-value landing is allowed
    assert int((d > 0).sum()) <= allowed, f"{what}: {frac:.4%} of elements differ (limit {max_frac:.2%})"
    return frac


EPS = {"bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}


def assert_dot_close(got, want, dtype, max_frac=0.02, what="", mag=None):
    """Outputs of long dot products: within one T-ulp of the oracle, where the ulp is taken at max(|want|, max|want| / 128)
    (an element that cancels to nearly zero has a tiny ulp of its own, but its fp32 summation-order error is set by
    the magnitude of the terms), and at most `max_frac` of the elements differ at all.  `mag`: magnitude of an
    intermediate T-rounded value the element went through (e.g. the Linear output before its bias is added): a one-ulp
    landing there is carried into the final value unchanged."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    floor = np.abs(want).max() / 128.0
    ref = np.abs(want) if mag is None else np.maximum(np.abs(want), np.abs(np.asarray(mag, np.float64).reshape(-1)))
    tol = 2.0 * EPS[dtype] * np.maximum(ref, floor)
    bad = np.abs(got - want) > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond one ulp, worst {np.abs(got - want)[bad].max():.6g}"
    frac = float((got != want).mean())
    assert frac <= max_frac, f"{what}: {frac:.4%} of elements differ (limit {max_frac:.2%})"
    return frac


def assert_vec_close(got, want, dtype, c_max=4.0, c_rms=4.0, what=""):
    """End-to-end tolerance for activations / logits that passed through many 16-bit rounding points.
    Every op boundary rounds to T (eps = 2^-8 bf16, 2^-11 f16) and the HIP kernels accumulate in fp32 in a
    different order than the oracle, so single-ulp landings compound through the layers (measured on MI355X,
    2 layers: max error 2.5 eps*max|ref|, rms error 1.3-2.3 eps*rms(ref), see scripts/diag_parity.py).  Bound, stated in units of one ulp of the
    largest reference element:   max|got-want| <= c_max * eps * max|want|   and   rms(got-want) <= c_rms * eps * rms(want)."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    eps = EPS[dtype]
    scale = max(np.abs(want).max(), 1e-30)
    err = np.abs(got - want).max()
    assert err <= c_max * eps * scale, f"{what}: max abs err {err:.5f} > {c_max} * eps * {scale:.3f}"
    rms_w = max(np.sqrt(np.mean(want ** 2)), 1e-30)
    rms_e = np.sqrt(np.mean((got - want) ** 2))
    assert rms_e <= c_rms * eps * rms_w, f"{what}: rms err {rms_e:.6f} > {c_rms} * eps * rms(ref) {rms_w:.4f}"
    return err / (eps * scale)


def window_mask(L, o, W):
    """create_causal_mask(L, o, window_size=W) as an additive fp32 mask [L, o + L]."""
    i, j = np.arange(L)[:, None], np.arange(o + L)[None]
    return np.where((j <= o + i) & (j >= o + i - W), 0.0, -1e9).astype(np.float32)


def segment_mask(cu, N, dt):
    """The block-diagonal additive mask of vision.py:160-167 for cu_seqlens cu: 0 inside a segment, finfo(dt).min elsewhere, fp32 [N, N]."""
    from oracle import vision_oracle as vo
    m = np.full((N, N), vo.finfo_min(dt), np.float32)
    for i in range(1, len(cu)):
        m[cu[i - 1]:cu[i], cu[i - 1]:cu[i]] = 0.0
    return m


def to_dev(bits: np.ndarray, dtype: str, device="cuda") -> torch.Tensor:
    """numpy storage bits (uint16) -> device tensor of the 16-bit float dtype."""
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(device)
    return t.view(TORCH_DT[dtype])


def to_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def codes_dev(wq: np.ndarray, device="cuda") -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(wq).view(np.int32)).to(device)


# ------------------------------------------------------------------ long-context K / V histories (tests/test_gpu_long_context.py)
# With N(0,1) K and V at T = 32k the softmax is nearly uniform and the output nearly zero: dropping a row, reading one past T or
# losing one split's partial moves it by ~1/sqrt(T) of its scale, under every bound.  The recipe below makes single rows matter.
POISON = 1e4


def split_edges(T: int, splits: int) -> set:
    """Rows on both sides of every boundary attn_split (attention.hpp) cuts T attended positions into."""
    chunk = max(-(-T // splits), 32)
    return {r for b in range(chunk, T, chunk) for r in (b - 1, b)}


def marker_rows(T: int, plans=()) -> list:
    """Row 0, row T - 1, rows 8191 / 8192, and both sides of every split boundary of the plans [(attended T, splits)]."""
    rows = {0, T - 1, 8191, 8192}
    for t, s in plans:
        rows |= split_edges(t, s)
    return sorted(r for r in rows if 0 <= r < T)


def kv_history(rng, Hkv: int, T: int, D: int, dtype: str, markers, cap: int | None = None, k_scale=0.5, k_marker=4.0, v_marker=30.0,
               strong=()):
    """A synthetic K / V history [Hkv, cap, D] (fp32, representable in T): V = a per-dim mean + noise (outputs O(1)); at the marker
    rows |V| in [1, 2) x v_marker (30x the scale), of the mean's sign, so a softmax mixture of markers never cancels to a value whose
    ulp is far below its terms'; K has a larger norm there (rows 0 and T - 1, and the rows in `strong`, twice as large as the other
    markers), so softmax peaks on single rows, in an early split for some heads and the last for others.  Rows past T (up to cap) are
    poison: K = +-1e4, V = -+1e4.  Where the needles lift the softmax sum far above one ordinary row's term, a serial fp32 sum (the
    oracle's orc_sdpa) drops those terms: op-level references are float64 (sdpa_f64)."""
    cap = T if cap is None else cap
    k = rng.standard_normal((Hkv, cap, D), dtype=np.float32) * np.float32(k_scale)
    sd = np.sign(rng.standard_normal((Hkv, 1, D), dtype=np.float32))           # one sign per dim: no mixture of rows cancels to ~0
    v = sd * (np.abs(rng.standard_normal((Hkv, 1, D), dtype=np.float32)) + 0.5) + rng.standard_normal((Hkv, cap, D), dtype=np.float32) * np.float32(0.5)
    m = np.asarray(markers, np.int64)
    k[:, m] = rng.standard_normal((Hkv, m.size, D), dtype=np.float32) * np.float32(k_marker)
    for r in {0, T - 1, *strong}:
        k[:, r] *= 2.0
    v[:, m] = np.float32(v_marker) * sd * (1.0 + rng.random((Hkv, m.size, D), dtype=np.float32))
    if cap > T:
        sign = np.sign(rng.standard_normal((Hkv, cap - T, D), dtype=np.float32))
        k[:, T:], v[:, T:] = POISON * sign, -POISON * sign
    return po.round_T(k, dtype), po.round_T(v, dtype)


def plant_needles(k, q, rows, T, rep, dtype, rng):
    """Op level, where q is known: the K row of every marker aligned with the query of one head of its kv-group, scored ~ln T (row 0
    for head 0, row T - 1 for head 1 of every group: +3, so their maxima sit in the first and the last split)."""
    Hkv, _, D = k.shape
    base = np.log(T)
    for i, r in enumerate(rows):
        j = {0: 0, T - 1: 1 % rep}.get(r, i % rep)
        bump = 3.0 if r in (0, T - 1) else rng.uniform(-2.0, 1.0)
        for g in range(Hkv):
            qh = q[g * rep + j].reshape(-1)
            c = (base + bump) * np.sqrt(D) / float(qh @ qh)
            k[g, r] = po.round_T(c * qh, dtype)
    return k


def ordinary_row(k, v, T):
    """A copy of K / V whose row T - 1 is an ordinary row of the recipe (row 1's: split boundaries are never closer than 32 rows)."""
    k2, v2 = k.copy(), v.copy()
    k2[:, T - 1], v2[:, T - 1] = k[:, 1], v[:, 1]
    return k2, v2


def sdpa_f64(q, k, v, scale, T):
    """Decode attention in float64 (scores, softmax, P.V), one rounding to T by the caller: q [Hq, 1, D], k / v [Hkv, cap, D], the
    first T rows attended.  The reference at long T, where a serial fp32 sum loses the small terms next to a needle's."""
    Hq, Hkv = q.shape[0], k.shape[0]
    rep = Hq // Hkv
    out = np.empty((Hq, 1, q.shape[2]), np.float64)
    for g in range(Hkv):
        kg, vg = k[g, :T].astype(np.float64), v[g, :T].astype(np.float64)
        s = (q[g * rep:(g + 1) * rep, 0].astype(np.float64) * scale) @ kg.T
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[g * rep:(g + 1) * rep, 0] = (p @ vg) / p.sum(axis=1, keepdims=True)
    return out


# op-level long decode attention: (T, rep, D, dtype) with Hkv = 2; every pair of (rep, D, dtype) values at every T
LONG_OP_CASES = [(T, rep, D, dt) for T in (4096, 8193, 32768, 131071)
                 for rep, D, dt in ((4, 64, "bfloat16"), (4, 128, "float16"), (8, 64, "float16"), (8, 128, "bfloat16"))]
LONG_OP_HKV = 2


def long_op_case(T, rep, D, dt):
    """q [Hq, 1, D] and K / V [Hkv, cap, D] of one op-level case: the recipe with needles at the marker rows (split edges of the op's
    32-split plan, pie_sdpa_decode at T >= 2048) and poisoned capacity past T."""
    rng = np.random.default_rng(T + 10 * rep + D)
    Hq, cap = LONG_OP_HKV * rep, (T + 255) // 256 * 256 + 256
    q = po.round_T(rng.standard_normal((Hq, 1, D), dtype=np.float32), dt)
    rows = marker_rows(T, [(T, 32)])
    k, v = kv_history(rng, LONG_OP_HKV, T, D, dt, rows, cap=cap)
    for g in range(LONG_OP_HKV):                       # poison K of the sign of a query: attended, it is the maximum for that head
        k[g, T:] = POISON * np.sign(q[g * rep, 0] + 1e-30)
    return q, plant_needles(k, q, rows, T, rep, dt, rng), v
