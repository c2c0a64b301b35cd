"""No device: the float64 interval reference of the prompt-attention tests against the oracle's masked softmax, and the sensitivity of the
edge-needle data -- every case of tests/prefill_attn_reference.CASES notices each of its interval edges moved by one key, in every
affected row of every head.  tests/test_gpu_prefill_attn.py runs the same inputs on the device."""
import numpy as np
import pytest

from oracle import pie_oracle as po
from tests import prefill_attn_reference as ref
from tests._util import assert_dot_close, segment_mask, window_mask
from tests.prefill_attn_reference import Case


# ------------------------------------------------------------------ the reference against oracle.sdpa under the three additive masks
def _additive_mask(c: Case):
    if c.family == "causal":
        return po.causal_mask(c.L, c.off, c.dt)
    if c.family == "window":
        return window_mask(c.L, c.off, c.W)
    return segment_mask(list(c.cu), c.L, c.dt)


SMALL = [Case("causal", "needle", "float16", 64, 2, 3, 97, 19),
         Case("window", "needle", "bfloat16", 128, 1, 4, 150, 31, 40),
         Case("segments", "needle", "bfloat16", 128, 3, 1, 200, cu=(0, 40, 44, 108, 109, 200))]


@pytest.mark.parametrize("c", SMALL, ids=ref.case_id)
def test_interval_reference_agrees_with_the_oracle(c):
    q, k, v, lo, hi, want = ref.case_data(c)
    T = c.off + c.L
    assert T <= 200
    orc = po.sdpa(q, k, v, c.D ** -0.5, _additive_mask(c), c.dt, True, T=T)
    assert_dot_close(want, orc, c.dt, max_frac=0.05, what=ref.case_id(c))


def test_beyond_tolerance_is_the_bound_of_assert_dot_close():
    want = np.array([1.0, -0.5, 1e-4, 0.0], np.float64)
    for dt in ("bfloat16", "float16"):
        step = 2.0 * ref.EPS[dt] * np.maximum(np.abs(want), 1.0 / 128.0)
        for i in range(want.size):
            for f, over in ((0.99, False), (1.01, True)):
                got = want.copy()
                got[i] += f * step[i]
                assert ref.beyond_tolerance(got, want, dt).any() == over
                if over:
                    with pytest.raises(AssertionError, match="beyond one ulp"):
                        assert_dot_close(got, want, dt, max_frac=1.0)
                else:
                    assert_dot_close(got, want, dt, max_frac=1.0)


# ------------------------------------------------------------------ the tables reach what they are meant to reach
def test_case_tables_cover_the_launcher_paths():
    causal, window, seg = ref.CAUSAL_CASES, ref.WINDOW_CASES, ref.SEGMENT_CASES
    # (one query row goes to pie_sdpa_prefill directly in the device test and proves nothing about a ratio's many-row workgroup: not counted)
    assert {(c.rep, c.D, c.dt) for c in causal if c.L > 1} == {(r, D, dt) for r in range(1, 9) for D in (64, 128) for dt in ("bfloat16", "float16")}
    assert {c.L for c in causal} == {1, 31, 32, 33, 64, 65, 96, 97, 129} and {c.off for c in causal} == {0, 19, 31, 32, 100}
    assert all(c.off > 0 for c in causal if c.L == 1) and {c.D for c in causal if c.L == 1} == {64, 128}
    assert {c.Hkv for c in causal} == {1, 2} and {65, 96, 97} <= {c.L for c in causal if ref.two_tiles(c)}
    assert {(c.rep, c.D, c.dt) for c in causal if ref.two_tiles(c)} == {(r, D, dt) for r in (1, 2, 3, 4) for D in (64, 128) for dt in ("bfloat16", "float16")}
    # the windowed form with two query tiles per workgroup: every instantiation k_prefill_attn<T, D, R, 2, false, true> of the ratios in the table
    assert {(c.rep, c.D, c.dt) for c in window if ref.two_tiles(c)} == {(r, D, dt) for r in (1, 3, 4) for D in (64, 128) for dt in ("bfloat16", "float16")}
    assert {(c.W, c.L) for c in window if c.knob == 2} == {(c.W, c.L) for c in window if c.knob == 1} == {(W, L) for W in (5, 33, 40, 64, 1000)
                                                                                                           for L in (37, 97, 150, 200)}
    assert {c.rep for c in window} == {1, 3, 4, 8} and {c.off for c in window} == {0, 70}
    assert any(c.W >= c.off + c.L for c in window)
    # rows whose leading key block is wholly masked: the workgroup starts at its first row's block, a later row's window starts a block further on
    # (not in every case: W = 64 at offset 0 keeps the windows aligned with the 32-row tiles, and 37 rows at offset 0 end in the second block)
    masked, skipping = [], []
    for c in window:
        lo, _ = ref.case_bounds(c)
        bm = 64 if ref.two_tiles(c) else 32
        if any(lo[min(r0 + bm, c.L) - 1] // 32 > lo[r0] // 32 for r0 in range(0, c.L, bm)):
            masked.append(c)
        if lo[(c.L - 1) // bm * bm] // 32 > 0:                          # b_first > 0 in the last workgroup
            skipping.append(c)
        assert c.L < 150 or c.W >= c.off + c.L or (c in masked or c.W == 64) and c in skipping, c
    for some in (masked, skipping):
        assert {(ref.two_tiles(c), c.D, c.dt) for c in some} == {(t, D, dt) for t in (False, True) for D in (64, 128) for dt in ("bfloat16", "float16")}
    # the segmented form with two query tiles: k_prefill_attn<T, D, 1, 2, true>, by the launcher's own rule at the smallest N that meets it
    assert {(c.D, c.dt) for c in seg if ref.two_tiles(c)} == {(D, dt) for D in (64, 128) for dt in ("bfloat16", "float16")}
    assert min(c.L for c in seg if ref.two_tiles(c)) == 449 and not ref.two_tiles(Case("segments", "needle", "bfloat16", 64, 64, 1, 448, cu=(0, 448)))
    assert any(1 in np.diff(c.cu) and 4 in np.diff(c.cu) for c in seg)
    st = ref.STAIRCASE_CASES
    assert {(c.family, c.data, c.D, c.knob) for c in st} == {(f, d, D, kn) for f in ("causal", "window") for d in ("stair_up", "stair_down")
                                                             for D in (64, 128) for kn in (1, 2)}
    assert all(c.rep == 4 and c.L == 200 and c.off == 31 for c in st) and {c.dt for c in st} == {"bfloat16", "float16"}
    ids = [ref.case_id(c) for c in ref.CASES + st]
    assert len(set(ids)) == len(ids)
    assert all(c.off + c.L <= 300 or c.family == "segments" and c.L <= 512 for c in ref.CASES + st)          # tiny: a float64 reference in milliseconds


def test_staircase_moves_the_maximum_in_every_block():
    """Ascending: every row's maximum over each further 32-key block exceeds the one before it by about 8 natural-log units; descending:
    the maximum is at the row's first key."""
    for c in ref.STAIRCASE_CASES:
        q, k, v, lo, hi, _ = ref.case_data(c)
        s = np.einsum("hld,td->hlt", q[:c.rep].astype(np.float64), k[0].astype(np.float64)) * c.D ** -0.5
        for r in (0, c.L // 2, c.L - 1):
            row = s[:, r, lo[r]:hi[r]]
            if c.data == "stair_down":                      # (the 0.1 noise of K can lift the second or third key over the first)
                assert (row.argmax(axis=1) <= 2).all() and (row.shape[1] < 33 or (row.max(axis=1) - row[:, 32:].max(axis=1) > 4.0).all())
                continue
            b0 = lo[r] // 32
            blocks = [row[:, max(b * 32 - lo[r], 0):(b + 1) * 32 - lo[r]].max(axis=1) for b in range(b0, (hi[r] - 1) // 32 + 1)]
            steps = np.diff(np.stack(blocks), axis=0)
            assert steps.size == 0 or steps[:-1].size == 0 or (steps[:-1] > 4.0).all(), (ref.case_id(c), r)
            assert (steps > 0).all()


# ------------------------------------------------------------------ sensitivity: what makes the device test a test of the edges
@pytest.mark.parametrize("c", ref.CASES, ids=ref.case_id)
def test_every_edge_moved_by_one_key_is_noticed(c):
    q, k, v, lo, hi, want = ref.case_data(c)
    T = c.off + c.L
    affected = 0
    for which in ref.MUTATIONS:
        lo2, hi2 = ref.mutate_bounds(lo, hi, which, T)
        rows = np.flatnonzero((lo2 != lo) | (hi2 != hi))
        if rows.size == 0:
            continue
        affected += rows.size
        got = po.round_T(ref.attn_intervals_f64(q, k, v, c.D ** -0.5, lo2, hi2, c.rep).astype(np.float32), c.dt)
        bad = ref.beyond_tolerance(got, want, c.dt)                 # [Hq, L, D]
        assert not bad[:, np.setdiff1d(np.arange(c.L), rows)].any()
        missed = np.argwhere(~bad[:, rows].any(axis=2))
        assert missed.size == 0, f"{ref.case_id(c)} {which}: (head, row) {[(int(h), int(rows[i])) for h, i in missed[:8]]} of {rows.size} rows unmoved"
    assert affected > 0
