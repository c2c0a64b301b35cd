"""The long cases of tests/test_gpu_page_attn_long_context.py must make single rows, splits, pages and scales matter (no GPU): on the float64
reference alone, each error below moves at least one query row beyond assert_dot_close's element bound -- the bound the kernels must meet.
  marker      any one marker row left out (every marker, each in turn: at least one row of its segment moves)
  successor   every row attends one position more: rows behind which another row stands see their successor (asserted for each); the last
              row of a segment reads what lies behind every context -- NaN on 16-bit pages and behind an int8 sequence's last page
              (asserted), code -128 under the page's own finite scales inside an int8 page, which is quiet: printed, not asserted (the
              rows with a successor carry this error, through the same per-row mask)
  split       the middle split of the 32-split plan of the segment's longest row left out
  page        the page in the middle of that split's page run left out
  scale       int8: that page read under the scales of the page before it
A case whose data cannot tell one of these apart would let the same mistake in a kernel pass."""
import numpy as np
import pytest

from tests import page_attn_long_cases as lc


def check_segment(what, q, k, v, c0, rows, marks, D, dt, i8=None, behind=None):
    """One segment (verify: rows at contexts c0 .. c0 + rows - 1; chunk: the same with c0 = P + 1)."""
    scale, T = 1.0 / np.sqrt(D), c0 + rows - 1
    want = [lc.attend(q[i], k, v, scale, c0 + i) for i in range(rows)]
    assert all(np.isfinite(w).all() for w in want), what
    seen = np.zeros(len(marks), bool)
    for i in range(rows):                                              # a marker: at least one row of the segment tells
        here = [j for j, m in enumerate(marks) if m < c0 + i]
        seen[here] |= lc.moved(lc.without_each(q[i], k, v, scale, c0 + i, [marks[j] for j in here]), want[i], dt)
    assert seen.all(), f"{what}: markers {[m for m, s in zip(marks, seen) if not s]} can be lost unseen"
    past = [lc.moved(lc.attend(q[i], k, v, scale, c0 + i + 1), want[i], dt) for i in range(rows - 1)]
    assert all(past), f"{what}: rows {[i for i, p in enumerate(past) if not p]} may see their successor"
    if behind is not None:                                             # the last row, one position past: what the pages hold at position T
        kx, vx = (np.concatenate([x, b[:, None].astype(x.dtype)], 1) for x, b in zip((k, v), behind))
        tells = bool(lc.moved(lc.attend(q[rows - 1], kx, vx, scale, T + 1), want[rows - 1], dt))
        print(f"{what}: the last row reading position {T} {'moves' if tells else 'does NOT move'} (finite there: {bool(np.isfinite(behind[0]).all())})")
        assert tells or np.isfinite(behind[0]).all(), f"{what}: the last row may read position {T}"   # int8: code -128 under the page's own scales is finite and quiet
    for name, (lo, hi) in (("split", lc.split_of(T, lc.LONG_SPLITS)), ("page", lc.page_of(T, lc.LONG_SPLITS))):
        if lo > 0:                                                     # (a context of one split / one page has no middle one to lose); a split: the longest row tells
            told = [bool(lc.moved(lc.attend(q[i], k, v, scale, c0 + i, drop=(lo, hi)), want[i], dt)) for i in range(rows)]
            assert told[-1] if name == "split" else any(told), f"{what}: a lost {name} {lo}..{hi}"   # a page's one marker speaks to one row's query
    if i8 is not None and T > 128:
        k2, v2 = lc.other_scale(*i8, lc.page_of(T, lc.LONG_SPLITS)[0] // 64, T)
        assert lc.moved(lc.attend(q[rows - 1], k2, v2, scale, T), want[rows - 1], dt), f"{what}: the neighbouring page's scale"


def behind_i8(i8, T, D):
    """(K, V) [Hkv, D] as an int8 kernel would read position T: code -128 under the scales of T's page, NaN scales behind the last page."""
    k8, v8, ksc, vsc = i8
    sc = [x[T // 64].astype(np.float32) if T // 64 < len(x) else np.full(x.shape[1], np.nan, np.float32) for x in (ksc, vsc)]
    return tuple(np.repeat((np.float32(-128) * x)[:, None], D, 1) for x in sc)


@pytest.mark.parametrize("rep,D,dt", lc.LONG_CELLS)
def test_long_verify_data_on_16_bit_pages_has_teeth(rep, D, dt):
    (q, pool, tables, row_seq, row_ctx, seg_first, want), details = lc.long_attn_case(rep, D, dt)
    for s, (k, v, c0, rows, marks) in enumerate(details):
        check_segment(f"rep={rep} D={D} {dt} segment {s}", q[seg_first[s]:seg_first[s] + rows], k, v, c0, rows, marks, D, dt,
                      behind=tuple(pool[tables[s, (c0 + rows - 1) // 64], w, :, (c0 + rows - 1) % 64] for w in range(2)))
        T = c0 + rows - 1                                              # behind the last row's context: NaN, through the table
        assert np.isnan(pool[tables[s, T // 64], :, :, T % 64]).all() and np.isnan(pool[tables[1, -1]]).all()
    used = np.concatenate([tables[s, :(c0 + rows + 62) // 64] for s, (c0, rows) in enumerate(zip(lc.LONG_FIRST, lc.LONG_ROWS))])
    assert len(set(used)) == len(used) and not np.array_equal(used, np.sort(used))
    assert np.isnan(pool[np.setdiff1d(np.arange(lc.LONG_PAGES), used)]).all()


@pytest.mark.parametrize("rep,D,dt", lc.LONG_CELLS)
def test_long_verify_data_on_int8_pages_has_teeth(rep, D, dt):
    (q, slab, tables, row_seq, row_ctx, seg_first, want), details = lc.long_i8_case(rep, D, dt)
    for s, (k, v, c0, rows, marks, i8) in enumerate(details):
        check_segment(f"int8 rep={rep} D={D} {dt} segment {s}", q[seg_first[s]:seg_first[s] + rows], k, v, c0, rows, marks + list(range(c0, c0 + rows - 1)), D, dt, i8=i8,
                      behind=behind_i8(i8, c0 + rows - 1, D))
        T = c0 + rows - 1
        assert (slab[tables[s, T // 64], :2 * lc.LONG_HKV * 64 * D].view(np.int8).reshape(2, lc.LONG_HKV, 64, D)[:, :, T % 64] == -128).all()
        assert np.isnan(slab[tables[1, -1], 2 * lc.LONG_HKV * 64 * D:2 * lc.LONG_HKV * 64 * D + 4 * lc.LONG_HKV].view(np.float16)).all()


@pytest.mark.parametrize("rep,D,dt", lc.LONG_CELLS)
def test_long_chunk_data_has_teeth(rep, D, dt):
    (q, slab, tables, chunks, want), details = lc.long_chunk_case(rep, D, dt)
    for (first, M, P, s), (k, v, P_, M_, marks, i8) in zip(chunks, details):
        assert (P, M) == (P_, M_)
        check_segment(f"chunk rep={rep} D={D} {dt} pair {(M, P)}", q[first:first + M], k, v, P + 1, M, marks + list(range(P + 1, P + M)), D, dt, i8=i8,
                      behind=behind_i8(i8, P + M, D))


def test_recorded_share_of_the_fp32_restatement_is_what_it_measures():
    """The chunk kernel's arithmetic restated in fp32 (never the kernel) against float64 on the long chunk data: the limit of the one
    cell that exceeds the short cases' 0.03 on the GPU is twice this share, so the recorded figure must be the measured one."""
    for (rep, D, dt), recorded in lc.CHUNK_FP32_SHARE.items():
        measured = max(lc.chunk_fp32_share(rep, D, dt, salt) for salt in (0, 2))
        print(f"fp32 restatement rep={rep} D={D} {dt}: worst row's differing share {measured:.4f} (recorded {recorded:.4f})")
        assert abs(measured - recorded) <= 0.004, (rep, D, dt, measured)   # (two of a row's 512 elements: the order of a BLAS sum)
