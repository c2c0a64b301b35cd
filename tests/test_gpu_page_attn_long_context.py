"""-m gpu: the paged verify attention kernels (VALU and MFMA on 16-bit pages, MFMA on int8 pages) and the int8 chunk kernel where the
short tests never take them, each against float64, one query row at a time:
  1  one launch of an 8-row segment whose rows cross 8192 (129 pages; 32 splits of 257 positions, so every split walks 5 pages and begins
     and ends inside one) beside segments of 70 and 4097 positions and an idle slot -- 32, 1 and the library's own split count;
  2  the chunk kernel behind 8193, 8159, 4097 and 64 cached positions in one launch;
  3  every REP 1..8 with segments of 1..8 rows in one launch (every C = n * REP, 35 and 36 among them);
  4  all eight page-addressed ops on pages whose byte offsets lie on both sides of 2^31 and 2^32.
tests/test_page_attn_long_context_data.py shows on the CPU that the data of 1 and 2 tells a lost marker, split or page, a row too many
and a neighbour's scale apart under the bound used here.

Bound: assert_dot_close's element bound (one ulp of T around the float64 value; each kernel rounds once from fp32); the share of elements
that differ at all is printed per cell and held to the short tests' limits, 0.02 on 16-bit pages and 0.03 on int8 pages; one chunk cell
has a limit of its own, twice what the kernel's arithmetic restated in fp32 on the CPU gives on the same data (CHUNK_LIMIT)."""
import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests import page_attn_long_cases as lc
from tests._util import assert_dot_close, split_edges, to_bits, to_dev
from tests.test_gpu_prefill_attn_i8 import chunk_case
from tests.test_gpu_spec_batch import attn_case
from tests.test_gpu_spec_batch_i8 import i8_case

pytestmark = pytest.mark.gpu
MAX_FRAC = {"valu": 0.02, "mfma": 0.02, "i8": 0.03, "chunk": 0.03}     # the short cases' limits
KERNELS = ("valu", "mfma", "i8")
# The one cell whose limit is its own: twice the worst row's share of the kernel's arithmetic restated in fp32 on the CPU
# (page_attn_long_cases.chunk_fp32, never the kernel) against float64 on the same data -- 0.0547, the kernel itself: 0.0449.  In row 7 of
# the first chunk one head puts 0.35 of its weight on the row's own position, whose V has the other sign (the loud V of a successor), and
# 0.44 on two markers: the output cancels to 1e-4 of its terms in some dims, where an element's own f16 ulp is far below the 1e-6 of the
# terms that fp32 sums carry, so 28 of that head's 64 elements land on a neighbouring value.  The element bound, whose ulp
# has a floor at max|want| / 128 for this reason, is unchanged.  tests/test_page_attn_long_context_data.py holds the measurement.
CHUNK_LIMIT = {(4, 64, lc.F16): 2 * lc.CHUNK_FP32_SHARE[(4, 64, lc.F16)]}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.int32))).cuda()


def verify_op(kernel):
    from proxy_inference_engine_amd import hip_ops
    return {"valu": (hip_ops.paged_attn_verify, hip_ops.paged_attn_verify_splits), "mfma": (hip_ops.paged_attn_verify_mfma, hip_ops.paged_attn_verify_mfma_splits),
            "i8": (hip_ops.paged_attn_verify_i8, hip_ops.paged_attn_verify_i8_splits)}[kernel]


def rows_close(got, want, dt, what, rows=None):
    """Every row within the element bound -> the rows' differing shares."""
    assert np.isfinite(got).all(), what
    return [assert_dot_close(got[r], po.round_T(want[r], dt), dt, max_frac=1.0, what=f"{what} row {r}") for r in (range(len(want)) if rows is None else rows)]


def held(fracs, key, what, limit=None):
    limit = limit or MAX_FRAC[key]
    print(f"differing share {what}: mean {np.mean(fracs):.4f} max {np.max(fracs):.4f}")
    assert np.max(fracs) <= limit, f"{what}: {np.max(fracs):.4%} of a row's elements differ (limit {limit:.2%})"


@pytest.fixture(scope="module", autouse=True)
def cases():
    yield
    lc.clear()


# ---------------------------------------------------------------------------- 1. the verify kernels at 8200 positions
@pytest.mark.parametrize("rep,D,dt", lc.LONG_CELLS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_verify_attention_at_long_context(kernel, rep, D, dt):
    op, auto = verify_op(kernel)
    assert auto(len(lc.LONG_ROWS) + 1, lc.LONG_HKV, lc.LONG_BLOCKS) == lc.LONG_SPLITS == 32
    T = lc.LONG_FIRST[0] + lc.LONG_ROWS[0] - 1
    edges = sorted(split_edges(T, 32))                                 # tests/_util.py's restatement of attn_split (attention.hpp), the one the markers come from
    assert T == 8200 and edges[:2] == [256, 257] and len(edges) == 62 and all(e % 64 for e in edges[1::2]) and (T + 63) // 64 == lc.LONG_BLOCKS   # chunk 257, 32 active
    if kernel == "i8":
        from proxy_inference_engine_amd import _ffi
        assert lc.i8_page_bytes(lc.LONG_HKV, D) == int(_ffi.load().pie_page_i8_bytes(lc.LONG_HKV, D))
    (q, pool, tables, row_seq, row_ctx, seg_first, want), _ = lc.long_i8_case(rep, D, dt) if kernel == "i8" else lc.long_attn_case(rep, D, dt)
    slab = torch.from_numpy(pool).cuda() if kernel == "i8" else to_dev(po.to_bits(pool, dt), dt)
    args = (to_dev(po.to_bits(q, dt), dt), slab, lc.LONG_PAGES, dev(tables), dev(row_seq), dev(row_ctx), dev(seg_first), lc.LONG_HKV, 1.0 / np.sqrt(D))
    fracs = []
    for splits in (0, 1, 32):
        got = po.from_bits(to_bits(op(*args, splits=splits)), dt)
        fracs += rows_close(got, want, dt, f"{kernel} rep={rep} D={D} {dt} splits={splits}")
    held(fracs, kernel, f"long {kernel} rep={rep} D={D} {dt}")


# ---------------------------------------------------------------------------- 2. the chunk kernel behind 8193 cached positions
@pytest.mark.parametrize("rep,D,dt", lc.LONG_CELLS)
def test_prefill_attn_i8_at_long_context(knobs, rep, D, dt):
    """Measured on an MI355X (worst row's differing share / mean): rep 4 D 128 bf16 0.0283 / 0.0007, rep 4 D 64 f16 0.0449 / 0.0016,
    rep 8 D 128 f16 0.0122 / 0.0014, rep 5 D 64 bf16 0.0078 / 0.0004.  Every element of every cell is within the element bound."""
    from proxy_inference_engine_amd import hip_ops
    fracs = []
    for qt in ((None, 2) if rep <= 4 else (None,)):                    # the form of two 32-row tiles per workgroup, on data of its own
        if qt:
            knobs("prefill_qt", qt)
        (q, slab, tables, chunks, want), _ = lc.long_chunk_case(rep, D, dt, salt=qt or 0)
        got = po.from_bits(to_bits(hip_ops.prefill_attn_i8(to_dev(po.to_bits(q, dt), dt), torch.from_numpy(slab).cuda(), len(slab), torch.from_numpy(tables).cuda(),
                                                           chunks, lc.LONG_HKV, 1.0 / np.sqrt(D))), dt)
        assert not got[0].any()                                        # row 0 is outside every chunk: left zero
        fracs += rows_close(got, want, dt, f"chunk rep={rep} D={D} {dt} qt={qt}", rows=range(1, len(q)))
    held(fracs, "chunk", f"long chunk rep={rep} D={D} {dt}", limit=CHUNK_LIMIT.get((rep, D, dt)))


# ---------------------------------------------------------------------------- 3. every instantiation at short context
ALL_ROWS = (1, 2, 3, 4, 5, 6, 7, 8)
ALL_CTX = (1, 57, 63, 64, 65, 121, 127, 128)


@pytest.mark.parametrize("D,dt", [(128, lc.BF), (64, lc.F16)])
@pytest.mark.parametrize("rep", range(1, 9))
@pytest.mark.parametrize("kernel", KERNELS)
def test_verify_attention_with_every_rep_and_segment_length(kernel, rep, D, dt):
    """Eight segments of 1 .. 8 rows (36 rows: C = rep, 2 rep, .. 8 rep columns) and an idle slot in one launch."""
    op, _ = verify_op(kernel)
    rng = np.random.default_rng(D * 100 + rep * 10 + len(dt) + 2900)
    first = tuple(int(c) for c in rng.permutation(ALL_CTX))
    fracs = []
    for splits in (1, 3):
        if kernel == "i8":
            q, pool, tables, row_seq, row_ctx, seg_first, want = i8_case(rng, D, rep, dt, first, seg_rows=ALL_ROWS)
            slab = torch.from_numpy(pool).cuda()
        else:
            q, pool, tables, row_seq, row_ctx, seg_first, want = attn_case(rng, D, rep, dt, first, splits, seg_rows=ALL_ROWS)
            slab = to_dev(po.to_bits(pool, dt), dt)
        assert len(q) == 36 and len(seg_first) == 10
        got = po.from_bits(to_bits(op(to_dev(po.to_bits(q, dt), dt), slab, len(pool), dev(tables), dev(row_seq), dev(row_ctx), dev(seg_first), 2, 1.0 / np.sqrt(D),
                                      splits=splits)), dt)
        fracs += rows_close(got, want, dt, f"{kernel} rep={rep} D={D} {dt} first={first} splits={splits}")
    held(fracs, kernel, f"every length {kernel} rep={rep} D={D} {dt}")


# ---------------------------------------------------------------------------- 4. pages beyond 2^31 and 2^32 bytes
GB_HKV, GB_D, GB_REP, GB_DT = 8, 128, 2, lc.BF                         # the largest page, so the fewest pages
GB_FIRST, GB_ROWS = (128, 63), (3, 3)                                  # 3-row segments ending at 130 and 65 positions: 3 and 2 pages
GB_PAIRS = [(5, 125), (3, 62)]
NAN16 = 0x7FC0


def far_ids(page_bytes, n_pages):
    """The pages whose byte offsets are the last below and the first at or above 2^31 and 2^32, the last page -> (the tables' ids of the
    two sequences, a page that nothing uses, the untouched neighbours of the used ones and the first pages of the slab)."""
    edge = [e for b in (1 << 31, 1 << 32) for e in ((b - 1) // page_bytes, -(-b // page_bytes))]
    assert edge[0] * page_bytes < 1 << 31 <= edge[1] * page_bytes and edge[2] * page_bytes < 1 << 32 <= edge[3] * page_bytes and edge[3] < n_pages - 4
    used = [edge[3], edge[0], edge[2], edge[1], n_pages - 1]
    near = sorted({p + d for p in used for d in (-1, 1)} - set(used) - {n_pages})
    return [used[:3], used[3:]], n_pages - 3, near + [0, 1]


def slab_or_skip(need):
    free = torch.cuda.mem_get_info()[0]
    if free < 3 * need:
        pytest.skip(f"a slab of {need} bytes needs {3 * need} bytes free, {free} are")


@pytest.fixture(scope="module")
def slab16():
    page = 2 * 64 * GB_HKV * GB_D
    n_pages = (1 << 32) // (2 * page) + 8
    slab_or_skip(n_pages * page * 2)
    slab = torch.empty(n_pages * page, dtype=torch.int16, device="cuda")
    slab.fill_(NAN16)
    yield slab.view(torch.bfloat16).view(n_pages, 2, GB_HKV, 64, GB_D), n_pages
    del slab
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def slab8():
    from proxy_inference_engine_amd import _ffi, hip_ops
    pb = int(_ffi.load().pie_page_i8_bytes(GB_HKV, GB_D))
    n_pages = (1 << 32) // pb + 8
    slab_or_skip(n_pages * pb)
    slab = torch.empty(n_pages * pb, dtype=torch.int8, device="cuda")
    slab.fill_(-128)
    nan = torch.full((GB_HKV,), float("nan"), dtype=torch.float16, device="cuda")
    hip_ops.page_i8_set_scales(slab, n_pages, GB_HKV, GB_D, nan, nan)
    yield slab.view(n_pages, pb), n_pages, pb
    del slab
    torch.cuda.empty_cache()


def far_tables(tables, seqs, spare, n_blocks):
    """The case's small page ids -> the far ones: {small: far} and the tables rewritten (every other entry: the spare page)."""
    to = {int(tables[s, j]): seqs[s][j] for s in range(2) for j in range(n_blocks[s])}
    return to, np.vectorize(lambda p: to.get(int(p), spare))(tables).astype(np.int32)


def test_ops_on_16_bit_pages_beyond_4_gb(slab16):
    from proxy_inference_engine_amd import hip_ops
    slab, n_pages = slab16
    seqs, spare, near = far_ids(slab[0].numel() * 2, n_pages)
    scale, Ts = 1.0 / np.sqrt(GB_D), [c + r - 1 for c, r in zip(GB_FIRST, GB_ROWS)]
    assert seqs == [[16384, 8191, 16383], [8192, n_pages - 1]] and Ts == [130, 65]
    rng = np.random.default_rng(429)
    q, pool, tables, row_seq, row_ctx, seg_first, want = attn_case(rng, GB_D, GB_REP, GB_DT, GB_FIRST, 3, seg_rows=GB_ROWS, hkv=GB_HKV, max_blocks=3, n_pages=8)
    to, far = far_tables(tables, seqs, spare, [3, 2])
    bits = po.to_bits(pool, GB_DT)                                     # [8 pages, 2, Hkv, 64, D]
    small = to_dev(bits, GB_DT)
    table2, flat = dev(far[:2]), slab.view(-1)
    for p in range(max(Ts)):                                           # paged_kv_append, position by position (the shorter sequence idles behind its end)
        k, v = (torch.stack([small[int(tables[s, p // 64]), w, :, p % 64] if p < Ts[s] else small[0, w, :, 0] for s in range(2)]) for w in range(2))
        hip_ops.paged_kv_append(k.contiguous(), v.contiguous(), flat, n_pages, table2, dev([p if p < Ts[s] else -1 for s in range(2)]))
    for s in range(2):
        for j in range((Ts[s] + 63) // 64):
            n = min(64, Ts[s] - 64 * j)
            stored = to_bits(slab[seqs[s][j]])
            assert np.array_equal(stored[:, :, :n], bits[int(tables[s, j])][:, :, :n]), f"sequence {s} page {seqs[s][j]}: the appended rows"
            assert (stored[:, :, n:] == NAN16).all(), f"sequence {s} page {seqs[s][j]}: behind the context"
    qd = to_dev(po.to_bits(q, GB_DT), GB_DT)
    last = [seg_first[s] + GB_ROWS[s] - 1 for s in range(2)]
    got = po.from_bits(to_bits(hip_ops.paged_attention_decode(qd[last].contiguous(), flat, n_pages, table2, dev(Ts), GB_HKV, scale)), GB_DT)
    fracs = rows_close(got, want[last], GB_DT, "paged_attention_decode beyond 4 GB")
    held(fracs, "valu", "beyond 4 GB paged_attention_decode")
    for kernel in ("valu", "mfma"):
        fracs = []
        for splits in (0, 1):
            out = verify_op(kernel)[0](qd, flat, n_pages, dev(far), dev(row_seq), dev(row_ctx), dev(seg_first), GB_HKV, scale, splits=splits)
            fracs += rows_close(po.from_bits(to_bits(out), GB_DT), want, GB_DT, f"{kernel} beyond 4 GB splits={splits}")
        held(fracs, kernel, f"beyond 4 GB {kernel}")
    for p in near + [spare]:
        assert bool((slab[p].view(torch.int16) == NAN16).all()), f"page {p} no longer holds the fill"


def i8_transplant(slab8, small, tables, n_blocks, Ts, dt):
    """The case's pages onto the far ones through the ops: the scales by page_i8_set_scales, the rows by paged_kv_append_i8 from the T
    values of the codes (code * scale rounds to T within a quarter of a code, so the op's quantiser gives the code back) -> (far tables, ids)."""
    from proxy_inference_engine_amd import hip_ops
    slab, n_pages, pb = slab8
    seqs, spare, near = far_ids(pb, n_pages)
    to, far = far_tables(tables, seqs, spare, n_blocks)
    nc = 2 * GB_HKV * 64 * GB_D
    codes = small[:, :nc].view(np.int8).reshape(len(small), 2, GB_HKV, 64, GB_D)
    scales = small[:, nc:nc + 4 * GB_HKV].view(np.float16).reshape(len(small), 2, GB_HKV)
    flat = slab.view(-1)
    nan = torch.full((GB_HKV,), float("nan"), dtype=torch.float16, device="cuda")
    for big in to.values():                                            # the fill again, whatever a test before this one left on these pages
        slab[big].fill_(-128)
        hip_ops.page_i8_set_scales(flat, n_pages, GB_HKV, GB_D, nan, nan, page_ids=dev([big]))
    for sm, big in to.items():
        hip_ops.page_i8_set_scales(flat, n_pages, GB_HKV, GB_D, torch.from_numpy(scales[sm, 0].copy()).cuda(), torch.from_numpy(scales[sm, 1].copy()).cuda(), page_ids=dev([big]))
    rows = po.round_T((codes.astype(np.float32) * scales.astype(np.float32)[:, :, :, None, None]), dt)
    assert all(np.array_equal(po.kv_i8_quantize(rows[sm, w, :, :n].transpose(1, 0, 2), scales[sm, w]).transpose(1, 0, 2), codes[sm, w, :, :n])
               for s in range(2) for j, sm in enumerate(tables[s, :n_blocks[s]]) for n in [min(64, Ts[s] - 64 * j)] for w in range(2))
    rows_d, table2 = to_dev(po.to_bits(np.nan_to_num(rows), dt), dt), dev(far[:2])
    for p in range(max(Ts)):
        k, v = (torch.stack([rows_d[int(tables[s, p // 64]), w, :, p % 64] if p < Ts[s] else rows_d[0, w, :, 0] for s in range(2)]) for w in range(2))
        hip_ops.paged_kv_append_i8(k.contiguous(), v.contiguous(), flat, n_pages, table2, dev([p if p < Ts[s] else -1 for s in range(2)]))
    for s in range(2):
        for j in range(n_blocks[s]):
            n, page = min(64, Ts[s] - 64 * j), slab[seqs[s][j]].cpu().numpy()
            stored = page[:nc].reshape(2, GB_HKV, 64, GB_D)
            assert np.array_equal(stored[:, :, :n], codes[int(tables[s, j])][:, :, :n]), f"sequence {s} page {seqs[s][j]}: the appended codes"
            assert (stored[:, :, n:] == -128).all(), f"sequence {s} page {seqs[s][j]}: behind the context"
            assert np.array_equal(page[nc:nc + 4 * GB_HKV].view(np.float16).reshape(2, GB_HKV), scales[int(tables[s, j])]), f"page {seqs[s][j]}: the scales"
    return flat, n_pages, far, near + [spare]


def i8_fill_kept(slab8, pages):
    slab, n_pages, pb = slab8
    nc = 2 * GB_HKV * 64 * GB_D
    for p in pages:
        page = slab[p].cpu().numpy()
        assert (page[:nc] == -128).all() and np.isnan(page[nc:nc + 4 * GB_HKV].view(np.float16)).all(), f"page {p} no longer holds the fill"


def test_verify_and_decode_on_int8_pages_beyond_4_gb(slab8):
    from proxy_inference_engine_amd import hip_ops
    scale, Ts = 1.0 / np.sqrt(GB_D), [c + r - 1 for c, r in zip(GB_FIRST, GB_ROWS)]
    rng = np.random.default_rng(430)
    q, small, tables, row_seq, row_ctx, seg_first, want = i8_case(rng, GB_D, GB_REP, GB_DT, GB_FIRST, seg_rows=GB_ROWS, hkv=GB_HKV, max_blocks=3, n_pages=8)
    flat, n_pages, far, kept = i8_transplant(slab8, small, tables, [3, 2], Ts, GB_DT)
    qd = to_dev(po.to_bits(q, GB_DT), GB_DT)
    last = [seg_first[s] + GB_ROWS[s] - 1 for s in range(2)]
    got = po.from_bits(to_bits(hip_ops.paged_attention_decode_i8(qd[last].contiguous(), flat, n_pages, dev(far[:2]), dev(Ts), GB_HKV, scale)), GB_DT)
    held(rows_close(got, want[last], GB_DT, "paged_attention_decode_i8 beyond 4 GB"), "i8", "beyond 4 GB paged_attention_decode_i8")
    fracs = []
    for splits in (0, 1):
        out = hip_ops.paged_attn_verify_i8(qd, flat, n_pages, dev(far), dev(row_seq), dev(row_ctx), dev(seg_first), GB_HKV, scale, splits=splits)
        fracs += rows_close(po.from_bits(to_bits(out), GB_DT), want, GB_DT, f"i8 beyond 4 GB splits={splits}")
    held(fracs, "i8", "beyond 4 GB i8")
    i8_fill_kept(slab8, kept)


def test_chunks_on_int8_pages_beyond_4_gb(slab8):
    from proxy_inference_engine_amd import hip_ops
    Ts = [m + p for m, p in GB_PAIRS]
    assert Ts == [130, 65]
    q, small, tables, chunks, want = chunk_case(np.random.default_rng(431), GB_D, GB_REP, GB_DT, GB_PAIRS, hkv=GB_HKV)
    flat, n_pages, far, kept = i8_transplant(slab8, small, tables, [3, 2], Ts, GB_DT)
    got = po.from_bits(to_bits(hip_ops.prefill_attn_i8(to_dev(po.to_bits(q, GB_DT), GB_DT), flat, n_pages, dev(far), chunks, GB_HKV, 1.0 / np.sqrt(GB_D))), GB_DT)
    assert not got[0].any()
    held(rows_close(got, want, GB_DT, "chunk beyond 4 GB", rows=range(1, len(q))), "chunk", "beyond 4 GB chunk")
    i8_fill_kept(slab8, kept)
