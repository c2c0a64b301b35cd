"""-m gpu: pie_logits_count_penalty_rows against tests/count_penalty_reference.py, bit for bit on bf16 and f16: the formula on
every path of the kernel (vector slots, scalar heads and tails, misaligned rows), the rows that are skipped, and the counting rule."""
import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests._util import to_bits, to_dev
from tests.count_penalty_reference import count_penalty_reference

pytestmark = pytest.mark.gpu
PARAMS = [(0.5, 0.0), (0.0, 1.5), (-1.0, -0.25), (2.0, 2.0)]


def specials(dt: str) -> np.ndarray:
    """-inf, -0.0, +0.0, the largest finite magnitudes (f16: +-65504, which a penalty of either sign overflows)."""
    return np.array([0xFC00, 0x8000, 0x0000, 0x7BFF, 0xFBFF] if dt == "float16" else [0xFF80, 0x8000, 0x0000, 0x7F7F, 0xFF7F], np.uint16)


def block(rng, rows: int, V: int, dt: str):
    """Logits bits [rows, V] with the special values spread over every row, counts [rows, V] holding 0 (most), 1, 7 and 70000 -- each
    special value under each of them somewhere."""
    bits = po.to_bits((rng.standard_normal((rows, V)) * 6).astype(np.float32), dt)
    counts = rng.choice(np.array([0, 0, 0, 1, 7, 70000], np.int32), size=(rows, V))
    sp = specials(dt)
    for r in range(rows):
        at = rng.permutation(V)[:4 * len(sp)].reshape(4, -1)
        for j, c in enumerate((0, 1, 7, 70000)):
            bits[r, at[j]], counts[r, at[j]] = sp[:at.shape[1]], c
        bits[r, [0, V - 1]], counts[r, [0, V - 1]] = sp[0], (7, 1)       # -inf at both ends stays -inf
    return bits, counts.astype(np.int32)


def records(params, start=0, counted=None, device="cuda"):
    from proxy_inference_engine_amd import hip_ops
    return hip_ops.count_penalty_records([hip_ops.count_penalty_pack(f, p, start, counted) for f, p in params], device)


def reference(bits, counts, params, dt):
    return np.stack([count_penalty_reference(bits[r], counts[r], *params[r], dt) if params[r] != (0.0, 0.0) else bits[r] for r in range(len(params))])


def assert_bits(got, want, what):
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:6].tolist())


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("V, rows", [(37, 1), (37, 3), (37, 33), (1003, 1), (1003, 3), (1003, 33), (4096, 1), (4096, 3), (4096, 33), (128256, 3)])
def test_formula_bit_for_bit(dt, V, rows):
    """Every (f, p) pair, a (0, 0) row among them; V below one workgroup's 512 elements, odd (rows 1.. start misaligned: heads and tails),
    aligned, and the workload's own."""
    from proxy_inference_engine_amd import hip_ops
    rng = np.random.default_rng(V * 100 + rows + len(dt))
    bits, counts = block(rng, rows, V, dt)
    for shift in range(len(PARAMS) if V < 100000 else 1):
        params = [PARAMS[(r + shift) % len(PARAMS)] for r in range(rows)]
        if rows > 1:
            params[1] = (0.0, 0.0)
        logits, cnt, rec = to_dev(bits, dt), torch.from_numpy(counts).cuda(), records(params)
        out = hip_ops.logits_count_penalty_rows(logits, rec, cnt)
        assert out.data_ptr() == logits.data_ptr()
        got, want = to_bits(logits), reference(bits, counts, params, dt)
        assert not np.isnan(po.from_bits(want, dt)).any()
        assert_bits(got, want, (V, rows, shift))
        assert np.array_equal(got[counts == 0], bits[counts == 0])                      # c == 0: the stored value, whatever it is
        if rows > 1:
            assert np.array_equal(got[1], bits[1])                                      # the (0, 0) row among penalised rows
        assert np.array_equal(cnt.cpu().numpy(), counts) and np.array_equal(rec.cpu().numpy(), records(params, device=None).numpy())   # nothing counted without ctx
    assert np.isneginf(po.from_bits(got, dt)[:, [0, V - 1]]).all()                      # -inf stays -inf under every pair
    if dt == "float16":  # the overflow cases are really in the block: some +-65504 under a penalty that grows it became +-inf
        grown = (bits == 0xFBFF) & (counts > 0)
        assert grown.any()


def test_f16_overflow_under_a_negative_penalty():
    from proxy_inference_engine_amd import hip_ops
    bits = np.array([[0x7BFF, 0x7BFF, 0xFBFF, 0xFBFF, 0x7BFF, 0x0000, 0x8000]], np.uint16)
    counts = np.array([[1, 70000, 1, 0, 0, 7, 7]], np.int32)
    for f, p, want in ((-1.0, -0.25, [0x7BFF, 0x7C00, 0xFBFF, 0xFBFF, 0x7BFF]), (-2.0, -16.0, [0x7C00, 0x7C00, 0xFBFE, 0xFBFF, 0x7BFF]),
                       (2.0, 14.0, [0x7BFE, 0xFC00, 0xFC00, 0xFBFF, 0x7BFF])):
        logits = to_dev(bits, "float16")
        hip_ops.logits_count_penalty_rows(logits, records([(f, p)]), torch.from_numpy(counts).cuda())
        got = to_bits(logits)
        assert_bits(got, count_penalty_reference(bits, counts, f, p, "float16"), (f, p))
        assert got[0, :5].tolist() == want, (f, p, [hex(v) for v in got[0]])


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
def test_idle_rows_and_rows_out_of_range_are_skipped(dt):
    from proxy_inference_engine_amd import hip_ops
    V, rows = 1003, 5
    rng = np.random.default_rng(5)
    bits, counts = block(rng, rows, V, dt)
    params = [(0.5, 0.25)] * rows
    ids = torch.tensor([3, 4, 5, 6, 7, 8, 9], dtype=torch.int32, device="cuda")
    ctx = torch.tensor([11, 0, 12, 13, 14, 15, 16], dtype=torch.int32, device="cuda")     # source row 1 is idle
    out_rows = torch.tensor([0, 1, 7, -1, 4], dtype=torch.int32, device="cuda")           # 7 and -1 are out of range
    logits, cnt, rec = to_dev(bits, dt), torch.from_numpy(counts).cuda(), records(params, start=100)    # every position is a prompt's: nothing counted
    hip_ops.logits_count_penalty_rows(logits, rec, cnt, ids, ctx, out_rows)
    got = to_bits(logits)
    for r in range(rows):
        want = count_penalty_reference(bits[r], counts[r], 0.5, 0.25, dt) if r in (0, 4) else bits[r]
        assert_bits(got[r], want, r)
    assert np.array_equal(cnt.cpu().numpy(), counts) and np.array_equal(rec.cpu().numpy(), records(params, start=100, device=None).numpy())
    # without out_rows: output row s reads source row s
    logits = to_dev(bits, dt)
    hip_ops.logits_count_penalty_rows(logits, rec, cnt, ids, ctx)
    got = to_bits(logits)
    assert np.array_equal(got[1], bits[1]) and all(np.array_equal(got[r], count_penalty_reference(bits[r], counts[r], 0.5, 0.25, dt)) for r in (0, 2, 3, 4))


@pytest.mark.parametrize("V", [37, 1003, 4096])
def test_counting_rule(V):
    """A generated position increments exactly one count and is used at once; the same position again counts nothing; pos < start counts
    nothing; an input id of -1 or V is skipped; a (0, 0) row counts nothing."""
    from proxy_inference_engine_amd import hip_ops
    dt, rows, start = "bfloat16", 6, 10
    rng = np.random.default_rng(V)
    bits = po.to_bits((rng.standard_normal((rows, V)) * 4).astype(np.float32), dt)
    counts = np.zeros((rows, V), np.int32)
    counts[:, 5], counts[2, V - 1] = 2, 7
    params = [(0.5, 0.25), (1.0, 0.0), (2.0, 2.0), (0.0, 0.0), (0.5, 0.0), (0.5, 0.0)]
    #        row 0: counted     1: pos < start   2: id V - 1     3: zero record   4: id -1       5: id V
    ids = np.array([5, 5, V - 1, 5, -1, V], np.int32)
    pos = np.array([start, start - 1, start + 3, start, start, start], np.int32)
    cnt, rec = torch.from_numpy(counts).cuda(), records(params, start=start)
    t_ids, t_ctx = torch.from_numpy(ids).cuda(), torch.from_numpy(pos + 1).cuda()
    want_counts = counts.copy()
    want_counts[0, 5] += 1
    want_counts[2, V - 1] += 1
    want_rec = records(params, start=start, device=None).numpy().copy()
    want_rec[0, 3], want_rec[2, 3] = start, start + 3
    for run in range(2):   # the second launch re-runs every position: nothing is counted twice
        logits = to_dev(bits, dt)
        hip_ops.logits_count_penalty_rows(logits, rec, cnt, t_ids, t_ctx)
        assert np.array_equal(cnt.cpu().numpy(), want_counts), (run, np.argwhere(cnt.cpu().numpy() != want_counts)[:4].tolist())
        assert np.array_equal(rec.cpu().numpy(), want_rec), run
        assert_bits(to_bits(logits), reference(bits, want_counts, params, dt), run)      # the incremented count is the one used
    assert int((cnt.cpu().numpy() - counts).sum()) == 2
    # the next generated position of row 0 counts again, another id
    t_ids[0], t_ctx[0] = 9, start + 2
    hip_ops.logits_count_penalty_rows(to_dev(bits, dt), rec, cnt, t_ids, t_ctx)
    want_counts[0, 9] += 1
    assert np.array_equal(cnt.cpu().numpy(), want_counts) and int(rec[0, 3].item()) == start + 1


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("V", [1003, 4096])
def test_a_row_alone_equals_the_row_among_neighbours(dt, V):
    from proxy_inference_engine_amd import hip_ops
    rows = 33
    rng = np.random.default_rng(V + 1)
    bits, counts = block(rng, rows, V, dt)
    params = [PARAMS[r % 4] for r in range(rows)]
    ids = rng.integers(0, V, rows).astype(np.int32)
    ctx = np.full(rows, 21, np.int32)
    logits, cnt, rec = to_dev(bits, dt), torch.from_numpy(counts).cuda(), records(params, start=20)
    hip_ops.logits_count_penalty_rows(logits, rec, cnt, torch.from_numpy(ids).cuda(), torch.from_numpy(ctx).cuda())
    got, got_c = to_bits(logits), cnt.cpu().numpy()
    for r in (0, 1, 16, 32):
        one, one_c, one_r = to_dev(bits[r:r + 1], dt), torch.from_numpy(counts[r:r + 1].copy()).cuda(), records(params[r:r + 1], start=20)
        hip_ops.logits_count_penalty_rows(one, one_r, one_c, torch.from_numpy(ids[r:r + 1]).cuda(), torch.from_numpy(ctx[r:r + 1]).cuda())
        assert_bits(to_bits(one)[0], got[r], r)
        assert np.array_equal(one_c.cpu().numpy()[0], got_c[r]) and int(got_c[r, ids[r]]) == int(counts[r, ids[r]]) + 1


def test_argument_rules():
    from proxy_inference_engine_amd import _ffi, hip_ops
    import ctypes as C
    lib = _ffi.load()
    V = 64
    logits = torch.zeros((2, V), dtype=torch.bfloat16, device="cuda")
    cnt, rec = torch.zeros((2, V), dtype=torch.int32, device="cuda"), records([(0.5, 0.0)] * 2)
    ids = torch.zeros(2, dtype=torch.int32, device="cuda")
    call = lambda lg, rows, v, r, c, i, x, n: lib.pie_logits_count_penalty_rows(lg, rows, v, _ffi.PIE_BF16, r, c, i, x, None, n, None)
    L, R, K, I = _ffi.p(logits), _ffi.p(rec), _ffi.p(cnt), _ffi.p(ids)
    assert call(None, 2, V, R, K, None, None, 0) == -1 and call(L, 2, V, None, K, None, None, 0) == -1 and call(L, 2, V, R, None, None, None, 0) == -1
    assert call(L, 0, V, R, K, None, None, 0) == -1 and call(L, 2, V, R, K, None, I, 2) == -1          # ctx without ids
    assert call(L, 65536, V, R, K, None, None, 0) == -2 and call(L, 2, 0, R, K, None, None, 0) == -2
    assert call(L, 2, V, R, K, I, I, 0) == -2 and call(L, 2, V, R, K, I, I, 1) == -2                   # no source row for row 1
    assert call(L, 2, V, C.c_void_p(rec.data_ptr() + 2), K, None, None, 0) == -3 and call(L, 2, V, R, C.c_void_p(cnt.data_ptr() + 1), None, None, 0) == -3
    assert lib.pie_logits_count_penalty_rows(L, 2, V, 7, R, K, None, None, None, 0, None) == -1        # dtype
    torch.cuda.synchronize()
    assert not logits.any() and not cnt.any()
    for bad in (dict(records=rec.long()), dict(counts=cnt[:, :V - 1].contiguous()), dict(counts=cnt.long()), dict(ids=ids), dict(ctx=ids),
                dict(ids=ids, ctx=ids[:1]), dict(ids=ids, ctx=ids, out_rows=ids[:1]), dict(ids=ids.long(), ctx=ids)):
        kw = dict(records=rec, counts=cnt, ids=None, ctx=None, out_rows=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            hip_ops.logits_count_penalty_rows(logits, kw["records"], kw["counts"], kw["ids"], kw["ctx"], kw["out_rows"])
    with pytest.raises(ValueError):
        hip_ops.logits_count_penalty_rows(logits.float(), rec, cnt)
