"""-m gpu: pie_logits_dry_penalty and pie_logits_dry_penalty_rows against tests/dry_penalty_reference.py, bit for bit on bf16 and
f16: window lengths around the 64 cap and up to one thread per position at 1024, alphabets from degenerate to all-distinct, periodic tails,
breakers, ids outside the vocabulary, special values, the ring's wrap, skipped rows, the zero record and the argument rules.

Bits are compared exactly.  The one exception is an element whose REFERENCE result is a NaN (a NaN logit under a penalty, +inf minus an
infinite penalty): IEEE leaves a NaN's payload open, so there both sides must be NaN; every NaN that is not penalised keeps its bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests import dry_penalty_reference as ref
from tests._util import to_bits, to_dev

pytestmark = pytest.mark.gpu
MULT, BASE = 0.8, 1.75
LENGTHS = (1, 2, 3, 63, 64, 65, 66, 130, 1023, 1024)
ALPHABETS = (1, 2, 4, "V")
POISON = -7   # what a ring slot holds where the kernel has to record the input id


def window(rng, n: int, alphabet, V: int) -> np.ndarray:
    """n ids over `alphabet` symbols spread over [0, V).  Alphabet "V": no id equals the last one (all distinct where n <= V), so the rule
    has no candidate whatever n is -- the case that must keep every bit."""
    if alphabet == "V":
        if n <= V:
            return rng.permutation(V)[:n].astype(np.int32)
        last = int(rng.integers(0, V))
        body = rng.integers(0, V - 1, n - 1)
        return np.append(body + (body >= last), last).astype(np.int32)
    symbols = rng.permutation(V)[:alphabet]
    return symbols[rng.integers(0, alphabet, n)].astype(np.int32)


def logit_bits(rng, rows: int, V: int, dt: str) -> np.ndarray:
    return po.to_bits((rng.standard_normal((rows, V)) * 6).astype(np.float32), dt)


def records(params, device="cuda"):
    """params: (multiplier, base, allowed_length, range, breakers) per row -> (records, breakers [rows, 64])"""
    from proxy_inference_engine_amd import hip_ops
    rec = hip_ops.dry_penalty_records([hip_ops.dry_penalty_pack(m, b, a, r, len(br)) for m, b, a, r, br in params], device)
    brk = torch.stack([hip_ops.dry_breaker_table(br) for *_, br in params])
    return rec, brk if device is None else brk.to(device)


def rings(feds, positions) -> np.ndarray:
    """int32 [rows, 1024]: ring[s][q & 1023] = feds[s][q] for the 1023 positions in front of positions[s]; POISON at the position itself
    (the kernel records it) and the row's last id -- a bogus candidate if it were read -- in every slot no position maps to."""
    out = np.empty((len(feds), 1024), np.int32)
    for s, (fed, pos) in enumerate(zip(feds, positions)):
        out[s] = fed[pos]
        for q in range(max(0, pos - 1023), pos):
            out[s, q & 1023] = fed[q]
        out[s, pos & 1023] = POISON
    return out


def run_rows(bits, dt, feds, positions, params, out_rows=None, ctx=None):
    """The rows op on rows whose fed ids by position are feds[s] (input id feds[s][positions[s]]); returns (bits, ring)."""
    from proxy_inference_engine_amd import hip_ops
    rec, brk = records(params)
    ring = torch.from_numpy(rings(feds, positions)).cuda()
    ids = torch.tensor([int(f[p]) for f, p in zip(feds, positions)], dtype=torch.int32, device="cuda")
    ctx = torch.tensor([p + 1 for p in positions] if ctx is None else ctx, dtype=torch.int32, device="cuda")
    logits = to_dev(bits, dt)
    out = hip_ops.logits_dry_penalty_rows(logits, rec, brk, ring, ids, ctx, None if out_rows is None else torch.tensor(out_rows, dtype=torch.int32, device="cuda"))
    assert out.data_ptr() == logits.data_ptr()
    return to_bits(logits), ring.cpu().numpy()


def run_one(bits, dt, win, m=MULT, b=BASE, a=2, breakers=()):
    from proxy_inference_engine_amd import hip_ops
    logits = to_dev(bits, dt)
    hip_ops.logits_dry_penalty(logits, torch.from_numpy(np.asarray(win, np.int32)).cuda(), m, b, a, breakers)
    return to_bits(logits)


def assert_bits(got, want, dt, what):
    nan = np.isnan(po.from_bits(want, dt))
    assert np.array_equal(got[~nan], want[~nan]), (what, np.argwhere((got != want) & ~nan)[:6].tolist())
    assert np.isnan(po.from_bits(got, dt)[nan]).all(), what


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("V, rows", [(37, 1), (37, 3), (37, 33), (1003, 3), (4096, 33), (128256, 3)])
def test_windows_bit_for_bit(dt, V, rows):
    """Every (window length, alphabet) pair, `rows` of them per launch of the rows op (the row's window is its ring at pos = n - 1) and, at
    rows == 1, through the one-vector op as well.  allowed_length alternates between 1 and 2."""
    rng = np.random.default_rng(V * 100 + rows)
    cases = [(n, alpha) for n in LENGTHS for alpha in ALPHABETS]
    for start in range(0, len(cases), rows):
        chunk = cases[start:start + rows]
        feds = [window(rng, n, alpha, V) for n, alpha in chunk]
        params = [(MULT, BASE, 1 + (start + k) % 2, 1024, ()) for k in range(len(chunk))]
        bits = logit_bits(rng, len(chunk), V, dt)
        want = np.stack([ref.apply(bits[k], dt, feds[k], MULT, BASE, params[k][2]) for k in range(len(chunk))])
        for k, (n, alpha) in enumerate(chunk):   # nothing passes vacuously
            pen = ref.penalties(feds[k], V, MULT, BASE, params[k][2])
            if alpha == "V":
                assert not pen and np.array_equal(want[k], bits[k]), (n, alpha)
            elif n >= 64:
                assert pen and not np.array_equal(want[k], bits[k]), (n, alpha)
        got, ring = run_rows(bits, dt, feds, [len(f) - 1 for f in feds], params)
        assert_bits(got, want, dt, (V, rows, start))
        for k, f in enumerate(feds):
            assert ring[k, (len(f) - 1) & 1023] == f[-1], (start, k)   # the input id reached the ring
        if rows == 1:
            assert_bits(run_one(bits[0], dt, feds[0], a=params[0][2]), want[0], dt, ("op", chunk[0]))


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("period", [3, 5])
def test_a_periodic_tail_reaches_the_cap(dt, period):
    V = 1003
    rng = np.random.default_rng(period)
    for n in (70, 200, 1024):
        win = np.tile(rng.permutation(V)[:period], n // period + 1)[:n]
        for a in (1, 2, 64):
            pen = ref.penalties(win, V, MULT, BASE, a)
            assert [L for L, _ in pen.values()] == [64]   # the two runs overlap: the match runs to the cap
            bits = logit_bits(rng, 1, V, dt)[0]
            assert_bits(run_one(bits, dt, win, a=a), ref.apply(bits, dt, win, MULT, BASE, a), dt, (n, a))
    win = np.tile(np.arange(period), 30)[:63]             # one short of the cap: allowed_length 64 penalises nothing
    bits = logit_bits(rng, 1, V, dt)[0]
    assert not ref.penalties(win, V, MULT, BASE, 64) and np.array_equal(run_one(bits, dt, win, a=64), bits)


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
def test_breakers(dt):
    """A breaker as the last id (no penalty), as c[i+1] (the position is skipped), inside a match (the match stops in front of it)."""
    V = 37
    rng = np.random.default_rng(11)
    win = np.tile(np.arange(5), 40)        # last id 4, t = 0, matches to the cap
    bits = logit_bits(rng, 1, V, dt)[0]
    assert ref.penalties(win, V, MULT, BASE, 2)[0][0] == 64
    for brk, want_L in (((4,), None), ((0,), None), ((2,), 2), ((3,), None), ((3,), 1), ((30, 31, 2, 33), 2), (tuple(range(5, 37)), 64)):
        a = 1 if want_L == 1 else 2
        pen = ref.penalties(win, V, MULT, BASE, a, brk)
        assert ({t: L for t, (L, _) in pen.items()} == ({} if want_L is None else {0: want_L})), (brk, pen)
        assert_bits(run_one(bits, dt, win, a=a, breakers=brk), ref.apply(bits, dt, win, MULT, BASE, a, brk), dt, brk)
    brk = tuple(range(100, 164))           # a full table of 64 that matches nothing
    assert_bits(run_one(bits, dt, win, breakers=brk), ref.apply(bits, dt, win, MULT, BASE, 2, brk), dt, "64 breakers")


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("V", [37, 4096])
def test_ids_outside_the_vocabulary(dt, V):
    """Ids outside [0, V) compare like any id inside a match, and are skipped -- never indexed -- as c[i+1]."""
    rng = np.random.default_rng(V)
    bits = logit_bits(rng, 1, V, dt)[0]
    for out in (-1, V, V + 5, 2 ** 31 - 1, -2 ** 31):
        tiled = np.tile(np.array([3, out, 9], np.int64), 30)
        for cut, want in ((88, set()), (89, {9}), (90, {3})):      # the window ends on 3 (t = out: skipped), on `out`, on 9
            win = tiled[:cut]
            pen = ref.penalties(win, V, MULT, BASE, 2)
            assert set(pen) == want and all(L == 64 for L, _ in pen.values()), (out, cut, pen)
            assert_bits(run_one(bits, dt, win), ref.apply(bits, dt, win, MULT, BASE, 2), dt, (out, cut))


def test_f16_penalty_beyond_the_format_is_minus_inf():
    """base 4, allowed_length 1, a match of 64: p = 0.8 * 4^63, finite in fp32; the f16 result is -inf, the bf16 one finite."""
    V, win = 37, np.full(70, 5, np.int32)
    pen = ref.penalties(win, V, MULT, 4.0, 1)
    assert pen[5][0] == 64 and np.isfinite(pen[5][1]) and pen[5][1] > 1e37
    for dt, bits_of_result in (("float16", 0xFC00), ("bfloat16", None)):
        bits = logit_bits(np.random.default_rng(1), 1, V, dt)[0]
        got = run_one(bits, dt, win, b=4.0, a=1)
        assert_bits(got, ref.apply(bits, dt, win, MULT, 4.0, 1), dt, dt)
        assert got[5] == bits_of_result if bits_of_result else np.isfinite(po.from_bits(got[5:6], dt)).all()
        assert np.array_equal(np.delete(got, 5), np.delete(bits, 5))


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
def test_special_values(dt):
    """-inf, +inf, NaN and the largest finite magnitudes at the penalised ids and beside them; -inf stays -inf; an infinite penalty (base 8
    beyond fp32) turns +inf into NaN and everything finite into -inf."""
    V = 37
    sp = [0xFC00, 0x7C00, 0x7E01, 0x7BFF, 0xFBFF] if dt == "float16" else [0xFF80, 0x7F80, 0x7FC1, 0x7F7F, 0xFF7F]
    rng = np.random.default_rng(3)
    win = rng.integers(0, 4, 1024).astype(np.int32)
    assert sorted(ref.penalties(win, V, MULT, BASE, 2)) == [0, 1, 2, 3]
    for shift in range(len(sp)):
        bits = logit_bits(rng, 1, V, dt)[0]
        for k in range(8):     # ids 0..3 are penalised, 4..7 are not
            bits[k] = sp[(k + shift) % len(sp)]
        want = ref.apply(bits, dt, win, MULT, BASE, 2)
        got = run_one(bits, dt, win)
        assert_bits(got, want, dt, shift)
        assert np.array_equal(got[4:], bits[4:])                                     # not penalised: the stored bits, NaN payload included
        assert all(got[k] == sp[0] for k in range(4) if bits[k] == sp[0])            # -inf stays -inf
    ones = np.full(70, 2, np.int32)                                                  # p = 0.8 * 8^63 = inf in fp32
    assert np.isposinf(ref.penalties(ones, V, MULT, 8.0, 1)[2][1])
    for v in sp:
        bits = logit_bits(rng, 1, V, dt)[0]
        bits[2] = v
        assert_bits(run_one(bits, dt, ones, b=8.0, a=1), ref.apply(bits, dt, ones, MULT, 8.0, 1), dt, hex(v))


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("range_", [1024, 100, 2, 1])
def test_ring_positions(dt, range_):
    """pos = 0, 1, 1022, 1023, 1024, 1500, 5000 in one launch: the ring's wrap, windows shorter than the ring, range < pos.  Slots outside
    the window hold the row's last id, which would be a candidate if it were read."""
    V = 1003
    positions = [0, 1, 1022, 1023, 1024, 1500, 5000]
    rng = np.random.default_rng(range_)
    feds = [window(rng, p + 1, 2, V) for p in positions]
    params = [(MULT, BASE, 2, range_, ())] * len(positions)
    bits = logit_bits(rng, len(positions), V, dt)
    want = np.stack([ref.apply(bits[k], dt, ref.ring_window(feds[k], p, range_), MULT, BASE, 2) for k, p in enumerate(positions)])
    if range_ >= 100:
        assert all(not np.array_equal(want[k], bits[k]) for k in range(2, len(positions)))
    else:
        assert np.array_equal(want, bits)     # (range 2 can reach L = 1 only, range 1 has n < 2)
    got, ring = run_rows(bits, dt, feds, positions, params)
    assert_bits(got, want, dt, range_)
    assert all(ring[k, p & 1023] == feds[k][p] for k, p in enumerate(positions))


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
def test_idle_rows_rows_out_of_range_and_zero_records(dt):
    V, rows = 1003, 6
    rng = np.random.default_rng(8)
    feds = [window(rng, 200, 2, V) for _ in range(7)]                   # 7 source rows
    pos = [199] * 7
    bits = logit_bits(rng, rows, V, dt)
    zero = (0.0, BASE, 2, 1024, ())
    params = [(MULT, BASE, 2, 1024, ())] * 5 + [zero]
    out_rows = [0, 1, 7, -1, 4, 5]                                      # 7 and -1 are out of range
    ctx = [200, 0, 200, 200, 200, 200, 200]                             # source row 1 is idle
    from proxy_inference_engine_amd import hip_ops
    rec, brk = records(params)
    src = [feds[i] if 0 <= i < 7 else feds[0] for i in out_rows]        # the ring of output row s holds its source row's history
    ring0 = rings(src, [199] * rows)
    ring = torch.from_numpy(ring0).cuda()
    logits = to_dev(bits, dt)
    hip_ops.logits_dry_penalty_rows(logits, rec, brk, ring, torch.tensor([int(f[199]) for f in feds], dtype=torch.int32, device="cuda"),
                                    torch.tensor(ctx, dtype=torch.int32, device="cuda"), torch.tensor(out_rows, dtype=torch.int32, device="cuda"))
    got, ring = to_bits(logits), ring.cpu().numpy()
    for s in range(rows):
        live, armed = s in (0, 4, 5), s in (0, 4)
        want = ref.apply(bits[s], dt, src[s], MULT, BASE, 2) if armed else bits[s]
        assert armed == (not np.array_equal(want, bits[s]))
        assert_bits(got[s], want, dt, s)
        want_ring = ring0[s].copy()
        if live:
            want_ring[199] = src[s][199]                                # recorded on every live row, the zero record's too
        assert np.array_equal(ring[s], want_ring), s


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
def test_a_row_alone_equals_the_row_among_neighbours(dt):
    V, rows = 4096, 33
    rng = np.random.default_rng(9)
    feds = [window(rng, 300 + 20 * s, 1 + s % 4, V) for s in range(rows)]
    pos = [len(f) - 1 for f in feds]
    params = [(MULT * (1 + s % 3), BASE, 1 + s % 3, 1024 if s % 2 else 150, tuple(int(v) for v in feds[s][:s % 3])) for s in range(rows)]
    bits = logit_bits(rng, rows, V, dt)
    got, ring = run_rows(bits, dt, feds, pos, params)
    for s in (0, 1, 16, 32):
        one, one_ring = run_rows(bits[s:s + 1], dt, feds[s:s + 1], pos[s:s + 1], params[s:s + 1])
        assert np.array_equal(one[0], got[s]) and np.array_equal(one_ring[0], ring[s]), s
        m, b, a, r, brk = params[s]
        assert_bits(got[s], ref.apply(bits[s], dt, ref.ring_window(feds[s], pos[s], r), m, b, a, brk), dt, s)


def test_record_fields_are_clamped():
    """The kernel does not trust a record's bytes: allowed_length 0 / 1000 act as 1 / 64, range 5000 as 1024, range 0 as 1, n_breakers 1000 as 64."""
    dt, V = "bfloat16", 1003
    rng = np.random.default_rng(12)
    feds = [window(rng, 1024, 2, V) for _ in range(5)]
    raw = [(0, 1024, 0), (1000, 1024, 0), (2, 5000, 0), (2, 0, 0), (2, 1024, 1000)]     # allowed_length, range, n_breakers
    act = [(1, 1024, 0), (64, 1024, 0), (2, 1024, 0), (2, 1, 0), (2, 1024, 64)]
    rec, brk = records([(MULT, BASE, 2, 1024, ())] * 5, device=None)
    brk[:] = torch.arange(2000, 2064, dtype=torch.int32)     # 64 ids no window holds
    brk[4, 63] = int(feds[4][-1])                            # the 64th breaker of row 4 is its last id: read, so the row is left alone
    for s, (a, r, nb) in enumerate(raw):
        rec[s, 2], rec[s, 3], rec[s, 4] = a, r, nb
    bits = logit_bits(rng, 5, V, dt)
    want = np.stack([ref.apply(bits[s], dt, ref.ring_window(feds[s], 1023, r), MULT, BASE, a, brk[s, :nb].tolist()) for s, (a, r, nb) in enumerate(act)])
    assert [not np.array_equal(want[s], bits[s]) for s in range(5)] == [True, False, True, False, False]
    from proxy_inference_engine_amd import hip_ops
    logits, ring = to_dev(bits, dt), torch.from_numpy(rings(feds, [1023] * 5)).cuda()
    hip_ops.logits_dry_penalty_rows(logits, rec.cuda(), brk.cuda(), ring, torch.tensor([int(f[-1]) for f in feds], dtype=torch.int32, device="cuda"),
                                    torch.full((5,), 1024, dtype=torch.int32, device="cuda"))
    assert_bits(to_bits(logits), want, dt, "clamped")


def test_argument_rules():
    from proxy_inference_engine_amd import _ffi, hip_ops
    lib = _ffi.load()
    V = 64
    logits = torch.zeros((2, V), dtype=torch.bfloat16, device="cuda")
    ids = torch.zeros(8, dtype=torch.int32, device="cuda")
    rec, brk = records([(MULT, BASE, 2, 1024, ())] * 2)
    ring = torch.zeros((2, 1024), dtype=torch.int32, device="cuda")
    L, I, R, B, G = (_ffi.p(t) for t in (logits, ids, rec, brk, ring))
    odd = lambda t, by: C.c_void_p(t.data_ptr() + by)
    one = lambda lg=L, v=V, dt=_ffi.PIE_BF16, i=I, n=8, m=MULT, b=BASE, a=2, br=B, nb=1: lib.pie_logits_dry_penalty(lg, v, dt, i, n, m, b, a, br, nb, None)
    assert one(lg=None) == -1 and one(i=None) == -1 and one(br=None) == -1 and one(br=None, nb=0, m=0.0) == 0
    assert one(n=0) == -1 and one(n=1025) == -1 and one(m=-0.5) == -1 and one(m=float("nan")) == -1 and one(m=float("inf")) == -1
    assert one(b=0.0) == -1 and one(b=-1.0) == -1 and one(b=float("inf")) == -1 and one(a=0) == -1 and one(a=65) == -1 and one(nb=65) == -1 and one(nb=-1) == -1
    assert one(v=0) == -2 and one(i=odd(ids, 2)) == -3 and one(br=odd(brk, 1)) == -3 and one(lg=odd(logits, 1)) == -3 and one(dt=7) == -1
    rows = lambda lg=L, r=2, v=V, dt=_ffi.PIE_BF16, rc=R, br=B, rg=G, i=I, x=I, o=None, n=2: lib.pie_logits_dry_penalty_rows(lg, r, v, dt, rc, br, rg, i, x, o, n, None)
    assert rows(lg=None) == -1 and rows(rc=None) == -1 and rows(br=None) == -1 and rows(rg=None) == -1 and rows(i=None) == -1 and rows(x=None) == -1
    assert rows(r=0) == -1 and rows(r=65536) == -2 and rows(v=0) == -2 and rows(n=0) == -2 and rows(n=1) == -2          # no source row for row 1
    assert rows(rc=odd(rec, 2)) == -3 and rows(br=odd(brk, 2)) == -3 and rows(rg=odd(ring, 1)) == -3 and rows(dt=7) == -1
    torch.cuda.synchronize()
    assert not logits.any() and not ring.any()
    with pytest.raises(ValueError):
        hip_ops.logits_dry_penalty(logits.float()[0], ids, MULT)
    for bad in (dict(ids=ids.long()), dict(ids=ids[:0]), dict(multiplier=-1.0), dict(base=0.0), dict(allowed_length=0), dict(allowed_length=65),
                dict(breakers=tuple(range(65)))):
        kw = dict(ids=ids, multiplier=MULT, base=BASE, allowed_length=2, breakers=())
        kw.update(bad)
        with pytest.raises(ValueError):
            hip_ops.logits_dry_penalty(logits[0], **kw)
    for bad in (dict(records=rec.long()), dict(records=rec[:1]), dict(breakers=brk[:, :32].contiguous()), dict(recent_ids=ring[:, :512].contiguous()),
                dict(ids=ids[:1]), dict(ctx=ids[:3]), dict(out_rows=ids[:1])):
        kw = dict(records=rec, breakers=brk, recent_ids=ring, ids=ids, ctx=ids, out_rows=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            hip_ops.logits_dry_penalty_rows(logits, **kw)
