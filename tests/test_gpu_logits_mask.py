"""-m gpu: the token mask fused into the log-softmax's partials pass (pie_logprobs_argmax_masked).  Exact on storage bits:
the masked logits are numpy's where(bit, bits, -inf), and logprobs / token are the existing hip_ops.logprobs_argmax of those expected
logits -- the unchanged reference for the 256-tile partition and the first-argmax rule.  The one equivalence class: where the expected
logprob is a NaN (a row left without a finite logit) the result must be a NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests._util import to_bits, to_dev

pytestmark = pytest.mark.gpu
NINF = {"bfloat16": 0xFF80, "float16": 0xFC00}


def pack(bits: np.ndarray) -> np.ndarray:
    return np.packbits(np.pad(bits, (0, -bits.size % 32)), bitorder="little").view("<u4").copy()


def words_dev(words: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(words.view(np.int32).copy()).cuda()


def f32_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy().view(np.uint32).copy()


def check(base: np.ndarray, words: np.ndarray, dt: str, what):
    """One masked call against numpy + the unmasked op; returns (token, masked bits)."""
    from proxy_inference_engine_amd import hip_ops
    V = base.size
    i = np.arange(V)
    allowed = ((words[i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(bool)
    want = np.where(allowed, base, np.uint16(NINF[dt]))
    wtok, wlp = hip_ops.logprobs_argmax(to_dev(want, dt))
    logits = to_dev(base, dt)
    tok, lp = hip_ops.logprobs_argmax_masked(logits, words_dev(words))
    got = to_bits(logits)
    assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:8])
    assert int(tok.item()) == int(wtok.item()), what
    g, w = f32_bits(lp), f32_bits(wlp)
    nan = np.isnan(w.view(np.float32))
    assert np.array_equal(g[~nan], w[~nan]), (what, np.flatnonzero((g != w) & ~nan)[:8])
    assert np.isnan(g.view(np.float32)[nan]).all(), what
    return int(tok.item()), got


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("V", [1, 31, 32, 33, 255, 513, 4099, 128256])
def test_masked_tail_bit_for_bit(dt, V):
    from proxy_inference_engine_amd import hip_ops
    rng = np.random.default_rng(V + len(dt))
    base = po.to_bits((rng.standard_normal(V) * 6).astype(np.float32), dt)
    n_words = (V + 31) // 32
    raw_tok, raw_lp = hip_ops.logprobs_argmax(to_dev(base, dt))
    raw_arg = int(raw_tok.item())
    ones = np.full(n_words, 0xFFFFFFFF, np.uint32)

    # all ones: the unmasked op on every output (bits at or beyond V are set too, and ignored)
    tok, got = check(base, ones, dt, "all ones")
    assert tok == raw_arg and np.array_equal(got, base)
    lp = hip_ops.logprobs_argmax_masked(to_dev(base, dt), words_dev(ones))[1]
    assert np.array_equal(f32_bits(lp), f32_bits(raw_lp))

    def only(*ids):
        b = np.zeros(V, bool)
        b[list(ids)] = True
        return pack(b)

    assert check(base, only(0), dt, "only id 0")[0] == 0
    assert check(base, only(V - 1), dt, "only id V - 1")[0] == V - 1
    but_arg = np.ones(V, bool)
    but_arg[raw_arg] = False
    tok, got = check(base, pack(but_arg), dt, "everything but the raw argmax")   # V == 1: an all-zero mask -- token 0, NaN logprobs
    assert got[raw_arg] == NINF[dt] and (tok != raw_arg or V == 1)
    every_other = ones.copy()
    every_other[1::2] = 0
    check(base, every_other, dt, "every other word zero")
    # the final word: every bit at or beyond V set, the in-range ones clear except one; random words before it
    last = rng.integers(0, 1 << 32, n_words, dtype=np.uint64).astype(np.uint32)
    in_range = V - 32 * (n_words - 1)                                             # 1..32 bits of the final word lie below V
    keep = int(rng.integers(0, in_range))
    beyond = np.uint32(((1 << 32) - 1) & ~((1 << in_range) - 1))
    last[-1] = beyond | np.uint32(1 << keep)
    tok, got = check(base, last, dt, "final word")
    lo = 32 * (n_words - 1)
    assert [i for i in range(lo, V) if got[i] != NINF[dt]] == [lo + keep]
    if n_words == 1:
        assert tok == keep

    # ties: two equal maxima, the first masked -> the second; both allowed -> the first
    if V >= 2:
        tie = base.copy()
        a, b = sorted(rng.choice(V, 2, replace=False).tolist())
        tie[[a, b]] = po.to_bits(np.array([60.0], np.float32), dt)[0]
        first_masked = np.ones(V, bool)
        first_masked[a] = False
        assert check(tie, pack(first_masked), dt, "tie, first masked")[0] == b
        assert check(tie, ones, dt, "tie, both allowed")[0] == a
    # allowed ids that are -inf already: some of them, and all of them (the first allowed id answers, NaN logprobs)
    inf = base.copy()
    some = rng.random(V) < 0.5
    some[0] = True
    inf[some] = NINF[dt]
    allowed = rng.random(V) < 0.5
    allowed[[0, V - 1]] = True
    check(inf, pack(allowed), dt, "allowed ids already -inf")
    tok, _ = check(inf, pack(some), dt, "every allowed id already -inf")
    assert tok == 0


def test_masked_tail_refusals():
    from proxy_inference_engine_amd import _ffi, hip_ops
    V, dt = 513, "bfloat16"
    base = po.to_bits(np.linspace(-3, 3, V).astype(np.float32), dt)
    logits = to_dev(base, dt)
    words = words_dev(np.full(17, 0xFFFFFFFF, np.uint32))
    with pytest.raises(ValueError, match="ceil"):
        hip_ops.logprobs_argmax_masked(logits, words[:16])                       # 16 words cover 512 ids
    with pytest.raises(ValueError):
        hip_ops.logprobs_argmax_masked(logits, words.to(torch.int64))
    lib = _ffi.load()
    lp = torch.empty(V, dtype=torch.float32, device="cuda")
    tok = torch.empty(1, dtype=torch.int32, device="cuda")
    room = torch.zeros(4 * 18, dtype=torch.uint8, device="cuda")
    rc = lib.pie_logprobs_argmax_masked(_ffi.p(logits), V, _ffi.PIE_BF16, C.c_void_p(room.data_ptr() + 2), 17, _ffi.p(lp), _ffi.p(tok), _ffi.stream())
    assert rc == -3 and b"pie_logprobs_argmax_masked" in lib.pie_last_error()      # PIE_E_ALIGN, before any launch
    torch.cuda.synchronize()
    assert np.array_equal(to_bits(logits), base)                                   # nothing ran
