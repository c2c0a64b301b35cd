"""CPU: the host side of the step tail's token mask and logit bias -- the packed-mask layout, the two processors' torch
bodies against numpy, the four C entry points' refusals before any launch, the engine's wider routing predicate (with fused_tail_spec
unchanged on its own table) and the processor order make_processors builds."""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def np_pack(bits: np.ndarray) -> np.ndarray:
    """The layout, written out: token i is bit i & 31 of word i >> 5."""
    words = np.zeros((bits.size + 31) // 32, np.uint32)
    for i in np.flatnonzero(bits):
        words[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return words


def test_pack_token_mask_layout_and_refusals():
    from proxy_inference_engine_amd.hip_ops import pack_token_mask
    rng = np.random.default_rng(0)
    for V in (1, 31, 32, 33, 255, 513, 4099):
        bits = rng.random(V) < 0.4
        bits[V - 1] = True
        words = pack_token_mask(torch.from_numpy(bits), V)
        assert words.dtype == torch.int32 and words.shape == ((V + 31) // 32,) and not words.is_cuda
        assert np.array_equal(words.numpy().view(np.uint32), np_pack(bits)), V
        ids = np.flatnonzero(bits)
        assert torch.equal(pack_token_mask(ids.tolist(), V), words) and torch.equal(pack_token_mask(torch.from_numpy(ids), V), words)
        assert torch.equal(pack_token_mask(iter(ids.tolist() + ids.tolist()), V), words)     # an id listed twice is one bit
    assert pack_token_mask([0], 64).tolist() == [1, 0] and pack_token_mask([31], 64).tolist() == [-(1 << 31), 0]   # bit 31 is the int32's sign
    assert pack_token_mask([32, 63], 64).tolist() == [0, 1 - (1 << 31)]
    for bad, V in (([], 64), ([64], 64), ([-1], 64), (torch.zeros(64, dtype=torch.bool), 64), (torch.ones(63, dtype=torch.bool), 64), ([0], 0)):
        with pytest.raises(ValueError):
            pack_token_mask(bad, V)


def test_packed_and_unpacked_masks_round_trip_and_refuse_empty_ones():
    from proxy_inference_engine_amd.logits_processors import packed_token_mask, unpack_token_mask
    rng = np.random.default_rng(1)
    for V in (1, 33, 513):
        bits = rng.random(V) < 0.5
        bits[0] = True
        words = packed_token_mask(torch.from_numpy(bits), V)
        assert np.array_equal(unpack_token_mask(words, V).numpy(), bits)
        assert torch.equal(packed_token_mask(words, V), words)                             # packed words pass through
        assert torch.equal(packed_token_mask(np.flatnonzero(bits).tolist(), V), words)
    longer = torch.tensor([0, 5, 9], dtype=torch.int32)
    assert packed_token_mask(longer, 64).tolist() == [0, 5]                                # words beyond the vocabulary are dropped
    with pytest.raises(ValueError):
        packed_token_mask(torch.tensor([7], dtype=torch.int32), 33)                        # too few words
    with pytest.raises(ValueError):
        packed_token_mask(torch.tensor([0, -2], dtype=torch.int32), 33)                    # only bits at or beyond V are set
    assert packed_token_mask(torch.tensor([0, -1], dtype=torch.int32), 33).tolist() == [0, -1]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_processor_bodies_against_numpy(dt):
    from oracle import pie_oracle as po
    from proxy_inference_engine_amd.logits_processors import make_logit_bias, make_token_mask
    name = "bfloat16" if dt == torch.bfloat16 else "float16"
    rng = np.random.default_rng(2)
    V = 77
    base = po.to_bits((rng.standard_normal(V) * 6).astype(np.float32), name)
    as_t = lambda bits: torch.from_numpy(bits.view(np.int16).copy()).view(dt)[None]       # noqa: E731  [1, V] like logits[:, -1, :]
    bits_of = lambda t: t.reshape(-1).view(torch.int16).numpy().view(np.uint16)            # noqa: E731
    # bias: fp32 add, one rounding; ids beyond V skipped; untouched ids keep their bits
    table = {0: 3.25, 5: -100.0, V - 1: 0.001, V: 9.0, V + 100: -9.0}
    proc = make_logit_bias(table)
    assert proc.ids == tuple(table) and proc.values == tuple(table.values())
    got = bits_of(proc([1, 2, 3], as_t(base)))
    want = base.copy()
    for k, v in table.items():
        if k < V:
            want[k] = po.to_bits(po.from_bits(base[k:k + 1], name) + np.float32(v), name)[0]
    assert np.array_equal(got, want) and not np.array_equal(got, base)
    for bad in ({}, {-1: 1.0}, {3: math.inf}, {3: math.nan}, {i: 0.5 for i in range(1025)}):
        with pytest.raises(ValueError):
            make_logit_bias(bad)
    assert len(make_logit_bias({i: 0.5 for i in range(1024)}).ids) == 1024
    # mask: -inf where disallowed, bits kept where allowed; static (bool, packed) and callable forms
    allowed = rng.random(V) < 0.3
    allowed[4] = True
    ninf = 0xFF80 if name == "bfloat16" else 0xFC00
    want = np.where(allowed, base, np.uint16(ninf))
    static = make_token_mask(torch.from_numpy(allowed))
    assert static.mask_fn is None and np.array_equal(static.mask.numpy().view(np.uint32), np_pack(allowed))
    assert np.array_equal(bits_of(static([], as_t(base))), want)
    packed = make_token_mask(static.mask)
    assert packed.mask_fn is None and np.array_equal(bits_of(packed([], as_t(base))), want)
    seen = []
    fn = make_token_mask(lambda tokens: (seen.append(list(tokens)), torch.from_numpy(allowed))[1])
    assert fn.mask is None and callable(fn.mask_fn)
    assert np.array_equal(bits_of(fn([9, 8], as_t(base))), want) and seen == [[9, 8]]
    by_ids = make_token_mask(lambda tokens: np.flatnonzero(allowed).tolist())
    assert np.array_equal(bits_of(by_ids([], as_t(base))), want)
    with pytest.raises(ValueError):
        make_token_mask(lambda tokens: [])([], as_t(base))                                 # an all-zero mask, seen on the host
    with pytest.raises(ValueError):
        make_token_mask([1, 2, 3])
    # a static bool mask says which vocabulary it is for; static packed words that allow no token below V are refused when applied
    assert static.vocab_size == V and packed.vocab_size is None and fn.vocab_size is None
    with pytest.raises(ValueError, match="vocabulary"):
        static([], as_t(np.concatenate([base, base[:3]])))
    with pytest.raises(ValueError, match="no token"):
        make_token_mask(torch.tensor([0, 0, 1 << 20], dtype=torch.int32))([], as_t(base))     # bit 84 lies beyond V = 77
    for bad in ({2 ** 31: 1.0}, {-2 ** 31: 1.0}):
        with pytest.raises(ValueError):
            make_logit_bias(bad)


def test_header_declares_and_the_entry_points_refuse_before_any_launch_without_gpu():
    from proxy_inference_engine_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pie_hip.h").read_text(), flags=re.S)
    for proto in (r"int\s+pie_logprobs_argmax_masked\s*\(\s*void\s*\*logits,\s*int V,\s*int dtype,\s*const uint32_t\s*\*mask,\s*int mask_words,\s*"
                  r"float\s*\*logprobs,\s*int32_t\s*\*token,\s*void\s*\*stream\)",
                  r"int\s+pie_logits_bias\s*\(\s*void\s*\*logits,\s*int V,\s*int dtype,\s*const int32_t\s*\*ids,\s*const float\s*\*bias,\s*int n,\s*void\s*\*stream\)",
                  r"int\s+pie_decoder_set_logits_mask\s*\(\s*pie_decoder\s*\*d,\s*const uint32_t\s*\*mask,\s*int mask_words\)",
                  r"int\s+pie_decoder_set_logit_bias\s*\(\s*pie_decoder\s*\*d,\s*const int32_t\s*\*ids,\s*const float\s*\*bias,\s*int n\)"):
        assert re.search(proto, text), proto
    lib = _ffi.load()
    buf = ctypes.create_string_buffer(8192)
    base = (ctypes.addressof(buf) + 255) & ~255
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 2)   # host stand-ins, never dereferenced: every call below is refused first
    ARG, SHAPE, ALIGN = -1, -2, -3
    ok = [p, 513, _ffi.PIE_BF16, p, 17, p, p, None]   # logits, V, dtype, mask, mask_words, logprobs, token, stream
    for i, v, code in ((4, 16, SHAPE), (4, 0, SHAPE), (4, -1, SHAPE), (1, 0, SHAPE), (3, odd, ALIGN), (0, None, ARG), (3, None, ARG), (5, None, ARG),
                       (6, None, ARG), (2, 7, ARG)):
        rc = lib.pie_logprobs_argmax_masked(*(ok[:i] + [v] + ok[i + 1:]))
        err = lib.pie_last_error()
        assert rc == code and err.startswith(b"pie_logprobs_argmax_masked"), (i, v, rc, err)
    ok = [p, 513, _ffi.PIE_BF16, p, p, 300, None]     # logits, V, dtype, ids, bias, n, stream
    for i, v, code in ((5, 0, ARG), (5, -1, ARG), (5, 1025, ARG), (1, 0, SHAPE), (0, None, ARG), (3, None, ARG), (4, None, ARG), (3, odd, ALIGN),
                       (4, odd, ALIGN), (2, 7, ARG)):
        rc = lib.pie_logits_bias(*(ok[:i] + [v] + ok[i + 1:]))
        err = lib.pie_last_error()
        assert rc == code and b"bias" in err, (i, v, rc, err)
    assert lib.pie_decoder_set_logits_mask(None, p, 17) == ARG and b"pie_decoder_set_logits_mask" in lib.pie_last_error()
    assert lib.pie_decoder_set_logit_bias(None, p, p, 3) == ARG and b"pie_decoder_set_logit_bias" in lib.pie_last_error()


def test_wider_routing_predicate_and_unchanged_fused_tail_spec():
    from proxy_inference_engine_amd.engine.inference_engine import fused_tail_plan, fused_tail_spec
    from proxy_inference_engine_amd.logits_processors import make_logit_bias, make_repetition_penalty, make_token_mask
    from proxy_inference_engine_amd.samplers import greedy, make_sampler
    topk = make_sampler(temp=0.8, top_k=5)
    foreign = lambda x: x                                  # noqa: E731
    other_proc = lambda tokens, logits: logits             # noqa: E731
    pen, bias = make_repetition_penalty(1.1, 60), make_logit_bias({3: 1.5})
    mask, mask_fn = make_token_mask(torch.ones(40, dtype=torch.bool)), make_token_mask(lambda tokens: [1])
    pse = object()

    def plan(sampler=None, penalty=1.0, context=60, m=None, b=None):
        return dict(sampler=sampler, repetition_penalty=penalty, context_size=context, mask=m, bias=b)

    table = [
        ([], greedy, None, False, plan()),
        (None, greedy, None, False, plan()),
        ([mask], greedy, None, False, plan(m=mask)),
        ([mask_fn], topk, None, False, plan(("top_k", 0.8, 0.0, 5), m=mask_fn)),
        ([bias], greedy, None, False, plan(b=bias)),
        ([pen], greedy, None, False, plan(penalty=1.1)),
        ([mask, pen], greedy, None, False, plan(penalty=1.1, m=mask)),
        ([pen, bias], topk, None, False, plan(("top_k", 0.8, 0.0, 5), penalty=1.1, b=bias)),
        ([mask, bias], greedy, None, False, plan(m=mask, b=bias)),
        ([mask, pen, bias], topk, None, False, plan(("top_k", 0.8, 0.0, 5), 1.1, 60, mask, bias)),
        # order violations: the kernels define mask -> penalty -> bias
        ([pen, mask], greedy, None, False, None),
        ([bias, pen], greedy, None, False, None),
        ([bias, mask], greedy, None, False, None),
        ([mask, bias, pen], greedy, None, False, None),
        # one of each at the most
        ([mask, mask_fn], greedy, None, False, None),
        ([mask, mask], greedy, None, False, None),
        ([bias, bias], greedy, None, False, None),
        ([pen, pen], greedy, None, False, None),
        # everything fused_tail_spec refuses stays refused
        ([mask, other_proc], greedy, None, False, None),
        ([other_proc, bias], greedy, None, False, None),
        ([mask, make_repetition_penalty(2.0, 0)], greedy, None, False, None),
        ([make_repetition_penalty(2.0, 1025), bias], greedy, None, False, None),
        ([mask], foreign, None, False, None),
        ([bias], foreign, None, False, None),
        ([mask], greedy, pse, False, None),
        ([mask, pen, bias], topk, pse, False, None),
        ([mask], greedy, None, True, None),
        ([bias], topk, None, True, None),
    ]
    for procs, sampler, se, tp, want in table:
        assert fused_tail_plan(procs, sampler, se, tp) == want, (procs, sampler, se, tp)
    # fused_tail_spec itself (its own table: tests/test_step_tail_host.py) keeps refusing the new processors
    for procs in ([mask], [bias], [mask, pen], [pen, bias]):
        assert fused_tail_spec(procs, greedy) is None


class _PSE:
    def process_logits(self, tokens, logits):
        return logits

    def sample(self, logprobs, sampler):
        return sampler(logprobs)


def test_make_processors_order():
    from proxy_inference_engine_amd.engine.inference_engine import InferenceEngine
    eng = InferenceEngine(model=object())
    kinds = lambda procs: ["mask" if hasattr(p, "mask_fn") else "penalty" if hasattr(p, "penalty") else "bias" if hasattr(p, "ids") else "other"  # noqa: E731
                           for p in procs]
    fn = lambda tokens: [1]                                # noqa: E731
    assert eng.make_processors() == [] and eng.make_processors(logit_bias={}, token_mask=None, repetition_penalty=1.0) == []
    assert kinds(eng.make_processors(logit_bias={4: 2.0}, repetition_penalty=1.3, token_mask=fn)) == ["mask", "penalty", "bias"]
    assert kinds(eng.make_processors(logit_bias={4: 2.0}, token_mask=fn)) == ["mask", "bias"]
    assert kinds(eng.make_processors(repetition_penalty=1.3)) == ["penalty"]
    procs = eng.make_processors(logit_bias={4: 2.0, 9: -1.0}, repetition_penalty=1.3, context_size=7, token_mask=fn)
    assert procs[0].mask_fn is fn and (procs[1].penalty, procs[1].context_size) == (1.3, 7) and procs[2].ids == (4, 9) and procs[2].values == (2.0, -1.0)
    pse = InferenceEngine(model=object(), structuring_engine=_PSE())
    got = pse.make_processors(logit_bias={4: 2.0}, repetition_penalty=1.3, token_mask=fn)
    assert got[0] == pse.structuring_engine.process_logits and kinds(got[1:]) == ["mask", "penalty", "bias"]
    with pytest.raises(ValueError):
        eng.make_processors(logit_bias={-4: 2.0})
