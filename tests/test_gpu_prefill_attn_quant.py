"""Prompt and verify attention straight from the quantized KV cache: the kernel against float64 and against the prompt
kernel over the dequantized rows; the decoder's pass with PIE_OPT_KVQ_DIRECT on and off; the engine under SpeculativeParams(quantized_kv=True)."""
import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests._util import assert_dot_close, sdpa_f64, to_bits, to_dev
from tests.test_gpu_speculative import E2E_SEEDS, E2E_TOKENS, e2e_prompt, fresh_cache, load_tiny

pytestmark = pytest.mark.gpu

HKV = 2
SHAPES = [(M, off) for M in (1, 33, 65) for off in (0, 31, 95)]   # a key block's edge, a partial second tile, two tiles
# one sweep: every (bits, D, dtype) triple in cases 0..7, every rep and every group size (<= D) among them
CASES = [(M, off, (4, 8)[i % 2], (64, 128)[i // 2 % 2], ("bfloat16", "float16")[i // 4 % 2], (1, 4, 8)[(i + i // 3) % 3],
          min((32, 64, 128)[i % 3], (64, 128)[i // 2 % 2])) for i, (M, off) in enumerate(SHAPES)]
NAN_BITS = {"bfloat16": 0x7FC0, "float16": 0x7E00}


def dequant_T(codes, scales, biases, gs, bits, dt):
    """mx.dequantize: T(fp32(s q) + b) of codes uint32 [..., W], scales / biases storage bits [..., D / gs] -> fp32 [..., D]."""
    per = 32 // bits
    c = ((codes[..., None] >> (np.arange(per, dtype=np.uint32) * bits)) & ((1 << bits) - 1)).reshape(*codes.shape[:-1], -1).astype(np.float32)
    s, b = (np.repeat(po.from_bits(x, dt), gs, axis=-1) for x in (scales, biases))
    with np.errstate(invalid="ignore"):
        return po.round_T((s * c).astype(np.float32) + b, dt)


_DATA = {}


def case_data(M, off, bits, D, dt, rep, gs):
    """(q device [M, Hq, D], k / v device triples [HKV, cap, ...] whose capacity past off + M is poison, float64 reference rounded once to
    T, the dequantized K / V with that poison) -- built once per case and shared by the tests."""
    key = (M, off, bits, D, dt, rep, gs)
    if key not in _DATA:
        from proxy_inference_engine_amd import hip_ops
        rng = np.random.default_rng(CASES.index(key))
        T, cap, Hq = off + M, 256, HKV * rep
        q = po.round_T(rng.standard_normal((M, Hq, D), dtype=np.float32), dt)
        k = rng.standard_normal((HKV, cap, D), dtype=np.float32)
        sd = np.sign(rng.standard_normal((HKV, 1, D), dtype=np.float32))   # V: one sign per dim, so no mixture of rows cancels to ~0
        v = sd * (np.abs(rng.standard_normal((HKV, 1, D), dtype=np.float32)) + 0.5) + 0.5 * rng.standard_normal((HKV, cap, D), dtype=np.float32)
        trips, deq = [], []
        for x in (k, v):
            trip = [t.clone() for t in hip_ops.kv_quantize(to_dev(po.to_bits(x, dt), dt), gs, bits)]
            trip[0].view(torch.int32)[:, T:] = -1                                   # NaN-producing codes and scales behind the attended rows
            trip[1].view(torch.int16)[:, T:] = NAN_BITS[dt]
            trip[2].view(torch.int16)[:, T:] = NAN_BITS[dt]
            trips.append(tuple(trip))
            deq.append(dequant_T(trip[0].view(torch.int32).cpu().numpy().view(np.uint32), to_bits(trip[1]), to_bits(trip[2]), gs, bits, dt))
        assert np.isfinite(deq[0][:, :T]).all() and np.isnan(deq[0][:, T:]).all()
        want = np.stack([sdpa_f64(q[r][:, None], deq[0], deq[1], 1.0 / np.sqrt(D), off + r + 1)[:, 0] for r in range(M)])
        _DATA[key] = (to_dev(po.to_bits(q, dt), dt), trips[0], trips[1], po.round_T(want, dt), deq)
    return _DATA[key]


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("M,off,bits,D,dt,rep,gs", CASES)
def test_prefill_attn_quant_equals_float64(M, off, bits, D, dt, rep, gs, splits):
    from proxy_inference_engine_amd import hip_ops
    q, k, v, want, _ = case_data(M, off, bits, D, dt, rep, gs)
    got = po.from_bits(to_bits(hip_ops.prefill_attn_quant(q, k, v, 1.0 / np.sqrt(D), off, gs, bits, splits=splits)), dt)
    assert np.isfinite(got).all()
    frac = assert_dot_close(got, want, dt, max_frac=0.05, what=f"M={M} off={off} bits={bits} D={D} {dt} rep={rep} gs={gs} splits={splits}")
    print(f"differing share M={M} off={off} bits={bits} D={D} {dt} rep={rep} gs={gs} splits={splits}: {frac:.4f}")


@pytest.mark.parametrize("M,off,bits,D,dt,rep,gs", [c for c in CASES if c[0] > 1])   # (one query row takes the decode kernel there)
def test_one_split_is_the_prompt_kernel_over_the_dequantized_rows_bit_for_bit(M, off, bits, D, dt, rep, gs):
    from proxy_inference_engine_amd import hip_ops
    q, k, v, _, deq = case_data(M, off, bits, D, dt, rep, gs)
    got = hip_ops.prefill_attn_quant(q, k, v, 1.0 / np.sqrt(D), off, gs, bits, splits=1)
    kd, vd = (to_dev(po.to_bits(x, dt), dt)[None] for x in deq)
    if gs == 64:                                                            # the library's own dequantize agrees with the restatement
        mine = hip_ops.dequantize(k[0].reshape(-1, k[0].shape[-1]), k[1].reshape(-1, D // 64), k[2].reshape(-1, D // 64), 64, bits)
        assert np.array_equal(to_bits(mine).reshape(HKV, -1, D)[:, :off + M], to_bits(kd[0])[:, :off + M])
    want = hip_ops.scaled_dot_product_attention(q.transpose(0, 1)[None].contiguous(), kd, vd, 1.0 / np.sqrt(D), mask="causal", T=off + M)
    assert np.array_equal(to_bits(got), to_bits(want[0].transpose(0, 1)))


# ------------------------------------------------------------------ the decoder and the engine on the tiny golden model
def quantized_prefix(model, bits, ids):
    from proxy_inference_engine_amd.cache import QuantizedKVCache
    cache = [QuantizedKVCache(group_size=64, bits=bits) for _ in model.layers]
    model.set_kv_direct_attn(False)
    model.step(ids, cache)
    return cache


@pytest.mark.parametrize("bits", [4, 8])
def test_decoder_pass_with_the_option_equals_the_scratch_pass(golden_dir, bits):
    """A 40-row prompt behind 70 quantized positions, PIE_OPT_KVQ_DIRECT on and off: the same codes, scales and biases, and -- the rule
    takes one split for the four key blocks of 110 positions, where the kernel is the prompt kernel bit for bit -- the same logits."""
    cfg, dt, _, model = load_tiny(golden_dir, "tiny_llama_w4_bf16")
    rng = np.random.default_rng(bits)
    first, then = (torch.tensor(rng.integers(0, cfg["vocab_size"], n), dtype=torch.int32, device="cuda") for n in (70, 40))
    logits, caches = {}, {}
    try:
        for direct in (False, True):
            caches[direct] = quantized_prefix(model, bits, first)
            model.set_kv_direct_attn(direct)
            logits[direct] = model.step(then, caches[direct])[2].float().cpu().numpy().copy()
    finally:
        model.set_kv_direct_attn(False)
    for a, b in zip(caches[False], caches[True]):
        assert a.offset == b.offset == 110
        for x, y in zip((*a.keys, *a.values), (*b.keys, *b.values)):
            assert torch.equal(x[:, :, :110], y[:, :, :110])
    assert np.array_equal(logits[True], logits[False])


@pytest.mark.parametrize("seed", E2E_SEEDS["tiny_llama_w4_bf16"])
def test_engine_speculates_on_a_quantized_cache(golden_dir, seed):
    """generate(kv_bits=4, speculative=SpeculativeParams(quantized_kv=True)) against the same call without `speculative`, on the
    speculative end-to-end prompts of tests/test_gpu_speculative.py (a tiled base, so the continuation repeats it); the refusals."""
    from proxy_inference_engine_amd import InferenceEngine, SpeculativeParams
    from proxy_inference_engine_amd.cache import QuantizedKVCache
    from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine
    cfg, dt, _, model = load_tiny(golden_dir, "tiny_llama_w4_bf16")
    prompt = [int(t) for t in e2e_prompt(seed, cfg["vocab_size"])]

    def engine():   # (the session's model may have KV pages enabled by now: the request runs on contiguous caches)
        eng = InferenceEngine(model=model)
        eng.prompt_cache.cache = fresh_cache(model, "contiguous")
        return eng

    try:
        plain = [t for t, _ in engine().generate(prompt, max_completion_tokens=E2E_TOKENS, kv_bits=4)]
        eng = engine()
        got = [t for t, _ in eng.generate(prompt, max_completion_tokens=E2E_TOKENS, kv_bits=4, speculative=SpeculativeParams(quantized_kv=True))]
        print(f"seed {seed}: {eng.spec_stats}, first differing token {next((i for i, (x, y) in enumerate(zip(got, plain)) if x != y), None)}")
        assert got == plain and eng.spec_stats["passes"] > 0, (eng.spec_stats, got, plain)
        assert all(isinstance(c, QuantizedKVCache) and c.bits == 4 for c in eng.prompt_cache.cache)
        with pytest.raises(ValueError, match="speculative decoding is not available with kv_bits"):
            next(iter(InferenceEngine(model=model).generate(prompt, max_completion_tokens=2, kv_bits=4, speculative=SpeculativeParams())))
        with pytest.raises(ValueError, match="quantized_kv"):
            BatchedEngine(model, num_pages=8, speculative=SpeculativeParams(quantized_kv=True))
    finally:
        model.set_kv_direct_attn(False)
