"""-m gpu: the quantized KV cache (QuantizedKVCache, csrc/kv_quant.hip) through the C ABI on an MI355X.

- pie_kv_quantize is bit-identical with mx.quantize as the oracle restates it (A.1);
- pie_attn_decode_quant is within tolerance of quantized_scaled_dot_product_attention (models/base.py:56-89 of the reference),
  restated here on oracle.quantized_matmul (scores, qmv regime: exact fp32 affine sums) and an fp32 value product over the
  probabilities kept in fp32 (the one rounding point the split kernel does not reproduce);
- the decoder on QuantizedKVCache layers: the cached codes are the quantized rows of the 16-bit decoder, graph replay equals eager
  bit for bit, save -> load -> continue equals an uninterrupted run, generate(kv_bits=...) converts and reuses prefixes, and refused
  configurations raise without a launch.
"""
import json

import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests._util import assert_vec_close, codes_dev, to_bits, to_dev

pytestmark = pytest.mark.gpu
TDT = {"bfloat16": torch.bfloat16, "float16": torch.float16}


def t_values(rng, shape, dtype, scale=1.0):
    """Random values representable in T (returned as fp32 and as device T)."""
    x = po.round_T(rng.standard_normal(shape).astype(np.float32) * scale, dtype)
    return x, to_dev(po.to_bits(x, dtype), dtype)


# ------------------------------------------------------------------ pie_kv_quantize
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("gs", [32, 64, 128])
def test_kv_quantize_is_mx_quantize(dtype, bits, gs):
    from proxy_inference_engine_amd import hip_ops
    rng = np.random.default_rng(bits * 1000 + gs)
    H, n, cap, dcap, D = 3, 37, 40, 48, 128
    x = po.round_T(rng.standard_normal((H, cap, D)).astype(np.float32) * 3.0, dtype)
    x[0, 0] = 0.0                              # all-zero row
    x[0, 1] = po.round_T(np.float32(1.7), dtype)  # constant rows
    x[0, 2] = po.round_T(np.float32(-0.3), dtype)
    x[1, 3] = np.abs(x[1, 3])                   # |min| > |max| and the reverse
    x[1, 4] = -np.abs(x[1, 4])
    x[2, 5, ::2] *= 1e-3                        # tiny and large elements in one group
    xd = to_dev(po.to_bits(x, dtype), dtype)[None]
    codes = torch.full((1, H, dcap, D * bits // 32), 7, dtype=torch.int32, device="cuda")
    scales = torch.zeros((1, H, dcap, D // gs), dtype=TDT[dtype], device="cuda")
    biases = torch.zeros_like(scales)
    hip_ops.kv_quantize_rows(xd, n, codes, scales, biases, group_size=gs, bits=bits)
    wq, s, b = po.quantize(x[:, :n].reshape(-1, D), group_size=gs, bits=bits, dtype=dtype)
    got_c = codes[0, :, :n].cpu().numpy().view(np.uint32).reshape(-1, D * bits // 32)
    assert np.array_equal(got_c, wq)
    assert np.array_equal(to_bits(scales[0, :, :n]).reshape(s.shape), s)
    assert np.array_equal(to_bits(biases[0, :, :n]).reshape(b.shape), b)
    assert (codes[0, :, n:] == 7).all() and (scales[0, :, n:] == 0).all()  # rows beyond n untouched


def test_kv_quantize_refuses_unsupported_formats():
    from proxy_inference_engine_amd import _ffi, hip_ops
    x = torch.zeros((1, 2, 8, 64), dtype=torch.bfloat16, device="cuda")
    for bits, gs in ((2, 64), (3, 64), (6, 64), (4, 16)):
        with pytest.raises(ValueError):
            hip_ops.kv_quantize(x, group_size=gs, bits=bits)
    buf = torch.zeros(4096, dtype=torch.int32, device="cuda")
    lib = _ffi.load()
    for D, gs, bits in ((96, 32, 4), (64, 128, 4), (128, 64, 6), (128, 64, 2)):
        rc = lib.pie_kv_quantize(_ffi.p(buf), 1, 1, 1, D, gs, bits, _ffi.PIE_BF16, _ffi.p(buf), _ffi.p(buf), _ffi.p(buf), 1, _ffi.stream())
        assert rc < 0 and b"pie_kv_quantize" in lib.pie_last_error(), (D, gs, bits)


# ------------------------------------------------------------------ pie_attn_decode_quant
def dequant_f32(wq, s, b, gs, bits, dtype):
    """scale * code + bias in fp32 (qvm's arithmetic: nothing rounded to T)."""
    rows, words = wq.shape
    per = 32 // bits
    codes = ((wq[:, :, None] >> (np.arange(per, dtype=np.uint32) * bits)) & ((1 << bits) - 1)).reshape(rows, words * per).astype(np.float32)
    sf = np.repeat(po.from_bits(s, dtype), gs, axis=1)
    bf = np.repeat(po.from_bits(b, dtype), gs, axis=1)
    return sf * codes + bf


def ref_attention(q, kq, vq, Hkv, T, scale, gs, bits, dtype):
    """quantized_scaled_dot_product_attention for one query row: q fp32 [Hq, D], (codes, scales, biases) of K / V [Hkv*T, ...]."""
    Hq, D = q.shape
    rep = Hq // Hkv
    qs = po.round_T(po.round_T(np.float32(scale), dtype) * q, dtype)  # queries *= scale, in T
    out = np.empty((Hq, D), np.float32)
    for g in range(Hkv):
        rows = slice(g * T, (g + 1) * T)
        sc = po.quantized_matmul(qs[g * rep:(g + 1) * rep], kq[0][rows], kq[1][rows], kq[2][rows], group_size=gs, bits=bits, dtype=dtype)
        sc = po.round_T(sc, dtype).astype(np.float64)
        p = np.exp(sc - sc.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        vh = dequant_f32(vq[0][rows], vq[1][rows], vq[2][rows], gs, bits, dtype).astype(np.float64)
        out[g * rep:(g + 1) * rep] = (p @ vh).astype(np.float32)
    return out


CASES = [(D, rep, T, bits) for D in (64, 128) for rep in (1, 4, 8) for T in (1, 37, 1024, 1025, 8191, 32768) for bits in (4, 8)]


@pytest.mark.parametrize("D,rep,T,bits", CASES)
def test_attn_decode_quant_matches_reference(D, rep, T, bits):
    from proxy_inference_engine_amd import hip_ops
    dtype = "bfloat16" if (D + rep + T) % 2 else "float16"
    gs = {1: 32, 4: 64, 8: 128}[rep] if D == 128 else 64
    Hkv = 2
    Hq = Hkv * rep
    cap = T + 7
    rng = np.random.default_rng(D * 7 + rep * 13 + T + bits)
    q, qd = t_values(rng, (Hq, D), dtype)
    k = po.round_T(rng.standard_normal((Hkv, cap, D)).astype(np.float32), dtype)
    v = po.round_T(rng.standard_normal((Hkv, cap, D)).astype(np.float32), dtype)
    kq = po.quantize(k.reshape(-1, D), gs, bits, dtype)
    vq = po.quantize(v.reshape(-1, D), gs, bits, dtype)

    def dev(trip):
        c, s, b = trip
        return (codes_dev(c).reshape(Hkv, cap, -1), to_dev(s, dtype).reshape(Hkv, cap, -1), to_dev(b, dtype).reshape(Hkv, cap, -1))

    scale = 1.0 / np.sqrt(D)
    got = hip_ops.attn_decode_quant(qd, dev(kq), dev(vq), scale, group_size=gs, bits=bits, T=T).float().cpu().numpy()

    def rows(trip):
        return tuple(a.reshape(Hkv, cap, -1)[:, :T].reshape(Hkv * T, -1) for a in trip)

    want = ref_attention(q, rows(kq), rows(vq), Hkv, T, scale, gs, bits, dtype)
    assert_vec_close(got, want, dtype, what=f"D={D} rep={rep} T={T} bits={bits}")


def test_attn_decode_quant_refuses():
    from proxy_inference_engine_amd import _ffi
    lib = _ffi.load()
    buf = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    p = _ffi.p(buf)
    for Hq, Hkv, T, cap, D, gs, bits in ((8, 2, 4, 8, 64, 64, 2), (8, 2, 4, 8, 96, 32, 4), (8, 3, 4, 8, 64, 64, 4), (8, 2, 9, 8, 64, 64, 4),
                                         (24, 2, 4, 8, 64, 64, 8), (8, 2, 4, 8, 64, 128, 4)):
        rc = lib.pie_attn_decode_quant(p, p, p, p, p, p, p, Hq, Hkv, T, cap, D, gs, bits, 0.1, _ffi.PIE_BF16, p, p, _ffi.stream())
        assert rc < 0 and b"pie_attn_decode_quant" in lib.pie_last_error()


# ------------------------------------------------------------------ the decoder on QuantizedKVCache
@pytest.fixture(scope="module")
def tiny(golden_dir):
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    g = np.load(golden_dir / "tiny_llama_w4_bf16.npz")
    cfg = json.loads(str(g["config_json"]))
    w = {k[2:]: g[k] for k in g.files if k.startswith("w:")}
    dev = {k: codes_dev(v) if v.dtype == np.uint32 else to_dev(v, "bfloat16") for k, v in w.items()}
    return g, cfg, Model(ModelArgs(**cfg), dev)


def qcache(model, bits, gs=64):
    from proxy_inference_engine_amd.cache import QuantizedKVCache
    return [QuantizedKVCache(group_size=gs, bits=bits) for _ in model.layers]


def run(model, cache, prompt, n_steps, graph=True, token_by_token=False):
    """Prompt, then n_steps greedy steps; returns the logits of the prompt's last row and of every step (fp32 host arrays) and the tokens."""
    ids = torch.as_tensor(prompt, dtype=torch.int32, device="cuda")
    if token_by_token:
        for i in range(len(prompt)):
            tok, _, logits = model.step(ids[i:i + 1], cache, graph=graph)
    else:
        tok, _, logits = model.step(ids, cache, graph=graph)
    out, toks = [logits.float().cpu().numpy().copy()], [int(tok.item())]
    for _ in range(n_steps):
        tok, _, logits = model.step(None, cache, graph=graph)
        out.append(logits.float().cpu().numpy().copy())
        toks.append(int(tok.item()))
    return np.stack(out), toks


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("by_token", [False, True])  # the batched prompt pass / decode steps
def test_layer0_codes_are_the_quantized_16bit_rows(tiny, bits, by_token):
    """Layer 0's K / V rows of the prompt do not depend on the cache format: the quantized decoder's codes are quantize() of the 16-bit
    decoder's rows, bit for bit (the rows after the prompt follow greedy tokens, which the formats may choose differently)."""
    from proxy_inference_engine_amd import hip_ops
    g, cfg, model = tiny
    prompt = [int(t) for t in g["prompt"]]
    n = len(prompt)
    c16 = model.make_cache()
    run(model, c16, prompt, 0, token_by_token=by_token)
    cq = qcache(model, bits)
    run(model, cq, prompt, 0, token_by_token=by_token)
    assert cq[0].offset == c16[0].offset == n
    for src, dst in ((c16[0].keys, cq[0].keys), (c16[0].values, cq[0].values)):
        codes, scales, biases = hip_ops.kv_quantize(src[:, :, :n].contiguous(), 64, bits)
        assert torch.equal(dst[0][:, :, :n], codes) and torch.equal(dst[1][:, :, :n], scales) and torch.equal(dst[2][:, :, :n], biases)


def forced(model, cache, seq):
    """Teacher-forced decode steps over `seq`: the logits after every token (fp32 host array)."""
    ids = torch.as_tensor(seq, dtype=torch.int32, device="cuda")
    out = []
    for i in range(len(seq)):
        _, _, logits = model.step(ids[i:i + 1], cache)
        out.append(logits.float().cpu().numpy().copy())
    return np.stack(out)


def test_quantized_decode_tracks_the_16bit_decoder(tiny):
    """Teacher-forced over the prompt + 16 tokens: 8-bit KV moves the logits by a small fraction of their spread, 4-bit by more."""
    g, cfg, model = tiny
    seq = [int(t) for t in g["prompt"]] + list(range(3, 19))
    ref = forced(model, model.make_cache(), seq)
    err = {}
    for bits in (8, 4):
        got = forced(model, qcache(model, bits), seq)
        assert np.isfinite(got).all()
        err[bits] = float(np.sqrt(np.mean((got - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))
    print("relative rms logits error vs 16-bit KV:", err)
    assert err[8] < 0.05 and err[4] < 0.35 and err[8] < err[4], err


@pytest.mark.parametrize("n_prompt", [9, 1100])  # the merged-split plan, and the combine plan beyond 1024 cached positions
def test_graph_replay_equals_eager(tiny, n_prompt):
    g, cfg, model = tiny
    rng = np.random.default_rng(n_prompt)
    prompt = [int(t) for t in rng.integers(0, cfg["vocab_size"], n_prompt)]
    a, ta = run(model, qcache(model, 4), prompt, 16, graph=True)
    b, tb = run(model, qcache(model, 4), prompt, 16, graph=False)
    assert ta == tb and np.array_equal(a, b)


def test_save_load_continue_equals_uninterrupted(tiny, tmp_path):
    from proxy_inference_engine_amd.cache import BaseCache, QuantizedKVCache
    g, cfg, model = tiny
    prompt = [int(t) for t in g["prompt"]]
    full, tf = run(model, qcache(model, 8, gs=32), prompt, 12)
    cache = qcache(model, 8, gs=32)
    part, tp = run(model, cache, prompt, 4)
    BaseCache.save_cache(str(tmp_path / "q.safetensors"), cache, {"n": "1"})
    loaded, meta = BaseCache.load_cache(str(tmp_path / "q.safetensors"))
    assert meta == {"n": "1"} and all(isinstance(c, QuantizedKVCache) and c.offset == cache[0].offset for c in loaded)
    ids = torch.tensor([tp[-1]], dtype=torch.int32, device="cuda")
    rest = []
    tok, _, logits = model.step(ids, loaded)
    rest.append(logits.float().cpu().numpy().copy())
    for _ in range(7):
        tok, _, logits = model.step(None, loaded)
        rest.append(logits.float().cpu().numpy().copy())
    assert np.array_equal(np.concatenate([part, np.stack(rest)]), full)


def test_generate_with_kv_bits_converts_and_reuses_prefixes(tiny):
    from proxy_inference_engine_amd import InferenceEngine
    from proxy_inference_engine_amd.cache import QuantizedKVCache
    g, cfg, model = tiny
    prompt = [int(t) for t in g["prompt"]]
    eng = InferenceEngine(model=model)
    out = [t for t, _ in eng.generate(prompt, max_completion_tokens=8, kv_bits=8, kv_group_size=64)]
    assert len(out) == 8 and all(isinstance(c, QuantizedKVCache) and c.bits == 8 for c in eng.prompt_cache.cache)
    # a second request sharing the prompt's prefix reuses the quantized rows and decodes as a fresh engine that converts at the same point
    again = [t for t, _ in eng.generate(prompt + out[:3], max_completion_tokens=5, kv_bits=8, kv_group_size=64)]
    eng2 = InferenceEngine(model=model)
    first = [t for t, _ in eng2.generate(prompt, max_completion_tokens=8, kv_bits=8, kv_group_size=64)]
    assert first == out and len(again) == 5
    # the reused request against the same arithmetic without the prompt cache: its prefix rows are the converted prompt plus the quantized
    # rows of out[:2] (out[2] is the reused request's one new token), then the same greedy continuation
    from proxy_inference_engine_amd.cache import QuantizedKVCache as Q
    cache = model.make_cache()
    model(torch.tensor([prompt], device="cuda"), cache=cache)
    cache = [Q.from_cache(c, group_size=64, bits=8) for c in cache]
    ids = torch.tensor(out[:3], dtype=torch.int32, device="cuda")
    toks = []
    for i in range(3):
        tok, _, _ = model.step(ids[i:i + 1], cache)
    toks.append(int(tok.item()))
    for _ in range(4):
        tok, _, _ = model.step(None, cache)
        toks.append(int(tok.item()))
    assert again == toks
    with pytest.raises(ValueError):
        next(iter(InferenceEngine(model=model).generate(prompt, kv_bits=3)))


def test_refused_configurations_raise(tiny):
    from proxy_inference_engine_amd import _ffi
    from proxy_inference_engine_amd.cache import QuantizedKVCache
    g, cfg, model = tiny
    with pytest.raises(ValueError):
        QuantizedKVCache(group_size=64, bits=6)
    bad = [QuantizedKVCache(group_size=128, bits=4) for _ in model.layers]  # 128 does not divide head_dim 64
    with pytest.raises(ValueError):
        model.step(torch.tensor([1], dtype=torch.int32, device="cuda"), bad)
    lib = _ffi.load()
    n = len(model.layers)
    buf = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    arr = (_ffi.C.c_void_p * n)(*[buf.data_ptr()] * n)
    for gs, bits in ((64, 6), (128, 4), (16, 4)):
        rc = lib.pie_decoder_set_kv_quant(model._dec, arr, arr, arr, arr, arr, arr, 256, gs, bits, _ffi.stream())
        assert rc < 0 and b"pie_decoder_set_kv_quant" in lib.pie_last_error()
    # the decoder still runs on a 16-bit cache afterwards
    model._kv.invalidate()
    _, toks = run(model, model.make_cache(), [int(t) for t in g["prompt"]], 2)
    assert len(toks) == 3


# ------------------------------------------------------------------ the layer restated on oracle primitives
class RefQuantLlama:
    """The tiny Llama over a quantized KV cache, composed from oracle primitives (rms_norm, rope, quantized_matmul, silu_mul, add,
    quantize / dequantize, sdpa).  Attention follows the product's two routes:
      one row (decode step)   quantized_scaled_dot_product_attention: queries*scale and scores rounded to T, softmax and the value
                              product in fp32 over s*code+b (ref_attention above);
      a prompt (>= 6 rows)    update_and_fetch's quantized rows dequantized to T (mx.dequantize), then the fused causal sdpa over them.
    A 16-bit prompt (the conversion route) runs the fused sdpa over its T rows, which are quantized afterwards (KVCache.to_quantized)."""

    def __init__(self, cfg, w, bits, gs=64, dtype="bfloat16"):
        self.w, self.bits, self.gs, self.dt = w, bits, gs, dtype
        self.o = po.OracleLlama(cfg, w, dtype)
        self.H, self.nl, self.Hq, self.Hkv, self.D = self.o.hidden, self.o.n_layers, self.o.n_heads, self.o.n_kv_heads, self.o.head_dim
        self.eps = float(cfg["rms_norm_eps"])
        self.k = [np.zeros((self.Hkv, 0, self.D), np.float32) for _ in range(self.nl)]  # T rows (the 16-bit prompt only)
        self.v = [np.zeros((self.Hkv, 0, self.D), np.float32) for _ in range(self.nl)]
        self.kq = [None] * self.nl  # (codes, scales, biases) per layer, rows [Hkv * T] head-major
        self.vq = [None] * self.nl
        self.T = 0

    def lin(self, x, name, L):
        w = self.w
        regime = "qmm" if L >= po.get_qmm_min_rows() else "qmv"
        return po.quantized_matmul(x, w[name + ".weight"], w[name + ".scales"], w[name + ".biases"], group_size=64, bits=4, dtype=self.dt, regime=regime)

    def quantize_rows(self, x):  # x [Hkv, n, D] -> triple of [Hkv, n, ...]
        c, s, b = po.quantize(x.reshape(-1, self.D), self.gs, self.bits, self.dt)
        return tuple(a.reshape(self.Hkv, x.shape[1], -1) for a in (c, s, b))

    def append(self, li, kq, vq):
        if self.kq[li] is None:
            self.kq[li], self.vq[li] = kq, vq
        else:
            self.kq[li] = tuple(np.concatenate([a, b], axis=1) for a, b in zip(self.kq[li], kq))
            self.vq[li] = tuple(np.concatenate([a, b], axis=1) for a, b in zip(self.vq[li], vq))

    def convert(self):  # KVCache.to_quantized of the T rows
        for li in range(self.nl):
            self.kq[li], self.vq[li] = self.quantize_rows(self.k[li]), self.quantize_rows(self.v[li])

    def forward(self, ids, quantized=True, extra=None):
        """ids [L] at offset self.T -> logits of the last row (T-rounded fp32).  extra[li]: rows attended after the new ones (a kernel's
        read past the end, for the long-context tests' sensitivity checks): quantized triples [Hkv, n, ...] on a step, fp32 (K, V)
        [Hkv, n, D] on a 16-bit prompt, where only its last row sees them.  Not stored."""
        w, dt, D, L = self.w, self.dt, self.D, len(ids)
        e = "model.embed_tokens"
        h = po.dequantize(w[e + ".weight"][ids], w[e + ".scales"][ids], w[e + ".biases"][ids], 64, 4, dt)
        off = self.T
        for li in range(self.nl):
            p = f"model.layers.{li}"
            xn = po.rms_norm(h, w[p + ".input_layernorm.weight"], self.eps, dt)
            q = self.lin(xn, p + ".self_attn.q_proj", L).reshape(L, self.Hq, D).transpose(1, 0, 2)
            k = self.lin(xn, p + ".self_attn.k_proj", L).reshape(L, self.Hkv, D).transpose(1, 0, 2)
            v = self.lin(xn, p + ".self_attn.v_proj", L).reshape(L, self.Hkv, D).transpose(1, 0, 2)
            q = po.rope(np.ascontiguousarray(q), self.o.freqs, off, dt)
            k = po.rope(np.ascontiguousarray(k), self.o.freqs, off, dt)
            v = np.ascontiguousarray(v)
            scale = 1.0 / np.sqrt(D)
            if not quantized:  # 16-bit prompt
                self.k[li] = np.concatenate([self.k[li], k], axis=1)
                self.v[li] = np.concatenate([self.v[li], v], axis=1)
                ks, vs, mask = self.k[li], self.v[li], po.causal_mask(L, off, dt)
                if extra is not None:
                    n = extra[li][0].shape[1]
                    ks, vs = np.concatenate([ks, extra[li][0]], axis=1), np.concatenate([vs, extra[li][1]], axis=1)
                    tail = np.full((L, n), mask.min(), np.float32)
                    tail[-1] = 0.0
                    mask = np.ascontiguousarray(np.concatenate([mask, tail], axis=1))
                o = po.sdpa(q, ks, vs, scale, mask, dt, fused=True)
            else:
                self.append(li, self.quantize_rows(k), self.quantize_rows(v))
                T = off + L
                if L == 1:
                    kq, vq, Ta = self.kq[li], self.vq[li], T
                    if extra is not None:
                        kq, vq = (tuple(np.concatenate([a, b], axis=1) for a, b in zip(t, e)) for t, e in ((kq, extra[li][0]), (vq, extra[li][1])))
                        Ta += extra[li][0][0].shape[1]
                    flat = lambda t: tuple(a.reshape(self.Hkv * Ta, -1) for a in t)  # noqa: E731
                    o = ref_attention(q[:, 0], flat(kq), flat(vq), self.Hkv, Ta, scale, self.gs, self.bits, dt)[:, None]
                else:
                    deq = lambda t: po.dequantize(*(a.reshape(self.Hkv * T, -1) for a in t), self.gs, self.bits, dt).reshape(self.Hkv, T, D)  # noqa: E731
                    o = po.sdpa(q, deq(self.kq[li]), deq(self.vq[li]), scale, po.causal_mask(L, off, dt), dt, fused=True)
                o = po.round_T(o, dt)
            o = np.ascontiguousarray(o.transpose(1, 0, 2)).reshape(L, self.Hq * D)
            h = po.add(h, self.lin(o, p + ".self_attn.o_proj", L), dt)
            xn = po.rms_norm(h, w[p + ".post_attention_layernorm.weight"], self.eps, dt)
            a = po.silu_mul(self.lin(xn, p + ".mlp.gate_proj", L), self.lin(xn, p + ".mlp.up_proj", L), dt)
            h = po.add(h, self.lin(a, p + ".mlp.down_proj", L), dt)
        self.T += L
        xn = po.rms_norm(h[-1:], w["model.norm.weight"], self.eps, dt)
        return self.lin(xn, "lm_head", 1)[0]


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("route", ["native", "convert"])
def test_decoder_matches_the_oracle_restatement(golden_dir, bits, route):
    """The tiny golden model, prompt + 16 greedy steps on a quantized cache, against RefQuantLlama (teacher-forced with the decoder's
    tokens).  native: the prompt runs on the quantized cache (the batched pass); convert: a 16-bit prompt, then from_cache.
    Bound: the end-to-end one of tests/_util.assert_vec_close at 8 bits; at 4 bits a one-ulp landing of a K / V element that sits on a
    rounding edge moves its code by one step of 1/15 of the group's range, so the bound is four times wider."""
    from proxy_inference_engine_amd.cache import QuantizedKVCache
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    g = np.load(golden_dir / "tiny_llama_w4_bf16.npz")
    cfg = json.loads(str(g["config_json"]))
    w = {k[2:]: g[k] for k in g.files if k.startswith("w:")}
    model = Model(ModelArgs(**cfg), {k: codes_dev(v) if v.dtype == np.uint32 else to_dev(v, "bfloat16") for k, v in w.items()})
    ref = RefQuantLlama(cfg, w, bits)
    prompt = [int(t) for t in g["prompt"]]
    c = 4.0 if bits == 8 else 16.0
    if route == "native":
        cache = qcache(model, bits)
        got = model(torch.tensor([prompt], device="cuda"), cache=cache)[0, -1].float().cpu().numpy()
        want = ref.forward(np.array(prompt), quantized=True)
    else:
        cache = model.make_cache()
        got = model(torch.tensor([prompt], device="cuda"), cache=cache)[0, -1].float().cpu().numpy()
        want = ref.forward(np.array(prompt), quantized=False)
        cache = [QuantizedKVCache.from_cache(x, group_size=64, bits=bits) for x in cache]
        ref.convert()
    assert_vec_close(got, want, "bfloat16", c_max=c, c_rms=c, what=f"{route} prompt")
    tok = int(np.argmax(got))
    for i in range(16):
        _, _, logits = model.step(torch.tensor([tok], dtype=torch.int32, device="cuda"), cache)
        got = logits.float().cpu().numpy()
        want = ref.forward(np.array([tok]), quantized=True)
        assert_vec_close(got, want, "bfloat16", c_max=c, c_rms=c, what=f"{route} step {i}")
        tok = int(np.argmax(got))
