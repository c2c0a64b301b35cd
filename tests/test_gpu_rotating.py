"""-m gpu: the rotating KV cache (RotatingKVCache, csrc/rotating.hip, the RING decode attention and the windowed prompt attention).

- pie_sdpa_prefill_window against oracle.sdpa with the windowed causal mask (create_causal_mask(L, o', window_size=W), models/base.py);
- the decoder on RotatingKVCache layers against a restatement on oracle primitives (RefRotatingLlama): prompts shorter and longer than
  the window, steps across the wrap, chunks on a full ring;
- graph replay equals eager bit for bit across the wrap, the buffers stay bounded, save -> load -> continue equals an uninterrupted run,
  generate(max_kv_size=...) equals a Model.step loop, and refused configurations raise before any launch.
"""
import json

import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests._util import assert_vec_close, codes_dev, to_dev, window_mask

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ pie_sdpa_prefill_window
CASES = [(D, rep, o, L) for D in (64, 128) for rep in (1, 4) for o in (0, 512) for L in (37, 700)] + [(128, 4, 512, 4096), (64, 1, 0, 4096)]


@pytest.mark.parametrize("D,rep,o,L", CASES)
def test_windowed_prefill_attention(D, rep, o, L):
    from proxy_inference_engine_amd import hip_ops
    dt, W, Hkv = "bfloat16", 512, 1
    rng = np.random.default_rng(D + rep * 7 + o + L)
    Hq, T = Hkv * rep, o + L
    q = po.round_T(rng.standard_normal((Hq, L, D)).astype(np.float32), dt)
    k = po.round_T(rng.standard_normal((Hkv, T + 5, D)).astype(np.float32), dt)
    v = po.round_T(rng.standard_normal((Hkv, T + 5, D)).astype(np.float32), dt)
    dev = lambda x: to_dev(po.to_bits(x, dt), dt)[None]  # noqa: E731
    got = hip_ops.sdpa_prefill_window(dev(q), dev(k), dev(v), D ** -0.5, o, W)[0].float().cpu().numpy()
    want = po.sdpa(q, k, v, D ** -0.5, window_mask(L, o, W), dt, True, T=T)
    assert_vec_close(got, want, dt, what=f"D={D} rep={rep} o={o} L={L}")


def test_ring_order_moves_rows():
    from proxy_inference_engine_amd import hip_ops
    k = torch.arange(2 * 12 * 64, dtype=torch.float32).reshape(1, 2, 12, 64).to(torch.bfloat16).cuda()
    v = -k
    k0, v0 = k.clone(), v.clone()
    hip_ops.kv_ring_order(k, v, 3, 8, 5, 6)  # rows 3 + j <- rows 3 + (j + 5) % 8, j < 6
    idx = [3 + (j + 5) % 8 for j in range(6)]
    assert torch.equal(k[:, :, 3:9], k0[:, :, idx]) and torch.equal(v[:, :, 3:9], v0[:, :, idx])
    assert torch.equal(k[:, :, :3], k0[:, :, :3]) and torch.equal(k[:, :, 9:], k0[:, :, 9:])


@pytest.mark.parametrize("D,rep,keep", [(64, 2, 4), (128, 4, 4), (128, 1, 0)])
def test_ring_decode_slot_and_length_across_the_wrap(D, rep, keep):
    """pie_sdpa_decode_ring step by step from an empty ring of W = 100 rows to past its second wrap: every step writes its row to slot(pos)
    and attends exactly the sinks and the newest rows (all rows before the ring is full), against oracle.sdpa over those positions."""
    from proxy_inference_engine_amd import hip_ops
    dt, W, Hkv = "bfloat16", 100, 2
    Hq, cap = Hkv * rep, W
    rng = np.random.default_rng(D + rep + keep)
    dev = lambda x: to_dev(po.to_bits(x, dt), dt)  # noqa: E731
    k = torch.zeros((Hkv, cap, D), dtype=torch.bfloat16, device="cuda")
    v = torch.zeros_like(k)
    rows = {}
    for p in range(2 * W + 37):
        q = po.round_T(rng.standard_normal((Hq, D)).astype(np.float32), dt)
        kn = po.round_T(rng.standard_normal((Hkv, D)).astype(np.float32), dt)
        vn = po.round_T(rng.standard_normal((Hkv, D)).astype(np.float32), dt)
        rows[p] = (kn, vn)
        got = hip_ops.sdpa_decode_ring(dev(q), k, v, dev(kn), dev(vn), D ** -0.5, p, W, keep, W).float().cpu().numpy()
        slot = p if p < W else keep + (p - W) % (W - keep)
        assert torch.equal(k[:, slot], dev(kn)) and torch.equal(v[:, slot], dev(vn)), p
        seen = list(range(p + 1)) if p < W else list(range(keep)) + list(range(p + 1 - (W - keep), p + 1))
        ks = np.stack([rows[t][0] for t in seen], 1)
        vs = np.stack([rows[t][1] for t in seen], 1)
        want = po.sdpa(q[:, None], ks, vs, D ** -0.5, None, dt, True)[:, 0]
        assert_vec_close(got, want, dt, what=f"pos {p}")


# ------------------------------------------------------------------ the decoder on RotatingKVCache
@pytest.fixture(scope="module")
def tiny(golden_dir):
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    g = np.load(golden_dir / "tiny_llama_w4_bf16.npz")
    cfg = json.loads(str(g["config_json"]))
    w = {k[2:]: g[k] for k in g.files if k.startswith("w:")}
    dev = {k: codes_dev(v) if v.dtype == np.uint32 else to_dev(v, "bfloat16") for k, v in w.items()}
    return g, cfg, w, Model(ModelArgs(**cfg), dev)


def ring(model, W, keep=4):
    from proxy_inference_engine_amd.cache import RotatingKVCache
    return [RotatingKVCache(W, keep=keep) for _ in model.layers]


class RefRotatingLlama:
    """The tiny Llama over a rotating cache, composed from oracle primitives.  The rows are kept by position in the reference's row order
    (rotating.py): a single row goes to the write index and attends every stored row (no mask); a chunk sees the retained window in
    temporal order plus itself under create_causal_mask(L, o', window_size=W).  RoPE at the absolute position."""

    def __init__(self, cfg, w, W, keep, dtype="bfloat16"):
        self.w, self.dt, self.W, self.keep = w, dtype, W, keep
        self.o = po.OracleLlama(cfg, w, dtype)
        self.nl, self.Hq, self.Hkv, self.D = self.o.n_layers, self.o.n_heads, self.o.n_kv_heads, self.o.head_dim
        self.eps = float(cfg["rms_norm_eps"])
        self.rows, self.idx, self.offset = [], 0, 0  # positions in row order
        self.kv = [dict() for _ in range(self.nl)]   # per layer: position -> (k [Hkv, D], v [Hkv, D])

    def lin(self, x, name, L):
        w = self.w
        regime = "qmm" if L >= po.get_qmm_min_rows() else "qmv"
        return po.quantized_matmul(x, w[name + ".weight"], w[name + ".scales"], w[name + ".biases"], group_size=64, bits=4, dtype=self.dt, regime=regime)

    def window(self):
        if self.offset <= self.W:
            return list(range(self.offset))
        return list(range(self.keep)) + list(range(self.offset - (self.W - self.keep), self.offset))

    def plan(self, L):
        """Row order after an update of L rows, and the mask the new rows attend with."""
        new = list(range(self.offset, self.offset + L))
        if L >= 2:
            win = self.window() if self.rows else []
            self.rows, self.idx = win + new, len(win) + L
            return window_mask(L, len(win), self.W)
        if len(self.rows) > self.W:
            self.rows, self.idx = self.window(), self.W
        if self.idx == self.W:
            self.idx = self.keep
        if self.idx == len(self.rows):
            self.rows.append(new[0])
        else:
            self.rows[self.idx] = new[0]
        self.idx += 1
        return None

    def forward(self, ids, extra=None):
        """extra[li]: (K, V) [Hkv, n, D] attended after the stored rows by a single-row update (a kernel's read of a row too many, for the
        long-context tests' sensitivity checks)."""
        w, dt, D, L = self.w, self.dt, self.D, len(ids)
        e = "model.embed_tokens"
        h = po.dequantize(w[e + ".weight"][ids], w[e + ".scales"][ids], w[e + ".biases"][ids], 64, 4, dt)
        off = self.offset
        mask = self.plan(L)
        self.offset += L
        for li in range(self.nl):
            p = f"model.layers.{li}"
            xn = po.rms_norm(h, w[p + ".input_layernorm.weight"], self.eps, dt)
            q = self.lin(xn, p + ".self_attn.q_proj", L).reshape(L, self.Hq, D).transpose(1, 0, 2)
            k = self.lin(xn, p + ".self_attn.k_proj", L).reshape(L, self.Hkv, D).transpose(1, 0, 2)
            v = self.lin(xn, p + ".self_attn.v_proj", L).reshape(L, self.Hkv, D).transpose(1, 0, 2)
            q = po.rope(np.ascontiguousarray(q), self.o.freqs, off, dt)
            k = po.rope(np.ascontiguousarray(k), self.o.freqs, off, dt)
            for i in range(L):
                self.kv[li][off + i] = (k[:, i], v[:, i])
            ks = np.stack([self.kv[li][r][0] for r in self.rows], 1)
            vs = np.stack([self.kv[li][r][1] for r in self.rows], 1)
            rows_seen = len(self.rows) if L >= 2 or self.offset >= self.W else self.offset
            if extra is not None:
                ks, vs = np.concatenate([ks[:, :rows_seen], extra[li][0]], 1), np.concatenate([vs[:, :rows_seen], extra[li][1]], 1)
                rows_seen += extra[li][0].shape[1]
            o = po.sdpa(q, ks, vs, 1.0 / np.sqrt(D), mask, dt, fused=True, T=rows_seen)
            o = np.ascontiguousarray(po.round_T(o, dt).transpose(1, 0, 2)).reshape(L, self.Hq * D)
            h = po.add(h, self.lin(o, p + ".self_attn.o_proj", L), dt)
            xn = po.rms_norm(h, w[p + ".post_attention_layernorm.weight"], self.eps, dt)
            a = po.silu_mul(self.lin(xn, p + ".mlp.gate_proj", L), self.lin(xn, p + ".mlp.up_proj", L), dt)
            h = po.add(h, self.lin(a, p + ".mlp.down_proj", L), dt)
        xn = po.rms_norm(h[-1:], w["model.norm.weight"], self.eps, dt)
        return self.lin(xn, "lm_head", 1)[0]


def check_updates(model, cfg, w, W, keep, updates, dtype="bfloat16"):
    """Feed `updates` (lists of token ids) through Model.__call__ on a fresh ring and through RefRotatingLlama: the last row's logits, the
    offset and the write index after every update, and finally the stored rows of layer 0 in the restatement's row order."""
    cache, ref = ring(model, W, keep), RefRotatingLlama(cfg, w, W, keep, dtype)
    for n, ids in enumerate(updates):
        ids = [int(t) for t in ids]
        got = model(torch.tensor([ids], device="cuda"), cache=cache)[0, -1].float().cpu().numpy()
        want = ref.forward(np.array(ids))
        assert_vec_close(got, want, dtype, what=f"W={W} keep={keep} update {n} (L={len(ids)})")
        assert cache[0].offset == ref.offset and cache[0].meta_state[3:] == (str(ref.offset), str(ref.idx))
    sk, _ = cache[0].state
    want_k = np.stack([ref.kv[0][r][0] for r in ref.rows], 1)
    assert_vec_close(sk[0].float().cpu().numpy(), want_k, dtype, what="stored rows")
    return cache


@pytest.mark.parametrize("W", [16, 32])
@pytest.mark.parametrize("keep", [0, 4])
def test_decoder_matches_the_oracle_restatement(tiny, W, keep):
    """A 24-token prompt (shorter and longer than the window), 3 W teacher-forced steps across the wrap, a 3-row and a 9-row chunk on the
    full ring, then more steps; the stored rows, offset and write index follow the restatement throughout."""
    g, cfg, w, model = tiny
    rng = np.random.default_rng(W + keep)
    V = cfg["vocab_size"]
    updates = [rng.integers(0, V, 24)] + [[t] for t in rng.integers(0, V, 3 * W)] + [rng.integers(0, V, 3), rng.integers(0, V, 9)] + \
        [[t] for t in rng.integers(0, V, 6)]
    cache = check_updates(model, cfg, w, W, keep, updates)
    assert cache[0].capacity <= 256  # the 24-row prompt's buffers; after the first step the window's


def test_decoder_8b_geometry_matches_the_oracle_restatement():
    """Two layers at Llama-3-8B geometry (H 4096, 32 / 8 heads, D 128): the RING step attention and the windowed pass the 8B model runs."""
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    cfg = {"model_type": "llama", "hidden_size": 4096, "num_hidden_layers": 2, "intermediate_size": 14336,
           "num_attention_heads": 32, "num_key_value_heads": 8, "rms_norm_eps": 1e-5, "vocab_size": 8192,
           "rope_theta": 500000.0, "max_position_embeddings": 8192, "tie_word_embeddings": False,
           "quantization": {"group_size": 64, "bits": 4}}
    w = po.synth_checkpoint(cfg, seed=1, dtype="bfloat16", lm_head_gain=4.0)
    model = Model(ModelArgs(**cfg), {k: codes_dev(v) if v.dtype == np.uint32 else to_dev(v, "bfloat16") for k, v in w.items()})
    rng = np.random.default_rng(8)
    W, V = 16, cfg["vocab_size"]
    updates = [rng.integers(0, V, 24)] + [[t] for t in rng.integers(0, V, 2 * W)] + [rng.integers(0, V, 3), rng.integers(0, V, 9)] + \
        [[t] for t in rng.integers(0, V, 4)]
    check_updates(model, cfg, w, W, 4, updates)


def test_updates_longer_than_a_prompt_chunk(tiny, knobs):
    """Prompt chunks of 16 rows: a 40-row prompt, then two 40-row updates back to back on the full ring (both start at row W), then steps.
    The pass advances its row state chunk by chunk; every update must start again from the row the host bound."""
    g, cfg, w, model = tiny
    knobs("prefill_chunk", 16)
    rng = np.random.default_rng(40)
    V = cfg["vocab_size"]
    updates = [rng.integers(0, V, 40), [5], [6], rng.integers(0, V, 40), rng.integers(0, V, 40)] + [[t] for t in rng.integers(0, V, 8)]
    check_updates(model, cfg, w, 32, 4, updates)


def test_buffers_shrink_back_to_the_window_after_a_long_prompt(tiny):
    g, cfg, w, model = tiny
    cache = ring(model, 64)
    model.step(torch.tensor(np.random.default_rng(3).integers(0, cfg["vocab_size"], 700), dtype=torch.int32, device="cuda"), cache)
    assert cache[0].capacity == 768
    for _ in range(3):
        model.step(None, cache)
    assert cache[0].capacity == 256 and cache[0].state[0].shape[2] == 64


def test_ring_wider_than_the_run_tracks_the_contiguous_cache(tiny):
    """Nothing evicted: the ring decoder (windowed pass, RING attention over the staged rows) follows the contiguous decoder, teacher-forced
    with the contiguous run's tokens, within the end-to-end tolerance."""
    g, cfg, w, model = tiny
    prompt = [int(t) for t in np.random.default_rng(5).integers(0, cfg["vocab_size"], 24)]
    a_cache, b_cache = model.make_cache(), ring(model, 512)
    ids = torch.tensor(prompt, dtype=torch.int32, device="cuda")
    for n in range(41):
        ta, _, la = model.step(ids, a_cache)
        la = la.float().cpu().numpy().copy()
        _, _, lb = model.step(ids, b_cache)
        assert_vec_close(lb.float().cpu().numpy(), la, "bfloat16", what=f"update {n}")
        ids = ta.clone().reshape(1)


def run(model, cache, prompt, n_steps, graph=True):
    tok, _, logits = model.step(torch.tensor(prompt, dtype=torch.int32, device="cuda"), cache, graph=graph)
    out, toks = [logits.float().cpu().numpy().copy()], [int(tok.item())]
    for _ in range(n_steps):
        tok, _, logits = model.step(None, cache, graph=graph)
        out.append(logits.float().cpu().numpy().copy())
        toks.append(int(tok.item()))
    return np.stack(out), toks


@pytest.mark.parametrize("W,n_prompt,n_steps", [(64, 9, 4 * 64), (1100, 1090, 40)])  # merged-split plan / combine plan, both across the wrap
def test_graph_replay_equals_eager_and_memory_is_bounded(tiny, W, n_prompt, n_steps):
    from proxy_inference_engine_amd.cache import RotatingKVCache
    g, cfg, w, model = tiny
    prompt = [int(t) for t in np.random.default_rng(W).integers(0, cfg["vocab_size"], n_prompt)]
    ca, cb = ring(model, W), ring(model, W)
    a, ta = run(model, ca, prompt, n_steps, graph=True)
    b, tb = run(model, cb, prompt, n_steps, graph=False)
    assert ta == tb and np.array_equal(a, b)
    # bounded: the buffers hold the window; offset, state and meta_state are those of the host protocol fed the same updates
    host = RotatingKVCache(W, keep=4)
    z = torch.zeros((1, 1, 1, 1))
    host.update_and_fetch(z.expand(1, 1, n_prompt, 1).contiguous(), z.expand(1, 1, n_prompt, 1).contiguous())
    for _ in range(n_steps):
        host.update_and_fetch(z, z)
    c = ca[0]
    assert c.offset == n_prompt + n_steps and c.meta_state == host.meta_state
    assert c.capacity <= ((max(W, n_prompt) + 255) // 256) * 256 and c.state[0].shape[2] == host.state[0].shape[2] == W


def test_save_load_continue_equals_uninterrupted(tiny, tmp_path):
    from proxy_inference_engine_amd.cache import BaseCache, RotatingKVCache
    g, cfg, w, model = tiny
    prompt = [int(t) for t in g["prompt"]]
    full, tf = run(model, ring(model, 16), prompt, 30)
    cache = ring(model, 16)
    part, tp = run(model, cache, prompt, 20)
    BaseCache.save_cache(str(tmp_path / "r.safetensors"), cache, {"n": "1"})
    loaded, meta = BaseCache.load_cache(str(tmp_path / "r.safetensors"))
    assert meta == {"n": "1"} and all(isinstance(c, RotatingKVCache) and c.meta_state == cache[0].meta_state for c in loaded)
    rest = []
    tok, _, logits = model.step(torch.tensor([tp[-1]], dtype=torch.int32, device="cuda"), loaded)
    rest.append(logits.float().cpu().numpy().copy())
    for _ in range(9):
        tok, _, logits = model.step(None, loaded)
        rest.append(logits.float().cpu().numpy().copy())
    assert np.array_equal(np.concatenate([part, np.stack(rest)]), full)


def test_generate_with_max_kv_size(tiny):
    from proxy_inference_engine_amd import InferenceEngine
    from proxy_inference_engine_amd.cache import BaseCache, RotatingKVCache
    g, cfg, w, model = tiny
    prompt = [int(t) for t in g["prompt"]]
    eng = InferenceEngine(model=model)
    out = [t for t, _ in eng.generate(prompt, max_completion_tokens=40, max_kv_size=16)]
    assert len(out) == 40 and all(isinstance(c, RotatingKVCache) and c.max_size == 16 for c in eng.prompt_cache.cache)
    cache = BaseCache.make_kv_cache(model, max_kv_size=16)
    _, toks = run(model, cache, prompt, 39)
    assert out == toks
    # the ring has evicted rows: a request sharing the prefix starts on fresh rings and decodes as a fresh engine
    again = [t for t, _ in eng.generate(prompt, max_completion_tokens=5, max_kv_size=16)]
    assert again == out[:5]
    # nothing evicted yet: the prefix is reused
    eng2 = InferenceEngine(model=model)
    first = [t for t, _ in eng2.generate(prompt[:4], max_completion_tokens=2, max_kv_size=64)]
    assert len(first) == 2 and eng2.prompt_cache.cache[0].is_trimmable()
    common = 4 + int(prompt[4] == first[0])  # the history is prompt[:4] + [first[0]]
    second = [t for t, _ in eng2.generate(prompt, max_completion_tokens=3, max_kv_size=64)]
    assert eng2.prompt_cache.cache[0].offset == len(prompt) + 2
    cache = BaseCache.make_kv_cache(model, max_kv_size=64)  # the same updates on a fresh ring: the reused rows, then the suffix
    model.step(torch.tensor(prompt[:4], dtype=torch.int32, device="cuda"), cache)
    if common == 5:
        model.step(torch.tensor(first[:1], dtype=torch.int32, device="cuda"), cache)
    _, want = run(model, cache, prompt[common:], 2)
    assert second == want


def test_refused_configurations_raise_without_launch(tiny):
    from proxy_inference_engine_amd import InferenceEngine, _ffi
    from proxy_inference_engine_amd.cache import RotatingKVCache
    g, cfg, w, model = tiny
    for W, keep in ((0, 0), (4, 4)):
        with pytest.raises(ValueError):
            RotatingKVCache(W, keep=keep)
    with pytest.raises(ValueError):
        next(iter(InferenceEngine(model=model).generate([1, 2, 3], max_kv_size=3)))  # keep=4 needs a window of 5+
    mixed = ring(model, 16)
    mixed[-1] = model.make_cache()[0]
    with pytest.raises(TypeError):
        model.step(torch.tensor([1, 2], dtype=torch.int32, device="cuda"), mixed)
    assert mixed[0].keys is None  # refused before anything was allocated or launched
    with pytest.raises(TypeError):
        model.step_batch(torch.tensor([1], dtype=torch.int32, device="cuda"), [ring(model, 16)])
    lib = _ffi.load()
    model._kv.invalidate()
    for W, keep in ((8, 8), (-1, 0)):
        rc = lib.pie_decoder_set_kv_ring(model._dec, W, keep, W, 0, 65536, _ffi.stream())
        assert rc < 0 and b"pie_decoder_set_kv_ring" in lib.pie_last_error()
    _, toks = run(model, model.make_cache(), [int(t) for t in g["prompt"]], 2)
    assert len(toks) == 3
