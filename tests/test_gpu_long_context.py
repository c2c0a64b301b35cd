"""-m gpu: long context at the Llama-3-8B head geometry (32 query heads, 8 kv-heads, head_dim 128) against the oracle.

Long context is reached by loading state, not by prefilling: one synthetic K / V history (tests/_util.kv_history: V with a non-zero mean,
marker rows of large |V| and K norm at row 0, row T - 1, both sides of every split boundary the plan uses and rows 8191 / 8192, poison
past T) goes into the product's cache through `state` / `meta_state` and, identically, into the oracle's.  Each 16-bit decoder case first
shows, on the CPU, that its data tells an off-by-one row apart: the step restated without the row T - 1 marker, and with the first poison
row attended, both miss the bound the product must then meet.  Bounds are the existing helpers' defaults (4-bit KV: the c = 16 of
test_gpu_kv_quant.test_decoder_matches_the_oracle_restatement, with its argument).
"""
import gc

import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests._util import (LONG_OP_CASES, LONG_OP_HKV, assert_bits_close, assert_vec_close, codes_dev, kv_history, long_op_case,
                         marker_rows, ordinary_row, sdpa_f64, to_bits, to_dev)
from tests.test_gpu_decode import build, margin_bound
from tests.test_gpu_kv_quant import RefQuantLlama
from tests.test_gpu_rotating import RefRotatingLlama

pytestmark = pytest.mark.gpu
DT = "bfloat16"
HKV, D, NL = 8, 128, 2
CFG = {"model_type": "llama", "hidden_size": 4096, "num_hidden_layers": NL, "intermediate_size": 14336,
       "num_attention_heads": 32, "num_key_value_heads": HKV, "rms_norm_eps": 1e-5, "vocab_size": 8192,
       "rope_theta": 500000.0, "max_position_embeddings": 131072, "tie_word_embeddings": False,
       "rope_scaling": {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                        "original_max_position_embeddings": 8192},
       "quantization": {"group_size": 64, "bits": 4}}


def round256(n):
    return (n + 255) // 256 * 256


def decoder_splits(cap, pinned=0):
    """plan_attention (decoder.hip) at 8 kv-heads: 4 splits merged by o_proj up to capacity 1024, then cap / 64 in [4, 32]."""
    if pinned:
        return min(pinned, 32)
    return 4 if cap <= 1024 else max(4, min(cap // 64, 256 // HKV, 32))


@pytest.fixture(scope="module")
def m8b():
    w = po.synth_checkpoint(CFG, seed=1, dtype=DT, lm_head_gain=4.0)
    return w, po.OracleLlama(CFG, w, DT), build(CFG, w)


def history(rng, T, cap, plans, more=(), cfg=CFG, dt=DT, **kw):
    """One (K, V) history [Hkv, cap, D] per layer (fp32, representable in T); `more`: marker rows besides marker_rows', with
    the K norm of rows 0 and T - 1.  cfg / dt: another geometry than this file's; kw: kv_history's scales."""
    more = [r for r in more if 0 <= r < T]
    rows = sorted(set(marker_rows(T, plans)) | set(more))
    return [kv_history(rng, cfg["num_key_value_heads"], T, cfg["head_dim"] if "head_dim" in cfg else D, dt, rows, cap=cap, strong=more, **kw)
            for _ in range(cfg["num_hidden_layers"])]


def dev_rows(x):
    return to_dev(po.to_bits(x, DT), DT)[None]


def product_cache(layers, T):
    """ReusableKVCache per layer: the loaded capacity's rows through `state`, then trim to T (the rows past T stay poison)."""
    from proxy_inference_engine_amd.cache import ReusableKVCache
    out = []
    for k, v in layers:
        c = ReusableKVCache()
        c.state = (dev_rows(k), dev_rows(v))
        assert c.trim(k.shape[1] - T) == k.shape[1] - T and c.offset == T
        out.append(c)
    return out


def oracle_cache(layers, T):
    out = []
    for k, v in layers:
        c = po.OracleKVCache()
        c.keys, c.values, c.offset = k[None].copy(), v[None].copy(), T
        out.append(c)
    return out


def ref_step16(w, freqs, token, pos, kv, extra=None, cfg=CFG, dt=DT, regime="qmv", new_row=None):
    """One 16-bit decode step composed from oracle primitives over explicit rows: kv[li] = (K, V) [Hkv, pos, D] cached, the new row at
    `pos`, then extra[li] (rows a kernel that reads past the end would see).  Returns the logits.  cfg / dt: another geometry than this
    file's; regime: the oracle's Linear regime for the pass's row count; new_row(li, k, v) -> (k, v): what the cache holds of the new row
    (an int8 page: its dequantised codes) and, as a side effect, a record of it."""
    e, Hq, HKV, NL = "model.embed_tokens", cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["num_hidden_layers"]
    D, DT = cfg["head_dim"] if "head_dim" in cfg else cfg["hidden_size"] // Hq, dt

    def lin(x, name):
        return po.quantized_matmul(x, w[name + ".weight"], w[name + ".scales"], w[name + ".biases"], group_size=64, bits=4, dtype=DT, regime=regime)

    h = po.dequantize(w[e + ".weight"][[token]], w[e + ".scales"][[token]], w[e + ".biases"][[token]], 64, 4, DT)
    for li in range(NL):
        p = f"model.layers.{li}"
        xn = po.rms_norm(h, w[p + ".input_layernorm.weight"], 1e-5, DT)
        q = po.rope(lin(xn, p + ".self_attn.q_proj").reshape(Hq, 1, D), freqs, pos, DT)
        k = po.rope(lin(xn, p + ".self_attn.k_proj").reshape(HKV, 1, D), freqs, pos, DT)
        v = lin(xn, p + ".self_attn.v_proj").reshape(HKV, 1, D)
        if new_row is not None:
            k, v = new_row(li, k, v)
        ks, vs = [kv[li][0], k], [kv[li][1], v]
        if extra is not None:
            ks.append(extra[li][0]), vs.append(extra[li][1])
        o = po.sdpa(q, np.concatenate(ks, 1), np.concatenate(vs, 1), D ** -0.5, None, DT, True)
        h = po.add(h, lin(po.round_T(o, DT).reshape(1, Hq * D), p + ".self_attn.o_proj"), DT)
        xn = po.rms_norm(h, w[p + ".post_attention_layernorm.weight"], 1e-5, DT)
        a = po.silu_mul(lin(xn, p + ".mlp.gate_proj"), lin(xn, p + ".mlp.up_proj"), DT)
        h = po.add(h, lin(a, p + ".mlp.down_proj"), DT)
    return lin(po.rms_norm(h, w["model.norm.weight"], 1e-5, DT), "lm_head")[0]


def sensitivity_self_check(w, orc, layers, T, token):
    """The first step restated without the row T - 1 marker and with the first poison row (T + 1: the step writes row T) attended:
    each must miss the bound.  Returns the unmodified restatement (checked against the oracle by the caller)."""
    kv = [(k[:, :T], v[:, :T]) for k, v in layers]
    base = ref_step16(w, orc.freqs, token, T, kv)
    no_marker = ref_step16(w, orc.freqs, token, T, [ordinary_row(k, v, T) for k, v in kv])
    poison = ref_step16(w, orc.freqs, token, T, kv, extra=[(k[:, T + 1:T + 2], v[:, T + 1:T + 2]) for k, v in layers])
    for what, got in (("without the row T - 1 marker", no_marker), ("with the first poison row", poison)):
        with pytest.raises(AssertionError):
            assert_vec_close(got, base, DT, what=what)
    return base


def decode(model, cache, first, n, graph):
    """n greedy steps from token `first`, each fed the decoder's own previous token: (input tokens, logits bits, output tokens)."""
    ins, bits, outs = [], [], []
    t = first
    for _ in range(n):
        ins.append(t)
        tok, _, logits = model.step(torch.tensor([t], dtype=torch.int32, device="cuda"), cache, graph=graph)
        bits.append(to_bits(logits).copy())
        t = int(tok.item())
        outs.append(t)
    return ins, bits, outs


def against_oracle(orc, ocache, run, what, first_want=None):
    ins, bits, outs = run
    for i, (t, b, tok) in enumerate(zip(ins, bits, outs)):
        want = orc.forward(np.array([t]), ocache)[0]
        if i == 0 and first_want is not None:
            assert_vec_close(first_want, want, DT, what=f"{what}: the restatement of step 0 against the oracle")
        assert_vec_close(po.from_bits(b, DT), want, DT, what=f"{what} step {i} offset {ocache[0].offset - 1}")
        top2 = np.sort(want)[-2:]
        if top2[1] - top2[0] > margin_bound(want):
            assert tok == int(np.argmax(want)), f"{what} step {i}"


def sixteen_bit_case(w, orc, model, T, seed, pinned=0, graph_modes=(False, True), n=8):
    cap = round256(T)
    plans = [(T + 1, decoder_splits(cap, pinned))]
    if T + n > cap:                                                   # the plan after the growth
        plans.append((cap + 1, decoder_splits(round256(max(int(cap * 1.5), cap + 1)), pinned)))
    rng = np.random.default_rng(seed)
    layers = history(rng, T, cap, plans)
    first = int(rng.integers(0, CFG["vocab_size"]))
    base = sensitivity_self_check(w, orc, layers, T, first)
    runs = {g: decode(model, product_cache(layers, T), first, n, g) for g in graph_modes}
    return layers, base, runs


# ------------------------------------------------------------------ 2. contiguous 16-bit decode
@pytest.mark.parametrize("T", [1020, 4097, 8193, 32766])
def test_decode_at_long_context_vs_oracle(m8b, T):
    """8 teacher-forced steps from T loaded positions: 1020 crosses capacity 1024 -> 1536 (fused 4-split plan -> 24 splits + combine,
    graph re-captured), 32766 crosses 32768 -> 49152.  Eager launches and graph replay are bit-equal."""
    w, orc, model = m8b
    layers, base, runs = sixteen_bit_case(w, orc, model, T, seed=T)
    (_, ea, ta), (_, ga, tg) = runs[False], runs[True]
    assert ta == tg and all(np.array_equal(a, b) for a, b in zip(ea, ga))
    ocache = oracle_cache(layers, T)
    del layers
    against_oracle(orc, ocache, runs[True], f"T={T}", first_want=base)


def test_fused_seam_across_the_plan_switch_at_1020(m8b, knobs):
    """T = 1020, capacity 1024 -> 1536 on the way: knob fuse_attn = 0 (two launches) gives bit-identical logits, tokens and caches; the
    graph holds n_layers launches more before the switch and the same number after it (no fusion with the combine plan)."""
    import ctypes as C
    from proxy_inference_engine_amd import _ffi
    w, orc, _ = m8b
    rng = np.random.default_rng(1020)
    layers = history(rng, 1020, 1024, [(1021, 4), (1025, 24)])
    first = int(rng.integers(0, CFG["vocab_size"]))
    out = {}
    for mode in (0, None):
        gc.collect()
        knobs("fuse_attn", mode)
        model = build(CFG, w)
        cache = product_cache(layers, 1020)
        ins, bits, outs = decode(model, cache, first, 1, True)
        before = model.graph_launches(True)
        more = decode(model, cache, outs[-1], 7, True)
        after = model.graph_launches(True)
        assert cache[0].capacity == 1536
        err = C.c_uint(1)
        _ffi.check(_ffi.load().pie_decoder_status(model._dec, C.byref(err)))
        assert err.value == 0
        out[mode] = (bits + more[1], outs + more[2], [(c.keys.clone(), c.values.clone()) for c in cache], before, after)
        del model, cache
    a, b = out[0], out[None]
    assert a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a[2], b[2]))
    assert a[3] - b[3] == NL and a[4] == b[4], (a[3], b[3], a[4], b[4])


def test_pinned_uneven_split_plan_vs_oracle(m8b):
    """kv_splits = 7 at T = 4097: chunk 586, the last split shorter than the others."""
    w, orc, _ = m8b
    gc.collect()
    model = build(CFG, w, kv_splits=7)
    layers, base, runs = sixteen_bit_case(w, orc, model, 4097, seed=7, pinned=7, graph_modes=(True,))
    del model
    ocache = oracle_cache(layers, 4097)
    del layers
    against_oracle(orc, ocache, runs[True], "kv_splits=7", first_want=base)


# ------------------------------------------------------------------ 3. a prompt suffix on a long cached prefix
@pytest.mark.parametrize("L,slack", [(6, 256), (33, 256), (200, 256), (6, 0)])
def test_prompt_suffix_on_a_32k_prefix_vs_oracle(m8b, L, slack):
    """PromptCache reuse: L new rows (the qmm regime) on 32768 loaded positions, last-row logits and hidden state, then 2 steps.
    slack 0: the loaded capacity is full, the suffix's rows cross the growth 32768 -> 49152.  Before the product runs, the prompt pass
    restated (RefQuantLlama's 16-bit prompt route) without the row T - 1 marker, and with the first poison row past the suffix attended
    by its last row (slack 256; at slack 0 the rows past T are the growth's zeros), must miss the bound."""
    w, orc, model = m8b
    T = 32768
    rng = np.random.default_rng(L + slack)
    cap = T + slack
    layers = history(rng, T, cap, [(T + 1, 32), (T + L, 32)])        # the split edges of the suffix's first and last rows
    ids = rng.integers(0, CFG["vocab_size"], L)
    ocache = oracle_cache(layers, T)
    want, want_h = orc.forward(ids, ocache, last_only=True, want_hidden=True)
    variants = [("without the row T - 1 marker", [ordinary_row(k[:, :T], v[:, :T], T) for k, v in layers], None)]
    if slack > L:
        variants.append(("with the first poison row", [(k[:, :T], v[:, :T]) for k, v in layers],
                         [(k[:, T + L:T + L + 1], v[:, T + L:T + L + 1]) for k, v in layers]))
    for what, kv, extra in variants:
        ref = RefQuantLlama(CFG, w, 8)
        ref.k, ref.v, ref.T = [k for k, _ in kv], [v for _, v in kv], T
        with pytest.raises(AssertionError):
            assert_vec_close(ref.forward(ids, quantized=False, extra=extra), want, DT, what=what)
    cache = product_cache(layers, T)
    del layers
    tok, _, logits = model.step(torch.from_numpy(ids).cuda(), cache)
    got, hid = logits.float().cpu().numpy(), model.hidden.float().cpu().numpy()
    assert cache[0].offset == T + L and cache[0].capacity == (cap if slack else 49152) == ocache[0].keys.shape[2]
    assert_vec_close(got, want, DT, what=f"suffix L={L} logits")
    assert_vec_close(hid, want_h[-1], DT, what=f"suffix L={L} hidden")
    against_oracle(orc, ocache, decode(model, cache, int(tok.item()), 2, True), f"after the L={L} suffix")


# ------------------------------------------------------------------ 4. quantized KV
def quant_triples(x, gs, bits):
    """po.quantize of the rows [Hkv, cap, D] -> (codes, scales, biases), each [Hkv, cap, ...]."""
    return tuple(a.reshape(HKV, x.shape[1], -1) for a in po.quantize(x.reshape(-1, D), gs, bits, DT))


@pytest.mark.parametrize("bits,gs", [(4, 64), (8, 64), (4, 32), (8, 128)])
def test_quantized_kv_at_32k_vs_the_restatement(m8b, bits, gs):
    """T = 32767 quantized rows loaded through state / meta_state (capacity 33024, the rows past T poison), 8 teacher-forced steps against
    RefQuantLlama seeded with the same codes.  Before the product runs, the first step restated without the row T - 1 marker and with the
    first poison row attended must miss the bound.  Bound: c = 4 at 8 bits, 16 at 4 bits (the argument of
    test_gpu_kv_quant.test_decoder_matches_the_oracle_restatement)."""
    from proxy_inference_engine_amd.cache import QuantizedKVCache
    w, orc, model = m8b
    T, cap = 32767, 33024
    rng = np.random.default_rng(bits * 100 + gs)
    layers = history(rng, T, cap, [(T + 1, 32)])
    ref = RefQuantLlama(CFG, w, bits, gs)
    cache, poison = [], []
    for li, (k, v) in enumerate(layers):
        kq, vq = quant_triples(k, gs, bits), quant_triples(v, gs, bits)
        ref.kq[li] = tuple(np.ascontiguousarray(a[:, :T]) for a in kq)
        ref.vq[li] = tuple(np.ascontiguousarray(a[:, :T]) for a in vq)
        poison.append(tuple(tuple(np.ascontiguousarray(a[:, T + 1:T + 2]) for a in t) for t in (kq, vq)))  # the step writes row T

        def dev(trip):
            c, s, b = trip
            return (codes_dev(c)[None], to_dev(s, DT)[None], to_dev(b, DT)[None])

        c = QuantizedKVCache(group_size=gs, bits=bits)
        c.state = (dev(kq), dev(vq))
        c.meta_state = ("256", str(T), str(gs), str(bits))
        cache.append(c)
    del layers
    ref.T = T
    cmax = 4.0 if bits == 8 else 16.0
    t = int(rng.integers(0, CFG["vocab_size"]))
    loaded = (list(ref.kq), list(ref.vq))
    base = ref.forward(np.array([t]), quantized=True)
    stepped = (list(ref.kq), list(ref.vq), ref.T)
    marker_gone = lambda trip: tuple(np.concatenate([a[:, :T - 1], a[:, 1:2]], axis=1) for a in trip)  # noqa: E731
    for what, kq, vq, extra in (("without the row T - 1 marker", [marker_gone(x) for x in loaded[0]], [marker_gone(x) for x in loaded[1]], None),
                                ("with the first poison row", loaded[0], loaded[1], poison)):
        ref.kq, ref.vq, ref.T = list(kq), list(vq), T
        got = ref.forward(np.array([t]), quantized=True, extra=extra)
        with pytest.raises(AssertionError):
            assert_vec_close(got, base, DT, c_max=cmax, c_rms=cmax, what=what)
    ref.kq, ref.vq, ref.T = stepped
    for i in range(8):
        tok, _, logits = model.step(torch.tensor([t], dtype=torch.int32, device="cuda"), cache)
        got = logits.float().cpu().numpy()
        want = base if i == 0 else ref.forward(np.array([t]), quantized=True)
        assert_vec_close(got, want, DT, c_max=cmax, c_rms=cmax, what=f"bits={bits} gs={gs} step {i}")
        t = int(tok.item())
    assert cache[0].offset == T + 8 and cache[0].capacity == cap


def test_quantized_from_cache_of_a_32k_cache_is_quantize(m8b):
    from proxy_inference_engine_amd.cache import QuantizedKVCache
    T = 32766
    rng = np.random.default_rng(5)
    layers = history(rng, T, 32768, [(T + 1, 32)])[:1]
    c16 = product_cache(layers, T)[0]
    for bits in (4, 8):
        q = QuantizedKVCache.from_cache(c16, group_size=64, bits=bits)
        assert q.offset == T and q.capacity == 32768
        for x, trip in ((layers[0][0], q.keys), (layers[0][1], q.values)):
            want = quant_triples(np.ascontiguousarray(x[:, :T]), 64, bits)
            assert np.array_equal(trip[0][0, :, :T].view(torch.int32).cpu().numpy().view(np.uint32), want[0])
            assert np.array_equal(to_bits(trip[1][0, :, :T]), want[1]) and np.array_equal(to_bits(trip[2][0, :, :T]), want[2])


# ------------------------------------------------------------------ 5. rotating cache
def ring_rows(off, W, keep):
    """Position held by every row of a ring at offset `off` (single steps from the start), and the write index."""
    if off < W:
        return list(range(off)), off
    span = W - keep
    rows = list(range(W))
    for r in range(keep, W):
        k = (off - 1 - W - (r - keep)) // span                       # the last pass of the write index over row r
        if k >= 0:
            rows[r] = W + (r - keep) + k * span
    return rows, keep + (off - W) % span


@pytest.mark.parametrize("off", [4095, 4100, 131075])
def test_rotating_cache_at_long_offsets_vs_the_restatement(m8b, off):
    """W = 4096, keep = 4: ring states loaded through state / meta_state at offset 4095 (the ring fills), 4100 (just wrapped) and 131075
    (positions past max_position_embeddings); single steps (4095: through the write index W -> keep), then a 9-row chunk on the full ring
    (the windowed prompt pass at a large offset); the stored K and V rows of every layer follow the restatement.  Before the product
    runs, the first step restated over the ring rows without the marker in the last buffer row, and with the row the step overwrites
    still attended (at 4095 the poison row, later the evicted position: a read of one row too many), must miss the bound."""
    from proxy_inference_engine_amd.cache import RotatingKVCache
    w, orc, model = m8b
    W, keep = 4096, 4
    rows, idx = ring_rows(off, W, keep)
    rng = np.random.default_rng(off)
    layers = history(rng, len(rows), W, [(min(off + 1, W), 32)], more=(idx - 1, idx))   # the newest row, the one the step overwrites
    ref = RefRotatingLlama(CFG, w, W, keep, DT)
    cache = []
    for li, (k, v) in enumerate(layers):
        ref.kv[li] = {p: (k[:, r], v[:, r]) for r, p in enumerate(rows)}
        c = RotatingKVCache(W, keep=keep)
        c.state = (dev_rows(k), dev_rows(v))
        c.meta_state = tuple(map(str, (keep, W, 256, off, idx)))
        cache.append(c)
    updates = [[int(t)] for t in rng.integers(0, CFG["vocab_size"], 6 if off < W else 3)] + [rng.integers(0, CFG["vocab_size"], 9)]
    loaded = [dict(d) for d in ref.kv]

    def restart(kv):
        ref.rows, ref.idx, ref.offset, ref.kv = list(rows), idx, off, [dict(d) for d in kv]

    restart(loaded)
    base = ref.forward(np.array(updates[0]))
    no_marker = [dict(d) for d in loaded]
    for d in no_marker:
        d[rows[-1]] = d[rows[1]]
    for what, kv, extra in (("without the last row's marker", no_marker, None),
                            ("with the overwritten row", loaded, [(k[:, idx:idx + 1], v[:, idx:idx + 1]) for k, v in layers])):
        restart(kv)
        with pytest.raises(AssertionError):
            assert_vec_close(ref.forward(np.array(updates[0]), extra=extra), base, DT, what=what)
    restart(loaded)
    del layers
    for n, ids in enumerate(updates):
        ids = [int(t) for t in ids]
        got = model(torch.tensor([ids], device="cuda"), cache=cache)[0, -1].float().cpu().numpy()
        want = ref.forward(np.array(ids))
        assert_vec_close(got, want, DT, what=f"offset {off} update {n} (L={len(ids)})")
        assert cache[0].offset == ref.offset and cache[0].meta_state[3:] == (str(ref.offset), str(ref.idx))
    for li in range(NL):
        sk, sv = cache[li].state
        for j, (what, x) in enumerate((("K", sk), ("V", sv))):
            want = np.stack([ref.kv[li][r][j] for r in ref.rows], 1)
            assert_vec_close(x[0].float().cpu().numpy(), want, DT, what=f"stored {what} rows of layer {li}")


# ------------------------------------------------------------------ 6. op level
@pytest.mark.parametrize("T,rep,D_,dt", LONG_OP_CASES)
def test_sdpa_decode_long_context_needles(T, rep, D_, dt):
    """pie_sdpa_decode at T up to 131071 (32 splits + combine), Hkv = 2, needles at row 0, T - 1 and every split edge, poisoned capacity
    past T (tests/test_long_context_data.py shows the data tells those rows apart under this bound), against a float64 reference: next
    to a needle the oracle's serial fp32 sum drops the ordinary rows' terms, by up to 3 ulps on 69 % of the elements at T = 131071."""
    from proxy_inference_engine_amd import hip_ops
    q, k, v = long_op_case(T, rep, D_, dt)
    Hq, cap = LONG_OP_HKV * rep, k.shape[1]
    want = sdpa_f64(q, k, v, D_ ** -0.5, T)
    dev = lambda x, n: to_dev(po.to_bits(x, dt), dt).view(1, n, -1, D_)  # noqa: E731
    got = hip_ops.scaled_dot_product_attention(dev(q, Hq), dev(k, LONG_OP_HKV), dev(v, LONG_OP_HKV), D_ ** -0.5, T=T)
    assert_bits_close(to_bits(got), po.to_bits(want, dt), max_ulp=2 if dt == "bfloat16" else 4, max_frac=0.05,
                      what=f"sdpa {Hq}/{LONG_OP_HKV} D{D_} T{T} cap{cap} {dt}")


@pytest.mark.parametrize("traditional", [False, True])
@pytest.mark.parametrize("offset", [8191, 8192, 65535, 131071])
def test_rope_at_long_offsets_with_llama3_scaling(offset, traditional):
    """hip_ops.rope with the Llama-3.1 scaled frequencies at positions up to 131071 + 2 (angles ~1e5 rad)."""
    from proxy_inference_engine_amd import hip_ops
    rs = CFG["rope_scaling"]
    rng = np.random.default_rng(offset + traditional)
    for Dr in (64, 128):
        f = po.llama3_rope_freqs(Dr, CFG["rope_theta"], float(CFG["max_position_embeddings"]), rs["factor"], rs["low_freq_factor"],
                                 rs["high_freq_factor"])
        x = po.round_T(rng.standard_normal((8, 3, Dr)), DT)
        got = hip_ops.rope(to_dev(po.to_bits(x, DT), DT), Dr, traditional=traditional, offset=offset, freqs=torch.from_numpy(f).cuda())
        assert_bits_close(to_bits(got), po.to_bits(po.rope(x, f, offset, DT, traditional), DT), what=f"rope D{Dr} offset {offset}")
