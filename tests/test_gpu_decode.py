"""-m gpu: the fused decode step / engine loop (HIP, through the C ABI) against the CPU oracle.

Parity bar: greedy token ids identical to the oracle on every teacher-forced step whose oracle
top-1/top-2 margin exceeds the 16-bit error bound; logits / logprobs / hidden states within
4 eps_T * max|ref| (max) and 4 eps_T * rms(ref) (rms), eps = 2^-8 (bf16) / 2^-11 (f16): tests/_util.py
assert_vec_close.  (BASELINE.md's absolute 2e-2 presumed O(1) logits; one bf16 ulp of a logit of 20 is 0.125.)
"""
import copy
import json

import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests._util import EPS, assert_vec_close, codes_dev, to_bits, to_dev

pytestmark = pytest.mark.gpu
DT = "bfloat16"


def margin_bound(logits, dtype=DT):
    """A greedy id is only required to match when the oracle's top-1/top-2 gap exceeds twice the logits bound."""
    return 2 * 4.0 * EPS[dtype] * float(np.abs(logits).max())


def device_weights(w: dict, dtype: str) -> dict:
    out = {}
    for k, v in w.items():
        out[k] = codes_dev(v) if v.dtype == np.uint32 else to_dev(v, dtype)
    return out


def build(cfg, w, dtype=DT, **kw):
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    return Model(ModelArgs(**cfg), device_weights(w, dtype), **kw)


@pytest.fixture(scope="module")
def tiny(golden_dir):
    g = np.load(golden_dir / "tiny_llama_w4_bf16.npz")
    cfg = json.loads(str(g["config_json"]))
    w = {k[2:]: g[k] for k in g.files if k.startswith("w:")}
    return g, cfg, w, build(cfg, w)


def test_model_call_matches_golden_prefill(tiny):
    g, cfg, w, model = tiny
    cache = model.make_cache()
    ids = torch.from_numpy(g["prompt"].astype(np.int64))[None].cuda()
    logits = model(ids, cache=cache)                                   # [1, L, V], lm_head on every position
    assert logits.shape == (1, len(g["prompt"]), cfg["vocab_size"]) and cache[0].offset == len(g["prompt"])
    assert_vec_close(logits[0, -1].float().cpu().numpy(), po.from_bits(g["prefill_last_logits"], DT), DT, what="prefill logits")
    assert_vec_close(model.hidden.float().cpu().numpy(), po.from_bits(g["prefill_hidden_last"], DT), DT, what="prefill hidden")
    # every position against the oracle (which also computes lm_head on all L positions)
    want = po.OracleLlama(cfg, w, DT).forward(g["prompt"], [po.OracleKVCache() for _ in range(cfg["num_hidden_layers"])])
    for l in range(len(g["prompt"])):
        assert_vec_close(logits[0, l].float().cpu().numpy(), want[l], DT, what=f"position {l}")
    assert cache[0].keys.shape == (1, cfg["num_key_value_heads"], 256, 64)   # step-256 capacity (reusable.py:154)


def test_engine_generate_step_matches_golden_tokens(tiny):
    from proxy_inference_engine_amd import InferenceEngine
    g, cfg, w, model = tiny
    eng = InferenceEngine(model=model)
    eng.prepare_engine(g["prompt"], temp=0)
    gen = eng.generate_step(torch.from_numpy(g["prompt"]))
    n = len(g["tokens"])
    mb = margin_bound(po.from_bits(g["prefill_last_logits"], DT))
    safe = int(np.argmax(g["margins"] < mb)) if (g["margins"] < mb).any() else n   # free-running prefix that must match
    for i in range(n):
        tok, lp = next(gen)
        lp = lp.cpu().numpy()
        if i < safe:
            assert int(tok.item()) == int(g["tokens"][i]), f"step {i}"
            assert_vec_close(lp, g["logprobs"][i], DT, what=f"logprobs step {i}")
        assert abs(np.exp(lp.astype(np.float64)).sum() - 1.0) < 1e-4
    assert safe >= 1
    assert eng.prompt_cache.cache[0].offset == len(g["prompt"]) + n - 1
    # second request with the same prompt: longest-common-prefix reuse re-processes exactly one token
    eng2_first = next(eng.generate_step(torch.from_numpy(g["prompt"])))[0]
    assert int(eng2_first.item()) == int(g["tokens"][0])
    assert eng.prompt_cache.cache[0].offset == len(g["prompt"])


def test_attention_warmup_cap_knob_changes_no_result(tiny, knobs):
    """PIE_KNOB_ATTN_WARM_MAX_MB: the attention launch's idle CUs read (and discard) at most that many MB of o_proj's weights to warm the
    Infinity Cache; 0 turns the role off.  A pure prefetch: the steps' logits are bit-identical with it off, capped to 1 MB and at the default."""
    g, cfg, w, model = tiny
    outs = []
    for mb in (0, 1, None):
        knobs("attn_warm_max_mb", mb)
        cache = model.make_cache()
        model.step(torch.from_numpy(g["prompt"]).cuda(), cache)
        bits = []
        for t in g["tokens"][:6]:
            _, _, logits = model.step(torch.tensor([int(t)], dtype=torch.int32, device="cuda"), cache, graph=False)
            bits.append(to_bits(logits).copy())
        outs.append(bits)
    for other in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], other))


def test_teacher_forced_steps_and_graph_replay_identical(tiny):
    g, cfg, w, model = tiny
    orc = po.OracleLlama(cfg, w, DT)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    orc.forward(g["prompt"], ocache)
    results = {}
    for graph in (False, True):
        cache = model.make_cache()
        model.step(torch.from_numpy(g["prompt"]).cuda(), cache)
        out = []
        for i, t in enumerate(g["tokens"][:-1]):
            tok, lp, logits = model.step(torch.tensor([int(t)], dtype=torch.int32, device="cuda"), cache, graph=graph)
            out.append((int(tok.item()), to_bits(logits).copy(), lp.cpu().numpy().copy()))
        results[graph] = out
    for (ta, la, _), (tb, lb, _) in zip(results[False], results[True]):
        assert ta == tb and np.array_equal(la, lb)                     # graph replay == eager launches, bit for bit
    checked = 0
    for i, t in enumerate(g["tokens"][:-1]):                           # teacher-forced against the oracle
        want = orc.forward(np.array([t]), ocache)[0]
        otok, olp = po.logprobs_argmax(want)
        tok, lbits, lp = results[True][i]
        assert_vec_close(po.from_bits(lbits, DT), want, DT, what=f"logits step {i}")
        assert_vec_close(lp, olp, DT, what=f"logprobs step {i}")
        top2 = np.sort(olp)[-2:]
        if top2[1] - top2[0] > margin_bound(want):
            assert tok == otok, f"step {i}"
            checked += 1
    assert checked >= 3


def test_step_equals_its_kernels_launched_by_name(tiny):
    """pie_decoder_step on an int4 checkpoint folds the embedding launch into layer 0's q|k|v launch (PRO_EMBED: every workgroup dequantises
    the token's row itself, workgroup 0 leaves the row in the residual stream and the step's RoPE table).  Launched by name
    (pie_decoder_launch_kernel) the embedding and layer 0's q|k|v are still two kernels: the logits of both routes must be the same bits."""
    g, cfg, w, model = tiny
    cache = model.make_cache()
    model.step(torch.from_numpy(g["prompt"]).cuda(), cache)
    for _ in range(3):
        # by name: does not advance the state, appends the same K / V rows the step will write again
        model.launch_kernel("embed")
        for li in range(cfg["num_hidden_layers"]):
            for name in ("qkv", "attn", "o_proj", "gate_up", "down"):
                model.launch_kernel(name, li)
        model.launch_kernel("lm_head")
        torch.cuda.synchronize()
        by_name = to_bits(model.logits).copy()
        hidden_by_name = to_bits(model.hidden).copy()
        tok, lp, logits = model.step(None, cache)
        assert np.array_equal(to_bits(logits), by_name), "the step's logits differ from its kernels launched one by one"
        assert np.array_equal(to_bits(model.hidden), hidden_by_name)


@pytest.mark.parametrize("merge_cap", [None, 256])
def test_cache_growth_across_step_boundary(tiny, merge_cap, knobs):
    """Decode across the 256-position capacity boundary: the cache re-allocates (256 -> 512) and the decoder must
    pick up the new buffers; compare logits right before / after the growth with the oracle.  merge_cap = 256 also
    moves the attention plan at the boundary: 4 splits merged by the o_proj prologue -> 8 splits + k_attn_combine, so the
    captured graph has to be rebuilt mid-stream."""
    g, cfg, w, model = tiny
    if merge_cap:
        knobs("attn_merge_max_cap", merge_cap)
        model = build(cfg, w)
    rng = np.random.default_rng(21)
    prompt = rng.integers(0, cfg["vocab_size"], 250)
    forced = rng.integers(0, cfg["vocab_size"], 12)
    orc = po.OracleLlama(cfg, w, DT)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    orc.forward(prompt, ocache)
    cache = model.make_cache()
    model.step(torch.from_numpy(prompt).cuda(), cache)
    assert cache[0].capacity == 256
    for i, t in enumerate(forced):
        want = orc.forward(np.array([t]), ocache)[0]
        _, _, logits = model.step(torch.tensor([int(t)], dtype=torch.int32, device="cuda"), cache)
        assert_vec_close(logits.float().cpu().numpy(), want, DT, what=f"step {i} offset {cache[0].offset}")
    assert cache[0].capacity == 512 and cache[0].offset == 262 and ocache[0].keys.shape[2] == 512
    assert float(cache[0].keys[0, :, 262:].abs().max()) == 0.0        # untouched tail stays zero-initialised


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_llama8b_shaped_layers_vs_oracle(dtype):
    """Real kernel geometry (H=4096, I=14336, 32/8 heads, D=128: K slices 2 and 7), 2 layers, V=8192."""
    cfg = {"model_type": "llama", "hidden_size": 4096, "num_hidden_layers": 2, "intermediate_size": 14336,
           "num_attention_heads": 32, "num_key_value_heads": 8, "rms_norm_eps": 1e-5, "vocab_size": 8192,
           "rope_theta": 500000.0, "max_position_embeddings": 8192, "tie_word_embeddings": False,
           "quantization": {"group_size": 64, "bits": 4}}
    w = po.synth_checkpoint(cfg, seed=1, dtype=dtype, lm_head_gain=4.0)
    model = build(cfg, w, dtype)
    orc = po.OracleLlama(cfg, w, dtype)
    prompt = np.random.default_rng(2).integers(0, cfg["vocab_size"], 6)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    want = orc.forward(prompt, ocache)[-1]
    cache = model.make_cache()
    tok, lp, logits = model.step(torch.from_numpy(prompt).cuda(), cache)
    assert_vec_close(logits.float().cpu().numpy(), want, dtype, what="prefill")
    for _ in range(3):
        t = int(tok.item())
        want = orc.forward(np.array([t]), ocache)[0]
        otok, olp = po.logprobs_argmax(want)
        tok, lp, logits = model.step(tok, cache)
        assert_vec_close(logits.float().cpu().numpy(), want, dtype, what="decode")
        top2 = np.sort(olp)[-2:]
        if top2[1] - top2[0] > margin_bound(want, dtype):
            assert int(tok.item()) == otok
    assert model.step_bytes(128) == sum(
        (n * k // 2 + 2 * (n * k // 64) * 2) for n, k in [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336)]) * 2 \
        + 2 * (2 * 4096 * 2 + 2 * 1024 * 2 * 128 + 2 * 1024 * 2) + (8192 * 4096 // 2 + 2 * (8192 * 4096 // 64) * 2) + 4096 * 2 + 8192 * 4


@pytest.mark.parametrize("dtype,quant", [("bfloat16", {"group_size": 64, "bits": 4}), ("float16", {"group_size": 64, "bits": 4}), ("bfloat16", None),
                                         ("bfloat16", {"group_size": 64, "bits": 8}), ("float16", {"group_size": 32, "bits": 4})])
def test_attention_behind_the_qkv_launch_seam_is_the_two_launches_bit_for_bit(dtype, quant, knobs):
    """32 / 8 / 128 heads (Llama-3-8B, Mistral-7B): the step's attention runs inside the q|k|v launch, behind an XCD-local seam (the rows of a
    kv-group are computed by the 32 workgroups of one XCD, which hand q / k / v to the group's attention workgroups through that XCD's L2:
    w4_gemv.hpp FUSE).  Same rows, same units, same order: knob fuse_attn = 0 (two launches) gives identical logits, caches and tokens, eagerly and
    through the replayed graph, across a cache growth, and the graph holds one launch per layer less."""
    import ctypes as C
    from proxy_inference_engine_amd import _ffi
    cfg = {"model_type": "llama", "hidden_size": 4096, "num_hidden_layers": 3, "intermediate_size": 14336,
           "num_attention_heads": 32, "num_key_value_heads": 8, "rms_norm_eps": 1e-5, "vocab_size": 8192,
           "rope_theta": 500000.0, "max_position_embeddings": 8192, "tie_word_embeddings": False}
    if quant:                        # int4 g=64 (the metric's format), dense 16-bit, int8, int4 g=32: every streaming format of the q|k|v matrix
        cfg["quantization"] = quant
    w = po.synth_checkpoint(cfg, seed=3, dtype=dtype, lm_head_gain=4.0)
    prompt = torch.from_numpy(np.random.default_rng(5).integers(0, cfg["vocab_size"], 250)).cuda()
    runs = {}
    for mode in (0, None):
        knobs("fuse_attn", mode)
        model = build(cfg, w, dtype)
        cache = model.make_cache()
        tok, _, logits = model.step(prompt, cache)
        rows = [logits.clone()]
        toks = [int(tok.item())]
        for _ in range(12):          # 250 + 12 tokens: the cache grows from 256 to 512 rows on the way
            tok, _, logits = model.step(tok, cache)
            rows.append(logits.clone()), toks.append(int(tok.item()))
        launches = model.graph_launches(True)
        runs[mode] = (torch.stack(rows), toks, cache[0].keys.clone(), cache[2].values.clone(), launches)
        err = C.c_uint(1)
        _ffi.check(_ffi.load().pie_decoder_status(model._dec, C.byref(err)))
        assert err.value == 0                                            # no bounded wait of the seam ever gave up
    a, b = runs[0], runs[None]
    assert a[1] == b[1] and torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert a[4] - b[4] == cfg["num_hidden_layers"], (a[4], b[4])
    # ... and on scattered 64-token T pages (the seam form of the paged attention body): across page boundaries, same logits as the contiguous cache
    paged = {}
    for mode in (0, None):
        knobs("fuse_attn", mode)
        model = build(cfg, w, dtype)
        pool = model.enable_paged_kv(num_pages=16, max_blocks=8)
        for _ in range(3):
            pool.allocate_page()
        pool.free_page(1)
        cache = model.make_cache()
        tok, _, logits = model.step(prompt[:120], cache)
        rows = [logits.clone()]
        for _ in range(12):          # positions 120 .. 131: the step at 128 opens a new page
            tok, _, logits = model.step(tok, cache)
            rows.append(logits.clone())
        paged[mode] = (torch.stack(rows), model.graph_launches(True))
    assert torch.equal(paged[0][0], paged[None][0]) and paged[0][1] - paged[None][1] == cfg["num_hidden_layers"]
    # ... with a pinned split count (1 / 2: four / eight attention workgroups per kv-group instead of sixteen)
    if quant == {"group_size": 64, "bits": 4} and dtype == "bfloat16":
        for splits in (1, 2):
            pinned = {}
            for mode in (0, None):
                knobs("fuse_attn", mode)
                model = build(cfg, w, dtype, kv_splits=splits)
                cache = model.make_cache()
                tok, _, logits = model.step(prompt[:70], cache)
                rows = [logits.clone()]
                for _ in range(6):
                    tok, _, logits = model.step(tok, cache)
                    rows.append(logits.clone())
                pinned[mode] = (torch.stack(rows), model.graph_launches(True))
            assert torch.equal(pinned[0][0], pinned[None][0]) and pinned[0][1] - pinned[None][1] == cfg["num_hidden_layers"], splits
    # ... and the library withdraws the fusion (and re-captures the graph) while the process holds more than four decoders: a waiting launch must
    # never starve another launch's producers
    knobs("fuse_attn", None)
    import gc
    gc.collect()
    model = build(cfg, w, dtype)
    cache = model.make_cache()
    tok, _, _ = model.step(prompt[:40], cache)
    for _ in range(3):
        tok, _, _ = model.step(tok, cache)
    fused_launches = model.graph_launches(True)
    small = dict(cfg, hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=1, vocab_size=512)
    ws = po.synth_checkpoint(small, seed=1, dtype=dtype)
    crowd = [build(small, ws, dtype) for _ in range(5)]
    tok, _, la = model.step(tok, cache)
    crowded_launches = model.graph_launches(True)
    del crowd
    gc.collect()
    assert crowded_launches - fused_launches in (0, cfg["num_hidden_layers"])   # (0: other tests' models already crowded the process)
    assert crowded_launches == a[4]                                                # the two-launch graph


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_tinyllama_shaped_layers_vs_oracle(dtype):
    """BASELINE.json configs[0] geometry (TinyLlama-1.1B: H=2048, I=5632 = 2.75 K-slices, 32/4 heads -> 8 q-heads per
    kv-head, D=64, V=32000), 2 layers, int4 g=64: ragged last K slice, REP=8 attention, D=64 RoPE / cache rows."""
    cfg = {"model_type": "llama", "hidden_size": 2048, "num_hidden_layers": 2, "intermediate_size": 5632,
           "num_attention_heads": 32, "num_key_value_heads": 4, "rms_norm_eps": 1e-5, "vocab_size": 32000,
           "rope_theta": 10000.0, "max_position_embeddings": 2048, "tie_word_embeddings": False,
           "quantization": {"group_size": 64, "bits": 4}}
    w = po.synth_checkpoint(cfg, seed=4, dtype=dtype, lm_head_gain=4.0)
    model = build(cfg, w, dtype)
    orc = po.OracleLlama(cfg, w, dtype)
    prompt = np.random.default_rng(8).integers(0, cfg["vocab_size"], 70)       # > 64 positions: several attention splits
    ocache = [po.OracleKVCache() for _ in orc.layers]
    want = orc.forward(prompt, ocache)[-1]
    cache = model.make_cache()
    tok, lp, logits = model.step(torch.from_numpy(prompt).cuda(), cache)
    assert_vec_close(logits.float().cpu().numpy(), want, dtype, what="prefill")
    matched = 0
    for _ in range(4):
        t = int(tok.item())
        want = orc.forward(np.array([t]), ocache)[0]
        otok, olp = po.logprobs_argmax(want)
        tok, lp, logits = model.step(None, cache)                               # device-side feed-back of the greedy token
        assert_vec_close(logits.float().cpu().numpy(), want, dtype, what="decode")
        top2 = np.sort(olp)[-2:]
        if top2[1] - top2[0] > margin_bound(want, dtype):
            assert int(tok.item()) == otok
            matched += 1
    assert cache[0].keys.shape == (1, 4, 256, 64) and cache[0].offset == 74 and matched >= 1


def test_long_generation_across_growth_and_plan_switch(tiny):
    """1300 graph-replayed decode steps after a 12-token prompt: the cache re-allocates 256 -> 512 -> 768 -> 1280 -> 2048
    (x1.5 rounded up to the 256 step, reusable.py:167-203) and past capacity 1024 the attention plan moves from 4 merged
    splits to 20 splits + combine, so
    the graph is re-captured mid-stream.  Teacher-forced with the oracle's greedy tokens; logits compared around every
    boundary and every 100 steps."""
    g, cfg, w, model = tiny
    orc = po.OracleLlama(cfg, w, DT)
    prompt = np.random.default_rng(44).integers(0, cfg["vocab_size"], 12)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    want = orc.forward(prompt, ocache, last_only=True)
    cache = model.make_cache()
    tok, lp, logits = model.step(torch.from_numpy(prompt).cuda(), cache)
    assert_vec_close(logits.float().cpu().numpy(), want, DT, what="prompt")
    check = set(range(0, 1300, 100)) | {o - 12 + d for o in (256, 512, 768, 1024, 1280) for d in (-2, -1, 0, 1)}
    caps = set()
    for i in range(1300):
        t = int(np.argmax(want))                                        # the oracle's greedy token feeds both sides
        want = orc.forward(np.array([t]), ocache)[0]
        tok, lp, logits = model.step(torch.tensor([t], dtype=torch.int32, device="cuda"), cache)
        caps.add(cache[0].capacity)
        if i in check:
            assert_vec_close(logits.float().cpu().numpy(), want, DT, what=f"step {i} offset {cache[0].offset} capacity {cache[0].capacity}")
    assert caps == {256, 512, 768, 1280, 2048} and cache[0].offset == 12 + 1300 == ocache[0].offset
    assert ocache[0].keys.shape[2] == cache[0].capacity             # the oracle's ReusableKVCache restatement grew the same way


def test_forced_split_counts_match_oracle(tiny):
    """kv_splits pins the attention plan: 1 and 4 (merged in the o_proj prologue), 8 and 32 (k_attn_combine launch)."""
    g, cfg, w, _ = tiny
    orc = po.OracleLlama(cfg, w, DT)
    prompt = np.random.default_rng(5).integers(0, cfg["vocab_size"], 150)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    want = orc.forward(prompt, ocache, last_only=True)
    ref_bits = None
    for splits in (1, 4, 8, 32):
        model = build(cfg, w, kv_splits=splits)
        cache = model.make_cache()
        _, _, logits = model.step(torch.from_numpy(prompt).cuda(), cache)
        assert_vec_close(logits.float().cpu().numpy(), want, DT, what=f"kv_splits={splits}")
        if splits == 4:
            ref_bits = to_bits(logits).copy()
    assert ref_bits is not None


def test_batched_prefill_chunks_and_regimes(tiny, knobs):
    """Prompt processing.  Prompts of >= 6 tokens (knob prefill_min) run as batched GEMMs on weights
    dequantised to T (MLX's qmm regime, oracle qmm_min_rows = 6), in chunks of `prefill_chunk` rows; shorter ones as
    iterated decode steps (qmv regime: exact fp32 affine sums).  Both against the oracle in the matching regime, every
    position, with a ragged last chunk (100 = 3 x 32 + 4) and a second call that continues at a non-zero offset."""
    g, cfg, w, model = tiny
    rng = np.random.default_rng(31)
    prompt, more = rng.integers(0, cfg["vocab_size"], 100), rng.integers(0, cfg["vocab_size"], 40)
    orc = po.OracleLlama(cfg, w, DT)
    # prefill_resident = 0: every chunk dequantises into the scratch again (the other prefill tests keep resident copies)
    for regime, rows, env in (("batched", 6, {"prefill_chunk": 32, "prefill_resident": 0}), ("iterated", 0, {"prefill_min": 100000})):
        for k in ("prefill_chunk", "prefill_min", "prefill_resident"):
            knobs(k, None)
        for k, v in env.items():
            knobs(k, v)
        po.set_qmm_min_rows(rows)
        try:
            ocache = [po.OracleKVCache() for _ in orc.layers]
            want1 = orc.forward(prompt, ocache)
            want2 = orc.forward(more, ocache)
        finally:
            po.set_qmm_min_rows(6)
        m = build(cfg, w) if regime == "batched" else model        # a fresh decoder: the resident budget is fixed at first use
        cache = m.make_cache()
        got1 = m(torch.from_numpy(prompt)[None].cuda(), cache=cache)[0].float().cpu().numpy()
        got2 = m(torch.from_numpy(more)[None].cuda(), cache=cache)[0].float().cpu().numpy()
        assert cache[0].offset == 140
        for l in range(100):
            assert_vec_close(got1[l], want1[l], DT, what=f"{regime} position {l}")
        for l in range(40):
            assert_vec_close(got2[l], want2[l], DT, what=f"{regime} continuation position {100 + l}")
        # the cache rows written by the batched RoPE + append kernel, against the oracle's cache
        k_gpu = cache[0].keys[0, :, :140].float().cpu().numpy()
        assert_vec_close(k_gpu.ravel(), ocache[0].keys[0, :, :140].ravel(), DT, what=f"{regime} layer-0 keys")


@pytest.mark.parametrize("L", [6, 9, 16, 24, 32, 33])
def test_short_prompt_int4_gemm_paths(tiny, knobs, L):
    """Prompts of 6..33 tokens on the three int4 GEMM paths: the weight-streaming k_w4r_gemm (default), round 2's kernels (knob w4r = 0: the
    one-strip few-row kernel up to 32 rows, the many-row tile kernel at 33) and, with small_m = 0 as well, the many-row tile kernel below 33
    rows too: same qmm contract, every position against the oracle, and the paths within one rounding of each other."""
    g, cfg, w, _ = tiny
    rng = np.random.default_rng(L)
    prompt = rng.integers(0, cfg["vocab_size"], L)
    orc = po.OracleLlama(cfg, w, DT)
    want = orc.forward(prompt, [po.OracleKVCache() for _ in orc.layers])
    outs = {}
    for name, w4r, small in (("w4r", None, None), ("round-2 kernels", 0, 32), ("many-row kernel", 0, 0)):
        knobs("w4r", w4r)
        knobs("small_m", small)
        m = build(cfg, w)
        cache = m.make_cache()
        got = m(torch.from_numpy(prompt)[None].cuda(), cache=cache)[0].float().cpu().numpy()
        for l in range(L):
            assert_vec_close(got[l], want[l], DT, what=f"{name} L={L} position {l}")
        tok, _, logits = m.step(None, cache)                           # decode continues on the cache the short prompt filled
        outs[name] = (got, logits.float().cpu().numpy())
    for name in ("round-2 kernels", "many-row kernel"):
        assert_vec_close(outs["w4r"][0][-1], outs[name][0][-1], DT, what=f"w4r vs {name}")
        assert_vec_close(outs["w4r"][1], outs[name][1], DT, what=f"decode after w4r vs {name} prompt")


@pytest.mark.parametrize("L", [30, 40])
def test_short_prompt_int4_gemm_paths_with_linear_biases(knobs, L):
    """The Linear biases (attention_bias / mlp_bias) on each int4 many-row route of the tiny model: k_w4r_gemm (default); with knob w4r = 0 the
    few-row kernel's store / SwiGLU / RoPE epilogues at 30 rows and the tile kernels at 40 (gate|up declined for fusion because of its bias; down,
    K = 704 = 11 groups, on the 8-wave k_w4l_gemm, the K = 256 matrices on k_w4l2_gemm); with small_m = 0 as well the tile kernels at 30 rows too.
    Every position against the oracle, then one decode step on the cache the prompt filled."""
    cfg = dict(po.TINY_CONFIG, attention_bias=True, mlp_bias=True, tie_word_embeddings=False)
    w = po.synth_checkpoint(cfg, seed=33, dtype=DT, lm_head_gain=4.0)
    assert "model.layers.0.self_attn.k_proj.bias" in w and "model.layers.1.mlp.down_proj.bias" in w
    prompt = np.random.default_rng(L).integers(0, cfg["vocab_size"], L)
    orc = po.OracleLlama(cfg, w, DT)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    want = orc.forward(prompt, ocache)
    want_next = {}                                                     # the oracle's decode step per token a route sampled (one, bar a near-tie)
    for name, w4r, small in (("w4r", None, None), ("round-2 kernels", 0, 32), ("many-row kernel", 0, 0)):
        knobs("w4r", w4r)
        knobs("small_m", small)
        m = build(cfg, w)
        cache = m.make_cache()
        got = m(torch.from_numpy(prompt)[None].cuda(), cache=cache)[0].float().cpu().numpy()
        for l in range(L):
            assert_vec_close(got[l], want[l], DT, what=f"bias, {name} L={L} position {l}")
        t = int(m.token.item())
        if t not in want_next:
            want_next[t] = orc.forward(np.array([t]), copy.deepcopy(ocache))[0]
        tok, _, logits = m.step(None, cache)
        assert_vec_close(logits.float().cpu().numpy(), want_next[t], DT, what=f"bias, decode after {name} L={L}")


def test_batched_prefill_llama8b_shapes(knobs):
    """The real GEMM shapes (N = 6144 / 4096 / 28672, K = 4096 / 14336) on two Llama-3-8B-shaped layers: 48-token prompt
    through the batched path, then decode steps on the cache it filled."""
    dtype = "bfloat16"
    cfg = {"model_type": "llama", "hidden_size": 4096, "num_hidden_layers": 2, "intermediate_size": 14336,
           "num_attention_heads": 32, "num_key_value_heads": 8, "rms_norm_eps": 1e-5, "vocab_size": 8192,
           "rope_theta": 500000.0, "max_position_embeddings": 8192, "tie_word_embeddings": False,
           "quantization": {"group_size": 64, "bits": 4}}
    w = po.synth_checkpoint(cfg, seed=3, dtype=dtype, lm_head_gain=4.0)
    model = build(cfg, w, dtype)
    orc = po.OracleLlama(cfg, w, dtype)
    prompt = np.random.default_rng(12).integers(0, cfg["vocab_size"], 48)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    want, hid = orc.forward(prompt, ocache, last_only=True, want_hidden=True)
    cache = model.make_cache()
    tok, lp, logits = model.step(torch.from_numpy(prompt).cuda(), cache)
    assert_vec_close(model.hidden.float().cpu().numpy(), hid[-1], dtype, what="prefill hidden")
    assert_vec_close(logits.float().cpu().numpy(), want, dtype, what="prefill logits")
    for _ in range(2):
        t = int(tok.item())
        want = orc.forward(np.array([t]), ocache)[0]
        tok, lp, logits = model.step(None, cache)
        assert_vec_close(logits.float().cpu().numpy(), want, dtype, what="decode after batched prefill")


@pytest.mark.parametrize("bias,L", [(False, 200), (True, 200), (False, 70)])
def test_k_split_prompt_gemm_slabs_summed_by_their_consumers(knobs, bias, L):
    """Prompts of a few dozen to a few hundred rows split K in the many-row int4 GEMM; the fp32 partial slabs are summed by the kernels that
    consume the product (RoPE + append for q|k|v, residual add + RMSNorm for o_proj / down) instead of a reduce launch of their own.  Same
    arithmetic in the same order: logits, hidden state and the decode steps that follow are bit-identical to the reduce-launch form
    (knob w4l_slabs = 0), and both follow the oracle.  Two Llama-3-8B-shaped layers, 200- and 70-token prompts; with Linear biases the q|k|v product
    keeps its reduce launch and o_proj / down add the bias after their own rounding."""
    dtype = "bfloat16"
    cfg = {"model_type": "llama", "hidden_size": 4096, "num_hidden_layers": 2, "intermediate_size": 14336,
           "num_attention_heads": 32, "num_key_value_heads": 8, "rms_norm_eps": 1e-5, "vocab_size": 8192,
           "rope_theta": 500000.0, "max_position_embeddings": 8192, "tie_word_embeddings": False,
           "attention_bias": bias, "mlp_bias": bias, "quantization": {"group_size": 64, "bits": 4}}
    w = po.synth_checkpoint(cfg, seed=5, dtype=dtype, lm_head_gain=4.0)
    orc = po.OracleLlama(cfg, w, dtype)
    prompt = np.random.default_rng(21).integers(0, cfg["vocab_size"], L)   # (70 rows: the RoPE consumer runs four workgroups per row)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    want, hid = orc.forward(prompt, ocache, last_only=True, want_hidden=True)
    outs = {}
    for mode in ("1", "0"):
        knobs("w4l_slabs", int(mode))
        model = build(cfg, w, dtype)
        cache = model.make_cache()
        tok, lp, logits = model.step(torch.from_numpy(prompt).cuda(), cache)
        rec = [model.hidden.clone(), logits.clone(), int(tok.item())]
        for _ in range(2):
            tok, lp, logits = model.step(None, cache)
            rec += [logits.clone(), int(tok.item())]
        outs[mode] = rec
    assert_vec_close(outs["1"][0].float().cpu().numpy(), hid[-1], dtype, what="prefill hidden")
    assert_vec_close(outs["1"][1].float().cpu().numpy(), want, dtype, what="prefill logits")
    for a, b in zip(outs["1"], outs["0"]):
        if isinstance(a, int):
            assert a == b
        else:
            assert torch.equal(a, b), "slab-consuming kernels differ from the reduce launch"


@pytest.mark.parametrize("L", [9, 24, 32, 64, 100, 130, 200, 256])
def test_prompt_rows_on_8b_shapes_weight_streaming_gemm_vs_round2_kernels(knobs, L):
    """Prompts / suffixes of 9..256 rows on the real layer shapes: k_w4r_gemm in each of its row-block geometries (1, 2, 4, 5, 7 -> 8, 8 blocks) --
    gate|up with the SwiGLU epilogue, q|k|v / o_proj / down as K-split fp32 slabs summed by their consumers -- against the oracle and against
    round 2's kernels (knob w4r = 0); the two differ only in the order of fp32 additions."""
    dtype = "bfloat16"
    cfg = {"model_type": "llama", "hidden_size": 4096, "num_hidden_layers": 2, "intermediate_size": 14336,
           "num_attention_heads": 32, "num_key_value_heads": 8, "rms_norm_eps": 1e-5, "vocab_size": 8192,
           "rope_theta": 500000.0, "max_position_embeddings": 8192, "tie_word_embeddings": False,
           "quantization": {"group_size": 64, "bits": 4}}
    w = po.synth_checkpoint(cfg, seed=9, dtype=dtype, lm_head_gain=4.0)
    orc = po.OracleLlama(cfg, w, dtype)
    prompt = np.random.default_rng(L).integers(0, cfg["vocab_size"], L)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    want, hid = orc.forward(prompt, ocache, last_only=True, want_hidden=True)
    outs = {}
    for mode in (None, 0):
        knobs("w4r", mode)
        model = build(cfg, w, dtype)
        cache = model.make_cache()
        tok, lp, logits = model.step(torch.from_numpy(prompt).cuda(), cache)
        assert_vec_close(model.hidden.float().cpu().numpy(), hid[-1], dtype, what=f"hidden, w4r={mode}")
        assert_vec_close(logits.float().cpu().numpy(), want, dtype, what=f"logits, w4r={mode}")
        outs[mode] = logits.float().cpu().numpy()
    assert_vec_close(outs[None], outs[0], dtype, what="k_w4r_gemm vs round-2 kernels")   # (a few bf16 roundings flip downstream of the reordered sums)


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_prefill_flash_attention_vs_valu_rows_and_oracle(dtype, knobs):
    """head_dim 128 prompts use the MFMA causal flash-attention kernel (prefill_attn.hpp).  One Llama-3-8B-shaped layer,
    300-token prompt (ten key blocks, diagonal masking, a ragged last query tile: 300 = 9 x 32 + 12) and a 45-token
    continuation at offset 300 (query rows that start in the middle of a key block): against the oracle and against the
    VALU kernel run once per query row (knob prefill_attn_valu = 1), on logits, hidden state and the cache rows."""
    cfg = {"model_type": "llama", "hidden_size": 4096, "num_hidden_layers": 1, "intermediate_size": 14336,
           "num_attention_heads": 32, "num_key_value_heads": 8, "rms_norm_eps": 1e-5, "vocab_size": 2048,
           "rope_theta": 500000.0, "max_position_embeddings": 8192, "tie_word_embeddings": False,
           "quantization": {"group_size": 64, "bits": 4}}
    w = po.synth_checkpoint(cfg, seed=9, dtype=dtype, lm_head_gain=4.0)
    model = build(cfg, w, dtype)
    orc = po.OracleLlama(cfg, w, dtype)
    rng = np.random.default_rng(17)
    p1, p2 = rng.integers(0, cfg["vocab_size"], 300), rng.integers(0, cfg["vocab_size"], 45)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    want1 = orc.forward(p1, ocache)
    want2 = orc.forward(p2, ocache)
    got = {}
    for mode in ("mfma", "valu"):
        knobs("prefill_attn_valu", 1 if mode == "valu" else None)
        cache = model.make_cache()
        a = model(torch.from_numpy(p1)[None].cuda(), cache=cache)[0].float().cpu().numpy()
        b = model(torch.from_numpy(p2)[None].cuda(), cache=cache)[0].float().cpu().numpy()
        got[mode] = (a, b)
        for l in (0, 1, 31, 32, 33, 63, 64, 150, 287, 288, 299):
            assert_vec_close(a[l], want1[l], dtype, what=f"{mode} position {l}")
        for l in (0, 3, 4, 20, 44):
            assert_vec_close(b[l], want2[l], dtype, what=f"{mode} continuation position {300 + l}")
    # the two attention kernels agree to about one T rounding (rms), half the oracle tolerance
    for x, y in zip(got["mfma"], got["valu"]):
        d = np.abs(x - y)
        assert d.max() <= 2 * EPS[dtype] * np.abs(y).max() and np.sqrt((d ** 2).mean()) <= 2 * EPS[dtype] * np.sqrt((y ** 2).mean())


def test_engine_with_stochastic_samplers(tiny):
    """The reference's DEFAULT request samples (temp = 1.0, inference_engine.py:305).  generate_step with top-k = 1 must
    reproduce the greedy sequence token for token (the filter leaves one candidate), a min-p run must only emit tokens
    the filter keeps, and the prompt cache must record the DRAWN tokens (they are what the KV cache encodes)."""
    from proxy_inference_engine_amd import InferenceEngine
    from proxy_inference_engine_amd import samplers
    g, cfg, w, model = tiny
    prompt = torch.from_numpy(g["prompt"])
    eng = InferenceEngine(model=model)
    eng.prepare_engine(prompt, temp=0)
    gen = eng.generate_step(prompt)
    greedy = [int(next(gen)[0].item()) for _ in range(8)]
    eng = InferenceEngine(model=model)
    eng.prepare_engine(prompt, temp=0.7, top_k=1)
    gen = eng.generate_step(prompt)
    assert [int(next(gen)[0].item()) for _ in range(8)] == greedy
    samplers.seed(3)
    eng = InferenceEngine(model=model)
    eng.prepare_engine(prompt, temp=1.0, min_p=0.2)
    gen = eng.generate_step(prompt)
    drawn = []
    for _ in range(12):
        tok, lp = next(gen)
        lp = lp.float().cpu().numpy()
        t = int(tok.item())
        assert lp[t] >= lp.max() + np.log(0.2) - 1e-6                   # inside the min-p set of THIS step's distribution
        drawn.append(t)
    assert eng.prompt_cache.computed_ids[-11:] == drawn[:11] and eng.prompt_cache.cache[0].offset == len(g["prompt"]) + 11
    assert len(set(drawn)) > 1 or drawn != greedy[:12]                 # it actually sampled something


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_dense_checkpoint_prefill_and_decode(dtype):
    """BASELINE.json configs[0] / [2]: UNQUANTISED 16-bit checkpoints (nn.Linear / nn.Embedding, models/utils.py:96-97).
    TinyLlama-proportioned dense model (H=512, I=1408 -> ragged last 512-wide K slice, 8/2 heads, D=64, 3 layers): a
    9-token prompt through iterated decode steps, a 40-token prompt through the batched GEMM path, then greedy decode
    with device-side feedback, all against the oracle's dense path (orc_linear)."""
    cfg = {"model_type": "llama", "hidden_size": 512, "num_hidden_layers": 3, "intermediate_size": 1408,
           "num_attention_heads": 8, "num_key_value_heads": 2, "rms_norm_eps": 1e-5, "vocab_size": 1024,
           "rope_theta": 10000.0, "max_position_embeddings": 2048, "tie_word_embeddings": True}
    w = po.synth_checkpoint(cfg, seed=21, dtype=dtype, lm_head_gain=4.0)
    assert "model.embed_tokens.scales" not in w
    model = build(cfg, w, dtype)
    assert model.dense
    orc = po.OracleLlama(cfg, w, dtype)
    rng = np.random.default_rng(6)
    for L in (9, 40):
        prompt = rng.integers(0, cfg["vocab_size"], L)
        ocache = [po.OracleKVCache() for _ in orc.layers]
        want_all = orc.forward(prompt, ocache)
        cache = model.make_cache()
        got_all = model(torch.from_numpy(prompt)[None].cuda(), cache=cache)[0].float().cpu().numpy()
        for l in range(L):
            assert_vec_close(got_all[l], want_all[l], dtype, what=f"dense L={L} position {l}")
        tok = model.token
        matched = 0
        for _ in range(4):
            t = int(tok.item())
            want = orc.forward(np.array([t]), ocache)[0]
            otok, olp = po.logprobs_argmax(want)
            tok, lp, logits = model.step(None, cache)
            assert_vec_close(logits.float().cpu().numpy(), want, dtype, what=f"dense decode after L={L}")
            top2 = np.sort(olp)[-2:]
            if top2[1] - top2[0] > margin_bound(want, dtype):
                assert int(tok.item()) == otok
                matched += 1
        assert matched >= 1
    assert model.step_bytes(100) > 2 * sum(v.size for k, v in w.items() if k.endswith("proj.weight"))  # 2 B per parameter


def test_tinyllama_dense_fp16_128_plus_64_greedy_vs_oracle():
    """BASELINE.json configs[0] AS WRITTEN: TinyLlama-1.1B geometry (H=2048, I=5632, 32/4 heads, D=64, V=32000, theta 1e4), UNQUANTISED
    fp16 (nn.Linear / nn.Embedding: no "quantization" entry, models/utils.py:96-97), greedy, a 128-token prompt + 64 generated tokens through
    InferenceEngine.generate_step (engine/inference_engine.py:228-297); 2 of the 22 layers (the oracle runs on the host).  The oracle decodes
    the same 64 steps teacher-forced with ITS greedy tokens; logits at every step within the end-to-end tolerance, greedy ids identical
    wherever the oracle's top-2 margin exceeds the bound, and once an id differs inside the bound the comparison stops (the runs diverge)."""
    from proxy_inference_engine_amd import InferenceEngine
    dtype = "float16"
    cfg = {"model_type": "llama", "hidden_size": 2048, "num_hidden_layers": 2, "intermediate_size": 5632,
           "num_attention_heads": 32, "num_key_value_heads": 4, "rms_norm_eps": 1e-5, "vocab_size": 32000,
           "rope_theta": 10000.0, "max_position_embeddings": 2048, "tie_word_embeddings": False}
    w = po.synth_checkpoint(cfg, seed=17, dtype=dtype, lm_head_gain=4.0)
    assert "model.layers.0.mlp.down_proj.scales" not in w and "model.embed_tokens.scales" not in w
    model = build(cfg, w, dtype)
    assert model.dense
    orc = po.OracleLlama(cfg, w, dtype)
    prompt = np.random.default_rng(128).integers(0, cfg["vocab_size"], 128)
    eng = InferenceEngine(model=model)
    eng.prepare_engine(prompt, temp=0)
    gen = eng.generate_step(torch.from_numpy(prompt))
    ocache = [po.OracleKVCache() for _ in orc.layers]
    want = orc.forward(prompt, ocache, last_only=True).reshape(-1)       # the batched prompt pass (128 rows: MLX's GEMM regime)
    checked = compared = 0
    for i in range(64):
        tok, lp = next(gen)
        otok, olp = po.logprobs_argmax(want)
        got_lp = lp.float().cpu().numpy().reshape(-1)
        err = float(np.abs(got_lp - olp).max())
        assert err <= 4 * 2.0 ** -11 * float(np.abs(want).max()) + 1e-3, f"token {i}: log-probabilities off by {err}"
        compared += 1
        top2 = np.sort(olp)[-2:]
        if top2[1] - top2[0] > margin_bound(want, dtype):
            assert int(tok.item()) == otok, f"token {i}: {int(tok.item())} vs oracle {otok} at margin {top2[1] - top2[0]:.4f}"
            checked += 1
        elif int(tok.item()) != otok:
            break                                                        # a near-tie decided differently: the sequences diverge from here
        want = orc.forward(np.array([otok]), ocache, last_only=True).reshape(-1)
    assert compared >= 16 and checked >= compared // 2, (compared, checked)
    assert model.make_cache and eng.prompt_cache.cache[0].offset >= 128 + compared - 1


def test_llama8b_dense_bf16_layers_vs_oracle():
    """BASELINE.json configs[2] at ITS geometry: two Llama-3-8B-shaped UNQUANTISED bf16 layers (H=4096, I=14336, 32/8 heads, D=128:
    W16S units of 512-wide K slices -> 8 and 28 slices per row; a config without a "quantization" entry keeps nn.Linear,
    models/utils.py:96-97), V=8192.  A 48-token and a 512-token prompt through the batched GEMM path (every 64th position and the
    last against the oracle), then 3 decode steps through the W16S streaming GEMV, same tolerances as the int4 test above."""
    dtype = "bfloat16"
    cfg = {"model_type": "llama", "hidden_size": 4096, "num_hidden_layers": 2, "intermediate_size": 14336,
           "num_attention_heads": 32, "num_key_value_heads": 8, "rms_norm_eps": 1e-5, "vocab_size": 8192,
           "rope_theta": 500000.0, "max_position_embeddings": 8192, "tie_word_embeddings": False}
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    from proxy_inference_engine_amd.models.utils import synthetic_checkpoint
    wd = synthetic_checkpoint(cfg, seed=31, dtype=torch.bfloat16, lm_head_gain=4.0)  # 470 M parameters: generated on the GPU, the oracle gets host copies
    assert "model.layers.0.mlp.down_proj.scales" not in wd
    w = {k: v.view(torch.int16).cpu().numpy().view(np.uint16) for k, v in wd.items()}
    model = Model(ModelArgs(**cfg), wd)
    del wd
    assert model.dense
    orc = po.OracleLlama(cfg, w, dtype)
    rng = np.random.default_rng(12)
    for L in (48, 512):
        prompt = rng.integers(0, cfg["vocab_size"], L)
        ocache = [po.OracleKVCache() for _ in orc.layers]
        want_all = orc.forward(prompt, ocache)
        cache = model.make_cache()
        got_all = model(torch.from_numpy(prompt)[None].cuda(), cache=cache)[0].float().cpu().numpy()
        for l in sorted(set(range(0, L, 64)) | {L - 1}):
            assert_vec_close(got_all[l], want_all[l], dtype, what=f"dense 8B geometry, L={L}, position {l}")
        tok = model.token
        matched = 0
        for i in range(3):
            want = orc.forward(np.array([int(tok.item())]), ocache)[0]
            otok, olp = po.logprobs_argmax(want)
            tok, lp, logits = model.step(None, cache)
            assert_vec_close(logits.float().cpu().numpy(), want, dtype, what=f"dense 8B geometry, decode step {i} after L={L}")
            top2 = np.sort(olp)[-2:]
            if top2[1] - top2[0] > margin_bound(want, dtype):
                assert int(tok.item()) == otok
                matched += 1
        assert matched >= 1
    n_lin = sum(v.size for k, v in w.items() if k.endswith("proj.weight"))
    assert model.step_bytes(100) > 2 * n_lin  # 2 B per parameter: 436 M parameters in two layers


def test_llama32_3b_shaped_layer():
    """Llama-3.2-3B geometry: H = 3072 (1.5 K-slices of 2048: ragged), I = 8192, 24/8 heads (3 q-heads per kv-head), D = 128,
    tied embeddings; one layer, f16."""
    dtype = "float16"
    cfg = {"model_type": "llama", "hidden_size": 3072, "num_hidden_layers": 1, "intermediate_size": 8192,
           "num_attention_heads": 24, "num_key_value_heads": 8, "head_dim": 128, "rms_norm_eps": 1e-5, "vocab_size": 2048,
           "rope_theta": 500000.0, "max_position_embeddings": 8192, "tie_word_embeddings": True,
           "rope_scaling": {"factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "rope_type": "llama3",
                            "original_max_position_embeddings": 8192},
           "quantization": {"group_size": 64, "bits": 4}}
    w = po.synth_checkpoint(cfg, seed=15, dtype=dtype, lm_head_gain=4.0)
    model = build(cfg, w, dtype)
    orc = po.OracleLlama(cfg, w, dtype)
    prompt = np.random.default_rng(4).integers(0, cfg["vocab_size"], 20)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    want = orc.forward(prompt, ocache, last_only=True)
    cache = model.make_cache()
    tok, lp, logits = model.step(torch.from_numpy(prompt).cuda(), cache)
    assert_vec_close(logits.float().cpu().numpy(), want, dtype, what="3B-shaped prefill logits")
    for _ in range(3):
        want = orc.forward(np.array([int(tok.item())]), ocache)[0]
        tok, lp, logits = model.step(None, cache)
        assert_vec_close(logits.float().cpu().numpy(), want, dtype, what="3B-shaped decode")


def test_qwen2vl_text_tower_shaped_layer():
    """BASELINE.json configs[3]'s text tower geometry (Qwen2-VL-7B: H = 3584, I = 18944 = 9.25 K-slices, 28/4 heads -> 7 q-heads
    per kv-head, D = 128) with q/k/v biases and NO o_proj bias, one layer, int4: batched prompt + decode vs the oracle.
    (The vision tower and image-token scatter are SURVEY 8f-3, not built.)"""
    dtype = "bfloat16"
    cfg = {"model_type": "llama", "hidden_size": 3584, "num_hidden_layers": 1, "intermediate_size": 18944,
           "num_attention_heads": 28, "num_key_value_heads": 4, "rms_norm_eps": 1e-6, "vocab_size": 2048,
           "rope_theta": 1000000.0, "max_position_embeddings": 32768, "tie_word_embeddings": False, "attention_bias": True,
           "quantization": {"group_size": 64, "bits": 4}}
    w = po.synth_checkpoint(cfg, seed=19, dtype=dtype, lm_head_gain=4.0)
    del w["model.layers.0.self_attn.o_proj.bias"]
    model = build(cfg, w, dtype)
    assert model.layers[0].bo is None and model.layers[0].bqkv is not None
    orc = po.OracleLlama(cfg, w, dtype)
    prompt = np.random.default_rng(6).integers(0, cfg["vocab_size"], 24)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    want = orc.forward(prompt, ocache, last_only=True)
    cache = model.make_cache()
    tok, lp, logits = model.step(torch.from_numpy(prompt).cuda(), cache)
    assert_vec_close(logits.float().cpu().numpy(), want, dtype, what="QV-shaped prefill logits")
    for _ in range(3):
        want = orc.forward(np.array([int(tok.item())]), ocache)[0]
        tok, lp, logits = model.step(None, cache)
        assert_vec_close(logits.float().cpu().numpy(), want, dtype, what="QV-shaped decode")


def test_llama70b_shaped_layer_on_one_gpu():
    """BASELINE.json configs[4] geometry (Llama-3-70B: H=8192, I=28672, 64/8 heads -> 8 q-heads per kv-head, D=128),
    one layer, int4 g=64.  The 70B int4 model is 40 GB and fits one 288 GB card, so it runs on the single-GPU path:
    two activation pieces per staging thread (K=8192), a 57 KB LDS activation image (K=28672, 14 K-slices), REP=8
    attention.  20-token batched prompt (MFMA attention with 8 waves per workgroup) + decode steps vs the oracle."""
    dtype = "bfloat16"
    cfg = {"model_type": "llama", "hidden_size": 8192, "num_hidden_layers": 1, "intermediate_size": 28672,
           "num_attention_heads": 64, "num_key_value_heads": 8, "rms_norm_eps": 1e-5, "vocab_size": 1024,
           "rope_theta": 500000.0, "max_position_embeddings": 8192, "tie_word_embeddings": False,
           "quantization": {"group_size": 64, "bits": 4}}
    w = po.synth_checkpoint(cfg, seed=5, dtype=dtype, lm_head_gain=4.0)
    model = build(cfg, w, dtype)
    orc = po.OracleLlama(cfg, w, dtype)
    prompt = np.random.default_rng(3).integers(0, cfg["vocab_size"], 20)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    want, hid = orc.forward(prompt, ocache, last_only=True, want_hidden=True)
    cache = model.make_cache()
    tok, lp, logits = model.step(torch.from_numpy(prompt).cuda(), cache)
    assert_vec_close(model.hidden.float().cpu().numpy(), hid[-1], dtype, what="70B-shaped prefill hidden")
    assert_vec_close(logits.float().cpu().numpy(), want, dtype, what="70B-shaped prefill logits")
    for _ in range(2):
        t = int(tok.item())
        want = orc.forward(np.array([t]), ocache)[0]
        tok, lp, logits = model.step(None, cache)
        assert_vec_close(logits.float().cpu().numpy(), want, dtype, what="70B-shaped decode")


@pytest.mark.parametrize("dtype,quant", [("bfloat16", True), ("float16", False)])
def test_attention_and_mlp_bias(dtype, quant):
    """ModelArgs.attention_bias / mlp_bias (language.py:24-25,42-53,117-126): q/k/v/o and gate/up/down carry a bias that
    is added to the T-rounded product and rounded again -- inside the fused epilogues (before RoPE, before SiLU, before
    the residual add) at decode, by a row kernel after the GEMM at prefill.  int4 and dense checkpoints."""
    cfg = dict(po.TINY_CONFIG, attention_bias=True, mlp_bias=True, tie_word_embeddings=False)
    if not quant:
        cfg.pop("quantization", None)
    w = po.synth_checkpoint(cfg, seed=33, dtype=dtype, lm_head_gain=4.0)
    assert "model.layers.0.self_attn.k_proj.bias" in w and "model.layers.1.mlp.down_proj.bias" in w
    model = build(cfg, w, dtype)
    orc = po.OracleLlama(cfg, w, dtype)
    rng = np.random.default_rng(2)
    for L in (7, 30):                                                  # iterated decode steps / batched GEMM prefill
        prompt = rng.integers(0, cfg["vocab_size"], L)
        ocache = [po.OracleKVCache() for _ in orc.layers]
        want_all = orc.forward(prompt, ocache)
        cache = model.make_cache()
        got_all = model(torch.from_numpy(prompt)[None].cuda(), cache=cache)[0].float().cpu().numpy()
        for l in range(L):
            assert_vec_close(got_all[l], want_all[l], dtype, what=f"bias L={L} position {l}")
        tok = model.token
        for _ in range(3):
            want = orc.forward(np.array([int(tok.item())]), ocache)[0]
            tok, lp, logits = model.step(None, cache)
            assert_vec_close(logits.float().cpu().numpy(), want, dtype, what=f"bias decode after L={L}")
    # the biases matter: dropping them moves the logits far outside the tolerance
    w0 = {k: v for k, v in w.items() if not k.endswith(".bias")}
    ref0 = po.OracleLlama(dict(cfg, attention_bias=False, mlp_bias=False), w0, dtype).forward(prompt, [po.OracleKVCache() for _ in orc.layers])
    assert np.abs(ref0[-1] - want_all[-1]).max() > 16 * EPS[dtype] * np.abs(want_all[-1]).max()


@pytest.mark.parametrize("quant", [True, False])
def test_load_checkpoint_directory(tmp_path, quant):
    """models.utils.load (models/utils.py:27-125): config.json + sharded model-*.safetensors in the reference's on-disk
    layout (HF names; MLX triplets with uint32 codes when config["quantization"] is set, plain 16-bit weights otherwise),
    through InferenceEngine(model_path) and a greedy generate_step, against the oracle on the same arrays."""
    from safetensors.numpy import save_file

    from proxy_inference_engine_amd import InferenceEngine
    dtype = "float16"                                                   # numpy can write f16 shards (bf16 has no numpy dtype)
    cfg = dict(po.TINY_CONFIG)
    if not quant:
        cfg.pop("quantization")
    w = po.synth_checkpoint(cfg, seed=41, dtype=dtype, lm_head_gain=4.0)
    arrays = {k: (v if v.dtype == np.uint32 else v.view(np.float16)) for k, v in w.items()}
    names = sorted(arrays)
    save_file({k: arrays[k] for k in names[::2]}, str(tmp_path / "model-00001-of-00002.safetensors"))
    save_file({k: arrays[k] for k in names[1::2]}, str(tmp_path / "model-00002-of-00002.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(dict(cfg, architectures=["LlamaForCausalLM"], torch_dtype="float16")))
    eng = InferenceEngine(str(tmp_path))
    assert eng.model.dense == (not quant) and eng.model.dtype == torch.float16
    prompt = np.random.default_rng(9).integers(0, cfg["vocab_size"], 20)
    eng.prepare_engine(prompt, temp=0)
    gen = eng.generate_step(torch.from_numpy(prompt))
    orc = po.OracleLlama(cfg, w, dtype)
    ogen = po.generate_step(orc, po.OraclePromptCache(), prompt)
    for i in range(4):
        tok, lp = next(gen)
        otok, olp = next(ogen)
        assert_vec_close(lp.cpu().numpy(), olp, dtype, what=f"loaded checkpoint step {i}")
        top2 = np.sort(olp)[-2:]
        if top2[1] - top2[0] > margin_bound(olp, dtype):
            assert int(tok.item()) == otok
        else:
            break
    with pytest.raises(FileNotFoundError):
        InferenceEngine(str(tmp_path / "nowhere"))


@pytest.mark.parametrize("n_heads,n_kv,D", [(4, 4, 128), (4, 2, 128), (8, 1, 128), (6, 2, 128), (5, 1, 128), (7, 1, 64), (6, 1, 64)])
def test_attention_head_groupings(n_heads, n_kv, D, knobs):
    """Every GQA ratio from 1 to 8 q-heads per kv-head (Llama-3.2-3B has 3, Qwen2.5-7B 7; the 8B / 70B tests cover 4 and 8
    at full size), head_dim 128 and 64: the MFMA prefill attention (64 .. 512-thread workgroups), then the decode
    attention + merged o_proj on the cache it filled.  75-token prompt + 37-token continuation, every position, 2 steps."""
    # two 32-row query tiles per workgroup wherever they fit (<= 4 q-heads per kv-head); the product only picks that form for
    # prompts long enough to fill the chip, which no parity test can afford
    knobs("prefill_qt", 2)
    cfg = {"model_type": "llama", "hidden_size": n_heads * D, "num_hidden_layers": 2, "intermediate_size": 768,
           "num_attention_heads": n_heads, "num_key_value_heads": n_kv, "rms_norm_eps": 1e-5, "vocab_size": 512,
           "rope_theta": 10000.0, "max_position_embeddings": 2048, "tie_word_embeddings": True,
           "quantization": {"group_size": 64, "bits": 4}}
    w = po.synth_checkpoint(cfg, seed=50 + n_kv, dtype=DT, lm_head_gain=4.0)
    model = build(cfg, w)
    orc = po.OracleLlama(cfg, w, DT)
    rng = np.random.default_rng(n_heads)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    cache = model.make_cache()
    off = 0
    for L in (75, 37):
        ids = rng.integers(0, cfg["vocab_size"], L)
        want = orc.forward(ids, ocache)
        got = model(torch.from_numpy(ids)[None].cuda(), cache=cache)[0].float().cpu().numpy()
        for l in range(L):
            assert_vec_close(got[l], want[l], DT, what=f"{n_heads}/{n_kv} heads D={D} position {off + l}")
        off += L
    tok = model.token
    for _ in range(2):
        want = orc.forward(np.array([int(tok.item())]), ocache)[0]
        tok, lp, logits = model.step(None, cache)
        assert_vec_close(logits.float().cpu().numpy(), want, DT, what=f"{n_heads}/{n_kv} heads D={D} decode")


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_int8_checkpoint_prefill_and_decode(dtype):
    """An MLX 8-bit checkpoint (config "quantization": {"group_size": 64, "bits": 8}) end to end: the tiny Llama with int8
    triplets for every Linear and the embedding, iterated and batched prompts, greedy decode, against the oracle."""
    cfg = dict(po.TINY_CONFIG, quantization={"group_size": 64, "bits": 8}, tie_word_embeddings=True)
    w = po.synth_checkpoint(cfg, seed=61, dtype=dtype, lm_head_gain=4.0)
    assert w["model.layers.0.mlp.down_proj.weight"].shape[1] == cfg["intermediate_size"] // 4       # 4 codes per word
    model = build(cfg, w, dtype)
    assert model.bits == 8
    orc = po.OracleLlama(cfg, w, dtype)
    rng = np.random.default_rng(10)
    for L in (5, 50):
        prompt = rng.integers(0, cfg["vocab_size"], L)
        ocache = [po.OracleKVCache() for _ in orc.layers]
        want_all = orc.forward(prompt, ocache)
        cache = model.make_cache()
        got_all = model(torch.from_numpy(prompt)[None].cuda(), cache=cache)[0].float().cpu().numpy()
        for l in range(L):
            assert_vec_close(got_all[l], want_all[l], dtype, what=f"int8 L={L} position {l}")
        tok = model.token
        for _ in range(3):
            want = orc.forward(np.array([int(tok.item())]), ocache)[0]
            tok, lp, logits = model.step(None, cache)
            assert_vec_close(logits.float().cpu().numpy(), want, dtype, what=f"int8 decode after L={L}")
    assert model.step_bytes(64) > 1.8 * build(dict(cfg, quantization={"group_size": 64, "bits": 4}),
                                              po.synth_checkpoint(dict(cfg, quantization={"group_size": 64, "bits": 4}), seed=61, dtype=dtype), dtype).step_bytes(64) * 0.9


@pytest.mark.parametrize("name", ["tiny_dense_f16_bias", "tiny_w8_bf16_trad"])
def test_variant_golden_fixtures(golden_dir, name):
    """The committed oracle vectors for the other checkpoint formats (dense f16 with Linear biases; int8 g=64 with traditional
    RoPE) through InferenceEngine.generate_step: tokens on the safe prefix, log-probabilities within tolerance."""
    from proxy_inference_engine_amd import InferenceEngine
    g = np.load(golden_dir / f"{name}.npz")
    dt = str(g["dtype"])
    cfg = json.loads(str(g["config_json"]))
    w = {k[2:]: g[k] for k in g.files if k.startswith("w:")}
    eng = InferenceEngine(model=build(cfg, w, dt))
    eng.prepare_engine(g["prompt"], temp=0)
    gen = eng.generate_step(torch.from_numpy(g["prompt"]))
    mb = margin_bound(g["logprobs"][0], dt)
    safe = int(np.argmax(g["margins"] < mb)) if (g["margins"] < mb).any() else len(g["tokens"])
    for i in range(len(g["tokens"])):
        tok, lp = next(gen)
        if i < safe:
            assert int(tok.item()) == int(g["tokens"][i]), f"{name} step {i}"
            assert_vec_close(lp.cpu().numpy(), g["logprobs"][i], dt, what=f"{name} logprobs step {i}")
    assert safe >= 1


@pytest.mark.parametrize("case", range(int(__import__("os").environ.get("PIE_FUZZ_CASES", "10"))))
def test_random_model_configs_end_to_end(case):
    """Seeded random Llama configurations (head counts / GQA ratio, head_dim, hidden and intermediate sizes that are odd
    multiples of 64, vocabulary, weight format, dtype, tied head, Linear biases, RoPE form and llama3 scaling): a batched
    prompt, a short iterated continuation and greedy decode steps, all against the oracle."""
    rng = np.random.default_rng(1000 + case)
    D = int(rng.choice([64, 128]))
    nkv = int(rng.choice([1, 2, 3, 4]))
    rep = int(rng.integers(1, 9))
    nh = nkv * rep
    H = 64 * int(rng.integers(2, 14))
    I = 64 * int(rng.integers(3, 40))
    V = 2 * int(rng.integers(100, 700))
    fmt = ("int4", "int8", "dense")[case % 3]
    dtype = ("bfloat16", "float16")[int(rng.integers(0, 2))]
    cfg = {"model_type": "llama", "hidden_size": H, "num_hidden_layers": int(rng.integers(1, 4)), "intermediate_size": I,
           "num_attention_heads": nh, "num_key_value_heads": nkv, "head_dim": D, "rms_norm_eps": 1e-5, "vocab_size": V,
           "rope_theta": float(rng.choice([10000.0, 500000.0])), "max_position_embeddings": 4096,
           "tie_word_embeddings": bool(rng.integers(0, 2)), "attention_bias": bool(rng.integers(0, 2)),
           "mlp_bias": bool(rng.integers(0, 2)), "rope_traditional": bool(rng.integers(0, 2))}
    if rng.integers(0, 2):
        cfg["rope_scaling"] = {"factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0}
    if fmt != "dense":
        cfg["quantization"] = {"group_size": 64, "bits": 4 if fmt == "int4" else 8}
    w = po.synth_checkpoint(cfg, seed=2000 + case, dtype=dtype, lm_head_gain=4.0)
    model = build(cfg, w, dtype)
    orc = po.OracleLlama(cfg, w, dtype)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    cache = model.make_cache()
    what = f"case {case}: {fmt} {dtype} H{H} I{I} {nh}/{nkv}xD{D} V{V} L{cfg['num_hidden_layers']}"
    prompts, prompt_bits = [], None
    for L in (int(rng.integers(17, 90)), int(rng.integers(2, 9))):      # batched (qmm regime), then iterated (qmv regime)
        ids = rng.integers(0, V, L)
        prompts.append(ids)
        want = orc.forward(ids, ocache)
        got_t = model(torch.from_numpy(ids)[None].cuda(), cache=cache)[0]
        prompt_bits = to_bits(got_t).copy()
        got = got_t.float().cpu().numpy()
        for l in (0, L // 2, L - 1):
            # 6 / 5 instead of 4 / 4: these tiny vocabularies (max |logit| ~ 1.5) and up to 3 layers put the max over a few hundred
            # elements at 2-2.6 eps typically and 3.7-4.0 in 1 of 80 seeded cases (PIE_FUZZ_CASES=80), with no outlier structure
            assert_vec_close(got[l], want[l], dtype, c_max=6.0, c_rms=5.0, what=f"{what} prompt L={L} position {l}")
    tok = model.token
    first = int(tok.item())
    dec_bits = []
    for _ in range(3):
        want1 = orc.forward(np.array([int(tok.item())]), ocache)[0]
        tok, lp, logits = model.step(None, cache)
        dec_bits.append(to_bits(logits).copy())
        assert_vec_close(logits.float().cpu().numpy(), want1, dtype, c_max=6.0, c_rms=5.0, what=f"{what} decode")
    # the same sequence with the KV cache in scattered 64-token pages: identical kernels on identical rows -> identical bits
    pool = model.enable_paged_kv(num_pages=8, max_blocks=int(rng.integers(1, 4)))
    for _ in range(int(rng.integers(0, 4))):
        pool.allocate_page()
    if pool.get_num_free_pages() < 8:
        pool.free_page(0)                                    # LIFO: the sequence's first page is page 0, the rest follow the held ones
    pcache = model.make_cache()
    model(torch.from_numpy(prompts[0])[None].cuda(), cache=pcache)
    got2 = model(torch.from_numpy(prompts[1])[None].cuda(), cache=pcache)[0]
    assert np.array_equal(to_bits(got2), prompt_bits), f"{what}: paged prompt logits differ from the contiguous cache's"
    tok2, _, logits2 = model.step(torch.tensor([first], dtype=torch.int32, device="cuda"), pcache)
    assert np.array_equal(to_bits(logits2), dec_bits[0]), f"{what}: paged decode logits differ"


def test_group_size_128_checkpoint_vs_oracle():
    """config["quantization"] = {"group_size": 128, "bits": 4} (nn.quantize forwards it unchanged, models/utils.py:96-111; mx.quantize's other
    common group size): the triplets carry one (scale, bias) per 128 weights, the streaming units one per 64 -- each is served to both halves.
    A 40-token prompt (qmm regime: the dequantised matrix is the same, bit for bit) and decode steps (qmv regime: the affine sums associate
    per 64 instead of per 128) against the oracle, which quantises and multiplies with 128-wide groups."""
    cfg = {"model_type": "llama", "hidden_size": 256, "num_hidden_layers": 2, "intermediate_size": 768, "num_attention_heads": 4,
           "num_key_value_heads": 2, "rms_norm_eps": 1e-5, "vocab_size": 512, "rope_theta": 10000.0, "max_position_embeddings": 2048,
           "tie_word_embeddings": False, "quantization": {"group_size": 128, "bits": 4}}
    w = po.synth_checkpoint(cfg, seed=41, dtype=DT, lm_head_gain=4.0)
    assert w["model.layers.0.mlp.down_proj.scales"].shape == (256, 768 // 128)
    model = build(cfg, w)
    assert model.group_size == 128
    orc = po.OracleLlama(cfg, w, DT)
    prompt = np.random.default_rng(4).integers(0, cfg["vocab_size"], 40)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    want = orc.forward(prompt, ocache)
    cache = model.make_cache()
    got = model(torch.from_numpy(prompt)[None].cuda(), cache=cache)[0].float().cpu().numpy()
    for l in range(40):
        assert_vec_close(got[l], want[l], DT, what=f"g=128 prompt position {l}")
    tok = int(np.argmax(want[-1]))
    for i in range(4):
        w1 = orc.forward(np.array([tok]), ocache)[0]
        _, _, g1 = model.step(torch.tensor([tok], dtype=torch.int32, device="cuda"), cache)
        assert_vec_close(g1.float().cpu().numpy(), w1, DT, what=f"g=128 decode step {i}")
        tok = int(np.argmax(w1))


@pytest.mark.parametrize("bits,group", [(2, 64), (3, 64), (6, 64), (3, 128), (6, 128), (4, 32), (3, 32), (2, 32), (8, 32), (6, 32)])
def test_narrow_code_and_group_32_checkpoints_vs_oracle(bits, group):
    """config["quantization"]["bits"] in {2, 3, 6} (nn.quantize forwards it unchanged, models/utils.py:96-111): 2-bit codes sixteen to a word,
    3- and 6-bit codes in MLX's byte-packed bit stream.  The loader re-packs the codes into the 4- / 8-bit streaming units without touching a
    value, so a 40-token prompt (qmm regime), decode steps (qmv regime) and the quantised embedding must be what the oracle computes from the
    narrow codes themselves."""
    cfg = {"model_type": "llama", "hidden_size": 256, "num_hidden_layers": 2, "intermediate_size": 768, "num_attention_heads": 4,
           "num_key_value_heads": 2, "rms_norm_eps": 1e-5, "vocab_size": 512, "rope_theta": 10000.0, "max_position_embeddings": 2048,
           "tie_word_embeddings": bits == 3, "quantization": {"group_size": group, "bits": bits}}
    w = po.synth_checkpoint(cfg, seed=50 + bits, dtype=DT, lm_head_gain=4.0)
    assert w["model.layers.0.mlp.down_proj.weight"].shape == (256, 768 * bits // 32)
    model = build(cfg, w)
    assert model.checkpoint_bits == bits and model.bits == (8 if bits in (6, 8) else 4) and model.group_size == group
    if group == 32:
        assert w["model.layers.0.mlp.down_proj.scales"].shape == (256, 768 // 32)
    orc = po.OracleLlama(cfg, w, DT)
    prompt = np.random.default_rng(bits).integers(0, cfg["vocab_size"], 40)
    ocache = [po.OracleKVCache() for _ in orc.layers]
    want = orc.forward(prompt, ocache)
    cache = model.make_cache()
    got = model(torch.from_numpy(prompt)[None].cuda(), cache=cache)[0].float().cpu().numpy()
    for l in range(40):
        assert_vec_close(got[l], want[l], DT, what=f"{bits}-bit g={group} prompt position {l}")
    tok = int(np.argmax(want[-1]))
    for i in range(4):
        w1 = orc.forward(np.array([tok]), ocache)[0]
        _, _, g1 = model.step(torch.tensor([tok], dtype=torch.int32, device="cuda"), cache)
        assert_vec_close(g1.float().cpu().numpy(), w1, DT, what=f"{bits}-bit g={group} decode step {i}")
        tok = int(np.argmax(w1))


@pytest.mark.parametrize("bits,group,tied,dtype", [(2, 64, True, "bfloat16"), (2, 128, False, "bfloat16"), (2, 64, False, "float16"),
                                                   (6, 64, True, "bfloat16"), (6, 128, False, "bfloat16"), (6, 64, False, "float16")])
def test_narrow_checkpoints_stream_native_units(bits, group, tied, dtype):
    """2- and 6-bit checkpoints in 64- / 128-wide groups run on W2S / W6S units: every Linear -- a tied lm_head included -- is packed
    from the narrow codes themselves at the checkpoint's 0.3125 / 0.8125 B per weight, pie_decoder_step_bytes counts exactly that, and a 5-row prompt
    (row-by-row streaming GEMV), a 40-token prompt (dequantise-to-T, 16-bit GEMM) and decode steps are what the oracle computes from the narrow codes."""
    cfg = {"model_type": "llama", "hidden_size": 256, "num_hidden_layers": 2, "intermediate_size": 768, "num_attention_heads": 4,
           "num_key_value_heads": 2, "rms_norm_eps": 1e-5, "vocab_size": 512, "rope_theta": 10000.0, "max_position_embeddings": 2048,
           "tie_word_embeddings": tied, "quantization": {"group_size": group, "bits": bits}}
    w = po.synth_checkpoint(cfg, seed=70 + bits, dtype=dtype, lm_head_gain=4.0)
    model = build(cfg, w, dtype)
    assert model.native_narrow == bits and model.checkpoint_bits == bits and model.native_w2 == (bits == 2)
    H, I, V, QKV = 256, 768, 512, 256 + 2 * 128
    n_lin = 2 * (QKV * H + H * H + 2 * I * H + H * I) + V * H          # weights of every Linear the step streams
    unit = 1280 if bits == 2 else 3328
    from proxy_inference_engine_amd import _ffi
    for m in (model.layers[0].wqkv, model.layers[0].wdown, model.lm_head):
        assert m.fmt == (_ffi.PIE_W_INT2_G64 if bits == 2 else _ffi.PIE_W_INT6_G64) and m.nbytes == (m.N // 2) * ((m.K + 2047) // 2048) * unit
    want_bytes = n_lin * (4 * bits + 2) // 32                              # `bits` per weight + a 16-bit (scale, bias) pair per 64 weights
    got_bytes = model.step_bytes(64)
    assert want_bytes <= got_bytes <= want_bytes + 200_000, (got_bytes, want_bytes)   # + norms, 64 positions of K / V, the tail
    orc = po.OracleLlama(cfg, w, dtype)
    rng = np.random.default_rng(group)
    for L in (5, 40):
        prompt = rng.integers(0, V, L)
        ocache = [po.OracleKVCache() for _ in orc.layers]
        want = orc.forward(prompt, ocache)
        cache = model.make_cache()
        got = model(torch.from_numpy(prompt)[None].cuda(), cache=cache)[0].float().cpu().numpy()
        for l in range(L):
            assert_vec_close(got[l], want[l], dtype, what=f"{bits}-bit g={group} L={L} position {l}")
        tok = int(np.argmax(want[-1]))
        for i in range(3):
            w1 = orc.forward(np.array([tok]), ocache)[0]
            _, _, g1 = model.step(torch.tensor([tok], dtype=torch.int32, device="cuda"), cache)
            assert_vec_close(g1.float().cpu().numpy(), w1, dtype, what=f"{bits}-bit g={group} decode step {i} after L={L}")
            tok = int(np.argmax(w1))


def test_tied_embeddings_and_errors(tiny):
    g, cfg, w, _ = tiny
    cfg2 = dict(cfg, tie_word_embeddings=True)
    w2 = {k: v for k, v in w.items() if not k.startswith("lm_head")}
    model = build(cfg2, w2)
    orc = po.OracleLlama(cfg2, w2, DT)
    ids = g["prompt"][:9]
    want = orc.forward(ids, [po.OracleKVCache() for _ in orc.layers])[-1]
    _, _, logits = model.step(torch.from_numpy(ids).cuda(), model.make_cache())
    assert_vec_close(logits.float().cpu().numpy(), want, DT, what="tied lm_head")
    with pytest.raises(ValueError):
        build(dict(cfg, quantization=None), w)                          # config says dense, checkpoint holds int4 triplets
    with pytest.raises(ValueError, match="group_size=16"):
        build(dict(cfg, quantization={"group_size": 16, "bits": 4}), w)  # not a group size mx.quantize knows
    with pytest.raises(ValueError, match="bits=5"):
        build(dict(cfg, quantization={"group_size": 64, "bits": 5}), w)
    # the reference decides per module ("{path}.scales" in weights, models/utils.py:99-109); Linears this build streams as ONE packed
    # matrix (q|k|v, gate|up) must agree -- a dense k_proj next to quantised q / v is refused by name
    bad = {k: v for k, v in w.items() if not k.startswith("model.layers.1.self_attn.k_proj.")}
    kv_rows = cfg["num_key_value_heads"] * (cfg.get("head_dim") or cfg["hidden_size"] // cfg["num_attention_heads"])
    bad["model.layers.1.self_attn.k_proj.weight"] = np.zeros((kv_rows, cfg["hidden_size"]), np.uint16)
    with pytest.raises(ValueError, match=r"q_proj.*quantised but .*k_proj dense"):
        build(cfg, bad)
    with pytest.raises(ValueError):
        model.step(torch.tensor([1], dtype=torch.int32, device="cuda"), model.make_cache()[:1])


def test_mixed_quantised_and_dense_modules_vs_oracle(tiny):
    """The reference's per-module quantisation predicate (models/utils.py:99-109: a module is quantised iff the checkpoint holds
    "{path}.scales"): an int4 checkpoint in which layer 1's o_proj and down_proj, layer 0's gate|up pair and the lm_head are plain 16-bit
    Linears.  Decode steps (GEMV per matrix format), a batched prompt (int4 MFMA GEMM next to the 16-bit GEMM) and greedy feedback,
    against the oracle, which applies the same predicate."""
    g, cfg, w, _ = tiny
    mixed = dict(w)

    def make_dense(name):
        deq = po.dequantize(mixed[f"{name}.weight"], mixed[f"{name}.scales"], mixed[f"{name}.biases"], dtype=DT)
        for k in ("scales", "biases"):
            del mixed[f"{name}.{k}"]
        mixed[f"{name}.weight"] = po.to_bits(deq, DT)

    for name in ("model.layers.1.self_attn.o_proj", "model.layers.1.mlp.down_proj", "model.layers.0.mlp.gate_proj", "model.layers.0.mlp.up_proj", "lm_head"):
        make_dense(name)
    model = build(cfg, mixed)
    assert model.mixed and not model.dense
    orc = po.OracleLlama(cfg, mixed, DT)
    rng = np.random.default_rng(12)
    for L in (5, 40):  # iterated steps; the batched path
        prompt = rng.integers(0, cfg["vocab_size"], L)
        ocache = [po.OracleKVCache() for _ in orc.layers]
        want_all = orc.forward(prompt, ocache)
        cache = model.make_cache()
        got_all = model(torch.from_numpy(prompt)[None].cuda(), cache=cache)[0].float().cpu().numpy()
        for l in range(L):
            assert_vec_close(got_all[l], want_all[l], DT, what=f"mixed checkpoint L={L} position {l}")
        tok = model.token
        for _ in range(3):
            t = int(tok.item())
            want = orc.forward(np.array([t]), ocache)[0]
            tok, lp, logits = model.step(None, cache)
            assert_vec_close(logits.float().cpu().numpy(), want, DT, what=f"mixed checkpoint decode after L={L}")
    # byte accounting follows the per-matrix formats: more than the all-int4 model, less than the all-dense one
    full = build(cfg, w)
    assert full.step_bytes(50) < model.step_bytes(50)


def test_long_prompt_gate_up_with_fused_swiglu_epilogue():
    """A 1536-token prompt on a wide-MLP layer (I = 4096: the packed gate|up matrix has 8192 columns, 32 x 6 = 192 tiles of the
    256-row prompt GEMM, so K is not split and the SwiGLU rides in k_w4l2_gemm's epilogue; q|k|v / o_proj / down take the K-split form
    with the fp32 reduce) against the oracle's many-row regime, every position."""
    dtype = "bfloat16"
    cfg = {"model_type": "llama", "hidden_size": 256, "num_hidden_layers": 1, "intermediate_size": 4096,
           "num_attention_heads": 4, "num_key_value_heads": 2, "rms_norm_eps": 1e-5, "vocab_size": 512,
           "rope_theta": 10000.0, "max_position_embeddings": 4096, "tie_word_embeddings": True,
           "quantization": {"group_size": 64, "bits": 4}}
    w = po.synth_checkpoint(cfg, seed=33, dtype=dtype, lm_head_gain=4.0)
    model = build(cfg, w, dtype)
    orc = po.OracleLlama(cfg, w, dtype)
    L = 1536
    prompt = np.random.default_rng(8).integers(0, cfg["vocab_size"], L)
    want = orc.forward(prompt, [po.OracleKVCache() for _ in orc.layers])
    got = model(torch.from_numpy(prompt)[None].cuda(), cache=model.make_cache())[0].float().cpu().numpy()
    for l in list(range(0, L, 97)) + [L - 1]:
        assert_vec_close(got[l], want[l], dtype, what=f"long prompt position {l}")
