"""-m gpu: the many-row passes of prefill.hip when weight copies are NOT resident.  linear_rows multiplies a W4M tile copy (int4 g=64) or a W16M
copy (everything else) of a matrix; a copy is kept while resident_budget lasts -- fixed at a decoder's first batched pass -- and a matrix without
one takes another route on every call: an int4 matrix leaves the 4-bit GEMMs (their RoPE + append and SwiGLU epilogues, their fp32 slabs) for
k_dequant_w4s -> s->wT -> w16m_from_rows_launch -> s->wM -> k_w16l_gemm with k_rope_append_rows, bias_rows and the 16-bit GEMM's epilogues; any
other matrix is expanded into the same two scratch buffers per call.  Three budgets: `default` (knob unset), `none` (prefill_resident = 0) and
`mixed` (prefill_resident_kb: SOME matrices resident and others not inside one pass, mixed_kb below).

Cases, checkpoints, prompts and oracle runs are those of tests/test_gpu_batch_configs.py; every model here is built fresh AFTER the knob is set
(the budget is read once per decoder).  Tolerance against the oracle: that file's, assert_vec_close at 4 / 4 -- the fallback multiplies weights
rounded to T, which is what the oracle's many-row regime does."""
import functools

import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests.test_gpu_batch_configs import (BASE, BF, CASES, MIXED_CASES, PREFILL_LENS, Checks, check_token, checkpoint, config, f32, mixed_sequences,
                                          oracle_mixed, oracle_prefill, prefill_alone, prefill_prompts, sequences, used_pages)
from tests.test_gpu_decode import build

pytestmark = pytest.mark.gpu

BUDGETS = ("none", "mixed")
# a. the int4-coded cases (PIE_W_INT4_G64 matrices: 3-bit codes and 128-wide groups are recoded into it): W4M tiles, or the fallback
INT4_CASES = ["int4_f16", "tied_head", "biases", "int4_dense_o_down", "int3_g64", "int4_g128", "heads_8_2_128", "rope_traditional"]
# b. every other format: the scratch copy is built by the kernels that build the resident one and multiplied by the same launch
EXACT_CASES = ["dense_bf16", "dense_f16", "int8_g64", "int8_g64_f16", "int4_g32", "int8_g32", "int2_g64", "int6_g64", "int6_g128_4_1_64_bias",
               "dense_f16_8_2_128_bias_trad"]
CHUNK_EXACT, CHUNK_ORACLE = ["dense_bf16", "int8_g64", "int2_g64"], ["int4_f16", "biases"]
GRAPH_CASES = ["int4_f16", "dense_bf16"]
# Worst measured (max, rms) error ratio on an MI355X, in assert_vec_close's units, per (case, budget): test a over its prefill_batch, step and
# step_mixed checks; test c ("chunked", case, budget) over every position and the layer-0 keys.  Every entry is inside 4 / 4: no case carries
# a bound of its own.
MEASURED = {
    ("int4_f16", "none"): (1.95, 1.55), ("int4_f16", "mixed"): (1.95, 1.71), ("tied_head", "none"): (1.12, 1.49), ("tied_head", "mixed"): (1.12, 1.49),
    ("biases", "none"): (1.21, 1.01), ("biases", "mixed"): (1.21, 1.01), ("int4_dense_o_down", "none"): (1.17, 1.33),
    ("int4_dense_o_down", "mixed"): (1.17, 1.33), ("int3_g64", "none"): (1.79, 1.25), ("int3_g64", "mixed"): (1.79, 1.25),
    ("int4_g128", "none"): (2.27, 1.59), ("int4_g128", "mixed"): (2.27, 1.59), ("heads_8_2_128", "none"): (1.84, 1.61),
    ("heads_8_2_128", "mixed"): (1.84, 1.61), ("rope_traditional", "none"): (2.26, 1.48), ("rope_traditional", "mixed"): (2.26, 1.52),
    ("chunked", "int4_f16", "none"): (1.92, 1.52), ("chunked", "int4_f16", "mixed"): (2.01, 1.57),
    ("chunked", "biases", "none"): (1.15, 1.03), ("chunked", "biases", "mixed"): (1.15, 1.03)}
assert {k for k in MEASURED if len(k) == 2} == {(n, b) for n in INT4_CASES for b in BUDGETS}


def copy_bytes(name):
    """Bytes of the copies linear_rows would keep of q|k|v, o_proj and gate|up of a case: W4M tiles of its int4 g=64 matrices, W16M tiles of the
    others (int4_dense_o_down: a dense o_proj next to int4 q|k|v and gate|up)."""
    from proxy_inference_engine_amd import _ffi
    lib, cfg = _ffi.load(), config(name)
    H, nh, nkv, I = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["intermediate_size"]
    D = cfg.get("head_dim", H // nh)

    def tiles(N, K, int4):
        return int(lib.pie_w4m_bytes(N, K) if int4 else lib.pie_w16m_bytes(N, K))

    int4 = name in INT4_CASES
    return tiles((nh + 2 * nkv) * D, H, int4), tiles(H, nh * D, int4 and not CASES[name]["mixed"]), tiles(2 * I, H, int4)


def mixed_kb(name):
    """The `mixed` budget B in KiB: bytes(q|k|v) + bytes(o_proj) <= B * 1024 < bytes(gate|up), the largest such B.  Matrices are admitted in
    first-use order (q|k|v, o_proj, gate|up, down_proj per layer), so layer 0's q|k|v and o_proj multiply resident copies, gate|up of every layer
    goes through the scratch (a matrix larger than the whole budget is never admitted), and the others land where the remainder puts them.
    Where q|k|v + o_proj alone outweigh gate|up (head_dim 128 with 8 query heads; a dense o_proj beside int4 tiles) no such B exists: there B is
    the smallest that admits the two, and what is left after them is less than gate|up needs -- the same three consequences, by the same order
    (the remainder only shrinks)."""
    qkv, o, gu = copy_bytes(name)
    if qkv + o < gu:
        kb = (gu - 1) // 1024
        assert qkv + o <= kb * 1024 < gu, (name, qkv, o, gu, kb)
    else:
        kb = (qkv + o + 1023) // 1024
        assert qkv + o <= kb * 1024 and kb * 1024 - (qkv + o) < gu, (name, qkv, o, gu, kb)
    return kb


def set_budget(knobs, name, budget):
    knobs("prefill_resident", None), knobs("prefill_resident_kb", None)
    if budget == "none":
        knobs("prefill_resident", 0)
    elif budget == "mixed":
        knobs("prefill_resident_kb", mixed_kb(name))
    else:
        assert budget == "default"


def fresh(knobs, name, budget):
    """A model of the case that nothing else has used: its decoder fixes its budget at ITS first batched pass, under the knob set here."""
    set_budget(knobs, name, budget)
    return build(*checkpoint(name))


_DEFAULT = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_default_runs():
    yield
    _DEFAULT.clear()
    for cached in (oracle_chunked,):
        cached.cache_clear()


def default_run(knobs, key, name, run):
    """run(model) on a `default` model of the case, once per module: the side test_gpu_batch_configs.py holds to the oracle."""
    if key not in _DEFAULT:
        _DEFAULT[key] = run(fresh(knobs, name, "default"))
    return _DEFAULT[key]


def assert_same(got, want, what):
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, f"{what}: {k}"
        assert torch.equal(got[k], want[k]), f"{what}: {k} differs from the default decoder's, {int((got[k] != want[k]).sum())} of {got[k].numel()} elements"


def keep(out, key, *tensors):
    for i, t in enumerate(tensors):
        out[f"{key} [{i}]"] = t.detach().cpu().clone()


def keep_kv0(out, key, caches):
    """The K and V rows layer 0 wrote for every sequence, gathered from its pages."""
    for i, c in enumerate(caches):
        keep(out, f"{key} layer-0 K/V of sequence {i}", *c[0].state)


# ---------------------------------------------------------------------------- a. int4-coded cases against the oracle
@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("name", INT4_CASES)
def test_int4_passes_without_tiles_vs_oracle(knobs, name, budget):
    """prefill_batch (prefill_varlen_t, 136 rows) + one step_batch at B = 5, and step_mixed where the case is one of MIXED_CASES, as
    test_prefill_batch_vs_oracle / test_step_mixed_vs_oracle run them, with no int4 matrix (`none`) or only some (`mixed`) on W4M tiles: the
    others go k_dequant_w4s -> wT -> w16m_from_rows -> wM -> k_w16l_gemm, q|k|v through k_rope_append_rows, Linear biases through bias_rows or the
    16-bit GEMM's epilogue, a tied / int4 lm_head through the scratch.  Same oracle runs, same bound, same page accounting."""
    model = fresh(knobs, name, budget)
    prompts, want = prefill_prompts(name), oracle_prefill(name)
    pool = model.enable_paged_kv(num_pages=12, max_blocks=2)
    caches = [model.make_cache() for _ in prompts]
    toks, logprobs, logits = model.prefill_batch([p.tolist() for p in prompts], caches)
    toks, got = toks.cpu().clone(), f32(logits)
    assert [c[0].offset for c in caches] == list(PREFILL_LENS) and used_pages(pool) == sum((n + 63) // 64 for n in PREFILL_LENS)
    assert np.all(np.abs(logprobs.double().exp().sum(dim=1).cpu().numpy() - 1.0) < 1e-4)
    feed = torch.tensor([int(np.argmax(w0)) for w0, _ in want], dtype=torch.int32)
    nxt, _, l2 = model.step_batch(feed, caches, graph=False)
    nxt, got2 = nxt.cpu().clone(), f32(l2)
    assert [c[0].offset for c in caches] == [n + 1 for n in PREFILL_LENS]
    assert used_pages(pool) == sum((n + 1 + 63) // 64 for n in PREFILL_LENS)
    checks = []
    chk = Checks(name, f"[{budget}] prefill_batch vs oracle")
    for i, n in enumerate(PREFILL_LENS):
        chk.add(got[i], want[i][0], f"prompt {i} ({n} tokens)")
    checks.append(chk)
    chk = Checks(name, f"[{budget}] step after prefill_batch vs oracle")
    for i, n in enumerate(PREFILL_LENS):
        chk.add(got2[i], want[i][1], f"prompt {i} ({n} tokens)")
    checks.append(chk)
    mixed = name in MIXED_CASES
    if mixed:
        d0, d1, fresh_p, prefix, suffix = mixed_sequences(name)
        firsts, want_m = oracle_mixed(name)
        pool = model.enable_paged_kv(num_pages=24, max_blocks=4)
        dcaches, _ = prefill_alone(model, [d0, d1])
        (pc,), _ = prefill_alone(model, [prefix])
        fc = model.make_cache()
        feed = torch.tensor([int(np.argmax(x)) for x in firsts], dtype=torch.int32)
        nxt_m, logprobs, logits = model.step_mixed(feed, dcaches, [fresh_p.tolist(), suffix.tolist()], [fc, pc])
        assert nxt_m.shape == (4,) and logits.shape == (4, BASE["vocab_size"])
        got_m, nxt_m = f32(logits), nxt_m.cpu()
        assert np.all(np.abs(logprobs.double().exp().sum(dim=1).cpu().numpy() - 1.0) < 1e-4)
        assert [c[0].offset for c in dcaches + [fc, pc]] == [64, 21, 9, 110]
        assert used_pages(pool) == 1 + 1 + 1 + 2
        chk = Checks(name, f"[{budget}] step_mixed vs oracle")
        for i, what in enumerate(("decode row 0 (63 cached)", "decode row 1 (20 cached)", "fresh 9-token prompt", "40 rows behind 70 cached")):
            chk.add(got_m[i], want_m[i], what)
        checks.append(chk)
    for chk in checks:
        chk.run()
    for i in range(len(prompts)):
        check_token(name, toks[i], want[i][0], f"[{budget}] prefill_batch prompt {i}")
        check_token(name, nxt[i], want[i][1], f"[{budget}] step after prefill_batch, prompt {i}")
    if mixed:
        for i in range(4):
            check_token(name, nxt_m[i], want_m[i], f"[{budget}] step_mixed row {i}")


# ---------------------------------------------------------------------------- b. bit for bit against the default decoder
def batch_passes(name, step_B, prompt_passes):
    """model -> every tensor test b compares.  step_B: step_batch (two steps each: the second reads the row the first appended) over
    sequences(name, B); prompt_passes: prefill_batch of the five prompts and step_mixed too.  run(model, knobs): the caches are filled by iterated
    decode steps (prefill_min: no many-row pass), so that int4 cases, whose prompt pass legitimately differs by budget, start from identical pages."""
    def run(model, knobs=None):
        out = {}
        if prompt_passes:
            model.enable_paged_kv(num_pages=12, max_blocks=2)
            caches = [model.make_cache() for _ in PREFILL_LENS]
            keep(out, "prefill_batch", *model.prefill_batch([p.tolist() for p in prefill_prompts(name)], caches))
            keep_kv0(out, "prefill_batch", caches)
        for B in step_B:
            model.enable_paged_kv(num_pages=2 * B + 4, max_blocks=2)
            if knobs:
                knobs("prefill_min", 100000)
            caches, toks = prefill_alone(model, sequences(name, B))
            if knobs:
                knobs("prefill_min", None)
            feed = torch.tensor(toks, dtype=torch.int32)
            keep(out, f"B={B} first tokens", feed)
            for st in range(2):
                res = model.step_batch(feed, caches, graph=False)
                keep(out, f"step_batch B={B} step {st}", *res)
                feed = res[0].cpu().clone()
            keep_kv0(out, f"step_batch B={B}", caches)
        if prompt_passes:
            d0, d1, fresh_p, prefix, suffix = mixed_sequences(name)
            model.enable_paged_kv(num_pages=24, max_blocks=4)
            dcaches, toks = prefill_alone(model, [d0, d1])
            (pc,), _ = prefill_alone(model, [prefix])
            fc = model.make_cache()
            keep(out, "step_mixed", *model.step_mixed(torch.tensor(toks, dtype=torch.int32), dcaches, [fresh_p.tolist(), suffix.tolist()], [fc, pc]))
            keep_kv0(out, "step_mixed", dcaches + [fc, pc])
        return out
    return run


@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("name", EXACT_CASES)
def test_scratch_copies_equal_resident_copies_bit_for_bit(knobs, name, budget):
    """Not int4 g=64: linear_rows builds the W16M copy with expand_weights either way -- k_dequant_w8s / _w2s / _w6s / _w4s<g32> -> wT ->
    w16m_from_rows_launch, or w16m_from_w16s_launch for dense modules -- into s->wM instead of a resident buffer, per call, and hands
    k_w16l_gemm the other pointer.  prefill_batch (136 rows), step_batch at B = 3, 6, 33, step_mixed: logits, log-probabilities, tokens
    and layer 0's K / V rows equal the default decoder's in every bit."""
    run = batch_passes(name, (3, 6, 33), True)
    want = default_run(knobs, ("batch", name), name, run)
    assert_same(run(fresh(knobs, name, budget)), want, f"{name} [{budget}]")


@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("name", INT4_CASES)
def test_few_row_int4_steps_never_enter_the_budget(knobs, name, budget):
    """step_batch at B = 3 and 5 on the int4-coded cases: fused_rows, the streaming GEMVs (w4s_gemv_rows_launch) and, for dense o_proj / down_proj,
    the W16M copy -- no W4M tile is asked for, so the rows equal the default decoder's bit for bit.  The pages are filled by iterated decode steps
    (prefill_min): a prompt pass on tiles and one through the scratch round differently, which test a bounds."""
    run = batch_passes(name, (3, 5), False)
    want = default_run(knobs, ("few", name), name, lambda m: run(m, knobs))
    assert_same(run(fresh(knobs, name, budget), knobs), want, f"{name} [{budget}]")


# ---------------------------------------------------------------------------- c. single sequence, chunked, every position
CHUNK_LENS = (40, 13)         # chunks of 16, 16, 8 rows, then a continuation at offset 40


def chunk_ids(name):
    rng = np.random.default_rng([CASES[name]["seed"], 300])
    return [rng.integers(0, BASE["vocab_size"], n).astype(np.int32) for n in CHUNK_LENS]


@functools.lru_cache(maxsize=None)
def oracle_chunked(name):
    """The oracle on both calls (its default regime: every call has six rows or more, weights rounded to T), and its layer-0 keys."""
    cfg, w, dt = checkpoint(name)
    orc = po.OracleLlama(cfg, w, dt)
    cache = [po.OracleKVCache() for _ in orc.layers]
    rows = [orc.forward(ids, cache) for ids in chunk_ids(name)]
    return np.concatenate(rows), cache[0].keys[0, :, :sum(CHUNK_LENS)].copy()


def chunked_calls(name, steps):
    def run(model):
        out, cache = {}, model.make_cache()
        for i, ids in enumerate(chunk_ids(name)):
            keep(out, f"call {i} logits", model(torch.from_numpy(ids)[None].cuda(), cache=cache)[0])
        assert cache[0].offset == sum(CHUNK_LENS)
        keep(out, "layer-0 K/V", cache[0].keys[0, :, :sum(CHUNK_LENS)], cache[0].values[0, :, :sum(CHUNK_LENS)])
        for st in range(steps):
            keep(out, f"step {st}", *model.step(None, cache))
        return out
    return run


@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("name", CHUNK_EXACT)
def test_chunked_prompt_all_positions_equal_default(knobs, name, budget):
    """prefill_t with prefill_chunk = 16 and logits on every position: the lm_head goes through the scratch (keep = false) and every layer
    matrix outside the budget is expanded again per chunk (3 chunks, then a 13-row call at offset 40).  Logits of all 53 positions, layer 0's K / V
    and four step(None) steps -- tokens, log-probabilities, logits -- equal the default decoder's bit for bit."""
    knobs("prefill_chunk", 16)
    run = chunked_calls(name, 4)
    want = default_run(knobs, ("chunked", name), name, run)
    assert_same(run(fresh(knobs, name, budget)), want, f"{name} [{budget}]")


@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("name", CHUNK_ORACLE)
def test_chunked_prompt_all_positions_int4_vs_oracle(knobs, name, budget):
    """The same two calls on int4 f16 and on int4 with Linear biases: per chunk k_dequant_w4s into the staging buffer for every matrix without
    tiles (the lm_head always: keep = false keeps nothing), k_rope_append_rows in place of the GEMM's RoPE epilogue, bias_rows.  Every position
    against OracleLlama in its many-row regime, and layer 0's keys against the oracle's cache."""
    knobs("prefill_chunk", 16)
    model = fresh(knobs, name, budget)
    want, want_k = oracle_chunked(name)
    cache, got = model.make_cache(), []
    for ids in chunk_ids(name):
        got.append(f32(model(torch.from_numpy(ids)[None].cuda(), cache=cache)[0]))
    got = np.concatenate(got)
    n = sum(CHUNK_LENS)
    assert cache[0].offset == n and got.shape == want.shape
    chk = Checks(name, f"[{budget}] chunked all positions vs oracle")
    for l in range(n):
        chk.add(got[l], want[l], f"position {l}")
    chk.add(f32(cache[0].keys[0, :, :n]).ravel(), want_k.ravel(), "layer-0 keys")
    chk.run()


# ---------------------------------------------------------------------------- d. graph replay with the expansion inside the graph
@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("name", GRAPH_CASES)
def test_step_batch_graph_holds_the_per_call_expansion(knobs, name, budget):
    """B = 8 on a decoder whose first batched pass is this step (the pages are filled by iterated decode steps): graph=True five times -- eager,
    capture, replays -- each fed the previous tokens, with the k_dequant_* / w16m_from_* launches of every matrix outside the budget among the
    captured nodes, against an identically built model running graph=False.  Then a prefill_batch (it grows the scratch and may admit matrices:
    alloc_gen moves) and two more graph=True steps: a graph captured before must not be replayed after.
    That the expansion IS inside the graph shows in its kernel nodes (pie_decoder_batch_graph_launches): more than a default decoder's graph
    of the same step holds, and for the dense model exactly one w16m_from_w16s launch more per matrix outside the budget -- all eight under
    `none`; under `mixed` five (layer 0's q|k|v and o_proj are resident by mixed_kb's inequality, and layer 1's q|k|v fits what they leave:
    703 KiB - 384 KiB >= 256 KiB, which then leaves too little for any other)."""
    B = 8

    def run(graph, model=None):
        model = model or fresh(knobs, name, budget)
        out = {}
        model.enable_paged_kv(num_pages=2 * B + 4 + 8, max_blocks=2)
        knobs("prefill_min", 100000)
        caches, toks = prefill_alone(model, sequences(name, B))
        knobs("prefill_min", None)
        feed = torch.tensor(toks, dtype=torch.int32)
        for st in range(5):
            res = model.step_batch(feed, caches, graph=graph)
            keep(out, f"step {st}", *res)
            feed = res[0].cpu().clone()
        launches, replays = model.batch_graph_launches(), model.batch_graph_replays()
        pcaches = [model.make_cache() for _ in PREFILL_LENS]
        keep(out, "prefill_batch", *model.prefill_batch([p.tolist() for p in prefill_prompts(name)], pcaches))
        for st in range(5, 7):
            res = model.step_batch(feed, caches, graph=graph)
            keep(out, f"step {st}", *res)
            feed = res[0].cpu().clone()
        return out, launches, replays

    resident = default_run(knobs, ("graph", name), name, lambda m: run(True, m)[1])
    want, _, _ = run(False)
    got, launches, replays = run(True)
    print(f"LAUNCHES {name} [{budget}] {launches} in the captured step, {resident} with every copy resident")
    assert launches > 0 and replays >= 3, f"{name} [{budget}]: the second call captures, the third to fifth replay ({launches} launches, {replays} replays)"
    assert launches > resident > 0
    if name == "dense_bf16":
        assert launches - resident == {"none": 8, "mixed": 5}[budget]
    assert_same(got, want, f"{name} [{budget}] graph=True against graph=False")


# ---------------------------------------------------------------------------- e. the weight scratch growing between passes
@functools.lru_cache(maxsize=None)
def wide_head_checkpoint(quant):
    cfg = dict(BASE, vocab_size=2048)
    if quant:
        cfg["quantization"] = {"group_size": 64, "bits": quant}
    else:
        del cfg["quantization"]
    return cfg, po.synth_checkpoint(cfg, seed=340 + quant, dtype=BF, lm_head_gain=4.0), BF


@pytest.mark.parametrize("budget", ("default", "none"))
@pytest.mark.parametrize("second_len", (17, 40))
@pytest.mark.parametrize("quant", (0, 8), ids=("dense_bf16", "int8_g64"))
def test_weight_scratch_grows_for_a_later_all_positions_call(knobs, quant, second_len, budget):
    """Vocabulary 2048: the lm_head's W16M copy is the largest.  model.step(prompt) sizes wT / wM without it (scratch_reserve for a prefill_t
    call that wants last-row logits only); a later model(ids) on a fresh cache wants logits on every position and the lm_head through the
    scratch: scratch_reserve must grow the two buffers -- its `w_elems > s->w_elems` branch for a second prompt of no more rows (17 after 24), the
    re-size of every chunk buffer carrying the larger of the two sizes for one of more (40).  Logits equal, bit for bit, a fresh model's that
    makes the second call only."""
    cfg, w, dt = wide_head_checkpoint(quant)
    rng = np.random.default_rng([quant, second_len])
    first, second = (torch.from_numpy(rng.integers(0, cfg["vocab_size"], n).astype(np.int32)) for n in (24, second_len))
    set_budget(knobs, None, budget)
    alone = build(cfg, w, dt)
    want = alone(second[None].cuda(), cache=alone.make_cache())[0].cpu().clone()
    model = build(cfg, w, dt)
    model.step(first.cuda(), model.make_cache())
    got = model(second[None].cuda(), cache=model.make_cache())[0].cpu().clone()
    assert got.shape == (second_len, 2048)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} logits differ after the weight scratch grew"
