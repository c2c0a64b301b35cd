"""-m gpu: the DRY penalty inside the decode step's configured tail against the host-orchestrated form: the unconfigured
step, then the definition's order on the host -- numpy's mask -> hip_ops.logits_penalty -> numpy's bias -> the count penalty's reference
-> the stand-alone hip_ops.logits_dry_penalty over the ids fed so far -> hip_ops.logprobs_argmax (-> the sampler closure on the same
seed).  Every comparison is exact on storage bits.  The prompts are a short pattern repeated (test_gpu_speculative.e2e_prompt); the
seeds were chosen with the CPU oracle so that the rule fires on well over a third of the steps, and every run asserts from
tests/dry_penalty_reference.py that it did."""
import numpy as np
import pytest
import torch

from tests import dry_penalty_reference as ref
from tests._util import codes_dev, to_bits, to_dev
from tests.count_penalty_reference import count_penalty_reference, generated_counts
from tests.test_gpu_logits_bias import biased
from tests.test_gpu_speculative import e2e_prompt
from tests.test_gpu_step_edits import NINF, PEN, bias_table, half_mask, pack, unconfigured_launches, vocab
from tests.test_gpu_step_tail import DT, PROMPT, IdentityStructuringEngine, assert_runs_equal, dev_ids, f32_bits, make_caches, tiny  # noqa: F401  (tiny: the fixture)

pytestmark = pytest.mark.gpu
STEPS = 24
DRY = (0.8, 1.75, 2, 1024, ())
DRY_ALL = (0.8, 1.75, 1, 40, (3, 77))      # beside the other edits: every repeat counts, a short range, two breakers
FP = (0.5, 0.25)
SEEDS = (5, 7)                             # e2e_prompt seeds: the oracle's DRY run fires on 14 and 15 of 24 steps; seed 7's own tail repeats (L = 33 at step 0)


def prompt_of(seed, cfg):
    return [int(t) for t in e2e_prompt(seed, vocab(cfg))]


def host_loop(model, cache, prompt, steps, dry, mask=None, penalty=None, bias=None, fp=None, sampler=None, graph=True):
    """dry: one record for every step, or a list of them.  Returns (per step: (token, logprobs bits, processed logits bits), steps on
    which the reference penalises at least one id)."""
    from proxy_inference_engine_amd import hip_ops
    model.set_step_tail()
    assert model.step_tail_dry is None
    V = model.logprobs.numel()
    fed, gen, out, fired, ids = [], [], [], 0, dev_ids(prompt)
    for i in range(steps):
        m, b, a, r, brk = dry[i] if isinstance(dry, list) else dry
        lg = model.step(ids, cache, graph=graph)[2]
        fed += ids.tolist()
        bits = to_bits(lg).copy()
        if mask is not None:
            bits = np.where(mask, bits, NINF)
        if penalty is not None:
            t = to_dev(bits, DT)
            hip_ops.logits_penalty(t, dev_ids(fed[-penalty[1]:]), penalty[0])
            bits = to_bits(t).copy()
        if bias is not None:
            bits = biased(bits, bias[0], bias[1], DT)
        if fp is not None:
            bits = count_penalty_reference(bits, generated_counts(gen, V), *fp, DT)
        want = ref.apply(bits, DT, fed[-r:], m, b, a, brk)
        fired += bool(ref.penalties(fed[-r:], V, m, b, a, brk))
        t = to_dev(bits, DT)
        hip_ops.logits_dry_penalty(t, dev_ids(fed[-r:]), m, b, a, brk)
        bits = to_bits(t).copy()
        assert np.array_equal(bits, want), i                          # the stand-alone op is the reference on these logits too
        tok, lp = hip_ops.logprobs_argmax(to_dev(bits, DT))
        if sampler is not None:
            tok = sampler(lp[None]).reshape(1).to(torch.int32)
        out.append((int(tok.item()), f32_bits(lp), bits))
        gen.append(int(tok.item()))
        ids = tok.reshape(1).to(torch.int32).clone()
    return out, fired


def fused_loop(model, cache, prompt, steps, dry, mask=None, penalty=None, bias=None, fp=None, sampler=None, graph=True, each_step=None):
    out = []
    words = pack(mask) if mask is not None else None
    for i in range(steps):
        model.set_step_tail(sampler=sampler.hip_spec if sampler is not None else None, repetition_penalty=penalty[0] if penalty else 1.0,
                            context_size=penalty[1] if penalty else 60, token_mask=words, logit_bias=bias,
                            frequency_penalty=fp[0] if fp else 0.0, presence_penalty=fp[1] if fp else 0.0, count_start=len(prompt) if fp and i == 0 else None,
                            dry=dry[i] if isinstance(dry, list) else dry)
        if each_step is not None:
            each_step(i)
        tok, lp, lg = model.step(dev_ids(prompt) if i == 0 else None, cache, graph=graph)
        out.append((int(tok.item()), f32_bits(lp), to_bits(lg).copy()))
    return out


def everything(V):
    from proxy_inference_engine_amd import samplers
    return dict(mask=half_mask(V, 1), penalty=PEN, bias=bias_table(V), fp=FP, sampler=samplers.make_sampler(temp=0.8, top_k=5))


# ------------------------------------------------------------------ 1. the step against the host loop
@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("name", ["alone", "all"])
@pytest.mark.parametrize("seed", SEEDS)
def test_step_with_dry_matches_host_loop(tiny, seed, name, graph):
    from proxy_inference_engine_amd import samplers
    g, cfg, model = tiny
    prompt = prompt_of(seed, cfg)
    kw = dict(everything(vocab(cfg)), graph=graph) if name == "all" else dict(graph=graph)
    dry = DRY_ALL if name == "all" else DRY
    try:
        samplers.seed(21)
        host, fired = host_loop(model, model.make_cache(), prompt, STEPS, dry, **kw)
        samplers.seed(21)
        fused = fused_loop(model, model.make_cache(), prompt, STEPS, dry, **kw)
        assert model.step_tail_dry == dry
        print(f"DRY fired on {fired} of {STEPS} steps ({name}, seed {seed})")
        assert 3 * fired >= STEPS, (name, seed, fired)                # nothing passes vacuously
        assert_runs_equal(fused, host, f"{name}, seed {seed}, graph {graph}")
    finally:
        model.set_step_tail()
    assert model.step_tail_dry is None and model.step_tail == (None, None)


def test_dry_changes_the_run_and_multiplier_zero_is_off(tiny):
    g, cfg, model = tiny
    prompt = prompt_of(SEEDS[1], cfg)
    try:
        plain = fused_loop(model, model.make_cache(), prompt, 8, None)
        zero = fused_loop(model, model.make_cache(), prompt, 8, (0.0, 1.75, 2, 1024, ()))
        assert model.step_tail_dry is None                            # a multiplier of 0 arms nothing
        strong = fused_loop(model, model.make_cache(), prompt, 8, (8.0, 1.75, 1, 1024, ()))
    finally:
        model.set_step_tail()
    assert_runs_equal(zero, plain, "multiplier 0")
    assert not np.array_equal(strong[0][2], plain[0][2])              # the prompt's own tail repeats: the first token is chosen against it
    with pytest.raises(ValueError):
        model.set_step_tail(dry=(0.8, 1.75, 2, 1024))
    with pytest.raises(ValueError):
        model.set_step_tail(dry=(0.8, 0.0, 2, 1024, ()))
    assert model.step_tail_dry is None


# ------------------------------------------------------------------ 2. replay, launches
def test_new_record_values_replay_the_captured_graph(tiny):
    """The record and the breaker table change every step behind their addresses: the step keeps replaying, and the logits follow."""
    g, cfg, model = tiny
    prompt = prompt_of(SEEDS[1], cfg)
    U = unconfigured_launches(model)
    recs = [DRY if i % 2 == 0 else (1.5, 2.0, 1, 50, (int(prompt[0]), 77)) for i in range(STEPS)]
    seen = []
    try:
        host, fired = host_loop(model, model.make_cache(), prompt, STEPS, recs)
        fused = fused_loop(model, model.make_cache(), prompt, STEPS, recs, each_step=lambda i: seen.append(model.graph_launches()))
        assert 3 * fired >= STEPS, fired
        assert_runs_equal(fused, host, "alternating records")
        # step 0 is the prompt pass, step 1 captures; from then on the graph is there BEFORE each step (a dropped one reads -1) and unchanged after
        assert seen[2:] == [U + 2] * (STEPS - 2) and model.graph_launches() == U + 2, seen
    finally:
        model.set_step_tail()


def test_launch_budget(tiny):
    """Launches of the captured step beyond the unconfigured step's U:
        DRY alone                                  2   its launch + the partials (nothing else had made them stale)
        DRY + mask                                 2   the mask rides the partials
        DRY + bias and / or repetition penalty     3   + their one edit launch
        DRY + count penalties                      3   + the count launch
        DRY + all of them                          4
    a sampler adds what it adds alone; nothing set: U."""
    from proxy_inference_engine_amd import samplers
    g, cfg, model = tiny
    V = vocab(cfg)
    U = unconfigured_launches(model)
    assert U > 0
    sampler = samplers.make_sampler(temp=0.8, top_k=5)
    try:
        fused_loop(model, model.make_cache(), PROMPT, 3, None, sampler=sampler)
        S = model.graph_launches() - U
        assert S > 0
        for kw, extra in ((dict(), 2), (dict(mask=half_mask(V, 1)), 2), (dict(bias=bias_table(V)), 3), (dict(penalty=PEN), 3), (dict(penalty=PEN, bias=bias_table(V)), 3),
                          (dict(fp=FP), 3), (dict(mask=half_mask(V, 1), penalty=PEN, bias=bias_table(V), fp=FP), 4)):
            for smp in (None, sampler):
                fused_loop(model, model.make_cache(), PROMPT, 3, DRY, sampler=smp, **kw)
                assert model.graph_launches() == U + extra + (S if smp is not None else 0), (sorted(kw), smp is not None)
    finally:
        model.set_step_tail()
    assert model.graph_launches() == -1                      # switching the feature off dropped the captured graphs
    assert unconfigured_launches(model) == U


# ------------------------------------------------------------------ 3. every cache kind
@pytest.mark.parametrize("kind", ["reusable", "pages", "quantized", "rotating"])
def test_dry_on_every_cache_kind(tiny, kind):
    from proxy_inference_engine_amd import samplers
    g, cfg, model = tiny
    V = vocab(cfg)
    prompt = prompt_of(8, cfg)
    # a mask and a bias beside DRY, greedy, and every repeat counts over everything fed: a run on which the rule fires on every cache kind
    # (7 or 8 of 12 steps; under the sampler and the other penalties of everything() the rotating cache's run repeats on 2 of 12 only)
    kw = dict(mask=half_mask(V, 1), bias=bias_table(V))
    dry = (0.8, 1.75, 1, 1024, ())
    try:
        samplers.seed(5)
        host, fired = host_loop(model, make_caches(model, kind), prompt, 12, dry, **kw)
        samplers.seed(5)
        fused = fused_loop(model, make_caches(model, kind), prompt, 12, dry, **kw)
        print(f"DRY fired on {fired} of 12 steps ({kind})")
        assert 3 * fired >= 12, fired
        assert_runs_equal(fused, host, kind)
    finally:
        model.set_step_tail()


# ------------------------------------------------------------------ 4. refusals and the raw outputs
def test_tensor_parallel_refuses_and_call_keeps_raw_logits(tiny):
    import ctypes as C
    from oracle import pie_oracle as po
    from proxy_inference_engine_amd import _ffi, hip_ops
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    from proxy_inference_engine_amd.tp import HipComm
    from tests.test_gpu_tp import CFG
    g, cfg, model = tiny
    lib = _ffi.load()
    w = po.synth_checkpoint(CFG, seed=72, dtype=DT, lm_head_gain=4.0)
    dev_w = {k: (codes_dev(v) if v.dtype == np.uint32 else to_dev(v, DT)) for k, v in w.items()}
    comm = HipComm(CFG["hidden_size"], backend="ipc")
    rec = hip_ops.dry_penalty_records([hip_ops.dry_penalty_pack(0.8)] * 2, "cuda")
    brk = torch.zeros((2, 64), dtype=torch.int32, device="cuda")
    ring = torch.zeros((2, 1024), dtype=torch.int32, device="cuda")
    R, B, G = _ffi.p(rec), _ffi.p(brk), _ffi.p(ring)
    try:
        tp = Model(ModelArgs(**CFG), dev_w, tp=comm)
        assert lib.pie_decoder_set_dry_penalty(tp._dec, R, B, G, 1024) == -5 and b"pie_decoder_set_dry_penalty" in lib.pie_last_error()
        assert lib.pie_decoder_set_dry_penalty(tp._dec, None, None, None, 0) == -5
        assert lib.pie_decoder_set_batch_dry_penalty(tp._dec, R, B, G, 2) == -5 and b"pie_decoder_set_batch_dry_penalty" in lib.pie_last_error()
        with pytest.raises(RuntimeError):
            tp.set_step_tail(dry=DRY)
        tp.set_step_tail()   # the defaults are what it already has: nothing is asked of the library
        del tp
    finally:
        comm.close()
    # the setters' own argument checks on a decoder that takes them
    odd = lambda t, by: C.c_void_p(t.data_ptr() + by)
    assert lib.pie_decoder_set_dry_penalty(model._dec, R, None, G, 1024) == -1 and lib.pie_decoder_set_dry_penalty(model._dec, R, B, None, 1024) == -1
    assert lib.pie_decoder_set_dry_penalty(model._dec, R, B, G, 0) == -1
    assert lib.pie_decoder_set_dry_penalty(model._dec, odd(rec, 2), B, G, 1024) == -3 and lib.pie_decoder_set_dry_penalty(model._dec, R, odd(brk, 1), G, 1024) == -3
    assert lib.pie_decoder_set_dry_penalty(model._dec, R, B, odd(ring, 2), 1024) == -3
    assert lib.pie_decoder_set_batch_dry_penalty(model._dec, R, None, G, 2) == -1 and lib.pie_decoder_set_batch_dry_penalty(model._dec, R, B, None, 2) == -1
    assert lib.pie_decoder_set_batch_dry_penalty(model._dec, R, B, G, 0) == -1 and lib.pie_decoder_set_batch_dry_penalty(model._dec, odd(rec, 2), B, G, 2) == -3
    assert lib.pie_decoder_set_batch_dry_penalty(model._dec, R, B, odd(ring, 1), 2) == -3
    assert model.step_tail_dry is None
    # Model.__call__ returns raw logits while DRY is set
    prompt = prompt_of(SEEDS[1], cfg)
    tokens = dev_ids(prompt).long()[None]
    raw = to_bits(model(tokens, cache=model.make_cache()))
    one = to_bits(model(tokens[:, :1], cache=model.make_cache()))
    try:
        model.set_step_tail(dry=(8.0, 1.75, 1, 1024, ()))
        got = to_bits(model(tokens, cache=model.make_cache()))
        got_one = to_bits(model(tokens[:, :1], cache=model.make_cache()))   # a single row: the decode step's launches with logits on every position
        stepped = to_bits(model.step(dev_ids(prompt), model.make_cache())[2])
    finally:
        model.set_step_tail()
    assert np.array_equal(got, raw) and np.array_equal(got_one, one)
    assert not np.array_equal(stepped, raw[0, -1])                    # (and the configured step does differ on this prompt)


def test_spec_step_refuses_a_dry_tail(tiny):
    from proxy_inference_engine_amd import _ffi
    from proxy_inference_engine_amd.cache import ReusableKVCache
    g, cfg, model = tiny
    lib, st = _ffi.load(), model._spec_state()
    rec, draft = st["rec"], dev_ids([1] * 7)
    cache = [ReusableKVCache() for _ in model.layers]
    model.step(dev_ids(np.random.default_rng(5).integers(0, vocab(cfg), 20)), cache)
    raw_call = lambda: lib.pie_decoder_spec_step(model._dec, _ffi.p(draft), 7, _ffi.p(rec[1:]), _ffi.p(rec[0:]), None, _ffi.p(st["ws"]), None, 0, None, _ffi.stream())
    try:
        model.set_step_tail(dry=DRY)
        with pytest.raises(ValueError, match="greedy and raw"):
            model.spec_step(draft, cache)
        assert raw_call() == -5                                       # PIE_E_STATE from the library too, before any launch
    finally:
        model.set_step_tail()
    before = all(c.offset == 20 for c in cache)
    tokens, n, _ = model.spec_step(draft, cache)                      # and after that the pass still runs
    assert before and 1 <= n <= 8 and all(c.offset == 20 + n for c in cache)


# ------------------------------------------------------------------ 5. the engine
def test_engine_fused_tail_equals_host_orchestrated_branch(tiny):
    """generate(dry_multiplier=...) through the fused tail equals the same request on the processor branch (a structuring engine forces
    it), token for token; a second request on the same engine reuses the first one's prefix; DRY changes what plain greedy generates."""
    from proxy_inference_engine_amd import InferenceEngine
    g, cfg, model = tiny
    prompt = prompt_of(SEEDS[1], cfg)
    kwargs = dict(temp=0, dry_multiplier=0.8, dry_base=1.75, dry_allowed_length=2, dry_range=1024, dry_sequence_breakers=[3, 77], max_completion_tokens=16)
    runs = {}
    try:
        for name, se in (("fused", None), ("host", IdentityStructuringEngine())):
            eng = InferenceEngine(model=model, structuring_engine=se)
            both = []
            for p in (prompt, prompt + prompt[:5]):                  # the second request reuses the first one's prefix
                eng.prepare_engine(p, **kwargs)
                both.append([t for t, _ in eng.generate(p, **kwargs)])
                assert (model.step_tail_dry is not None) == (name == "fused"), name
                if name == "fused":
                    assert model.step_tail_dry == (0.8, 1.75, 2, 1024, (3, 77))
            runs[name] = both
        plain = InferenceEngine(model=model)
        plain.prepare_engine(prompt, temp=0)
        greedy = [t for t, _ in plain.generate(prompt, temp=0, max_completion_tokens=16)]
    finally:
        model.set_step_tail()
    assert runs["fused"] == runs["host"] and all(len(r) == 16 for r in runs["fused"])
    assert runs["fused"][0] != greedy


def test_plain_generation_is_the_same_before_and_after_a_dry_one(tiny):
    from proxy_inference_engine_amd import InferenceEngine
    g, cfg, model = tiny
    prompt = prompt_of(SEEDS[1], cfg)

    def plain():
        eng = InferenceEngine(model=model)
        eng.prepare_engine(prompt, temp=0)
        gen = eng.generate_step(torch.tensor(prompt))
        toks, bits = [], []
        for _ in range(16):
            t, lp = next(gen)
            toks.append(int(t.item())), bits.append(f32_bits(lp))
        return toks, np.stack(bits), model.graph_launches()

    try:
        toks0, bits0, launches0 = plain()
        eng = InferenceEngine(model=model)
        eng.prepare_engine(prompt, temp=0, dry_multiplier=0.8)
        dry = [t for t, _ in eng.generate(prompt, temp=0, dry_multiplier=0.8, max_completion_tokens=16)]
        assert model.step_tail_dry is not None and model.graph_launches() == launches0 + 2
        toks1, bits1, launches1 = plain()
    finally:
        model.set_step_tail()
    assert launches0 > 0 and launches1 == launches0                  # the captured step's kernel count
    assert toks1 == toks0 and np.array_equal(bits0, bits1) and dry != toks0
