"""-m gpu: frequency and presence penalties inside the decode step's configured tail against the host-orchestrated form: the
unconfigured step, then the definition's order on the host -- numpy's mask -> hip_ops.logits_penalty -> numpy's bias ->
tests/count_penalty_reference.py over bincount(generated so far) -> hip_ops.logprobs_argmax (-> the sampler closure on the same seed).
Every comparison is exact on storage bits."""
import numpy as np
import pytest
import torch

from tests._util import codes_dev, to_bits, to_dev
from tests.count_penalty_reference import count_penalty_reference, generated_counts
from tests.test_gpu_logits_bias import biased
from tests.test_gpu_step_edits import NINF, PEN, bias_table, half_mask, pack, unconfigured_launches, vocab
from tests.test_gpu_step_tail import DT, PROMPT, IdentityStructuringEngine, assert_runs_equal, dev_ids, f32_bits, make_caches, tiny  # noqa: F401  (tiny: the fixture)

pytestmark = pytest.mark.gpu
STEPS = 24
FP = (0.5, 1.5)
START = len(PROMPT)


def host_loop(model, cache, prompt, steps, fp, mask=None, penalty=None, bias=None, sampler=None, graph=True):
    """fp: one (f, p) for every step, or a list of them.  Per step: (token, logprobs bits, processed logits bits)."""
    from proxy_inference_engine_amd import hip_ops
    model.set_step_tail()
    assert model.step_tail_counts[0] is None
    V = model.logprobs.numel()
    fed, gen, out, ids = [], [], [], dev_ids(prompt)
    for i in range(steps):
        f, p = fp[i] if isinstance(fp, list) else fp
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
        if (f, p) != (0.0, 0.0):
            bits = count_penalty_reference(bits, generated_counts(gen, V), f, p, DT)
        tok, lp = hip_ops.logprobs_argmax(to_dev(bits, DT))
        if sampler is not None:
            tok = sampler(lp[None]).reshape(1).to(torch.int32)
        out.append((int(tok.item()), f32_bits(lp), bits))
        gen.append(int(tok.item()))
        ids = tok.reshape(1).to(torch.int32).clone()
    return out


def fused_loop(model, cache, prompt, steps, fp, mask=None, penalty=None, bias=None, sampler=None, graph=True, each_step=None):
    out = []
    words = pack(mask) if mask is not None else None
    for i in range(steps):
        f, p = fp[i] if isinstance(fp, list) else fp
        model.set_step_tail(sampler=sampler.hip_spec if sampler is not None else None, repetition_penalty=penalty[0] if penalty else 1.0,
                            context_size=penalty[1] if penalty else 60, token_mask=words, logit_bias=bias,
                            frequency_penalty=f, presence_penalty=p, count_start=len(prompt) if i == 0 else None)
        if each_step is not None:
            each_step(i)
        tok, lp, lg = model.step(dev_ids(prompt) if i == 0 else None, cache, graph=graph)
        out.append((int(tok.item()), f32_bits(lp), to_bits(lg).copy()))
    return out


def counts_of(model) -> np.ndarray:
    return model.step_tail_counts[1].cpu().numpy()


# ------------------------------------------------------------------ 1. the step against the host loop
@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("name", ["alone", "all"])
def test_step_with_count_penalties_matches_host_loop(tiny, name, sampled, graph):
    from proxy_inference_engine_amd import samplers
    g, cfg, model = tiny
    V = vocab(cfg)
    everything = name == "all"
    kw = dict(mask=half_mask(V, 1) if everything else None, penalty=PEN if everything else None, bias=bias_table(V) if everything else None,
              sampler=samplers.make_sampler(temp=0.8, top_k=5) if sampled else None, graph=graph)
    try:
        samplers.seed(21)
        host = host_loop(model, model.make_cache(), PROMPT, STEPS, FP, **kw)
        samplers.seed(21)
        fused = fused_loop(model, model.make_cache(), PROMPT, STEPS, FP, **kw)
        assert model.step_tail_counts[0] == (*FP, START) and model.step_tail == (kw["sampler"].hip_spec if sampled else None, PEN if everything else None)
        assert_runs_equal(fused, host, f"{name}, sampled {sampled}, graph {graph}")
        # after n steps the counts are the generated tokens' multiplicities -- all but the last, which has not been fed yet -- and no prompt id
        toks = [f[0] for f in fused]
        assert np.array_equal(counts_of(model), generated_counts(toks[:-1], V)), name
        assert int(counts_of(model).sum()) == STEPS - 1
        absent = [t for t in set(PROMPT) if t not in toks[:-1]]
        assert absent and not counts_of(model)[absent].any()
    finally:
        model.set_step_tail()
    assert model.step_tail_counts[0] is None and model.step_tail == (None, None)


def test_positive_and_negative_pairs(tiny):
    """The largest pair of either sign: the first token is chosen against empty counts (the unpenalised logits), a run whose greedy tokens
    repeat is changed by the positive pair, and the negative pair -- penalties that reward repetition -- equals the host loop too."""
    g, cfg, model = tiny
    try:
        plain = fused_loop(model, model.make_cache(), PROMPT, 8, (0.0, 0.0))
        pos = fused_loop(model, model.make_cache(), PROMPT, 8, (2.0, 2.0))
        neg = fused_loop(model, model.make_cache(), PROMPT, 8, (-2.0, -2.0))
        host = host_loop(model, model.make_cache(), PROMPT, 8, (-2.0, -2.0))
    finally:
        model.set_step_tail()
    assert [f[0] for f in pos] != [f[0] for f in plain] or len(set(f[0] for f in plain)) == 8
    assert_runs_equal(neg, host, "negative penalties")
    assert np.array_equal(pos[0][2], plain[0][2])                             # the first token is chosen against empty counts


# ------------------------------------------------------------------ 2. replay, launches
def test_new_penalty_values_replay_the_captured_graph(tiny):
    """(f, p) change every step behind the record's address: the step keeps replaying, and the logits follow the new values."""
    g, cfg, model = tiny
    U = unconfigured_launches(model)
    fps = [(0.5, 0.0) if i % 2 == 0 else (-1.0, -0.25) for i in range(STEPS)]
    seen = []
    try:
        host = host_loop(model, model.make_cache(), PROMPT, STEPS, fps)
        fused = fused_loop(model, model.make_cache(), PROMPT, STEPS, fps, each_step=lambda i: seen.append(model.graph_launches()))
        assert_runs_equal(fused, host, "alternating penalties")
        # step 0 is the prompt pass, step 1 captures; from then on the graph is there BEFORE each step (a dropped one reads -1) and unchanged after
        assert seen[2:] == [U + 2] * (STEPS - 2) and model.graph_launches() == U + 2, seen
    finally:
        model.set_step_tail()


def test_launch_budget(tiny):
    """The count penalty alone: U + 2 (its launch, the partials); with a bias and / or a repetition penalty U + 3 (their edit launch, the
    count launch, the partials); a mask on top none; a sampler adds what it adds alone; nothing set: U."""
    from proxy_inference_engine_amd import samplers
    g, cfg, model = tiny
    V = vocab(cfg)
    U = unconfigured_launches(model)
    assert U > 0
    sampler = samplers.make_sampler(temp=0.8, top_k=5)
    try:
        fused_loop(model, model.make_cache(), PROMPT, 3, (0.0, 0.0), sampler=sampler)
        S = model.graph_launches() - U
        assert S > 0
        for kw, extra in ((dict(), 2), (dict(mask=half_mask(V, 1)), 2), (dict(bias=bias_table(V)), 3), (dict(penalty=PEN), 3),
                          (dict(mask=half_mask(V, 1), penalty=PEN, bias=bias_table(V)), 3)):
            for smp in (None, sampler):
                fused_loop(model, model.make_cache(), PROMPT, 3, FP, sampler=smp, **kw)
                assert model.graph_launches() == U + extra + (S if smp is not None else 0), (sorted(kw), smp is not None)
    finally:
        model.set_step_tail()
    assert model.graph_launches() == -1                      # switching the feature off dropped the captured graphs
    assert unconfigured_launches(model) == U


def test_reset_step_counts_rebuilds_the_state(tiny):
    """reset_step_counts rebuilds the counts from the generated ids (a trimmed cache, a request resumed in a fresh one): the prompt pass
    that follows applies them and counts nothing, the fed-back step after it counts its token."""
    g, cfg, model = tiny
    V = vocab(cfg)
    try:
        toks = [f[0] for f in fused_loop(model, model.make_cache(), PROMPT, 7, FP)]
        longer = PROMPT + toks[:6]
        model.set_step_tail()
        raw = to_bits(model.step(dev_ids(longer), model.make_cache())[2]).copy()
        model.set_step_tail(frequency_penalty=FP[0], presence_penalty=FP[1], count_start=START)
        assert not counts_of(model).any()
        model.reset_step_counts(START, toks[:6])
        assert np.array_equal(counts_of(model), generated_counts(toks[:6], V)) and model.step_tail_counts[0] == (*FP, START)
        cache = model.make_cache()
        tok, lp, lg = model.step(dev_ids(longer), cache)
        assert np.array_equal(to_bits(lg), count_penalty_reference(raw, generated_counts(toks[:6], V), *FP, DT))
        assert np.array_equal(counts_of(model), generated_counts(toks[:6], V))          # a prompt pass counts nothing
        first = int(tok.item())
        model.step(None, cache, graph=False)
        assert np.array_equal(counts_of(model), generated_counts(toks[:6] + [first], V))
        with pytest.raises(ValueError):
            model.set_step_tail(frequency_penalty=2.5)
        with pytest.raises(ValueError):
            model.set_step_tail(presence_penalty=float("nan"))
    finally:
        model.set_step_tail()
    with pytest.raises(RuntimeError):
        model.reset_step_counts(0)


# ------------------------------------------------------------------ 3. every cache kind
@pytest.mark.parametrize("kind", ["reusable", "pages", "quantized", "rotating"])
def test_count_penalties_on_every_cache_kind(tiny, kind):
    from proxy_inference_engine_amd import samplers
    g, cfg, model = tiny
    V = vocab(cfg)
    kw = dict(mask=half_mask(V, 3), penalty=PEN, bias=bias_table(V), sampler=samplers.make_sampler(temp=0.8, top_k=5))
    try:
        samplers.seed(5)
        host = host_loop(model, make_caches(model, kind), PROMPT, 12, (-1.0, -0.25), **kw)
        samplers.seed(5)
        fused = fused_loop(model, make_caches(model, kind), PROMPT, 12, (-1.0, -0.25), **kw)
        assert_runs_equal(fused, host, kind)
    finally:
        model.set_step_tail()


# ------------------------------------------------------------------ 4. refusals and the raw __call__
def test_tensor_parallel_refuses_and_call_keeps_raw_logits(tiny):
    import ctypes as C
    from oracle import pie_oracle as po
    from proxy_inference_engine_amd import _ffi, hip_ops
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    from proxy_inference_engine_amd.tp import HipComm
    from tests.test_gpu_tp import CFG
    g, cfg, model = tiny
    V = vocab(cfg)
    lib = _ffi.load()
    w = po.synth_checkpoint(CFG, seed=72, dtype=DT, lm_head_gain=4.0)
    dev_w = {k: (codes_dev(v) if v.dtype == np.uint32 else to_dev(v, DT)) for k, v in w.items()}
    comm = HipComm(CFG["hidden_size"], backend="ipc")
    rec = hip_ops.count_penalty_records([hip_ops.count_penalty_pack(0.5, 0.5, 3)] * 2, "cuda")
    try:
        tp = Model(ModelArgs(**CFG), dev_w, tp=comm)
        cnt = torch.zeros((2, CFG["vocab_size"]), dtype=torch.int32, device="cuda")
        assert lib.pie_decoder_set_count_penalty(tp._dec, _ffi.p(rec), _ffi.p(cnt)) == -5 and b"pie_decoder_set_count_penalty" in lib.pie_last_error()
        assert lib.pie_decoder_set_count_penalty(tp._dec, None, None) == -5
        assert lib.pie_decoder_set_batch_count_penalty(tp._dec, _ffi.p(rec), _ffi.p(cnt), 2) == -5 and b"pie_decoder_set_batch_count_penalty" in lib.pie_last_error()
        with pytest.raises(RuntimeError):
            tp.set_step_tail(frequency_penalty=0.5)
        tp.set_step_tail()   # the defaults are what it already has: nothing is asked of the library
        del tp
    finally:
        comm.close()
    # the setters' own argument checks on a decoder that takes them
    cnt = torch.zeros((2, V), dtype=torch.int32, device="cuda")
    assert lib.pie_decoder_set_count_penalty(model._dec, _ffi.p(rec), None) == -1
    assert lib.pie_decoder_set_count_penalty(model._dec, C.c_void_p(rec.data_ptr() + 2), _ffi.p(cnt)) == -3
    assert lib.pie_decoder_set_count_penalty(model._dec, _ffi.p(rec), C.c_void_p(cnt.data_ptr() + 1)) == -3
    assert lib.pie_decoder_set_batch_count_penalty(model._dec, _ffi.p(rec), None, 2) == -1 and lib.pie_decoder_set_batch_count_penalty(model._dec, _ffi.p(rec), _ffi.p(cnt), 0) == -1
    assert lib.pie_decoder_set_batch_count_penalty(model._dec, C.c_void_p(rec.data_ptr() + 2), _ffi.p(cnt), 2) == -3
    assert model.step_tail_counts[0] is None
    # Model.__call__ returns raw logits while the penalties are set, and counts nothing
    tokens = dev_ids(PROMPT).long()[None]
    raw = to_bits(model(tokens, cache=model.make_cache()))
    one = to_bits(model(tokens[:, :1], cache=model.make_cache()))
    try:
        model.set_step_tail(frequency_penalty=2.0, presence_penalty=2.0, count_start=0)
        model.reset_step_counts(0, PROMPT)                                              # non-zero counts: a processed row would differ
        got = to_bits(model(tokens, cache=model.make_cache()))
        got_one = to_bits(model(tokens[:, :1], cache=model.make_cache()))   # a single row: the decode step's launches with logits on every position
        assert np.array_equal(counts_of(model), generated_counts(PROMPT, V))
    finally:
        model.set_step_tail()
    assert np.array_equal(got, raw) and np.array_equal(got_one, one)


# ------------------------------------------------------------------ 5. the engine
def test_engine_fused_tail_equals_host_orchestrated_branch(tiny):
    """generate(frequency_penalty=, presence_penalty=) through the fused tail equals the same request on the processor branch (a
    structuring engine forces it), token for token; a second request on the same engine reuses the prompt's prefix and starts from zero
    counts."""
    from proxy_inference_engine_amd import InferenceEngine
    g, cfg, model = tiny
    V = vocab(cfg)
    kwargs = dict(temp=0, frequency_penalty=1.0, presence_penalty=0.5, max_completion_tokens=12)
    runs = {}
    try:
        for name, se in (("fused", None), ("host", IdentityStructuringEngine())):
            eng = InferenceEngine(model=model, structuring_engine=se)
            both = []
            for prompt in (PROMPT, PROMPT + [9, 450]):                               # the second request reuses the first one's prefix
                eng.prepare_engine(prompt, **kwargs)
                both.append([t for t, _ in eng.generate(prompt, **kwargs)])
                assert (model.step_tail_counts[0] is not None) == (name == "fused"), name
                if name == "fused":
                    assert model.step_tail_counts[0] == (1.0, 0.5, len(prompt))
                    assert np.array_equal(counts_of(model), generated_counts(both[-1][:-1], V))   # this request's tokens only
            runs[name] = both
        plain = InferenceEngine(model=model)
        plain.prepare_engine(PROMPT, temp=0)
        greedy = [t for t, _ in plain.generate(PROMPT, temp=0, max_completion_tokens=12)]
    finally:
        model.set_step_tail()
    assert runs["fused"] == runs["host"] and all(len(r) == 12 for r in runs["fused"])
    assert runs["fused"][0][0] == greedy[0]                                          # the first token is chosen against empty counts
