"""-m gpu: the token mask and the logit bias inside the decode step's configured tail against the host-orchestrated form
they replace: the unconfigured step, then numpy's mask -> hip_ops.logits_penalty -> numpy's bias -> hip_ops.logprobs_argmax (-> the
sampler closure on the same seed).  Every comparison is exact on storage bits; no expected value here is a NaN."""
import numpy as np
import pytest
import torch

from tests._util import codes_dev, to_bits, to_dev
from tests.test_gpu_logits_bias import biased
from tests.test_gpu_step_tail import DT, PROMPT, assert_runs_equal, dev_ids, f32_bits, make_caches, tiny  # noqa: F401  (tiny: the fixture)

pytestmark = pytest.mark.gpu
NINF = np.uint16(0xFF80)   # bf16 -inf
PEN = (1.8, 5)             # the window holds 301 three times and 77 twice
STEPS = 10


def vocab(cfg) -> int:
    return int(cfg["vocab_size"])


def half_mask(V: int, seed: int) -> np.ndarray:
    """About half of the ids allowed; 77 -- inside the penalty's window -- is not, 301 -- biased AND penalised -- is."""
    m = np.random.default_rng(seed).random(V) < 0.5
    m[77], m[301] = False, True
    return m


def bias_table(V: int):
    """301 carries a bias and the penalty; 17 and 450 sit further back in the prompt; V + 3 is out of range and skipped."""
    return (301, 17, 450, V + 3), (-4.0, 1.5, 2.25, 1.0)


def pack(m: np.ndarray) -> torch.Tensor:
    from proxy_inference_engine_amd import hip_ops
    return hip_ops.pack_token_mask(torch.from_numpy(m), m.size)


def host_loop(model, cache, prompt, steps, masks=None, penalty=None, bias=None, sampler=None, graph=True):
    """The unconfigured step, then the definition's order on the host.  Per step: (token, logprobs bits, processed logits bits)."""
    from proxy_inference_engine_amd import hip_ops
    model.set_step_tail()
    assert model.step_tail == (None, None) and model.step_tail_edits == (None, None)
    fed, out, ids = [], [], dev_ids(prompt)
    for i in range(steps):
        lg = model.step(ids, cache, graph=graph)[2]
        fed += ids.tolist()
        bits = to_bits(lg).copy()
        if masks is not None:
            bits = np.where(masks[i], bits, NINF)
        if penalty is not None:
            t = to_dev(bits, DT)
            hip_ops.logits_penalty(t, dev_ids(fed[-penalty[1]:]), penalty[0])
            bits = to_bits(t).copy()
        if bias is not None:
            bits = biased(bits, bias[0], bias[1], DT)
        tok, lp = hip_ops.logprobs_argmax(to_dev(bits, DT))
        if sampler is not None:
            tok = sampler(lp[None]).reshape(1).to(torch.int32)
        out.append((int(tok.item()), f32_bits(lp), bits))
        ids = tok.reshape(1).to(torch.int32).clone()
    return out


def fused_loop(model, cache, prompt, steps, masks=None, penalty=None, bias=None, sampler=None, graph=True, each_step=None):
    out = []
    for i in range(steps):
        model.set_step_tail(sampler=sampler.hip_spec if sampler is not None else None, repetition_penalty=penalty[0] if penalty else 1.0,
                            context_size=penalty[1] if penalty else 60, token_mask=pack(masks[i]) if masks is not None else None, logit_bias=bias)
        if each_step is not None:
            each_step(i)
        tok, lp, lg = model.step(dev_ids(prompt) if i == 0 else None, cache, graph=graph)
        out.append((int(tok.item()), f32_bits(lp), to_bits(lg).copy()))
    return out


def unconfigured_launches(model) -> int:
    model.set_step_tail()
    cache = model.make_cache()
    model.step(dev_ids(PROMPT), cache)
    model.step(None, cache)
    return model.graph_launches()


# ------------------------------------------------------------------ 1. every configuration, eager and graph, with and without a sampler
CONFIGS = {"mask": (True, False, False, 1), "bias": (False, False, True, 2), "penalty": (False, True, False, 2), "bias+penalty": (False, True, True, 2),
           "mask+penalty+bias": (True, True, True, 2)}   # mask, penalty, bias -> launches beyond the unconfigured step's


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("name", ["mask", "bias", "mask+penalty+bias"])
def test_step_with_edits_matches_host_loop(tiny, name, sampled, graph):
    from proxy_inference_engine_amd import samplers
    g, cfg, model = tiny
    V = vocab(cfg)
    with_mask, with_pen, with_bias, _ = CONFIGS[name]
    kw = dict(masks=[half_mask(V, 1)] * STEPS if with_mask else None, penalty=PEN if with_pen else None, bias=bias_table(V) if with_bias else None,
              sampler=samplers.make_sampler(temp=0.8, top_k=5) if sampled else None, graph=graph)
    try:
        samplers.seed(21)
        host = host_loop(model, model.make_cache(), PROMPT, STEPS, **kw)
        samplers.seed(21)
        fused = fused_loop(model, model.make_cache(), PROMPT, STEPS, **kw)
        assert model.step_tail == (kw["sampler"].hip_spec if sampled else None, PEN if with_pen else None)
        mask_set, bias_set = model.step_tail_edits
        assert (mask_set is not None) == with_mask and (bias_set is not None) == with_bias
        if with_bias:
            assert bias_set[0].tolist() == list(kw["bias"][0]) and bias_set[1].tolist() == list(kw["bias"][1])
        assert_runs_equal(fused, host, f"{name}, sampled {sampled}, graph {graph}")
        for i, (tok, lp, bits) in enumerate(fused):
            if with_mask:
                assert kw["masks"][i][tok] and (bits[~kw["masks"][i]] == NINF).all() and bits[77] == NINF, i
                assert int(np.isfinite(lp.view(np.float32)).sum()) == int(kw["masks"][i].sum()), i
    finally:
        model.set_step_tail()
    assert model.step_tail == (None, None) and model.step_tail_edits == (None, None)


def test_launch_budget(tiny):
    """mask alone U + 1; bias, penalty or both U + 2 (edit, partials); all three U + 2; a sampler adds what it adds alone; back to U."""
    from proxy_inference_engine_amd import samplers
    g, cfg, model = tiny
    V = vocab(cfg)
    U = unconfigured_launches(model)
    assert U > 0
    sampler = samplers.make_sampler(temp=0.8, top_k=5)
    try:
        fused_loop(model, model.make_cache(), PROMPT, 3, sampler=sampler)
        S = model.graph_launches() - U
        assert S > 0
        for name, (with_mask, with_pen, with_bias, extra) in CONFIGS.items():
            for smp in (None, sampler):
                fused_loop(model, model.make_cache(), PROMPT, 3, masks=[half_mask(V, 1)] * 3 if with_mask else None, penalty=PEN if with_pen else None,
                           bias=bias_table(V) if with_bias else None, sampler=smp)
                assert model.graph_launches() == U + extra + (S if smp is not None else 0), (name, smp is not None)
    finally:
        model.set_step_tail()
    assert model.graph_launches() == -1                      # switching the edits off dropped the captured graphs
    assert unconfigured_launches(model) == U


def test_new_mask_contents_replay_the_captured_graph(tiny):
    """The words behind the mask's address change every step; the step keeps replaying, and the tokens follow the new words."""
    g, cfg, model = tiny
    V = vocab(cfg)
    U = unconfigured_launches(model)
    low = np.arange(V) < V // 2
    masks = [low if i % 2 == 0 else ~low for i in range(STEPS)]
    seen = []
    try:
        host = host_loop(model, model.make_cache(), PROMPT, STEPS, masks=masks)
        fused = fused_loop(model, model.make_cache(), PROMPT, STEPS, masks=masks, each_step=lambda i: seen.append(model.graph_launches()))
        assert_runs_equal(fused, host, "alternating masks")
        assert [(f[0] < V // 2) for f in fused] == [i % 2 == 0 for i in range(STEPS)]
        # step 0 is the prompt pass, step 1 captures; from then on the graph is there BEFORE each step (a dropped one reads -1) and unchanged after
        assert seen[2:] == [U + 1] * (STEPS - 2) and model.graph_launches() == U + 1, seen
    finally:
        model.set_step_tail()


def test_penalty_zero_leaves_a_masked_id_minus_inf(tiny):
    """The documented deviation: a masked id is -inf in the processed logits whatever else is configured; the reference's order would
    give -inf * 0 = NaN for a masked id inside the window of a penalty of 0.0."""
    g, cfg, model = tiny
    V = vocab(cfg)
    m = half_mask(V, 2)
    assert 77 in PROMPT[-5:] and not m[77]
    try:
        for graph in (False, True):
            cache = model.make_cache()
            model.set_step_tail(repetition_penalty=0.0, context_size=5, token_mask=pack(m), logit_bias=((77, 5), (3.0, 1.0)))
            for i in range(3):
                tok, lp, lg = model.step(dev_ids(PROMPT) if i == 0 else None, cache, graph=graph)
                bits = to_bits(lg)
                assert bits[77] == NINF and (bits[~m] == NINF).all(), (graph, i)
                assert m[int(tok.item())], (graph, i)   # (x / 0 = +inf at an allowed id of the window makes the row's logprobs NaN, as without a mask)
    finally:
        model.set_step_tail()


@pytest.mark.parametrize("kind", ["reusable", "pages", "quantized", "rotating"])
def test_edits_on_every_cache_kind(tiny, kind):
    from proxy_inference_engine_amd import samplers
    g, cfg, model = tiny
    V = vocab(cfg)
    kw = dict(masks=[half_mask(V, 3)] * STEPS, penalty=PEN, bias=bias_table(V), sampler=samplers.make_sampler(temp=0.8, top_k=5))
    try:
        samplers.seed(5)
        host = host_loop(model, make_caches(model, kind), PROMPT, STEPS, **kw)
        samplers.seed(5)
        fused = fused_loop(model, make_caches(model, kind), PROMPT, STEPS, **kw)
        assert_runs_equal(fused, host, kind)
    finally:
        model.set_step_tail()


def test_tensor_parallel_refuses_and_call_keeps_raw_logits(tiny):
    from oracle import pie_oracle as po
    from proxy_inference_engine_amd import _ffi
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    from proxy_inference_engine_amd.tp import HipComm
    from tests.test_gpu_tp import CFG
    g, cfg, model = tiny
    V = vocab(cfg)
    lib = _ffi.load()
    w = po.synth_checkpoint(CFG, seed=72, dtype=DT, lm_head_gain=4.0)
    dev_w = {k: (codes_dev(v) if v.dtype == np.uint32 else to_dev(v, DT)) for k, v in w.items()}
    comm = HipComm(CFG["hidden_size"], backend="ipc")
    try:
        tp = Model(ModelArgs(**CFG), dev_w, tp=comm)
        words = torch.full(((CFG["vocab_size"] + 31) // 32,), -1, dtype=torch.int32, device="cuda")
        ids, vals = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, device="cuda")
        assert lib.pie_decoder_set_logits_mask(tp._dec, _ffi.p(words), words.numel()) == -5
        assert b"pie_decoder_set_logits_mask" in lib.pie_last_error()
        assert lib.pie_decoder_set_logit_bias(tp._dec, _ffi.p(ids), _ffi.p(vals), 4) == -5
        assert b"pie_decoder_set_logit_bias" in lib.pie_last_error()
        assert lib.pie_decoder_set_logits_mask(tp._dec, None, 0) == -5 and lib.pie_decoder_set_logit_bias(tp._dec, None, None, 0) == -5
        with pytest.raises(RuntimeError):
            tp.set_step_tail(token_mask=words.cpu())
        with pytest.raises(RuntimeError):
            tp.set_step_tail(logit_bias=((1, 2), (0.5, 0.5)))
        del tp
    finally:
        comm.close()
    # the setters' own argument checks on a decoder that takes them
    words = pack(half_mask(V, 1)).cuda()
    ids, vals = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, device="cuda")
    assert lib.pie_decoder_set_logits_mask(model._dec, _ffi.p(words), words.numel() - 1) == -2
    import ctypes as C
    assert lib.pie_decoder_set_logits_mask(model._dec, C.c_void_p(words.data_ptr() + 2), words.numel()) == -3
    for n in (-1, 1025):
        assert lib.pie_decoder_set_logit_bias(model._dec, _ffi.p(ids), _ffi.p(vals), n) == -1, n
    assert lib.pie_decoder_set_logit_bias(model._dec, None, _ffi.p(vals), 4) == -1 and lib.pie_decoder_set_logit_bias(model._dec, _ffi.p(ids), None, 4) == -1
    with pytest.raises(ValueError):
        model.set_step_tail(token_mask=words[:-1])
    with pytest.raises(ValueError, match="no token"):
        model.set_step_tail(token_mask=torch.zeros(words.numel(), dtype=torch.int32))   # host words that allow nothing: refused, not decoded
    with pytest.raises(ValueError):
        model.set_step_tail(logit_bias=((1, 2), (0.5,)))
    model.set_step_tail()
    assert model.step_tail == (None, None) and model.step_tail_edits == (None, None)
    # Model.__call__ returns raw logits while both are set
    tokens = dev_ids(PROMPT).long()[None]
    raw = to_bits(model(tokens, cache=model.make_cache()))
    one = to_bits(model(tokens[:, :1], cache=model.make_cache()))
    try:
        model.set_step_tail(token_mask=pack(half_mask(V, 1)), logit_bias=bias_table(V))
        got = to_bits(model(tokens, cache=model.make_cache()))
        got_one = to_bits(model(tokens[:, :1], cache=model.make_cache()))   # a single row: the decode step's launches with logits on every position
    finally:
        model.set_step_tail()
    assert np.array_equal(got, raw) and np.array_equal(got_one, one)


# ------------------------------------------------------------------ 2. the engine
SHORT = PROMPT[:5]   # under the many-row prompt pass's threshold: Model.__call__ (the host branch) and Model.step then run the same launches


def test_engine_logit_bias(tiny):
    from proxy_inference_engine_amd import InferenceEngine
    g, cfg, model = tiny
    try:
        def first(**kwargs):
            eng = InferenceEngine(model=model)
            eng.prepare_engine(PROMPT, temp=0, **kwargs)
            gen = eng.generate_step(torch.tensor(PROMPT))
            toks = [int(next(gen)[0].item()) for _ in range(3)]
            return toks, model.step_tail_edits
        greedy, edits = first()
        assert edits == (None, None)
        target = next(t for t in (123, 124, 125) if t not in greedy)
        toks, edits = first(logit_bias={target: 100.0})
        assert toks == [target] * 3 and edits[0] is None and edits[1][0].tolist() == [target]     # the fused branch ran it
        toks, edits = first(logit_bias={greedy[0]: -100.0})
        assert toks[0] != greedy[0] and edits[1][0].tolist() == [greedy[0]]
        # a static bool mask of another vocabulary's length (it packs to as many words) is refused on the fused path too
        eng = InferenceEngine(model=model)
        eng.prepare_engine(PROMPT, temp=0, token_mask=torch.ones(vocab(cfg) - 3, dtype=torch.bool))
        with pytest.raises(ValueError, match="vocabulary"):
            next(eng.generate_step(torch.tensor(PROMPT)))
    finally:
        model.set_step_tail()


def test_engine_callable_mask_equals_host_orchestrated_branch(tiny):
    """A toy grammar -- {a, b} at even history lengths, {c} at odd ones -- through token_mask=fn: the fused branch (one read-back and one
    16 KB upload per token, then a replay) against the same request on the host branch, which a foreign sampler callable forces."""
    from proxy_inference_engine_amd import InferenceEngine
    g, cfg, model = tiny
    a, b, c = 40, 350, 7
    calls = []

    def grammar(tokens):
        calls.append(len(tokens))
        return [a, b] if len(tokens) % 2 == 0 else [c]

    runs = {}
    try:
        for name in ("fused", "host"):
            calls.clear()
            eng = InferenceEngine(model=model)
            eng.prepare_engine(SHORT, temp=0, token_mask=grammar)
            if name == "host":
                inner = eng.samplers["root"]
                eng.samplers["root"] = lambda x: inner(x)    # a foreign callable: no is_greedy, no hip_spec
            gen = eng.generate_step(torch.tensor(SHORT))
            out = []
            for i in range(6):
                tok, lp = next(gen)
                out.append((int(tok.item()), f32_bits(lp)))
                assert (model.step_tail_edits[0] is not None) == (name == "fused"), (name, i)
            assert calls == [len(SHORT) + i for i in range(6)], (name, calls)
            runs[name] = out
    finally:
        model.set_step_tail()
    for i, (tok, lp) in enumerate(runs["fused"]):
        allowed = [a, b] if (len(SHORT) + i) % 2 == 0 else [c]
        assert tok in allowed and int(np.isfinite(lp.view(np.float32)).sum()) == len(allowed), i
        assert tok == runs["host"][i][0] and np.array_equal(lp, runs["host"][i][1]), i
