"""-m gpu: the token automaton inside the decode step's configured tail against the host loop it replaces -- the same step
under token_mask = the packed mask of the automaton's walk over the generated tokens, uploaded again before every step.  Every
comparison is exact on storage bits."""
import numpy as np
import pytest
import torch

from tests import token_automaton_reference as ref
from tests._util import to_bits
from tests.test_gpu_step_edits import PEN, bias_table, pack, unconfigured_launches, vocab
from tests.test_gpu_step_tail import PROMPT, assert_runs_equal, dev_ids, f32_bits, tiny  # noqa: F401  (tiny: the fixture)

pytestmark = pytest.mark.gpu
STEPS = 10
SHORT = PROMPT[:5]   # under the many-row prompt pass's threshold: the prompt's rows run as decode steps


def random_automaton(V: int, S: int, n_cols: int, seed: int, start: int = 0):
    """S states over V ids whose next-state table has n_cols distinct columns: about half of the ids allowed in every state, every state
    reachable, and 301 -- biased and penalised by the edits' fixtures -- allowed everywhere."""
    from proxy_inference_engine_amd.logits_processors import TokenAutomaton
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, S, size=(S, n_cols)).astype(np.int32)
    cols[rng.random((S, n_cols)) < 0.5] = -1
    cols[:, 0] = (np.arange(S) + 1) % S           # column 0 walks through every state: all of them are reachable and allow a token
    pick = rng.integers(0, n_cols, size=V)
    pick[301] = 0
    return TokenAutomaton.from_token_table(cols[:, pick], start)


def tail_kw(sampler, combined, V):
    return dict(sampler=sampler.hip_spec if sampler is not None else None, repetition_penalty=PEN[0] if combined else 1.0,
                context_size=PEN[1] if combined else 60, logit_bias=bias_table(V) if combined else None)


def mask_loop(model, A, prompt, steps, sampler=None, combined=False, graph=True):
    """The host's grammar loop: every step under the mask of the walk so far, uploaded into the step's mask buffer before it."""
    V, cache, gen, out = A.vocab_size, model.make_cache(), [], []
    for i in range(steps):
        model.set_step_tail(token_mask=pack(A.allowed(A.walk(gen))), **tail_kw(sampler, combined, V))
        tok, lp, lg = model.step(dev_ids(prompt) if i == 0 else None, cache, graph=graph)
        gen.append(int(tok.item()))
        out.append((gen[-1], f32_bits(lp), to_bits(lg).copy()))
    return out


def automaton_loop(model, A, prompt, steps, sampler=None, combined=False, graph=True, each_step=None):
    """The device's: the automaton is set once, the state reset once, and every later step passes nothing."""
    V, cache, out = A.vocab_size, model.make_cache(), []
    model.set_step_tail(token_automaton=A, **tail_kw(sampler, combined, V))
    model.reset_step_automaton()
    for i in range(steps):
        if each_step is not None:
            each_step(i)
        tok, lp, lg = model.step(dev_ids(prompt) if i == 0 else None, cache, graph=graph)
        out.append((int(tok.item()), f32_bits(lp), to_bits(lg).copy()))
    return out


def device_state(model) -> int:
    return int(model.step_tail_automaton[1].item())


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("combined", [False, True])
def test_step_under_an_automaton_matches_the_host_mask_loop(tiny, combined, sampled, graph):
    from proxy_inference_engine_amd import samplers
    g, cfg, model = tiny
    V = vocab(cfg)
    A = random_automaton(V, 6, 9, seed=11)
    sampler = samplers.make_sampler(temp=0.9, top_p=0.9) if sampled else None
    try:
        samplers.seed(33)
        host = mask_loop(model, A, PROMPT, STEPS, sampler, combined, graph)
        assert model.step_tail_automaton[0] is None
        samplers.seed(33)
        dev = automaton_loop(model, A, PROMPT, STEPS, sampler, combined, graph)
        assert_runs_equal(dev, host, f"combined {combined}, sampled {sampled}, graph {graph}")
        toks = [d[0] for d in dev]
        assert model.step_tail_automaton[0] is A and model.step_tail_edits[0] is None
        assert device_state(model) == A.walk(toks) >= 0
        # the part's mask buffer: the packed mask of the state the last step started in
        assert np.array_equal(model._dfa_mask.cpu().numpy().view(np.uint32), ref.pack(A.allowed(A.walk(toks[:-1]))))
        s = A.start
        for i, (tok, lp, bits) in enumerate(dev):   # every token was allowed where it was drawn, and only allowed ids stayed finite
            ok = A.allowed(s)
            assert ok[tok] and int(np.isfinite(lp.view(np.float32)).sum()) == int(ok.sum()), i
            s = A.step(s, tok)
    finally:
        model.set_step_tail()
    assert model.step_tail_automaton[0] is None and model.step_tail == (None, None)


def test_short_prompt_and_reset(tiny):
    """A prompt under the many-row threshold runs as decode steps: only its last row meets the tail, so the state moves once.  A reset to
    another state in stream order is what the next step masks with."""
    g, cfg, model = tiny
    A = random_automaton(vocab(cfg), 6, 9, seed=12, start=2)
    try:
        host = mask_loop(model, A, SHORT, 4)
        dev = automaton_loop(model, A, SHORT, 4)
        assert_runs_equal(dev, host, "short prompt")
        assert device_state(model) == A.walk([d[0] for d in dev])
        model.reset_step_automaton(4)
        assert device_state(model) == 4
        cache = model.make_cache()
        tok = int(model.step(dev_ids(PROMPT), cache)[0].item())
        assert A.allowed(4)[tok] and device_state(model) == A.step(4, tok)
        model.reset_step_automaton()
        assert device_state(model) == 2
        # a state outside the automaton -- it has been left -- constrains nothing and stays: the step equals the one under an all-ones mask
        model.reset_step_automaton(-1)
        tok, lp, lg = model.step(dev_ids(PROMPT), model.make_cache())
        left = (int(tok.item()), f32_bits(lp), to_bits(lg).copy())
        assert device_state(model) == -1
        model.set_step_tail(token_mask=pack(np.ones(A.vocab_size, dtype=bool)))
        tok, lp, lg = model.step(dev_ids(PROMPT), model.make_cache())
        assert_runs_equal([left], [(int(tok.item()), f32_bits(lp), to_bits(lg).copy())], "a left automaton")
        model.set_step_tail()
        with pytest.raises(RuntimeError):
            model.reset_step_automaton()
    finally:
        model.set_step_tail()


def test_launch_budget(tiny, golden_dir):
    """Automaton alone U + 3 (the mask's U + 1, plus the mask op and the advance); with a bias and / or a penalty U + 4; unconfigured U --
    what a decoder whose setter was never called reports."""
    from tests.test_gpu_batch_edits import make_model
    g, cfg, model = tiny
    V = vocab(cfg)
    fresh = make_model(golden_dir)[2]             # no setter of any tail part was ever called on this one
    cache = fresh.make_cache()
    fresh.step(dev_ids(PROMPT), cache), fresh.step(None, cache)
    U = unconfigured_launches(model)
    assert U > 0 and fresh.graph_launches() == U
    del fresh, cache
    A = random_automaton(V, 6, 9, seed=13)
    try:
        mask_loop(model, A, PROMPT, 3)
        assert model.graph_launches() == U + 1
        automaton_loop(model, A, PROMPT, 3)
        assert model.graph_launches() == U + 3
        automaton_loop(model, A, PROMPT, 3, combined=True)
        assert model.graph_launches() == U + 4
        model.set_step_tail(token_automaton=A, logit_bias=bias_table(V))
        cache = model.make_cache()
        model.step(dev_ids(PROMPT), cache), model.step(None, cache)
        assert model.graph_launches() == U + 4
    finally:
        model.set_step_tail()
    assert model.graph_launches() == -1                      # switching the part off dropped the captured graphs
    assert unconfigured_launches(model) == U


def test_new_automaton_and_reset_replay_the_captured_graph(tiny):
    """Another automaton that fits the arena, and a reset of the state, are copies in stream order: the captured graph keeps replaying."""
    g, cfg, model = tiny
    V = vocab(cfg)
    U = unconfigured_launches(model)
    A, B = random_automaton(V, 6, 9, seed=14), random_automaton(V, 4, 5, seed=15, start=1)
    assert B.words().size <= A.words().size and (B.n_states, B.n_classes) != (A.n_states, A.n_classes)
    seen = []
    try:
        automaton_loop(model, A, PROMPT, 4, each_step=lambda i: seen.append(model.graph_launches()))
        assert seen[2:] == [U + 3] * 2 and model.graph_launches() == U + 3, seen
        arena = model._dfa_arena.data_ptr()
        seen.clear()
        host = mask_loop(model, B, PROMPT, 4)          # (the mask part goes on and the automaton off: that does drop the graphs)
        dev = automaton_loop(model, B, PROMPT, 4, each_step=lambda i: seen.append(model.graph_launches()))
        assert_runs_equal(dev, host, "the second automaton")
        assert model._dfa_arena.data_ptr() == arena
        # while the part stays on: B -> A -> a reset, no new capture
        cache = model.make_cache()
        model.step(dev_ids(PROMPT), cache), model.step(None, cache)
        assert model.graph_launches() == U + 3
        model.set_step_tail(token_automaton=A)
        assert model.graph_launches() == U + 3 and device_state(model) == A.start and model._dfa_arena.data_ptr() == arena
        tok = int(model.step(None, cache)[0].item())
        assert A.allowed(A.start)[tok] and device_state(model) == A.step(A.start, tok)
        model.reset_step_automaton(3)
        tok = int(model.step(None, cache)[0].item())
        assert A.allowed(3)[tok] and device_state(model) == A.step(3, tok) and model.graph_launches() == U + 3
        model.set_step_tail(token_automaton=A)              # the same object again: nothing changes, the state included
        assert device_state(model) == A.step(3, tok)
        # a larger automaton: the arena grows, which is a new capture
        C = random_automaton(V, 12, 20, seed=16)
        model.set_step_tail(token_automaton=C)
        assert model.graph_launches() == -1 and model._dfa_arena.numel() == C.words().size
    finally:
        model.set_step_tail()


def test_refusals(tiny):
    from proxy_inference_engine_amd import _ffi, hip_ops
    from proxy_inference_engine_amd.logits_processors import TokenAutomaton
    g, cfg, model = tiny
    V = vocab(cfg)
    A = random_automaton(V, 6, 9, seed=17)
    lib = _ffi.load()
    n = (V + 31) // 32
    words = pack(np.ones(V, dtype=bool)).cuda()
    rec, st = hip_ops.token_dfa_records([(0, V, A.n_states, A.n_classes)], "cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    arena, mask = torch.from_numpy(A.words()).cuda(), torch.zeros(n, dtype=torch.int32, device="cuda")
    dfa = (_ffi.p(rec), _ffi.p(st), _ffi.p(arena), arena.numel(), _ffi.p(mask), n)
    try:
        with pytest.raises(ValueError, match="exclusive"):
            model.set_step_tail(token_mask=words, token_automaton=A)
        assert model.step_tail_edits == (None, None) and model.step_tail_automaton[0] is None
        # mask, then automaton -- and the other way round: whichever comes second is refused, naming the other
        assert lib.pie_decoder_set_logits_mask(model._dec, _ffi.p(words), n) == 0
        assert lib.pie_decoder_set_token_dfa(model._dec, *dfa) == -5 and b"a token mask is set" in lib.pie_last_error()
        assert lib.pie_decoder_set_logits_mask(model._dec, None, 0) == 0
        assert lib.pie_decoder_set_token_dfa(model._dec, *dfa) == 0
        assert lib.pie_decoder_set_logits_mask(model._dec, _ffi.p(words), n) == -5 and b"a token automaton is set" in lib.pie_last_error()
        # the setter's own argument checks
        assert lib.pie_decoder_set_token_dfa(model._dec, _ffi.p(rec), None, _ffi.p(arena), arena.numel(), _ffi.p(mask), n) == -1
        assert lib.pie_decoder_set_token_dfa(model._dec, _ffi.p(rec), _ffi.p(st), _ffi.p(arena), arena.numel(), None, n) == -1
        assert lib.pie_decoder_set_token_dfa(model._dec, _ffi.p(rec), _ffi.p(st), _ffi.p(arena), arena.numel(), _ffi.p(mask), n - 1) == -2
        assert lib.pie_decoder_set_token_dfa(model._dec, _ffi.p(rec), _ffi.p(st), _ffi.p(arena), 0, _ffi.p(mask), n) == -2
        import ctypes as C
        assert lib.pie_decoder_set_token_dfa(model._dec, _ffi.p(rec), C.c_void_p(st.data_ptr() + 2), _ffi.p(arena), arena.numel(), _ffi.p(mask), n) == -3
        assert lib.pie_decoder_set_token_dfa(model._dec, None, None, None, 0, None, 0) == 0
        # another vocabulary, another type
        with pytest.raises(ValueError, match="vocabulary"):
            model.set_step_tail(token_automaton=random_automaton(V - 1, 3, 4, seed=1))
        with pytest.raises(ValueError, match="TokenAutomaton"):
            model.set_step_tail(token_automaton=lambda t: [1])
        # speculation refuses a set automaton by name
        model.set_step_tail(token_automaton=A, repetition_penalty=1.5, context_size=8)
        with pytest.raises(ValueError, match="a token automaton"):
            model.spec_step_tail(torch.tensor([1, 2, 3, 4, 5, 6], dtype=torch.int32, device="cuda"), model.make_cache())
    finally:
        lib.pie_decoder_set_token_dfa(model._dec, None, None, None, 0, None, 0)
        lib.pie_decoder_set_logits_mask(model._dec, None, 0)
        model._dfa = None
        model.set_step_tail()
    assert isinstance(A, TokenAutomaton)
    # a tensor-parallel decoder's tail is vocabulary-parallel: both setters are refused
    from oracle import pie_oracle as po
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    from proxy_inference_engine_amd.tp import HipComm
    from tests._util import codes_dev, to_dev
    from tests.test_gpu_tp import CFG
    w = po.synth_checkpoint(CFG, seed=72, dtype="bfloat16", lm_head_gain=4.0)
    dev_w = {k: (codes_dev(v) if v.dtype == np.uint32 else to_dev(v, "bfloat16")) for k, v in w.items()}
    comm = HipComm(CFG["hidden_size"], backend="ipc")
    try:
        tp = Model(ModelArgs(**CFG), dev_w, tp=comm)
        assert lib.pie_decoder_set_token_dfa(tp._dec, *dfa) == -5 and b"pie_decoder_set_token_dfa" in lib.pie_last_error()
        assert lib.pie_decoder_set_token_dfa(tp._dec, None, None, None, 0, None, 0) == -5
        assert lib.pie_decoder_set_batch_token_dfa(tp._dec, 1, _ffi.p(rec), _ffi.p(st), _ffi.p(arena), arena.numel()) == -5
        with pytest.raises(RuntimeError):
            tp.set_step_tail(token_automaton=random_automaton(CFG["vocab_size"], 3, 4, seed=2))
        del tp
    finally:
        comm.close()


def test_call_keeps_raw_logits_and_the_state(tiny):
    """Model.__call__ asks for logits on every position: nothing of the part runs and the state does not move."""
    g, cfg, model = tiny
    A = random_automaton(vocab(cfg), 6, 9, seed=18, start=3)
    tokens = dev_ids(PROMPT).long()[None]
    raw = to_bits(model(tokens, cache=model.make_cache()))
    one = to_bits(model(tokens[:, :1], cache=model.make_cache()))
    try:
        model.set_step_tail(token_automaton=A)
        got = to_bits(model(tokens, cache=model.make_cache()))
        got_one = to_bits(model(tokens[:, :1], cache=model.make_cache()))
        assert device_state(model) == 3
    finally:
        model.set_step_tail()
    assert np.array_equal(got, raw) and np.array_equal(got_one, one)


def test_engine_automaton_equals_the_callable_host_mask(tiny):
    """InferenceEngine.generate under prepare_engine(token_automaton=A) against the same request under token_mask=fn, fn being the host's
    walk.  The automaton's request hands the engine no callable at all: there is nothing it could call per token."""
    from proxy_inference_engine_amd import InferenceEngine, samplers
    from proxy_inference_engine_amd.engine.inference_engine import SpeculativeParams
    g, cfg, model = tiny
    V = vocab(cfg)
    A = random_automaton(V, 6, 9, seed=19)
    calls = []

    def fn(tokens):
        calls.append(len(tokens))
        return torch.from_numpy(A.allowed(A.walk(list(tokens)[len(PROMPT):])))

    runs = {}
    try:
        for name, kw in (("automaton", dict(token_automaton=A)), ("callable", dict(token_mask=fn))):
            for temp in (0.0, 0.8):
                samplers.seed(44)
                eng = InferenceEngine(model=model)
                eng.prepare_engine(PROMPT, temp=temp, top_p=0.9, repetition_penalty=1.5, context_size=8, **kw)
                assert all(not callable(getattr(p, "mask_fn", None)) for p in eng.logits_processors["root"]) == (name == "automaton")
                runs[name, temp] = list(eng.generate(torch.tensor(PROMPT), max_completion_tokens=8, logprobs=True, top_logprobs=3))
                assert (model.step_tail_automaton[0] is A) == (name == "automaton") and (model.step_tail_edits[0] is not None) == (name == "callable")
                if name == "automaton":
                    assert device_state(model) == A.walk([t for t, _ in runs[name, temp]])
        assert calls == [len(PROMPT) + i for i in range(8)] * 2
        for temp in (0.0, 0.8):
            assert len(runs["automaton", temp]) == 8 and runs["automaton", temp] == runs["callable", temp], temp
        # the host-orchestrated branch (a foreign sampler callable forces it) runs the processor's torch body: the same tokens
        eng = InferenceEngine(model=model)
        eng.prepare_engine(SHORT, temp=0, token_automaton=A)
        fused = [t for t, _ in eng.generate(torch.tensor(SHORT), max_completion_tokens=6)]
        eng = InferenceEngine(model=model)
        eng.prepare_engine(SHORT, temp=0, token_automaton=A)
        inner = eng.samplers["root"]
        eng.samplers["root"] = lambda x: inner(x)
        hosted = [t for t, _ in eng.generate(torch.tensor(SHORT), max_completion_tokens=6)]
        assert model.step_tail_automaton[0] is None and hosted == fused and A.walk(fused) >= 0
        # speculation refuses the request by name
        for sp in (SpeculativeParams(), SpeculativeParams(configured_tail=True)):
            eng = InferenceEngine(model=model)
            eng.prepare_engine(PROMPT, temp=0, token_automaton=A)
            with pytest.raises(ValueError, match="a token automaton"):
                next(eng.generate_step(torch.tensor(PROMPT), speculative=sp))
    finally:
        model.set_step_tail()
