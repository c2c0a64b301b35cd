"""-m gpu: the decode step's configurable tail -- the repetition penalty and the stochastic samplers inside the replayed
step -- against the host-orchestrated forms they replace.  Every comparison is exact: the penalty is one fp32 multiplication or division
and one rounding (numpy computes the same bits), the log-softmax keeps pie_logprobs_argmax's partition and order, and the fused draw issues
the same pie_sample call on the same random stream as the sampler closures.  The one equivalence class: where the expected value is a NaN
(0 / 0 under penalty 0.0) the result must be a NaN; IEEE 754 leaves a NaN's sign and payload open and the host's differ from the GPU's."""
import json

import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests._util import codes_dev, to_bits, to_dev

pytestmark = pytest.mark.gpu
DT = "bfloat16"
# 24 ids; 301 three times and 77 twice inside the last five, 17 / 450 repeated further back (inside a window of 60)
PROMPT = [17, 450, 33, 17, 208, 96, 450, 5, 311, 64, 129, 17, 402, 250, 9, 450, 188, 73, 260, 301, 77, 301, 77, 301]


def penalise(bits: np.ndarray, window, penalty: float, dt: str) -> np.ndarray:
    """logits_processors/repetition.py:11-22 on storage bits: every distinct in-range id of `window` once, fp32 arithmetic, one rounding."""
    ids = np.unique([i for i in window if 0 <= i < bits.size]).astype(np.int64)
    out = bits.copy()
    if ids.size:
        s = po.from_bits(bits[ids], dt)
        with np.errstate(all="ignore"):
            out[ids] = po.to_bits(np.where(s < 0, s * np.float32(penalty), s / np.float32(penalty)).astype(np.float32), dt)
    return out


def assert_same_bits(got: np.ndarray, want: np.ndarray, dt: str, what):
    nan = np.isnan(po.from_bits(want, dt))
    assert np.array_equal(got[~nan], want[~nan]), (what, np.flatnonzero((got != want) & ~nan)[:8])
    assert np.isnan(po.from_bits(got, dt)[nan]).all(), what


def specials(dt: str) -> np.ndarray:
    """+-0.0, -inf, the smallest denormal and normal magnitudes, the largest finite ones (f16: +-65504, which a penalty overflows)."""
    if dt == "float16":
        return np.array([0x0000, 0x8000, 0xFC00, 0x0001, 0x8001, 0x0400, 0x8400, 0x7BFF, 0xFBFF], np.uint16)
    return np.array([0x0000, 0x8000, 0xFF80, 0x0001, 0x8001, 0x0080, 0x8080, 0x7F7F, 0xFF7F], np.uint16)


# ------------------------------------------------------------------ 1. the op
@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("V", [7, 4099, 128256])
def test_logits_penalty_op_bit_for_bit(dt, V):
    from proxy_inference_engine_amd import hip_ops
    rng = np.random.default_rng(V + len(dt))
    base = po.to_bits((rng.standard_normal(V) * 6).astype(np.float32), dt)
    sp = specials(dt)
    if V > 27:
        where = np.arange(len(sp)) * 3
        base[where], base[V - 1] = sp, sp[-1]                 # (the largest negative magnitude also at the last id)
    else:
        where = np.arange(7)
        base[where] = sp[[0, 1, 2, 3, 6, 7, 8]]
    hot = np.unique(np.concatenate([where, [0, V - 1]]))      # ids the windows favour: every special value gets penalised
    ids_dev = torch.empty(1024, dtype=torch.int32, device="cuda")
    checked = 0
    for n in (1, 60, 1024):
        for pi, penalty in enumerate((1.3, 1.8, 0.5, 0.0)):
            some = rng.integers(0, V, n)
            some[: min(n, len(hot))] = rng.permutation(hot)[: min(n, len(hot))]
            windows = {
                "all equal": np.full(n, hot[(pi + n) % len(hot)]),
                "pairs of duplicates": np.repeat(rng.permutation(some)[: (n + 1) // 2], 2)[:n],
                "ids 0 and V - 1": np.concatenate([[0, V - 1], some])[:n] if n > 1 else np.array([(0, V - 1)[pi % 2]]),
                "out of range": np.resize(np.array([-1, V]), n),
            }
            for name, win in windows.items():
                assert win.size == n
                logits = to_dev(base, dt)
                ids_dev[:n].copy_(torch.from_numpy(win.astype(np.int32)))
                out = hip_ops.logits_penalty(logits, ids_dev[:n], penalty)
                assert out.data_ptr() == logits.data_ptr()
                got, want = to_bits(logits), penalise(base, win.tolist(), penalty, dt)
                assert_same_bits(got, want, dt, (name, n, penalty))
                untouched = np.ones(V, bool)
                untouched[[i for i in win.tolist() if 0 <= i < V]] = False
                assert np.array_equal(got[untouched], base[untouched]), (name, n, penalty)     # NaN-free: raw bits
                if name == "out of range":
                    assert np.array_equal(got, base), (n, penalty)
                checked += 1
    assert checked == 48
    if dt == "float16":   # +-65504 overflow to +-inf under a penalty that grows them
        for value, penalty, want in ((0x7BFF, 0.5, 0x7C00), (0xFBFF, 1.8, 0xFC00)):
            idx = int(np.flatnonzero(base == value)[0])
            logits = to_dev(base, dt)
            hip_ops.logits_penalty(logits, torch.tensor([idx], dtype=torch.int32, device="cuda"), penalty)
            assert to_bits(logits)[idx] == want == penalise(base, [idx], penalty, dt)[idx]
    with pytest.raises(ValueError):
        hip_ops.logits_penalty(to_dev(base, dt), ids_dev[:4], -1.0)
    with pytest.raises(ValueError):
        hip_ops.logits_penalty(to_dev(base, dt), ids_dev[:0], 1.3)


# ------------------------------------------------------------------ the tiny golden model
@pytest.fixture(scope="module")
def tiny(golden_dir):
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    g = np.load(golden_dir / "tiny_llama_w4_bf16.npz")
    cfg = json.loads(str(g["config_json"]))
    w = {k[2:]: (codes_dev(g[k]) if g[k].dtype == np.uint32 else to_dev(g[k], DT)) for k in g.files if k.startswith("w:")}
    return g, cfg, Model(ModelArgs(**cfg), w)


def dev_ids(ids) -> torch.Tensor:
    return torch.tensor(list(ids), dtype=torch.int32, device="cuda")


def f32_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy().view(np.uint32).copy()


def host_loop(model, cache, prompt, steps, penalty=None, sampler=None, graph=True):
    """Today's orchestration on the unconfigured tail: model.step(explicit ids), the penalty on the host over a Python list of the fed
    ids, hip_ops.logprobs_argmax of the penalised logits, then the sampler closure.  Per step: (token, logprobs bits, logits bits, raw bits)."""
    from proxy_inference_engine_amd import hip_ops
    model.set_step_tail()
    fed, out, ids = [], [], dev_ids(prompt)
    for _ in range(steps):
        tok, lp, lg = model.step(ids, cache, graph=graph)
        fed += ids.tolist()
        raw = to_bits(lg)
        bits = raw
        if penalty is not None:
            bits = penalise(raw, fed[-penalty[1]:], penalty[0], DT)
            tok, lp = hip_ops.logprobs_argmax(to_dev(bits, DT))
        if sampler is not None:
            tok = sampler(lp[None]).reshape(1).to(torch.int32)
        out.append((int(tok.item()), f32_bits(lp), bits, raw))
        ids = tok.reshape(1).to(torch.int32).clone()
    return out


def fused_loop(model, cache, prompt, steps, penalty=None, sampler=None, graph=True):
    model.set_step_tail(sampler=sampler.hip_spec if sampler is not None else None,
                        repetition_penalty=penalty[0] if penalty else 1.0, context_size=penalty[1] if penalty else 60)
    out = []
    for i in range(steps):
        tok, lp, lg = model.step(dev_ids(prompt) if i == 0 else None, cache, graph=graph)
        out.append((int(tok.item()), f32_bits(lp), to_bits(lg)))
    return out


def assert_runs_equal(fused, host, what):
    assert [f[0] for f in fused] == [h[0] for h in host], what
    for i, (f, h) in enumerate(zip(fused, host)):
        assert np.array_equal(f[1], h[1]), f"{what}: logprobs, step {i}"
        assert np.array_equal(f[2], h[2]), f"{what}: logits, step {i}"


# ------------------------------------------------------------------ 2. penalty inside the step
@pytest.mark.parametrize("context_size,graph", [(5, True), (60, True), (5, False)])
def test_step_with_penalty_matches_host_penalised_loop(tiny, context_size, graph):
    from proxy_inference_engine_amd import hip_ops
    g, cfg, model = tiny
    steps, pen = 24, (1.8, context_size)
    try:
        # (a) one step: the output logits are the numpy formula over the unconfigured step's logits and prompt[-c:]
        model.set_step_tail()
        L0 = to_bits(model.step(dev_ids(PROMPT), model.make_cache(), graph=graph)[2])
        model.set_step_tail(repetition_penalty=pen[0], context_size=context_size)
        assert model.step_tail == (None, pen)
        tok, lp, lg = model.step(dev_ids(PROMPT), model.make_cache(), graph=graph)
        assert np.array_equal(to_bits(lg), penalise(L0, PROMPT[-context_size:], pen[0], DT))
        assert len(set(PROMPT[-context_size:])) < len(PROMPT[-context_size:])           # repeated ids inside the window
        # (b) the tail's token and logprobs are pie_logprobs_argmax of the logits it leaves
        rtok, rlp = hip_ops.logprobs_argmax(lg.clone())
        assert int(tok.item()) == int(rtok.item()) and np.array_equal(f32_bits(lp), f32_bits(rlp))
        # (c) / (d) 24 steps: the window slides off the prompt (c = 5) or is clipped at position 0 (c = 60)
        host = host_loop(model, model.make_cache(), PROMPT, steps, penalty=pen, graph=graph)
        fused = fused_loop(model, model.make_cache(), PROMPT, steps, penalty=pen, graph=graph)
        assert_runs_equal(fused, host, f"penalty, context {context_size}, graph {graph}")
        for i, h in enumerate(host):
            assert not np.array_equal(h[2], h[3]), f"step {i}: the penalty changed nothing"
        # fed-back ids were recorded on the device: fed_ids holds the prompt, then every chosen token but the last
        want_fed = PROMPT + [f[0] for f in fused[:-1]]
        assert model.fed_ids[:len(want_fed)].tolist() == want_fed
    finally:
        model.set_step_tail()
    assert model.step_tail == (None, None)


# ------------------------------------------------------------------ 3. sampler inside the step
SAMPLERS = {"categorical": dict(temp=1.0), "top_k": dict(temp=0.8, top_k=5), "top_p": dict(temp=0.9, top_p=0.9),
            "min_p": dict(temp=1.0, min_p=0.1, min_tokens_to_keep=2)}


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_step_with_sampler_matches_host_sampled_loop(tiny, name):
    from proxy_inference_engine_amd import samplers
    g, cfg, model = tiny
    prompt, steps = g["prompt"].tolist(), 16
    sampler = samplers.make_sampler(**SAMPLERS[name])
    try:
        samplers.seed(12)
        host = host_loop(model, model.make_cache(), prompt, steps, sampler=sampler)
        greedy_launches = model.graph_launches()                     # the host loop replays the unconfigured graph
        assert greedy_launches > 0
        samplers.seed(12)
        fused = fused_loop(model, model.make_cache(), prompt, steps, sampler=sampler)
        assert_runs_equal(fused, host, name)
        assert model.graph_launches() > greedy_launches
    finally:
        model.set_step_tail()
    cache = model.make_cache()
    toks = [int(model.step(dev_ids(prompt), cache)[0].item())] + [int(model.step(None, cache)[0].item()) for _ in range(len(g["tokens"]) - 1)]
    assert model.graph_launches() == greedy_launches
    assert toks == g["tokens"].tolist()


# ------------------------------------------------------------------ 4. every cache kind
def make_caches(model, kind):
    from proxy_inference_engine_amd.cache import QuantizedKVCache, RotatingKVCache
    if kind == "reusable":
        return model.make_cache()
    if kind == "pages":
        return model.make_paged_cache(num_pages=8, max_blocks=4)
    if kind == "quantized":
        return [QuantizedKVCache(group_size=64, bits=8) for _ in model.layers]
    return [RotatingKVCache(16, keep=4) for _ in model.layers]


@pytest.mark.parametrize("kind", ["reusable", "pages", "quantized", "rotating"])
def test_penalty_and_sampler_on_every_cache_kind(tiny, kind):
    from proxy_inference_engine_amd import samplers
    g, cfg, model = tiny
    sampler, pen, steps = samplers.make_sampler(temp=0.8, top_k=5), (1.8, 5), 16
    try:
        samplers.seed(5)
        host = host_loop(model, make_caches(model, kind), PROMPT, steps, penalty=pen, sampler=sampler)
        samplers.seed(5)
        fused = fused_loop(model, make_caches(model, kind), PROMPT, steps, penalty=pen, sampler=sampler)
        assert_runs_equal(fused, host, kind)
    finally:
        model.set_step_tail()


# ------------------------------------------------------------------ 5. the engine
class IdentityStructuringEngine:
    """Forces the engine onto its host-orchestrated branch without changing any value."""
    has_reached_accept_state = False

    def get_current_state(self):
        return None

    def process_logits(self, tokens, logits):
        return logits

    def sample(self, logprobs, sampler):
        return sampler(logprobs)


def test_engine_fused_tail_equals_host_orchestrated_branch(tiny):
    from proxy_inference_engine_amd import InferenceEngine, samplers
    g, cfg, model = tiny
    kwargs = dict(temp=0.8, top_k=5, repetition_penalty=2.0, context_size=20)   # 2.0: torch's x / 2.0 = x * 0.5 is exact, as IEEE division is
    runs = {}
    try:
        for name, se in (("fused", None), ("host", IdentityStructuringEngine())):
            samplers.seed(3)
            eng = InferenceEngine(model=model, structuring_engine=se)
            eng.prepare_engine(PROMPT, **kwargs)
            gen = eng.generate_step(torch.tensor(PROMPT))
            toks = []
            for i in range(12):
                toks.append(int(next(gen)[0].item()))
                if name == "fused":
                    assert model.step_tail == (("top_k", 0.8, 0.0, 5), (2.0, 20)), i
                else:
                    assert model.step_tail == (None, None), i
            runs[name] = toks
    finally:
        model.set_step_tail()
    assert runs["fused"] == runs["host"]


# ------------------------------------------------------------------ 6. refusals and the raw __call__
def test_tensor_parallel_refuses_and_call_keeps_raw_logits(tiny):
    import ctypes as C
    from proxy_inference_engine_amd import _ffi, hip_ops
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    from proxy_inference_engine_amd.tp import HipComm
    from tests.test_gpu_tp import CFG
    g, cfg, model = tiny
    lib = _ffi.load()
    w = po.synth_checkpoint(CFG, seed=72, dtype=DT, lm_head_gain=4.0)
    dev_w = {k: (codes_dev(v) if v.dtype == np.uint32 else to_dev(v, DT)) for k, v in w.items()}
    comm = HipComm(CFG["hidden_size"], backend="ipc")
    try:
        tp = Model(ModelArgs(**CFG), dev_w, tp=comm)
        ws = hip_ops.sample_workspace(tp.device, 1, CFG["vocab_size"])
        counter = torch.zeros(2, dtype=torch.int64, device="cuda")
        assert lib.pie_decoder_set_logits_penalty(tp._dec, 1.8, 5, _ffi.p(tp.fed_ids), tp.fed_ids.numel()) == -5
        assert b"pie_decoder_set_logits_penalty" in lib.pie_last_error()
        assert lib.pie_decoder_set_sampler(tp._dec, 1, 0.8, 0.0, 5, 1, _ffi.p(counter), _ffi.p(ws), ws.numel() * 8) == -5
        assert b"pie_decoder_set_sampler" in lib.pie_last_error()
        assert lib.pie_decoder_set_sampler(tp._dec, _ffi.PIE_SAMPLE_GREEDY, 1.0, 0.0, 0, 0, None, None, 0) == -5
        with pytest.raises(RuntimeError):
            tp.set_step_tail(repetition_penalty=1.8, context_size=5)
        tp.set_step_tail()   # the defaults are what it already has: nothing is asked of the library
        del tp
    finally:
        comm.close()
    # the setters' own argument checks on a decoder that takes them
    ws = hip_ops.sample_workspace(model.device, 1, cfg["vocab_size"])
    counter = torch.zeros(2, dtype=torch.int64, device="cuda")
    for args, code in (((-0.5, 5, _ffi.p(model.fed_ids), 64), -1), ((float("inf"), 5, _ffi.p(model.fed_ids), 64), -1), ((1.8, 1025, _ffi.p(model.fed_ids), 64), -1),
                       ((1.8, -1, _ffi.p(model.fed_ids), 64), -1), ((1.8, 5, None, 64), -1), ((1.8, 5, _ffi.p(model.fed_ids), 0), -1)):
        assert lib.pie_decoder_set_logits_penalty(model._dec, *args) == code, args
    for args, code in (((1, 0.8, 0.0, 512), -1), ((1, 0.0, 0.0, 5), -1), ((7, 1.0, 0.0, 0), -1), ((2, 1.0, 1.0, 0), -1), ((3, 1.0, 0.0, 1), -1)):
        assert lib.pie_decoder_set_sampler(model._dec, *args, 1, _ffi.p(counter), _ffi.p(ws), ws.numel() * 8) == code, args
    assert lib.pie_decoder_set_sampler(model._dec, 1, 0.8, 0.0, 5, 1, _ffi.p(counter), _ffi.p(ws), 64) == -2
    assert model.step_tail == (None, None)
    # Model.__call__ returns raw logits whatever tail is configured
    ids = dev_ids(PROMPT).long()[None]
    raw = to_bits(model(ids, cache=model.make_cache()))
    try:
        model.set_step_tail(sampler=("top_k", 0.8, 0.0, 5), repetition_penalty=1.8, context_size=5)
        got = to_bits(model(ids, cache=model.make_cache()))
        one = to_bits(model(ids[:, :1], cache=model.make_cache()))   # a single row: the decode step's launches with logits on every position
    finally:
        model.set_step_tail()
    assert np.array_equal(got, raw)
    assert np.array_equal(one, to_bits(model(ids[:, :1], cache=model.make_cache())))


# ------------------------------------------------------------------ 7. the ids_cap boundary of the step's window
def test_step_window_stops_at_ids_cap(tiny):
    """The step form checks every index into ids_by_pos against ids_cap.  The penalty is configured through the library with a cap of 6,
    far below the buffer's size; everything from index 6 on holds a sentinel id.  A 4-token prompt and seven un-graphed steps take pos
    from 3 to 10: the window (5 positions) first lies below the cap, then straddles it, then (the last step) lies wholly beyond it.
    Positions at or beyond the cap are neither read nor recorded."""
    from proxy_inference_engine_amd import _ffi, hip_ops
    g, cfg, model = tiny
    lib = _ffi.load()
    prompt, pen, ctx, cap, sentinel, steps = [17, 450, 33, 17], 1.8, 5, 6, 7, 7
    try:
        model.set_step_tail()
        model.fed_ids.zero_()
        model.fed_ids[cap:] = sentinel
        _ffi.check(lib.pie_decoder_set_logits_penalty(model._dec, pen, ctx, _ffi.p(model.fed_ids), cap))
        cache, got, fed = model.make_cache(), [], list(prompt)
        for i in range(1 + steps):
            tok, lp, lg = model.step(dev_ids(prompt) if i == 0 else None, cache, graph=False)
            got.append(to_bits(lg))
            seen = min(cap, len(fed))
            assert model.fed_ids[:seen].tolist() == fed[:seen], i                      # fed ids below the cap: recorded
            assert bool((model.fed_ids[cap:] == sentinel).all()), i                    # at or beyond it: nothing was written
            fed.append(int(tok.item()))
        assert sentinel not in fed
    finally:
        _ffi.check(lib.pie_decoder_set_logits_penalty(model._dec, 1.0, 0, None, 0))
        model.set_step_tail()
    # the raw logits of the same run: the unconfigured step over the same ids, fed explicitly
    cache = model.make_cache()
    for i in range(1 + steps):
        raw = model.step(dev_ids(prompt if i == 0 else fed[len(prompt) + i - 1:len(prompt) + i]), cache, graph=False)[2].clone()
        pos = len(prompt) + i - 1
        window = [fed[p] for p in range(max(0, pos + 1 - ctx), pos + 1) if p < cap]
        assert (len(window) == 0) == (i == steps) and (len(window) == ctx) == (i in (1, 2))
        want = hip_ops.logits_penalty(raw.clone(), dev_ids(window), pen) if window else raw
        assert np.array_equal(got[i], to_bits(want)), f"step {i}: window {window}"
        if window:
            assert not np.array_equal(got[i], to_bits(raw)), f"step {i}: the penalty changed nothing"
