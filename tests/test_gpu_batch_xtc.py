"""-m gpu: per-row XTC in the multi-sequence passes against host orchestration per row: the unarmed pass, then a one-row
pie_sample_xtc of the row's log-probabilities with the row's own record, seed and call counter.  Tokens, log-probabilities and logits
are compared exactly; the passes' logits and log-probabilities are those before XTC.  THRESHOLD lies below the second-largest
probability the tiny model gives on these prompts, and every run asserts that the op removed ids on every row that always takes XTC."""
import numpy as np
import pytest
import torch

from tests._util import to_bits
from tests.test_gpu_batch_dry_penalty import pattern_prompts
from tests.test_gpu_batch_edits import make_model, tiny  # noqa: F401  (tiny: the fixture)
from tests.test_gpu_batch_tail import dev_ids, f32_bits, prefilled
from tests.test_gpu_step_tail import PROMPT, IdentityStructuringEngine
from tests.test_gpu_step_xtc import THRESHOLD

pytestmark = pytest.mark.gpu
# by request: (sampler spec or None = greedy, seed, calls so far, XTC or None = a zero record)
REQS = [(("top_k", 0.8, 0.0, 5), 5, 0, (1.0, THRESHOLD, ())), (("categorical", 1.0, 0.0, 0), 6, 4, (0.5, THRESHOLD, (3,))),
        (None, 0, 0, (1.0, THRESHOLD, ())), (("top_p", 0.9, 0.9, 0), 7, 2 ** 32 + 1, None), (("min_p", 1.0, 0.05, 2), 8, 9, (1.0, THRESHOLD, ())),
        (("categorical", 0.7, 0.0, 0), 9, 1, (1.0, THRESHOLD, (5, 6))), (("top_k", 1.0, 0.0, 3), 10, 0, (0.0, THRESHOLD, ()))]


class XReq:
    """One request under host orchestration: a one-row pie_sample_xtc with counter {calls, 0}."""

    def __init__(self, spec, seed, calls, xtc):
        self.spec, self.seed, self.calls, self.xtc, self.removed = spec, seed, calls, xtc, []

    def swap(self, other):
        self.__dict__, other.__dict__ = other.__dict__, self.__dict__

    def record(self):
        from proxy_inference_engine_amd import hip_ops
        return hip_ops.row_tail_pack(*(self.spec or (None,)), seed=self.seed, calls=self.calls)

    def draw(self, lp_row, greedy_token):
        from proxy_inference_engine_amd import _ffi, hip_ops
        if self.spec is None:
            return int(greedy_token)
        lp = lp_row.reshape(1, -1).contiguous()
        V = lp.shape[1]
        counter = torch.tensor([self.calls, 0], dtype=torch.int64, device="cuda")
        rec = hip_ops.xtc_records([hip_ops.xtc_pack(*self.xtc) if self.xtc else _ffi.pie_xtc()], "cuda")
        tok = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        gone = torch.zeros(1, dtype=torch.int32, device="cuda")
        _ffi.check(_ffi.load().pie_sample_xtc(_ffi.p(lp), 1, V, hip_ops.SAMPLE_MODES[self.spec[0]], float(self.spec[1]), float(self.spec[2]), int(self.spec[3]),
                                              int(self.seed), _ffi.p(counter), _ffi.p(hip_ops.sample_workspace(lp.device, 1, V)), _ffi.p(tok), None, None,
                                              _ffi.p(rec), _ffi.p(gone), _ffi.stream()))
        self.calls += 1
        self.removed.append(int(gone.item()))
        return int(tok.item())


def xreqs(n):
    return [XReq(*REQS[i % len(REQS)]) for i in range(n)]


def arm(model, rows_cap, reqs, rows=None):
    rows = list(range(len(reqs))) if rows is None else rows
    model.set_batch_tail(rows_cap)
    model.write_batch_tail(rows, [r.record() for r in reqs])
    bx = model.set_batch_xtc(rows_cap)
    model.write_batch_xtc(rows, [r.xtc for r in reqs])
    return bx


def disarm(model):
    model.clear_batch_xtc(), model.clear_batch_tail()


def assert_bites(hosts):
    always = [h for h in hosts if h.spec is not None and h.xtc is not None and h.xtc[0] == 1.0]
    print("removed per always-on row:", [h.removed for h in always])
    assert always and all(h.removed and min(h.removed) >= 1 for h in always)          # nothing passes vacuously
    assert all(not any(h.removed) for h in hosts if h.xtc is None or h.xtc[0] == 0.0)


# ------------------------------------------------------------------ 1. the batched step
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("B", [3, 7])              # the fused few-sequence form; the general form
def test_step_batch_equals_host_orchestration(tiny, B, graph):
    g, cfg, model = tiny
    V, steps, swap_at = cfg["vocab_size"], 10, 5
    prompts = pattern_prompts(V, [9, 60, 30, 12, 7, 21, 33][:B], 3)
    disarm(model)
    model.enable_paged_kv(num_pages=48)
    caches, first = prefilled(model, prompts)
    hosts, feed, want = xreqs(B), list(first), []
    for st in range(steps):
        if st == swap_at:
            hosts[0].swap(hosts[1])                # rows 0 and 1 exchange their requests' parameters and streams
        nxt, lp, lg = model.step_batch(dev_ids(feed), caches, graph=graph)
        rows = [(h.draw(lp[i], nxt[i]), f32_bits(lp[i]), to_bits(lg[i])) for i, h in enumerate(hosts)]
        want.append(rows)
        feed = [r[0] for r in rows]
    assert_bites(hosts)
    caches, first_a = prefilled(model, prompts)
    assert first_a == first
    reqs = xreqs(B)
    try:
        arm(model, B, reqs)
        replays, feed = model.batch_graph_replays(), dev_ids(first)
        for st in range(steps):
            if st == swap_at:
                for r in reqs:
                    r.calls += swap_at if r.spec is not None else 0
                reqs[0].swap(reqs[1])
                model.write_batch_tail([0, 1], [r.record() for r in reqs[:2]])
                model.write_batch_xtc([0, 1], [r.xtc for r in reqs[:2]])     # new contents behind the same addresses
            nxt, lp, lg = model.step_batch(feed, caches, graph=graph)
            assert nxt.tolist() == [r[0] for r in want[st]], st
            for i in range(B):
                assert np.array_equal(f32_bits(lp[i]), want[st][i][1]) and np.array_equal(to_bits(lg[i]), want[st][i][2]), (st, i)
            feed = nxt.clone()
        assert model.batch_graph_replays() - replays == (steps - 2 if graph else 0)   # eager, capture, then replays only
    finally:
        disarm(model)


# ------------------------------------------------------------------ 2. launches and the graph's key
@pytest.mark.parametrize("B", [3, 7])
def test_launches_per_step(golden_dir, B):
    """With a batch tail, XTC records add one launch to the captured batched step; cleared, it launches what it launched; without a batch
    tail the records are a no-op."""
    g, cfg, model = make_model(golden_dir)
    model.enable_paged_kv(num_pages=64)
    prompts = pattern_prompts(cfg["vocab_size"], [5 + 2 * i for i in range(B)], 9)

    def count():
        caches, first = prefilled(model, prompts)
        feed = dev_ids(first)
        for _ in range(3):                         # eager, capture, replay
            feed = model.step_batch(feed, caches)[0].clone()
        for c in caches:
            c[0].page_manager.release()
        return model.batch_graph_launches()

    try:
        for tailed in (False, True):
            if tailed:
                model.set_batch_tail(B)
            base = count()
            assert base > 0
            model.set_batch_xtc(B)
            assert count() == base + (1 if tailed else 0), (B, tailed)
            model.clear_batch_xtc()
            assert count() == base, (B, tailed)
    finally:
        disarm(model)


def test_new_addresses_recapture_and_new_contents_replay(golden_dir):
    g, cfg, model = make_model(golden_dir)
    B = 3
    model.enable_paged_kv(num_pages=32)
    prompts = pattern_prompts(cfg["vocab_size"], [9, 20, 12], 4)
    caches, first = prefilled(model, prompts)
    feed = dev_ids(first)

    def step(n):
        nonlocal feed
        before = model.batch_graph_replays()
        for _ in range(n):
            feed = model.step_batch(feed, caches)[0].clone()
        return model.batch_graph_replays() - before

    try:
        model.set_batch_tail(B)
        model.write_batch_tail([0, 1, 2], [r.record() for r in xreqs(3)])
        assert step(3) == 1                                                    # eager, capture, replay
        bx = model.set_batch_xtc(B)
        model.write_batch_xtc([0, 1, 2], [REQS[0][3], None, REQS[4][3]])
        assert step(3) == 1                                                    # another key: eager, capture, replay
        model.write_batch_xtc([0, 1, 2], [None, REQS[1][3], None])             # new contents behind the same addresses
        assert step(2) == 2 and model.set_batch_xtc(B)["records"].data_ptr() == bx["records"].data_ptr()
        assert step(1) == 1                                                    # set again with the same buffer: the same key
        other = model.set_batch_xtc(B + 2)                                     # another rows_cap: another buffer, another key
        assert other["records"].data_ptr() != bx["records"].data_ptr()
        assert step(3) == 1
        model.clear_batch_xtc()
        assert step(3) == 1                                                    # the key of the tail alone: eager, capture, replay
    finally:
        disarm(model)


# ------------------------------------------------------------------ 3. the prompt passes
@pytest.mark.parametrize("S", [3, 7])
def test_prompt_passes(tiny, S):
    """prefill_batch and step_mixed with S output rows (decoding rows first) under mixed records."""
    g, cfg, model = tiny
    V = cfg["vocab_size"]
    prompts = pattern_prompts(V, [9, 20, 12, 7, 21, 33, 15][:S], 5)
    nd = S // 2
    disarm(model)
    model.enable_paged_kv(num_pages=48)
    fresh = lambda n: [model.make_cache() for _ in range(n)]
    nxt, lp, lg = model.prefill_batch(prompts, fresh(S))
    hosts = xreqs(S)
    want_pf = [(h.draw(lp[i], nxt[i]), f32_bits(lp[i]), to_bits(lg[i])) for i, h in enumerate(hosts)]
    assert_bites(hosts)
    dcs, dtoks = prefilled(model, prompts[:nd])
    nxt, lp, lg = model.step_mixed(dev_ids(dtoks), dcs, prompts[nd:], fresh(S - nd))
    hosts = xreqs(S)
    want_mx = [(h.draw(lp[i], nxt[i]), f32_bits(lp[i]), to_bits(lg[i])) for i, h in enumerate(hosts)]
    assert_bites(hosts)
    try:
        arm(model, S, xreqs(S))
        nxt, lp, lg = model.prefill_batch(prompts, fresh(S))
        for i in range(S):
            assert int(nxt[i]) == want_pf[i][0], i
            assert np.array_equal(f32_bits(lp[i]), want_pf[i][1]) and np.array_equal(to_bits(lg[i]), want_pf[i][2]), i
        dcs, dtoks2 = prefilled(model, prompts[:nd])
        assert dtoks2 == dtoks
        arm(model, S, xreqs(S))
        nxt, lp, lg = model.step_mixed(dev_ids(dtoks), dcs, prompts[nd:], fresh(S - nd))
        for i in range(S):
            assert int(nxt[i]) == want_mx[i][0], i
            assert np.array_equal(f32_bits(lp[i]), want_mx[i][1]) and np.array_equal(to_bits(lg[i]), want_mx[i][2]), i
    finally:
        disarm(model)


# ------------------------------------------------------------------ 4. refusals, each before any launch
def test_refusals(tiny):
    from proxy_inference_engine_amd import hip_ops
    g, cfg, model = tiny
    disarm(model)
    model.enable_paged_kv(num_pages=16)
    prompts = pattern_prompts(cfg["vocab_size"], [9, 20, 30], 3)
    caches, first = prefilled(model, prompts)
    model.step_batch(dev_ids(first), caches, graph=False)
    bx = model.set_batch_xtc(2)
    try:
        assert bx["records"].shape == (2, hip_ops.XTC_WORDS) and not bx["records"].any().item()
        offsets = [c[0].offset for c in caches]
        with pytest.raises(ValueError, match="rows_cap"):
            model.step_batch(dev_ids(first), caches, graph=False)
        assert [c[0].offset for c in caches] == offsets
        with pytest.raises(ValueError, match="rows_cap"):
            model.prefill_batch(prompts, [model.make_cache() for _ in prompts])
        with pytest.raises(ValueError, match="rows_cap"):
            model.step_mixed(dev_ids(first[:1]), caches[:1], prompts[:2], [model.make_cache(), model.make_cache()])
        for bad in ((1.5, 0.1, ()), (0.5, 0.0, ()), (0.5, 0.6, ()), (0.5, 0.1, tuple(range(17))), (float("nan"), 0.1, ())):
            with pytest.raises(ValueError):
                model.write_batch_xtc([0], [bad])
        with pytest.raises(ValueError):
            model.write_batch_xtc([0, 1], [REQS[0][3]])
        model.write_batch_xtc([1], [(0.25, 0.5, (7, 9))])
        words = bx["records"][1]
        assert words[:2].view(torch.float32).tolist() == [float(np.float32(np.log(0.5))), 0.25] and words[2:6].tolist() == [2, 0, 7, 9]
        model.write_batch_xtc([1], [None])
        assert not bx["records"].any().item()
    finally:
        model.clear_batch_xtc()
    assert model.step_batch(dev_ids(first), caches, graph=False)[0].shape == (3,)
    with pytest.raises(RuntimeError):
        model.write_batch_xtc([0], [None])
    with pytest.raises(ValueError):
        model.set_batch_xtc(0)


# ------------------------------------------------------------------ 5. the engines
def test_batched_engine_generates_with_mixed_params(tiny):
    """Every request of a mixed batch generates what it generates alone through the same engine.
    The passes of a mixed batch and of a request alone are not the same launches, and their log-probabilities differ in the last bits
    (test_gpu_batch_dry_penalty.py's note).  A kept set that is decided by a cumulative mass is discontinuous in those bits: with
    top_p = 0.9 behind XTC the fifth request drew id 234 alone and 447 in the batch from its very first distribution, where 234 sits on
    top-p's boundary -- each equal to the one-row op on its own pass's log-probabilities.  So the sampled requests here use top-k and the
    plain categorical draw, whose kept sets do not move with the last bits, and the unarmed engine's batch-invariance is asserted first."""
    from proxy_inference_engine_amd.engine import BatchedEngine, SamplingParams
    g, cfg, model = tiny
    V, new = cfg["vocab_size"], 10
    disarm(model)
    prompts = pattern_prompts(V, [12, 70, 5, 33, 64], 27)
    params = [SamplingParams(temp=0.8, top_k=5, seed=21, xtc_probability=1.0, xtc_threshold=THRESHOLD),
              SamplingParams(temp=1.0, seed=22, xtc_probability=0.5, xtc_threshold=THRESHOLD, xtc_special_tokens=(3, 4)),
              SamplingParams(xtc_probability=1.0, xtc_threshold=THRESHOLD),                      # greedy: XTC is ignored
              SamplingParams(temp=0.8, top_k=5, seed=21), SamplingParams(temp=0.9, top_k=5, seed=23, xtc_probability=1.0, xtc_threshold=0.05)]
    eng = BatchedEngine(model, num_pages=64, max_batch=3, stop_tokens=[V - 1])
    assert params[0].xtc(eng.stop_tokens) == (1.0, THRESHOLD, (V - 1,)) and params[2].xtc() is None and params[3].xtc() is None
    plain = eng.generate(prompts, new)
    assert plain == [eng.generate([p], new)[0] for p in prompts]                        # the precondition: the unarmed engine is batch-invariant here
    out = eng.generate(prompts, new, sampling=params)
    assert model._batch_xtc is None and model._batch_tail is None                      # cleared on the way out
    assert out == eng.generate(prompts, new, sampling=params)
    assert out[2] == plain[2]
    no_xtc = eng.generate(prompts, new, sampling=[SamplingParams(temp=sp.temp, top_k=sp.top_k, top_p=sp.top_p, seed=sp.seed) for sp in params])
    assert out[3] == no_xtc[3] and out[0] != no_xtc[0]                                  # same seed: XTC changed the stream of the request that has it
    alone = [eng.generate([prompts[r]], new, sampling=params[r])[0] for r in range(5)]
    assert out == alone
    with pytest.raises(ValueError):
        eng.generate(prompts[:1], new, sampling=SamplingParams(temp=1.0, xtc_probability=0.5, xtc_threshold=0.7))


def test_inference_engine_fused_tail_equals_host_orchestrated_branch(tiny):
    """generate(xtc_probability=...) through the fused tail equals the same request on the host-orchestrated branch (a structuring engine
    forces it), token for token; the special tokens default to the engine's stop tokens."""
    from proxy_inference_engine_amd import InferenceEngine, samplers
    g, cfg, model = tiny
    kwargs = dict(temp=0.8, top_k=5, xtc_probability=0.5, xtc_threshold=THRESHOLD, max_completion_tokens=16)
    stop = [cfg["vocab_size"] - 1]
    runs = {}
    try:
        for name, se in (("fused", None), ("host", IdentityStructuringEngine())):
            samplers.seed(3)
            eng = InferenceEngine(model=model, structuring_engine=se, stop_tokens=stop)
            eng.prepare_engine(PROMPT, **kwargs)
            runs[name] = [t for t, _ in eng.generate(PROMPT, **kwargs)]
            assert (model.step_xtc_record is not None) == (name == "fused"), name
            if name == "fused":
                assert model._xtc == (0.5, THRESHOLD, (stop[0],))
        samplers.seed(3)
        eng = InferenceEngine(model=model, stop_tokens=stop)
        plain_kw = dict(temp=0.8, top_k=5, max_completion_tokens=16)
        eng.prepare_engine(PROMPT, **plain_kw)
        plain = [t for t, _ in eng.generate(PROMPT, **plain_kw)]
        assert model.step_xtc_record is None
    finally:
        model.set_step_tail()
    assert runs["fused"] == runs["host"] and len(runs["fused"]) >= 1
    assert runs["fused"] != plain
