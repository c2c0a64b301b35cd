"""-m gpu: top-n log-probabilities on the device -- the op, the single-sequence step's tail, the three multi-sequence
passes and both engines -- against tests/top_logprobs_reference.py.  Every comparison is exact: ids equal, values bit-equal as uint32."""
import json

import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests import sampler_rows as sr
from tests import top_logprobs_reference as ref
from tests._util import codes_dev, to_bits, to_dev
from tests.test_gpu_batch_tail import prefilled, repeating_prompts, three_requests

pytestmark = pytest.mark.gpu
DT = "bfloat16"
NEG_INF = 0xFF800000


def dev_ids(ids) -> torch.Tensor:
    return torch.tensor([int(i) for i in ids], dtype=torch.int32, device="cuda")


def bits_of(t: torch.Tensor) -> np.ndarray:
    return t.detach().contiguous().cpu().numpy().view(np.uint32).copy()


def assert_record(ids, vals, want, what):
    """ids / vals: one row of the op's outputs (tensors); want: reference(...)."""
    got_ids, got_bits = ids.cpu().numpy(), bits_of(vals)
    assert got_ids.tolist() == want[0].tolist(), (what, got_ids.tolist(), want[0].tolist())
    assert np.array_equal(got_bits, want[1]), (what, got_bits, want[1])


def sentinels(rows, n):
    return (torch.full((rows, n + 1), ref.SENTINEL_ID, dtype=torch.int32, device="cuda"),
            torch.full((rows, n + 1), 123.0, dtype=torch.float32, device="cuda"))


# ------------------------------------------------------------------ 1. the op against the reference
@pytest.fixture(scope="module")
def rows_by_vocab():
    return {V: ref.family_rows(V) for V in (7, 512, 1500, 4099)}


@pytest.mark.parametrize("n", [1, 5, 20])
@pytest.mark.parametrize("V", [7, 512, 1500, 4099])   # a slice smaller than n; one full slice; three slices, the last ragged; a last slice of 3 ids
def test_op_equals_reference_on_designed_rows(rows_by_vocab, V, n):
    from proxy_inference_engine_amd import hip_ops
    rows = rows_by_vocab[V]
    lp = torch.from_numpy(np.stack([r for _, r in rows])).cuda()
    R = len(rows)
    tokens = [(5 * s + 3) % V for s in range(R)]
    tokens[0], tokens[1] = V, -3                       # ids outside the row: slot 0 is (-1, -inf) and nothing is indexed
    ids, vals = hip_ops.top_logprobs(lp, n, tokens=dev_ids(tokens))
    none_ids, none_vals = hip_ops.top_logprobs(lp, n)
    for s, (name, row) in enumerate(rows):
        assert_record(ids[s], vals[s], ref.reference(row, n, token=tokens[s]), (name, V, n))
        assert_record(none_ids[s], none_vals[s], ref.reference(row, n), (name, V, n, "no tokens"))
    assert ids[0, 0] == -1 and ids[1, 0] == -1 and bits_of(vals[:2, 0]).tolist() == [NEG_INF] * 2
    if V >= 64 and n == 20:                            # the 20th place falls inside the tie class: its 8 lowest ids win
        s = [name for name, _ in rows].index("boundary_tie")
        _, above, tie = ref.boundary_tie_row(V)
        got = ids[s, 1:].tolist()
        assert sorted(got[:12]) == sorted(above.tolist()) and got[12:] == np.sort(tie)[:8].tolist()


def test_op_rows_and_counts():
    from proxy_inference_engine_amd import hip_ops
    V, n = 1500, 20
    fam = [sr.quantized(V, 1), sr.wide_tie(V, 2), sr.uniform(V), sr.topp_tie(V, 4), sr.all_inf(V), sr.quantized(V, 5), sr.sparse(V, 3, 6)]
    lp = torch.from_numpy(np.stack([r.lp for r in fam])).cuda()
    tokens = dev_ids([11, 700, 1499, 0, 3, 512, 1024])
    ws = hip_ops.top_logprobs_workspace("cuda", 7, V, n)
    ws.fill_(-1)                                       # the workspace needs no initialisation: garbage must not show
    counts = [20, 5, 0, -1, 99, 1, -7]
    for call in range(2):
        out = sentinels(7, n)
        ids, vals = hip_ops.top_logprobs(lp, n, tokens=tokens, count=dev_ids(counts), workspace=ws, out=out)
        for s, c in enumerate(counts):
            what = (call, s, c)
            if c < 0:                                  # the row's record is left alone
                assert ids[s].tolist() == [ref.SENTINEL_ID] * (n + 1) and bits_of(vals[s]).tolist() == [ref.SENTINEL_BITS] * (n + 1), what
                continue
            assert_record(ids[s], vals[s], ref.reference(fam[s].lp, n, token=int(tokens[s]), count=c), what)
            one = hip_ops.top_logprobs(lp[s:s + 1].contiguous(), n, tokens=tokens[s:s + 1].contiguous(), count=dev_ids([min(c, n)]))
            assert torch.equal(one[0][0], ids[s]) and np.array_equal(bits_of(one[1][0]), bits_of(vals[s])), what
            if c == 99:
                full = hip_ops.top_logprobs(lp[s:s + 1].contiguous(), n, tokens=tokens[s:s + 1].contiguous())
                assert torch.equal(full[0][0], ids[s]) and np.array_equal(bits_of(full[1][0]), bits_of(vals[s])), what
        counts = counts[3:] + counts[:3]               # the same workspace, the counts rotated: nothing is carried over


def test_op_at_the_largest_vocabulary():
    """V = 524288: 1024 slices, the 1024-thread form of the second launch."""
    from proxy_inference_engine_amd import hip_ops
    V = sr.V_MAX
    lp = sr.quantized(V, 2).lp
    ids, vals = hip_ops.top_logprobs(torch.from_numpy(lp).cuda(), 20, tokens=dev_ids([V - 1]))
    assert_record(ids[0], vals[0], ref.reference(lp, 20, token=V - 1), "V_MAX")


# ------------------------------------------------------------------ the tiny golden model
@pytest.fixture(scope="module")
def tiny(golden_dir):
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    g = np.load(golden_dir / "tiny_llama_w4_bf16.npz")
    cfg = json.loads(str(g["config_json"]))
    w = {k[2:]: (codes_dev(g[k]) if g[k].dtype == np.uint32 else to_dev(g[k], DT)) for k in g.files if k.startswith("w:")}
    return g, cfg, Model(ModelArgs(**cfg), w)


def make_caches(model, kind):
    from proxy_inference_engine_amd.cache import QuantizedKVCache, RotatingKVCache
    if kind == "reusable":
        return model.make_cache()
    if kind == "pages":
        return model.make_paged_cache(num_pages=8, max_blocks=4)
    if kind == "quantized":
        return [QuantizedKVCache(group_size=64, bits=8) for _ in model.layers]
    return [RotatingKVCache(16, keep=4) for _ in model.layers]


TAIL = dict(sampler=("top_k", 0.8, 0.0, 5), repetition_penalty=1.3)
STEP_LAUNCHES = 2          # what DESIGN.md 13 states: the slices' launch and the merge


def run_steps(model, cache, prompt, n, graph, steps=6, **tail):
    """6 steps (the prompt pass, then fed-back steps) under set_step_tail(top_logprobs=n): every record is the reference of the step's own
    logprobs with the returned token."""
    from proxy_inference_engine_amd import samplers
    samplers.seed(9)
    model.set_step_tail(top_logprobs=n, **tail)
    toks = []
    for i in range(steps):
        tok, lp, _ = model.step(dev_ids(prompt) if i == 0 else None, cache, graph=graph)
        ids, vals = model.step_top_logprobs
        assert ids.shape == (n + 1,) and vals.shape == (n + 1,)
        want = ref.reference(lp.cpu().numpy(), max(n, 1), token=int(tok.item()))
        assert_record(ids, vals, (want[0][:n + 1], want[1][:n + 1]), (i, n, graph, sorted(tail)))
        assert int(ids[0]) == int(tok.item()) >= 0
        toks.append(int(tok.item()))
    return toks


@pytest.mark.parametrize("graph", [False, True])
def test_step_records_equal_reference(tiny, graph):
    from proxy_inference_engine_amd import hip_ops
    g, cfg, model = tiny
    prompt, V = g["prompt"].tolist(), cfg["vocab_size"]
    try:
        plain = run_steps(model, model.make_cache(), prompt, 5, graph, **TAIL)
        allowed = torch.zeros(V, dtype=torch.bool)
        allowed[::3] = True
        masked = run_steps(model, model.make_cache(), prompt, 5, graph, token_mask=hip_ops.pack_token_mask(allowed, V), **TAIL)
        assert all(t % 3 == 0 for t in masked) and len(plain) == len(masked) == 6
        run_steps(model, model.make_cache(), prompt, 0, graph, **TAIL)        # slot 0 only
        run_steps(model, model.make_cache(), prompt, 20, graph)               # on the greedy tail alone: slot 0 and slot 1 agree
        assert int(model.step_top_logprobs[0][0]) == int(model.step_top_logprobs[0][1])
    finally:
        model.set_step_tail()
    with pytest.raises(RuntimeError):
        model.step_top_logprobs
    with pytest.raises(ValueError, match="top_logprobs"):
        model.set_step_tail(top_logprobs=21)


def test_step_graph_launches(tiny):
    from proxy_inference_engine_amd import samplers
    g, cfg, model = tiny
    prompt = g["prompt"].tolist()

    def launches(**tail):
        samplers.seed(1)
        model.set_step_tail(**tail)
        cache = model.make_cache()
        model.step(dev_ids(prompt), cache)
        model.step(None, cache)
        return model.graph_launches()

    try:
        greedy, tailed = launches(), launches(**TAIL)
        assert greedy > 0 and tailed > greedy
        assert launches(top_logprobs=5) - greedy == STEP_LAUNCHES <= 2
        assert launches(top_logprobs=5, **TAIL) - tailed == STEP_LAUNCHES
        assert launches(top_logprobs=0, **TAIL) - tailed == STEP_LAUNCHES
        assert launches(**TAIL) == tailed and launches() == greedy           # switched off: exactly the launches from before
    finally:
        model.set_step_tail()


@pytest.mark.parametrize("kind", ["pages", "quantized", "rotating"])
def test_step_records_on_every_cache_kind(tiny, kind):
    g, cfg, model = tiny
    try:
        run_steps(model, make_caches(model, kind), g["prompt"].tolist(), 5, True, **TAIL)
    finally:
        model.set_step_tail()


# ------------------------------------------------------------------ the multi-sequence passes
def check_rows(bufs, counts, nxt, lp, n, what):
    for s, c in enumerate(counts):
        if c < 0:
            assert bufs["ids"][s].tolist() == [ref.SENTINEL_ID] * (n + 1) and bits_of(bufs["vals"][s]).tolist() == [ref.SENTINEL_BITS] * (n + 1), (what, s)
        else:
            assert_record(bufs["ids"][s], bufs["vals"][s], ref.reference(lp[s].cpu().numpy(), n, token=int(nxt[s]), count=c), (what, s, c))


def preset(bufs):
    bufs["ids"].fill_(ref.SENTINEL_ID), bufs["vals"].fill_(123.0)


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("graph", [False, True])
def test_step_batch_records(tiny, graph, tail):
    g, cfg, model = tiny
    V, steps, n = cfg["vocab_size"], 6, 5
    prompts = repeating_prompts(V, [9, 63, 30], 3)
    model.clear_batch_tail(), model.clear_batch_top_logprobs()
    model.enable_paged_kv(num_pages=16)

    def run(armed):
        caches, first = prefilled(model, prompts)
        bufs, out = None, []
        try:
            if tail:
                reqs = three_requests(prompts)
                model.set_batch_tail(3)
                model.write_batch_tail([0, 1, 2], [r.record() for r in reqs], [r.fed for r in reqs])
            if armed:
                bufs = model.set_batch_top_logprobs(3, n)
            replays, feed = model.batch_graph_replays(), dev_ids(first)
            for st in range(steps):
                counts = [5, -1, 2] if st < 3 else [0, 3, -1]       # rewritten between replays: contents only
                if armed:
                    bufs["count"].copy_(dev_ids(counts))
                    preset(bufs)
                nxt, lp, lg = model.step_batch(feed, caches, graph=graph)
                if armed:
                    check_rows(bufs, counts, nxt, lp, n, (graph, tail, st))
                out.append((nxt.tolist(), bits_of(lp), to_bits(lg)))
                feed = nxt.clone()
            # eager, capture, then replays only -- through the rewritten counts as well
            assert model.batch_graph_replays() - replays == (steps - 2 if graph else 0)
            return out, model.batch_graph_launches()
        finally:
            model.clear_batch_tail(), model.clear_batch_top_logprobs()

    unarmed, base_launches = run(False)
    armed, launches = run(True)
    for st, (a, u) in enumerate(zip(armed, unarmed)):       # the pass's own outputs do not notice
        assert a[0] == u[0] and np.array_equal(a[1], u[1]) and np.array_equal(a[2], u[2]), st
    if graph:
        assert launches - base_launches == STEP_LAUNCHES


def test_prompt_passes_records(tiny):
    g, cfg, model = tiny
    V, n = cfg["vocab_size"], 20
    p7, p70, pd = repeating_prompts(V, [7, 70, 20], 5)
    model.clear_batch_tail(), model.clear_batch_top_logprobs()
    model.enable_paged_kv(num_pages=24)
    bufs = model.set_batch_top_logprobs(4, n)
    try:
        bufs["count"].copy_(dev_ids([20, 3, -1, -1]))
        preset(bufs)
        nxt, lp, _ = model.prefill_batch([p7, p70], [model.make_cache(), model.make_cache()])
        check_rows(bufs, [20, 3], nxt, lp, n, "prefill_batch")
        assert bufs["ids"][2:].eq(ref.SENTINEL_ID).all()                    # rows beyond the pass's: untouched
        (dc,), (dtok,) = prefilled(model, [pd])
        bufs["count"].copy_(dev_ids([1, -1, 20, 7]))
        preset(bufs)
        nxt, lp, _ = model.step_mixed(dev_ids([dtok]), [dc], [p7, p70], [model.make_cache(), model.make_cache()])   # the decode row first, then the prompts
        check_rows(bufs, [1, -1, 20], nxt, lp, n, "step_mixed")
        assert bufs["ids"][3].eq(ref.SENTINEL_ID).all()
    finally:
        model.clear_batch_top_logprobs()


# ------------------------------------------------------------------ the engines
class IdentityStructuringEngine:
    """Forces the engine onto its host-orchestrated branch without changing any value."""
    has_reached_accept_state = False

    def get_current_state(self):
        return None

    def process_logits(self, tokens, logits):
        return logits

    def sample(self, logprobs, sampler):
        return sampler(logprobs)


@pytest.mark.parametrize("branch", ["fused", "host"])
def test_inference_engine_maps(tiny, branch, monkeypatch):
    from proxy_inference_engine_amd import InferenceEngine, samplers
    g, cfg, model = tiny
    prompt, steps = g["prompt"].tolist(), 8
    se = (lambda: IdentityStructuringEngine()) if branch == "host" else (lambda: None)
    calls = []
    real_topk = torch.topk
    monkeypatch.setattr(torch, "topk", lambda *a, **k: (calls.append(1), real_topk(*a, **k))[1])
    try:
        samplers.seed(3)
        eng = InferenceEngine(model=model, structuring_engine=se())
        eng.prepare_engine(prompt, temp=0.8, top_k=5)
        got = list(eng.generate(prompt, logprobs=True, top_logprobs=3, max_completion_tokens=steps))
        assert (model.step_tail[0] is not None) == (branch == "fused")
        samplers.seed(3)
        eng2 = InferenceEngine(model=model, structuring_engine=se())
        eng2.prepare_engine(prompt, temp=0.8, top_k=5)
        gen = eng2.generate_step(torch.tensor(prompt))
        assert len(got) == steps
        for i in range(steps):
            tok, lp = next(gen)
            tok = int(tok.item())
            assert got[i][0] == tok, i
            assert list(got[i][1].items()) == ref.to_map(*ref.reference(lp.cpu().numpy(), 3, token=tok), 3), i
        assert not calls                                                     # no library sort anywhere
        with pytest.raises(ValueError, match="top_logprobs"):
            next(InferenceEngine(model=model).generate(prompt, logprobs=True, top_logprobs=21))
    finally:
        model.set_step_tail()


class Recorder:
    """Wraps the three passes on the instance: every pass's returned tokens and logprobs, cloned, in order."""

    def __init__(self, model):
        self.model, self.passes = model, []
        for name in ("step_batch", "step_mixed", "prefill_batch"):
            setattr(model, name, self.wrap(getattr(model, name)))

    def wrap(self, fn):
        def inner(*a, **k):
            out = fn(*a, **k)
            self.passes.append((out[0].clone(), out[1].clone()))
            return out
        return inner

    def remove(self):
        for name in ("step_batch", "step_mixed", "prefill_batch"):
            delattr(self.model, name)


@pytest.mark.parametrize("sampled", [False, True])
def test_batched_engine_maps(tiny, sampled):
    from proxy_inference_engine_amd.engine import BatchedEngine, SamplingParams
    g, cfg, model = tiny
    prompts = repeating_prompts(cfg["vocab_size"], [12, 70, 5, 33], 11)
    tops = [3, 0, 20, 1]
    sampling = [SamplingParams(temp=0.8, top_k=5, seed=21), SamplingParams(), SamplingParams(temp=1.0, top_p=0.9, repetition_penalty=1.1, seed=22),
                SamplingParams(repetition_penalty=1.3, repetition_context_size=8)] if sampled else None
    try:
        eng = BatchedEngine(model, num_pages=32, max_batch=4)
        plain = eng.generate(prompts, 8, sampling=sampling)
        rec = Recorder(model)
        try:
            outputs, maps = eng.generate(prompts, 8, sampling=sampling, logprobs=True, top_logprobs=tops)
        finally:
            rec.remove()
        assert outputs == plain and [len(o) for o in outputs] == [8] * 4
        passes = [(t.tolist(), lp.cpu().numpy()) for t, lp in rec.passes]
        for i, (out, ms) in enumerate(zip(outputs, maps)):
            assert len(ms) == len(out)
            at = 0                                                           # every map is a recorded row's reference, in pass order
            for j, (tok, m) in enumerate(zip(out, ms)):
                items = list(m.items())
                assert tok in m and len(m) in (max(tops[i], 1), tops[i] + 1), (i, j)
                assert all((a[1] > b[1]) or (a[1] == b[1] and a[0] < b[0]) for a, b in zip(items[:tops[i]], items[1:tops[i]])), (i, j)
                if (sampling is None or sampling[i].plain) and tops[i]:
                    assert items[0][0] == tok, (i, j)                        # greedy: the token is the best id
                found = None
                for k in range(at, len(passes)):
                    toks, lp = passes[k]
                    if any(t == tok and ref.to_map(*ref.reference(lp[s], max(tops[i], 1), token=t, count=tops[i]), tops[i]) == items for s, t in enumerate(toks)):
                        found = k
                        break
                assert found is not None, (i, j, tok)
                at = found + 1
        assert eng.generate(prompts, 8, sampling=sampling) == plain           # the arming was cleared: today's passes again
    finally:
        model.clear_batch_tail(), model.clear_batch_top_logprobs()
        model.enable_paged_kv(num_pages=16)


# ------------------------------------------------------------------ refusals
def test_refusals(tiny):
    from proxy_inference_engine_amd import _ffi
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    from proxy_inference_engine_amd.tp import HipComm
    from tests.test_gpu_tp import CFG
    g, cfg, model = tiny
    lib = _ffi.load()
    model.clear_batch_tail(), model.clear_batch_top_logprobs()
    model.enable_paged_kv(num_pages=16)
    prompts = repeating_prompts(cfg["vocab_size"], [9, 20, 30], 3)
    caches, first = prefilled(model, prompts)
    model.step_batch(dev_ids(first), caches, graph=False)
    bufs = model.set_batch_top_logprobs(2, 5)
    try:
        buf = model._batch_bufs[3]
        buf["next"].fill_(-9)
        with pytest.raises(ValueError, match="rows_cap"):                   # more rows than records: before any launch
            model.step_batch(dev_ids(first), caches, graph=False)
        torch.cuda.synchronize()
        assert buf["next"].tolist() == [-9] * 3
        with pytest.raises(ValueError, match="rows_cap"):
            model.prefill_batch(prompts, [model.make_cache() for _ in prompts])
        args = [_ffi.p(bufs["ids"]), _ffi.p(bufs["vals"]), _ffi.p(bufs["count"]), _ffi.p(bufs["ws"])]
        assert lib.pie_decoder_set_batch_top_logprobs(model._dec, 21, 2, *args) == -1
        assert lib.pie_decoder_set_batch_top_logprobs(model._dec, 5, 0, *args) == -2
        assert lib.pie_decoder_set_batch_top_logprobs(model._dec, 5, 2, args[0], args[1], args[2], bufs["ws"].data_ptr() + 4) == -3
        assert lib.pie_decoder_set_top_logprobs(model._dec, 21, args[0], args[1], args[3], 1 << 20) == -1
        assert lib.pie_decoder_set_top_logprobs(model._dec, 5, args[0], args[1], args[3], 8) == -2
        with pytest.raises(ValueError):
            model.set_batch_top_logprobs(2, 0)
    finally:
        model.clear_batch_top_logprobs()
    assert model.step_batch(dev_ids(first), caches, graph=False)[0].shape == (3,)
    # a tensor-parallel decoder's tail is vocabulary-parallel: both setters are refused
    w = po.synth_checkpoint(CFG, seed=72, dtype=DT, lm_head_gain=4.0)
    dev_w = {k: (codes_dev(v) if v.dtype == np.uint32 else to_dev(v, DT)) for k, v in w.items()}
    comm = HipComm(CFG["hidden_size"], backend="ipc")
    try:
        tp = Model(ModelArgs(**CFG), dev_w, tp=comm)
        assert lib.pie_decoder_set_top_logprobs(tp._dec, 5, args[0], args[1], args[3], 1 << 20) == -5
        assert b"pie_decoder_set_top_logprobs" in lib.pie_last_error()
        assert lib.pie_decoder_set_batch_top_logprobs(tp._dec, 5, 2, *args) == -5
        assert b"pie_decoder_set_batch_top_logprobs" in lib.pie_last_error()
        with pytest.raises(RuntimeError):
            tp.set_step_tail(top_logprobs=3)
        with pytest.raises(RuntimeError):
            tp.set_batch_top_logprobs(2, 5)
        del tp
    finally:
        comm.close()
