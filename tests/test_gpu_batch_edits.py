"""-m gpu: per-row token masks and logit biases in the multi-sequence passes against the single-row ops they are defined
by -- pie_logprobs_argmax_masked, pie_logits_bias, pie_logits_penalty, pie_logprobs_argmax and a one-row pie_sample (themselves pinned by
tests/test_gpu_step_edits.py, test_gpu_logits_tail.py and test_gpu_batch_tail.py).  Every comparison is exact: a row of
pie_logprobs_argmax_rows_masked IS pie_logprobs_argmax_masked of that row (or pie_logprobs_argmax, when the row is off), a row of
pie_logits_bias_rows IS pie_logits_bias with the row's table, and the passes' tail is those around the rows' penalties and samplers."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests._util import codes_dev, to_bits, to_dev
from tests.test_gpu_batch_tail import dev_ids, f32_bits, prefilled, rec, repeating_prompts, sample_one

pytestmark = pytest.mark.gpu
DT = "bfloat16"


def pack(bits: np.ndarray, words: int | None = None) -> np.ndarray:
    """bool [n] -> int32 words, LSB first (hip_ops.pack_token_mask's layout, without its checks: bits beyond V are wanted here)."""
    n = bits.size if words is None else 32 * words
    padded = np.zeros(n + (-n % 32), bool)
    padded[:bits.size] = bits
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)


# ------------------------------------------------------------------ 1. the ops against the single-row ops
def seven_masks(V, rng):
    """-> (on [7], words int32 [7, W], allowed bool [7, V]); W = ceil(V / 32) + 1: a whole word lies beyond the vocabulary."""
    W = (V + 31) // 32 + 1
    allowed = np.zeros((7, V), bool)
    allowed[0] = True                                                     # off
    allowed[1, V // 3] = True                                             # one allowed id
    allowed[2, V - 1] = True                                              # a single allowed id, the row's last
    allowed[3, ::2] = True                                                # alternating bits
    allowed[4] = True                                                     # all allowed
    allowed[5] = rng.random(V) < 0.3                                      # bits at and beyond V are set as well (below)
    allowed[6] = True                                                     # off, the words are garbage
    words = np.stack([pack(a, W) for a in allowed])
    beyond = np.zeros(32 * W, bool)
    beyond[V:] = True
    words[5] |= pack(beyond, W)
    words[6] = rng.integers(-2 ** 31, 2 ** 31, W).astype(np.int32)
    words[0] = 0
    on = np.array([0, 1, 7, -1, 1, 1, 0], np.int32)                      # nonzero means on
    return on, words, allowed


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("V", [200, 1500, 4099])   # fewer ids than tiles and a partial last word; tiles that straddle words, V % 32 != 0
def test_rows_masked_is_the_single_row_op_per_row(V, dt):
    from proxy_inference_engine_amd import hip_ops
    rng = np.random.default_rng(V + len(dt))
    on, words, allowed = seven_masks(V, rng)
    base = po.to_bits((rng.standard_normal((7, V)) * 6).astype(np.float32), dt)
    base[:, 1] = base[:, V - 2]                                           # a tie
    base[3, 4] = 0xFC00 if dt == "float16" else 0xFF80                    # a -inf of the row's own
    logits = to_dev(base, dt)
    masks, mask_on = torch.from_numpy(words).cuda(), torch.from_numpy(on).cuda()
    tok, lp = hip_ops.logprobs_argmax_rows_masked(logits, masks, mask_on)
    got = to_bits(logits)
    for r in range(7):
        row = to_dev(base[r], dt)
        if on[r]:
            wtok, wlp = hip_ops.logprobs_argmax_masked(row, masks[r].clone())
            assert not np.array_equal(to_bits(row), base[r]) or allowed[r].all(), r
        else:
            wtok, wlp = hip_ops.logprobs_argmax(row)
            assert np.array_equal(got[r], base[r]), (V, dt, r)            # an off row keeps every bit
        assert np.array_equal(got[r], to_bits(row)), (V, dt, r, "logits")
        assert np.array_equal(f32_bits(lp[r]), f32_bits(wlp)), (V, dt, r, "logprobs")
        assert int(tok[r]) == int(wtok.item()), (V, dt, r, "token")
        if on[r]:
            assert allowed[r][int(tok[r])], r
            assert np.array_equal(np.isfinite(lp[r].cpu().numpy()), allowed[r] & np.isfinite(to_dev(base[r], dt).float().cpu().numpy())), r


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("V", [200, 1500])
def test_bias_rows_is_the_single_row_op_per_row(V, dt):
    from proxy_inference_engine_amd import hip_ops
    rng = np.random.default_rng(V + 3 * len(dt))
    cap, rows = 6, 8
    base = po.to_bits((rng.standard_normal((rows, V)) * 6).astype(np.float32), dt)
    ids = rng.integers(0, V, (rows, cap)).astype(np.int32)
    vals = (rng.standard_normal((rows, cap)) * 4).astype(np.float32)
    n = np.array([0, 1, cap, cap + 3, 5, cap, cap, -2], np.int32)         # none; one; all; above cap (clamped); ...; below zero (none)
    ids[2] = [17, 3, 99, 150, 0, V - 1]
    ids[4, :5] = [5, 5, 9, 5, 9]                                          # duplicates: the first owns the id
    ids[5] = [-1, V, 12, -2 ** 31, 2 ** 31 - 1, V - 1]                    # ids outside [0, V) are skipped
    ids[6] = ids[2]                                                       # another row names the same ids, with other values
    vals[6] = -vals[2] + 1.5
    logits = to_dev(base, dt)
    d_ids, d_vals, d_n = torch.from_numpy(ids).cuda(), torch.from_numpy(vals).cuda(), torch.from_numpy(n).cuda()
    out = hip_ops.logits_bias_rows(logits, d_ids, d_vals, d_n)
    assert out.data_ptr() == logits.data_ptr()
    got = to_bits(logits)
    for r in range(rows):
        m = min(max(int(n[r]), 0), cap)
        if m == 0:
            assert np.array_equal(got[r], base[r]), (V, dt, r)            # every bit stays
            continue
        want = hip_ops.logits_bias(to_dev(base[r], dt), d_ids[r, :m].clone(), d_vals[r, :m].clone())
        assert np.array_equal(got[r], to_bits(want)), (V, dt, r)
        assert not np.array_equal(got[r], base[r]), (V, dt, r)
    assert not np.array_equal(got[2], got[6])


# ------------------------------------------------------------------ the tiny golden model
def make_model(golden_dir):
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    g = np.load(golden_dir / "tiny_llama_w4_bf16.npz")
    cfg = json.loads(str(g["config_json"]))
    w = {k[2:]: (codes_dev(g[k]) if g[k].dtype == np.uint32 else to_dev(g[k], DT)) for k in g.files if k.startswith("w:")}
    return g, cfg, Model(ModelArgs(**cfg), w)


@pytest.fixture(scope="module")
def tiny(golden_dir):
    return make_model(golden_dir)


class Req:
    """One request under host orchestration: the single-row ops, in DESIGN.md 12's order, over a Python list of the fed ids."""

    def __init__(self, V, fed, mask=None, bias=None, penalty=1.0, context=60, spec=None, seed=0, calls=0):
        self.V, self.fed, self.mask, self.bias = V, list(fed), mask, bias
        self.penalty, self.context, self.spec, self.seed, self.calls = penalty, context, spec, seed, calls

    def record(self):
        return rec(*(self.spec or (None,)), seed=self.seed, calls=self.calls, penalty=self.penalty, context=self.context)

    def swap(self, other):
        for name in ("mask", "bias", "penalty", "context", "spec", "seed", "calls"):
            a, b = getattr(self, name), getattr(other, name)
            setattr(self, name, b), setattr(other, name, a)

    def tail(self, logits_row, fed_now):
        """-> (token, logprobs bits, processed logits bits) of this row's raw logits after feeding `fed_now`."""
        from proxy_inference_engine_amd import hip_ops
        self.fed += [int(t) for t in fed_now]
        row = logits_row.clone()
        if self.penalty != 1.0:
            hip_ops.logits_penalty(row, dev_ids(self.fed[-self.context:]), self.penalty)
        if self.bias is not None:
            hip_ops.logits_bias(row, dev_ids(self.bias[0]), torch.tensor(self.bias[1], dtype=torch.float32, device="cuda"))
        if self.mask is not None:
            tok, lp = hip_ops.logprobs_argmax_masked(row, torch.from_numpy(pack(self.mask)).cuda())
        else:
            tok, lp = hip_ops.logprobs_argmax(row)
        tok = int(tok.item())
        if self.spec is not None:
            tok = sample_one(lp, self.spec, self.seed, self.calls)[0]
            self.calls += 1
        return tok, f32_bits(lp), to_bits(row)


def request(V, kind, i, fed, tailed, hot):
    """kind 0: mask + penalty + bias; 1: mask only (stochastic with a tail); 2: bias only, penalty exactly 1.0; 3: nothing.  hot: an id the
    bias table names twice (the first entry owns it) -- a fed id, so that with a penalty it is penalised first and biased after."""
    rng = np.random.default_rng(100 + i)
    mask = rng.random(V) < 0.5
    bias = ([int(hot), int(rng.integers(0, V)), int(hot), V + 5], [2.5, -1.25, 50.0, 9.0])       # (the last id is out of range: skipped)
    return Req(V, fed, mask=mask if kind in (0, 1) else None, bias=bias if kind in (0, 2) else None, penalty=1.3 if tailed and kind == 0 else 1.0,
               context=8, spec=("top_k", 0.8, 0.0, 5) if tailed and kind == 1 else None, seed=77 + i, calls=3 * i)


def requests(V, prompts, tailed):
    return [request(V, i % 4, i, p, tailed, p[-1]) for i, p in enumerate(prompts)]


def write_rows(model, be, reqs):
    """The requests' masks and bias tables into the armed buffers, row by row."""
    rows = list(range(len(reqs)))
    model.write_batch_edits(rows, masks=[None if r.mask is None else torch.from_numpy(r.mask) for r in reqs] if be["masks"] is not None else None,
                            biases=[r.bias for r in reqs] if be["bias_ids"] is not None else None)


# ------------------------------------------------------------------ 2. the launch table
@pytest.mark.parametrize("B", [3, 7])              # the fused few-sequence form; the general form
def test_launches_per_step_follow_the_table(golden_dir, B):
    g, cfg, model = make_model(golden_dir)         # a decoder whose setter was never called
    V = cfg["vocab_size"]
    model.enable_paged_kv(num_pages=64)
    prompts = repeating_prompts(V, [5 + 2 * i for i in range(B)], 9)

    def count():
        caches, first = prefilled(model, prompts)
        feed = dev_ids(first)
        for _ in range(3):                         # eager, capture, replay
            feed = model.step_batch(feed, caches)[0].clone()
        for c in caches:
            c[0].page_manager.release()
        return model.batch_graph_launches()

    extra = {(False, "masks"): 0 if B == 7 else 1, (False, "bias"): 1 if B == 7 else 2, (True, "masks"): 0, (True, "bias"): 0}
    for tailed in (False, True):
        if tailed:
            model.set_batch_tail(B)
        try:
            base = count()
            assert base > 0
            for part, kw in (("masks", dict(masks=True)), ("bias", dict(masks=False, bias_cap=4)), ("bias", dict(masks=True, bias_cap=4))):
                model.set_batch_edits(B, **kw)
                assert count() == base + extra[(tailed, part)], (B, tailed, kw)
            model.clear_batch_edits()
            assert count() == base, (B, tailed)    # nothing set: what it launched before the setter was ever called
        finally:
            model.clear_batch_edits()
            model.clear_batch_tail()


# ------------------------------------------------------------------ 3. the batched step with edits
@pytest.mark.parametrize("tailed", [False, True])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("B", [3, 7])
def test_step_batch_with_edits_equals_host_orchestration(tiny, B, graph, tailed):
    from proxy_inference_engine_amd import hip_ops
    g, cfg, model = tiny
    V, steps, swap_at = cfg["vocab_size"], 10, 5
    prompts = repeating_prompts(V, [9, 60, 30, 12, 7, 21, 33][:B], 3)      # (60: the sequence crosses a page boundary during the steps)
    model.clear_batch_tail(), model.clear_batch_edits()
    model.enable_paged_kv(num_pages=48)
    # run B: nothing armed, the single-row ops per row on the host
    caches, first = prefilled(model, prompts)
    hosts, feed, want = requests(V, prompts, tailed), list(first), []
    for st in range(steps):
        if st == swap_at:
            hosts[0].swap(hosts[1])
        _, _, logits = model.step_batch(dev_ids(feed), caches, graph=graph)
        rows = [h.tail(logits[i], [feed[i]]) for i, h in enumerate(hosts)]
        want.append(rows)
        feed = [r[0] for r in rows]
    # run A: fresh caches, the same requests as rows of the armed buffers
    caches, first_a = prefilled(model, prompts)
    assert first_a == first
    reqs = requests(V, prompts, tailed)
    try:
        bt = None
        if tailed:
            bt = model.set_batch_tail(B)
            model.write_batch_tail(list(range(B)), [r.record() for r in reqs], [r.fed for r in reqs])
            ring_ref, dummy = bt["recent"].clone(), torch.zeros((B, V), dtype=torch.bfloat16, device="cuda")
        be = model.set_batch_edits(B, masks=True, bias_cap=6)
        be["masks"].copy_(torch.randint(-2 ** 31, 2 ** 31, be["masks"].shape, dtype=torch.int64).to(torch.int32))   # off rows hold garbage
        write_rows(model, be, reqs)
        replays, feed = model.batch_graph_replays(), dev_ids(first)
        for st in range(steps):
            if st == swap_at:                       # two rows' occupants trade parameters: contents only, every address stays
                reqs[0].swap(reqs[1])
                write_rows(model, be, reqs)
                if tailed:
                    bt["table"][[0, 1]] = bt["table"][[1, 0]]
            if tailed:                              # what pie_logits_penalty_rows alone leaves in the rings
                ctx = torch.tensor([c[0].offset + 1 for c in caches], dtype=torch.int32, device="cuda")
                hip_ops.logits_penalty_rows(dummy, bt["table"], ring_ref, feed.clone(), ctx)
            nxt, lp, lg = model.step_batch(feed, caches, graph=graph)
            assert nxt.tolist() == [r[0] for r in want[st]], st
            for i in range(B):
                assert np.array_equal(to_bits(lg[i]), want[st][i][2]), (st, i, "logits")
                assert np.array_equal(f32_bits(lp[i]), want[st][i][1]), (st, i, "logprobs")
                assert reqs[i].mask is None or reqs[i].mask[int(nxt[i])], (st, i)
            feed = nxt.clone()
        # eager, capture, then replays only -- through the rewritten masks and tables as well
        assert model.batch_graph_replays() - replays == (steps - 2 if graph else 0)
        if tailed:
            assert torch.equal(bt["recent"], ring_ref)
            assert any(h.spec is not None for h in hosts)
    finally:
        model.clear_batch_edits()
        model.clear_batch_tail()


# ------------------------------------------------------------------ 4. the prompt passes
@pytest.mark.parametrize("tailed", [False, True])
def test_prompt_passes_edit_the_row_of_every_prompt(tiny, tailed):
    g, cfg, model = tiny
    V = cfg["vocab_size"]
    pd0, pd1, p9, p20 = repeating_prompts(V, [20, 11, 9, 20], 5)
    model.clear_batch_tail(), model.clear_batch_edits()
    model.enable_paged_kv(num_pages=48)

    def four():
        # decode rows 0 and 1: bias only / mask + penalty + bias; prompt rows 2 and 3: mask only (stochastic) / mask + penalty + bias
        return [request(V, 2, 0, pd0, tailed, pd0[0]), request(V, 0, 1, pd1, tailed, pd1[-1]), request(V, 1, 2, [], tailed, 1),
                request(V, 0, 3, [], tailed, p20[-1])]

    def fresh():
        return [model.make_cache(), model.make_cache()]

    # host orchestration on the unarmed passes
    hosts = four()
    _, _, logits = model.prefill_batch([p9, p20], fresh())
    want_pf = [hosts[2].tail(logits[0], p9), hosts[3].tail(logits[1], p20)]
    hosts = four()
    dcs, dtoks = prefilled(model, [pd0, pd1])
    _, _, logits = model.step_mixed(dev_ids(dtoks), dcs, [p9, p20], fresh())
    want_mx = [hosts[0].tail(logits[0], [dtoks[0]]), hosts[1].tail(logits[1], [dtoks[1]]), hosts[2].tail(logits[2], p9), hosts[3].tail(logits[3], p20)]
    try:
        reqs = four()
        if tailed:
            model.set_batch_tail(4)
            model.write_batch_tail([0, 1], [reqs[2].record(), reqs[3].record()], [p9, p20])
        be = model.set_batch_edits(4, masks=True, bias_cap=4)
        write_rows(model, be, reqs[2:])
        nxt, lp, lg = model.prefill_batch([p9, p20], fresh())
        for i in range(2):
            assert int(nxt[i]) == want_pf[i][0] and reqs[2 + i].mask[int(nxt[i])], i
            assert np.array_equal(f32_bits(lp[i]), want_pf[i][1]) and np.array_equal(to_bits(lg[i]), want_pf[i][2]), i
        dcs, dtoks2 = prefilled(model, [pd0, pd1])
        assert dtoks2 == dtoks
        if tailed:
            model.write_batch_tail([0, 1, 2, 3], [r.record() for r in reqs], [pd0, pd1, p9, p20])
        write_rows(model, be, reqs)
        nxt, lp, lg = model.step_mixed(dev_ids(dtoks), dcs, [p9, p20], fresh())
        for i in range(4):
            assert int(nxt[i]) == want_mx[i][0], i
            assert np.array_equal(f32_bits(lp[i]), want_mx[i][1]) and np.array_equal(to_bits(lg[i]), want_mx[i][2]), i
            assert reqs[i].mask is None or reqs[i].mask[int(nxt[i])], i
    finally:
        model.clear_batch_edits()
        model.clear_batch_tail()


# ------------------------------------------------------------------ 5. BatchedEngine.generate
def test_engine_generates_with_per_request_edits(tiny):
    from proxy_inference_engine_amd import InferenceEngine
    from proxy_inference_engine_amd.engine import BatchedEngine, SamplingParams
    g, cfg, model = tiny
    V, new = cfg["vocab_size"], 8
    model.clear_batch_tail(), model.clear_batch_edits()
    prompts = repeating_prompts(V, [12, 70, 5, 33, 64], 11)
    static = np.random.default_rng(1).random(V) < 0.4
    topk_mask = np.random.default_rng(2).random(V) < 0.25
    seen = []

    def grammar(tokens):
        seen.append(list(tokens))
        return [(int(tokens[-1]) + 1) % V, (int(tokens[-1]) + 2) % V]

    plain = BatchedEngine(model, num_pages=48, max_batch=3).generate(prompts, new)
    target = next(t for t in (123, 124, 125) if t not in plain[2])
    params = [SamplingParams(token_mask=torch.from_numpy(static)), SamplingParams(token_mask=grammar), SamplingParams(logit_bias={target: 100.0}),
              SamplingParams(), SamplingParams(temp=0.8, top_k=5, seed=21, token_mask=torch.from_numpy(topk_mask))]
    assert [sp.plain for sp in params] == [False, False, False, True, False]

    def check(prompts, plain, out, maps=None):
        assert [len(o) for o in out] == [new] * 5
        assert all(static[t] for t in out[0]) and all(topk_mask[t] for t in out[4])
        fed = list(prompts[1])
        for t in out[1]:
            assert t in ((fed[-1] + 1) % V, (fed[-1] + 2) % V)
            fed.append(t)
        assert out[2] == [target] * new
        assert out[3] == plain[3]                                          # the unconstrained greedy request: a run with no edits at all
        # the callable saw the prompt alone first, then the prompt plus every generated token
        mine = [s for s in seen if s[:len(prompts[1])] == prompts[1]]
        assert mine[-new:] == [prompts[1] + out[1][:i] for i in range(new)]
        if maps is None:
            return
        for r, allowed in ((0, static), (4, topk_mask)):
            for m in maps[r]:
                assert all(allowed[t] for t, v in m.items() if np.isfinite(v)), r
        fed = list(prompts[1])
        for t, m in zip(out[1], maps[1]):
            assert {k for k, v in m.items() if np.isfinite(v)} <= {(fed[-1] + 1) % V, (fed[-1] + 2) % V}
            fed.append(t)

    one = BatchedEngine(model, num_pages=48, max_batch=3).generate(prompts, new, sampling=params)
    check(prompts, plain, one)
    assert len(seen) == new and model._batch_edits is None and model._batch_tail is None   # one call per token; both cleared on the way out
    # the same requests on one sequence
    try:
        for r, kw in ((0, dict(token_mask=torch.from_numpy(static))), (1, dict(token_mask=grammar)), (2, dict(logit_bias={target: 100.0}))):
            single = InferenceEngine(model=model)
            single.prepare_engine(prompts[r], temp=0, **kw)
            gen = single.generate_step(torch.tensor(prompts[r]))
            assert [int(next(gen)[0].item()) for _ in range(new)] == one[r], r
    finally:
        model.set_step_tail()
    out, maps = BatchedEngine(model, num_pages=48, max_batch=3).generate(prompts, new, sampling=params, logprobs=True, top_logprobs=5)
    assert out == one
    check(prompts, plain, out, maps)
    # Chunked prefill and a shared prefix seat the same requests in other rows of other passes.  Such a run repeats itself and keeps every
    # property above; it is not compared token by token with the run above, whose prompt rows went through other kernels (the engine's
    # own chunked runs agree with its plain ones only up to low-margin steps: tests/test_gpu_paged.py).
    shared = [prompts[1][:66] + p for p in prompts]
    for kw, ps in ((dict(prefill_chunk=4), prompts), (dict(share_prefix=True), shared)):
        v_plain = BatchedEngine(model, num_pages=64, max_batch=3, **kw).generate(ps, new)
        a = BatchedEngine(model, num_pages=64, max_batch=3, **kw).generate(ps, new, sampling=params)
        check(ps, v_plain, a)
        b, maps = BatchedEngine(model, num_pages=64, max_batch=3, **kw).generate(ps, new, sampling=params, logprobs=True, top_logprobs=5)
        assert a == b, kw
        check(ps, v_plain, b, maps)


# ------------------------------------------------------------------ 6. refusals, each before any launch
def test_refusals(tiny):
    from proxy_inference_engine_amd import _ffi
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    from proxy_inference_engine_amd.tp import HipComm
    from tests.test_gpu_tp import CFG
    g, cfg, model = tiny
    lib, V = _ffi.load(), cfg["vocab_size"]
    W = (V + 31) // 32
    model.clear_batch_tail(), model.clear_batch_edits()
    model.enable_paged_kv(num_pages=16)
    prompts = repeating_prompts(V, [9, 20, 30], 3)
    caches, first = prefilled(model, prompts)
    model.step_batch(dev_ids(first), caches, graph=False)                   # (the B = 3 buffers exist from here on)
    be = model.set_batch_edits(2, masks=True, bias_cap=4)
    try:
        # more rows than rows_cap
        buf = model._batch_bufs[3]
        buf["next"].fill_(-9), buf["logprobs"].fill_(7.0)
        offsets = [c[0].offset for c in caches]
        with pytest.raises(ValueError, match="rows_cap"):
            model.step_batch(dev_ids(first), caches, graph=False)
        torch.cuda.synchronize()
        assert buf["next"].tolist() == [-9] * 3 and bool((buf["logprobs"] == 7.0).all())     # nothing ran
        assert [c[0].offset for c in caches] == offsets
        with pytest.raises(ValueError, match="rows_cap"):
            model.prefill_batch(prompts, [model.make_cache() for _ in prompts])
        with pytest.raises(ValueError, match="rows_cap"):
            model.step_mixed(dev_ids(first[:1]), caches[:1], prompts[:2], [model.make_cache(), model.make_cache()])
        # the setter's own checks; the edits that were set stay
        m, on, bi, bv, bn = (_ffi.p(be[k]) for k in ("masks", "mask_on", "bias_ids", "bias_vals", "bias_n"))
        off = lambda t, k: C.c_void_p(t.data_ptr() + k)
        call = lambda *a: lib.pie_decoder_set_batch_logits_edits(model._dec, *a)
        assert call(2, m, W - 1, on, bi, bv, bn, 4) == -2                   # mask_words < ceil(V / 32)
        for cap in (-1, 1025):
            assert call(2, m, W, on, bi, bv, bn, cap) == -1
        assert call(-1, m, W, on, bi, bv, bn, 4) == -1
        assert call(2, None, 0, None, None, None, None, 0) == -1            # neither part
        assert call(2, m, W, None, bi, bv, bn, 4) == -1 and call(2, None, 0, on, bi, bv, bn, 4) == -1
        assert call(2, m, W, on, None, bv, bn, 4) == -1 and call(2, m, W, on, bi, None, bn, 4) == -1 and call(2, m, W, on, bi, bv, None, 4) == -1
        for args in ((off(be["masks"], 2), W, on, bi, bv, bn), (m, W, off(be["mask_on"], 2), bi, bv, bn), (m, W, on, off(be["bias_ids"], 2), bv, bn),
                     (m, W, on, bi, off(be["bias_vals"], 1), bn), (m, W, on, bi, bv, off(be["bias_n"], 3))):
            assert call(2, *args, 4) == -3, args
        with pytest.raises(ValueError, match="rows_cap"):                   # (still armed with 2 rows)
            model.step_batch(dev_ids(first), caches, graph=False)
        # an all-zero mask is refused on the host; the rows named with it are not written
        before = be["mask_on"].clone()
        with pytest.raises(ValueError, match="no token is allowed"):
            model.write_batch_edits([0, 1], masks=[torch.ones(V, dtype=torch.bool), torch.zeros(W, dtype=torch.int32)])
        with pytest.raises(ValueError, match="no token is allowed"):
            model.write_batch_edits([0], masks=[[]])
        assert torch.equal(be["mask_on"], before)
        with pytest.raises(ValueError):
            model.write_batch_edits([0], biases=[((1, 2, 3, 4, 5), (0.0,) * 5)])   # more entries than bias_cap
        # the ops' checks
        lg = torch.zeros((2, V), dtype=torch.bfloat16, device="cuda")
        lp, tk = torch.zeros((2, V), device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
        rm = lambda *a: lib.pie_logprobs_argmax_rows_masked(_ffi.p(lg), *a, _ffi.p(lp), _ffi.p(tk), _ffi.stream())
        assert rm(2, V, 1, m, W - 1, on) == -2 and rm(0, V, 1, m, W, on) == -1 and rm(2, V, 1, off(be["masks"], 2), W, on) == -3
        assert rm(2, V, 1, m, W, off(be["mask_on"], 1)) == -3 and rm(2, V, 1, m, W, None) == -1 and rm(2, V, 7, m, W, on) == -1
        br = lambda rows, ids, vals, n, cap: lib.pie_logits_bias_rows(_ffi.p(lg), rows, V, 1, ids, vals, n, cap, _ffi.stream())
        assert br(2, bi, bv, bn, 0) == -1 and br(2, bi, bv, bn, 1025) == -1 and br(0, bi, bv, bn, 4) == -1
        assert br(2, off(be["bias_ids"], 2), bv, bn, 4) == -3 and br(2, bi, bv, off(be["bias_n"], 2), 4) == -3 and br(2, bi, None, bn, 4) == -1
        torch.cuda.synchronize()
        assert not lg.any() and not lp.any()                                # nothing ran
    finally:
        model.clear_batch_edits()
    nxt, _, _ = model.step_batch(dev_ids(first), caches, graph=False)       # off again: the step takes three rows
    assert nxt.shape == (3,)
    with pytest.raises(RuntimeError):
        model.write_batch_edits([0], masks=[[1]])                           # nothing is armed
    with pytest.raises(ValueError):
        model.set_batch_edits(2, masks=False, bias_cap=0)
    # a tensor-parallel decoder's tail is vocabulary-parallel: the setter is refused
    w = po.synth_checkpoint(CFG, seed=72, dtype=DT, lm_head_gain=4.0)
    dev_w = {k: (codes_dev(v) if v.dtype == np.uint32 else to_dev(v, DT)) for k, v in w.items()}
    comm = HipComm(CFG["hidden_size"], backend="ipc")
    try:
        tp = Model(ModelArgs(**CFG), dev_w, tp=comm)
        assert lib.pie_decoder_set_batch_logits_edits(tp._dec, 2, m, W, on, bi, bv, bn, 4) == -5
        assert b"pie_decoder_set_batch_logits_edits" in lib.pie_last_error()
        assert lib.pie_decoder_set_batch_logits_edits(tp._dec, 0, None, 0, None, None, None, None, 0) == -5
        with pytest.raises(RuntimeError):
            tp.set_batch_edits(2)
        del tp
    finally:
        comm.close()
