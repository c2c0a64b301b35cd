"""-m gpu: per-row samplers and repetition penalties in the multi-sequence passes against the single-row ops they are
defined by -- pie_sample, pie_logits_penalty, pie_logprobs_argmax (themselves pinned to tests/sampler_reference.py and the oracle by
tests/test_gpu_sampler.py, test_gpu_logits_tail.py and test_gpu_step_tail.py).  Every comparison is exact: a row of pie_sample_rows IS a
one-row pie_sample with counter {calls, 0}, a row of pie_logits_penalty_rows IS pie_logits_penalty over the window its ring holds, and
the passes' tail is those two around the unchanged log-softmax."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests import sampler_rows as sr
from tests._util import codes_dev, to_bits, to_dev

pytestmark = pytest.mark.gpu
DT = "bfloat16"
UNKNOWN_MODE = 17


def rec(mode=None, temp=1.0, p=0.0, k=0, seed=0, calls=0, penalty=1.0, context=60):
    from proxy_inference_engine_amd import hip_ops
    return hip_ops.row_tail_pack(mode, temp, p, k, seed=seed, calls=calls, penalty=penalty, context_size=context)


def upload(records) -> torch.Tensor:
    from proxy_inference_engine_amd import hip_ops
    return hip_ops.row_tail_table(records, "cuda")


def download(table: torch.Tensor) -> list:
    from proxy_inference_engine_amd import _ffi
    raw = table.cpu().numpy().tobytes()
    n = C.sizeof(_ffi.pie_row_tail)
    return [_ffi.pie_row_tail.from_buffer_copy(raw[i * n:(i + 1) * n]) for i in range(table.shape[0])]


def f32_bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy().view(np.uint32).copy()


def dev_ids(ids) -> torch.Tensor:
    return torch.tensor([int(i) for i in ids], dtype=torch.int32, device="cuda")


def sample_one(lp: torch.Tensor, spec, seed: int, calls: int):
    """The yardstick: pie_sample on ONE row with counter {calls, 0}.  spec = (mode name, temp, p, k).  -> (token, kept count, kept mask)."""
    from proxy_inference_engine_amd import _ffi, hip_ops
    lp = lp.reshape(1, -1).contiguous()
    V = lp.shape[1]
    counter = torch.tensor([calls, 0], dtype=torch.int64, device="cuda")
    ws = hip_ops.sample_workspace(lp.device, 1, V)
    tok = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    kept = torch.zeros(1, dtype=torch.int32, device="cuda")
    mask = torch.zeros((1, V), dtype=torch.uint8, device="cuda")
    _ffi.check(_ffi.load().pie_sample(_ffi.p(lp), 1, V, hip_ops.SAMPLE_MODES[spec[0]], float(spec[1]), float(spec[2]), int(spec[3]), int(seed), _ffi.p(counter),
                                      _ffi.p(ws), _ffi.p(tok), _ffi.p(kept), _ffi.p(mask), _ffi.stream()))
    assert counter.tolist() == [calls + 1, 0]
    return int(tok.item()), int(kept.item()), mask[0].cpu().numpy()


# ------------------------------------------------------------------ 1. pie_sample_rows
def seven_rows(V):
    """7 designed rows (ties at the top-k boundary, across the top-p threshold, an all -inf row) and 7 records: greedy, categorical, top-k,
    top-p, min-p keeping one, min-p with min_tokens_to_keep = 5, an unknown mode; distinct seeds and starting counters."""
    rows = [sr.quantized(V, 1, temp=0.7), sr.wide_tie(V, 2), sr.wide_tie(V, 3), sr.topp_tie(V, 4), sr.all_inf(V), sr.quantized(V, 5), sr.topp_tie(V, 6)]
    lp = torch.from_numpy(np.stack([r.lp for r in rows])).cuda()
    specs = [None, ("categorical", 1.0, 0.0, 0), ("top_k", 0.8, 0.0, rows[2].top_k), ("top_p", 1.0, rows[3].top_p, 0), ("min_p", 1.0, 0.1, 1),
             ("min_p", 0.7, 0.05, 5), "unknown"]
    records = []
    for i, spec in enumerate(specs):
        r = rec(*(spec if isinstance(spec, tuple) else (None,)), seed=0x9E3779B97F4A7C15 * (i + 1) & (2 ** 64 - 1), calls=3 + 7 * i)
        if spec == "unknown":
            r = rec("categorical", seed=77, calls=5)
            r.mode = UNKNOWN_MODE
        records.append(r)
    return lp, specs, records


@pytest.mark.parametrize("V", [512, 1500, 4099])   # one slice; three slices, the last ragged; a last slice of 3 ids
def test_sample_rows_is_a_one_row_pie_sample_per_row(V):
    from proxy_inference_engine_amd import _ffi, hip_ops
    lp, specs, records = seven_rows(V)
    n = len(records)
    ws = torch.zeros(int(_ffi.load().pie_sample_workspace_bytes(n, V)) // 8, dtype=torch.int64, device="cuda")   # ONE workspace for all three calls
    order = list(range(n))                            # slot s holds records[order[s]]
    for call in range(3):
        table = upload([records[order[s]] for s in range(n)])
        preset = torch.arange(-5, -5 - n, -1, dtype=torch.int32, device="cuda")
        tokens, kept, mask = hip_ops.sample_rows(lp, table, tokens=preset.clone(), workspace=ws, want_mask=True)
        after = download(table)
        tokens, kept, mask = tokens.tolist(), kept.tolist(), mask.cpu().numpy()
        for s in range(n):
            spec, before = specs[order[s]], records[order[s]]
            what = (V, call, s, spec)
            if not isinstance(spec, tuple):           # greedy, unknown mode: the row is left alone
                assert tokens[s] == -5 - s and kept[s] == 0 and not mask[s].any(), what
                assert bytes(after[s]) == bytes(before), what
                continue
            tok, cnt, m = sample_one(lp[s], spec, before.seed, before.calls)
            assert tokens[s] == tok and kept[s] == cnt, what
            assert np.array_equal(mask[s], m), what
            assert after[s].calls == before.calls + 1, what
            before.calls += 1                         # the request's stream moves on, wherever it sits next
            assert bytes(after[s]) == bytes(before), what
        # the header word the next k_smp_init relies on is zero for EVERY row, whatever the row just ran
        words = ws.numel() // n
        assert ws.view(n, words)[:, 0].tolist() == [0] * n
        order = order[2:] + order[:2]                 # slot 0: greedy -> top-k -> min-p; slot 5: min-p -> unknown -> categorical; ...
        if call == 1:
            order = list(range(n))                    # ... and back: slot 0 is greedy again, slot 2 top-k again


def test_a_rows_draw_does_not_depend_on_its_slot():
    from proxy_inference_engine_amd import hip_ops
    V = 1500
    lp, specs, records = seven_rows(V)
    mine, row = rec("top_k", 0.8, 0.0, 40, seed=4242, calls=11), lp[1:2].contiguous()
    alone = hip_ops.sample_rows(row, upload([mine]), workspace=torch.zeros_like(hip_ops.sample_workspace("cuda", 1, V)), want_mask=True)
    block = lp.clone()
    block[5] = row[0]
    others = [rec("categorical", seed=1 + i, calls=i) for i in range(7)]
    others[5] = mine
    among = hip_ops.sample_rows(block, upload(others), workspace=torch.zeros_like(hip_ops.sample_workspace("cuda", 7, V)), want_mask=True)
    assert int(alone[0][0]) == int(among[0][5]) and int(alone[1][0]) == int(among[1][5]) == 40
    assert torch.equal(alone[2][0], among[2][5])
    assert int(alone[0][0]) == sample_one(row, ("top_k", 0.8, 0.0, 40), 4242, 11)[0]


# ------------------------------------------------------------------ 2. pie_logits_penalty_rows
@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("gather", [False, True])
def test_logits_penalty_rows_is_the_single_row_op_per_row(dt, gather):
    from proxy_inference_engine_amd import hip_ops
    V, n = 512, 5
    rng = np.random.default_rng(len(dt) + gather)
    base = po.to_bits((rng.standard_normal((n, V)) * 6).astype(np.float32), dt)
    base[:, :4] = np.array([0x0000, 0x8000, 0xFC00 if dt == "float16" else 0xFF80, 0x0001], np.uint16)     # +-0, -inf, a denormal: penalised below
    #            penalty, context, pos (ctx - 1), input id
    cases = [(1.0, 60, 700, 9),      # no penalty: the logits stay bit for bit
             (1.3, 60, -1, 11),      # an idle slot (ctx = 0)
             (1.3, 60, 2, 0),        # a window shorter than the context
             (1.8, 1024, 1500, 1),   # the ring wraps
             (0.5, 30, 40, 2)]       # repeated ids and ids outside [0, V)
    ring = np.full((n, 1024), -3, np.int32)
    for s, (_, _, pos, _) in enumerate(cases):
        for q in range(max(0, pos - 1023), max(pos, 0)):
            ring[s, q & 1023] = int(rng.integers(0, V)) if s != 3 else int(rng.integers(0, 300))
    ring[4, 12:40] = np.resize(np.array([3, 3, -1, V, 7, 3, V + 100, 0, 7, -2 ** 31, 2 ** 31 - 1, 2], np.int32), 28)
    ring0 = ring.copy()
    table = upload([rec(penalty=p, context=c) for p, c, _, _ in cases])
    ids = np.array([c[3] for c in cases], np.int32)
    ctx = np.array([c[2] + 1 for c in cases], np.int32)
    out_rows = None
    if gather:                                        # the prompt passes' form: output row s reads source row out_rows[s] of longer arrays
        src = np.array([7, 2, 9, 0, 4], np.int32)
        big_ids, big_ctx = np.full(10, 5, np.int32), np.full(10, 33, np.int32)
        big_ids[src], big_ctx[src] = ids, ctx
        ids, ctx, out_rows = big_ids, big_ctx, dev_ids(src)
    logits, ring_dev = to_dev(base, dt), torch.from_numpy(ring).cuda()
    out = hip_ops.logits_penalty_rows(logits, table, ring_dev, dev_ids(ids), dev_ids(ctx), out_rows)
    assert out.data_ptr() == logits.data_ptr()
    got, ring = to_bits(logits), ring_dev.cpu().numpy()
    for s, (penalty, context, pos, tok) in enumerate(cases):
        if pos < 0:
            assert np.array_equal(ring[s], ring0[s]) and np.array_equal(got[s], base[s])
            continue
        assert ring[s, pos & 1023] == tok                                  # the row's own input id was recorded first
        changed = ring[s] != ring0[s]
        assert changed.sum() <= 1 and not np.delete(changed, pos & 1023).any()
        if penalty == 1.0:
            assert np.array_equal(got[s], base[s])
            continue
        window = [int(ring[s, q & 1023]) for q in range(max(0, pos + 1 - context), pos + 1)]
        assert len(window) == min(context, pos + 1)
        want = hip_ops.logits_penalty(to_dev(base[s], dt), dev_ids(window), penalty)
        assert np.array_equal(got[s], to_bits(want)), (dt, s)
        assert not np.array_equal(got[s], base[s]), (dt, s)
    assert len(set(w for w in ring[4, 11:41].tolist())) < 30              # (the last case's window does repeat ids)


# ------------------------------------------------------------------ the tiny golden model
@pytest.fixture(scope="module")
def tiny(golden_dir):
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    g = np.load(golden_dir / "tiny_llama_w4_bf16.npz")
    cfg = json.loads(str(g["config_json"]))
    w = {k[2:]: (codes_dev(g[k]) if g[k].dtype == np.uint32 else to_dev(g[k], DT)) for k in g.files if k.startswith("w:")}
    return g, cfg, Model(ModelArgs(**cfg), w)


class HostRow:
    """One request under host orchestration: today's single-row ops over a Python list of the fed ids."""

    def __init__(self, spec, seed, calls, penalty, context, fed):
        self.spec, self.seed, self.calls, self.penalty, self.context, self.fed = spec, seed, calls, penalty, context, list(fed)

    def record(self):
        return rec(*(self.spec or (None,)), seed=self.seed, calls=self.calls, penalty=self.penalty, context=self.context)

    def tail(self, logits_row: torch.Tensor, fed_now):
        """-> (token, logprobs bits, processed logits bits) for this row's raw logits after feeding `fed_now`."""
        from proxy_inference_engine_amd import hip_ops
        self.fed += [int(t) for t in fed_now]
        row = logits_row.clone()
        if self.penalty != 1.0:
            hip_ops.logits_penalty(row, dev_ids(self.fed[-self.context:]), self.penalty)
        tok, lp = hip_ops.logprobs_argmax(row)
        tok = int(tok.item())
        if self.spec is not None:
            tok = sample_one(lp, self.spec, self.seed, self.calls)[0]
            self.calls += 1
        return tok, f32_bits(lp), to_bits(row)


def three_requests(prompts):
    return [HostRow(None, 1, 0, 1.3, 8, prompts[0]),                              # greedy + penalty 1.3 over 8
            HostRow(("top_k", 0.8, 0.0, 5), 0xABCDEF0123, 4, 1.0, 60, prompts[1]),   # top-k 5 at temp 0.8
            HostRow(("top_p", 1.0, 0.9, 0), 99, 0, 1.1, 60, prompts[2])]           # top-p 0.9 + penalty 1.1 over 60


def repeating_prompts(vocab, lens, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, vocab, n).astype(np.int32)[rng.integers(0, max(n // 2, 1), n)].tolist() for n in lens]   # ids drawn from half as many: repeats


def prefilled(model, prompts):
    caches, toks = [], []
    for p in prompts:
        c = model.make_cache()
        tok, _, _ = model.step(dev_ids(p), c)
        caches.append(c), toks.append(int(tok.item()))
    return caches, toks


# ------------------------------------------------------------------ 3. the batched step with a tail
@pytest.mark.parametrize("graph", [False, True])
def test_step_batch_with_a_tail_equals_host_orchestration(tiny, graph):
    g, cfg, model = tiny
    V, steps, swap_at = cfg["vocab_size"], 12, 6
    prompts = repeating_prompts(V, [9, 63, 30], 3)                          # (63: the sequence crosses a page boundary during the steps)
    model.clear_batch_tail()
    model.enable_paged_kv(num_pages=16)
    # run B: no tail, the single-row ops per row on the host
    caches, first = prefilled(model, prompts)
    hosts, feed, want = three_requests(prompts), list(first), []
    for st in range(steps):
        if st == swap_at:
            for name in ("spec", "seed", "calls", "penalty", "context"):
                a, b = getattr(hosts[1], name), getattr(hosts[2], name)
                setattr(hosts[1], name, b), setattr(hosts[2], name, a)
        _, _, logits = model.step_batch(dev_ids(feed), caches, graph=graph)
        rows = [h.tail(logits[i], [feed[i]]) for i, h in enumerate(hosts)]
        want.append(rows)
        feed = [r[0] for r in rows]
    # run A: fresh caches, the same requests as records of the tail
    caches, first_a = prefilled(model, prompts)
    assert first_a == first
    reqs = three_requests(prompts)
    bt = model.set_batch_tail(3)
    try:
        model.write_batch_tail([0, 1, 2], [r.record() for r in reqs], [r.fed for r in reqs])
        replays, feed = model.batch_graph_replays(), dev_ids(first)
        for st in range(steps):
            if st == swap_at:                                               # two rows' records trade places: contents only, the addresses stay
                bt["table"][[1, 2]] = bt["table"][[2, 1]]
            nxt, lp, lg = model.step_batch(feed, caches, graph=graph)
            assert nxt.tolist() == [r[0] for r in want[st]], st
            for i in range(3):
                assert np.array_equal(to_bits(lg[i]), want[st][i][2]), (st, i, "logits")
                assert np.array_equal(f32_bits(lp[i]), want[st][i][1]), (st, i, "logprobs")
            feed = nxt.clone()
        # eager, capture, then replays only -- through the swap as well
        assert model.batch_graph_replays() - replays == (steps - 2 if graph else 0)
        got = download(bt["table"])
        assert [r.calls for r in got] == [h.calls if h.spec else r.calls for h, r in zip(hosts, got)]
    finally:
        model.clear_batch_tail()


# ------------------------------------------------------------------ 4. the prompt passes
def test_prompt_passes_draw_first_tokens_per_record(tiny):
    g, cfg, model = tiny
    V = cfg["vocab_size"]
    p7, p70, pd = repeating_prompts(V, [7, 70, 20], 5)                      # 70: crosses a page; the third decodes
    model.clear_batch_tail()
    model.enable_paged_kv(num_pages=24)

    def requests():
        return [HostRow(("categorical", 1.0, 0.0, 0), 5, 2, 1.3, 8, pd), HostRow(("top_k", 0.8, 0.0, 5), 6, 0, 1.0, 60, []),
                HostRow(("top_p", 1.0, 0.9, 0), 7, 0, 1.1, 60, [])]

    # host orchestration on the untailed passes
    hosts = requests()
    caches = [model.make_cache(), model.make_cache()]
    _, _, logits = model.prefill_batch([p7, p70], caches)
    want_pf = [hosts[1].tail(logits[0], p7), hosts[2].tail(logits[1], p70)]
    hosts = requests()
    (dc,), (dtok,) = prefilled(model, [pd])
    caches = [model.make_cache(), model.make_cache()]
    _, _, logits = model.step_mixed(dev_ids([dtok]), [dc], [p7, p70], caches)
    want_mx = [hosts[0].tail(logits[0], [dtok]), hosts[1].tail(logits[1], p7), hosts[2].tail(logits[2], p70)]
    # the same passes with the tail set
    model.set_batch_tail(4)
    try:
        reqs = requests()
        model.write_batch_tail([0, 1], [reqs[1].record(), reqs[2].record()], [p7, p70])
        caches = [model.make_cache(), model.make_cache()]
        nxt, lp, lg = model.prefill_batch([p7, p70], caches)
        for i in range(2):
            assert int(nxt[i]) == want_pf[i][0], i
            assert np.array_equal(f32_bits(lp[i]), want_pf[i][1]) and np.array_equal(to_bits(lg[i]), want_pf[i][2]), i
        (dc,), (dtok2,) = prefilled(model, [pd])
        assert dtok2 == dtok
        model.write_batch_tail([0, 1, 2], [r.record() for r in reqs], [pd, p7, p70])
        caches = [model.make_cache(), model.make_cache()]
        nxt, lp, lg = model.step_mixed(dev_ids([dtok]), [dc], [p7, p70], caches)
        for i in range(3):
            assert int(nxt[i]) == want_mx[i][0], i
            assert np.array_equal(f32_bits(lp[i]), want_mx[i][1]) and np.array_equal(to_bits(lg[i]), want_mx[i][2]), i
    finally:
        model.clear_batch_tail()


# ------------------------------------------------------------------ 5. BatchedEngine.generate(sampling=...)
def engine_case(V):
    from proxy_inference_engine_amd.engine import SamplingParams
    prompts = repeating_prompts(V, [12, 70, 5, 33, 64], 11)
    params = [SamplingParams(temp=0.8, top_k=5, seed=21), SamplingParams(), SamplingParams(temp=1.0, top_p=0.9, repetition_penalty=1.1, seed=22),
              SamplingParams(repetition_penalty=1.3, repetition_context_size=8), SamplingParams(temp=0.7, min_p=0.05, min_tokens_to_keep=2, seed=23)]
    return prompts, params


def test_engine_generates_with_per_request_sampling(tiny):
    from proxy_inference_engine_amd.engine import BatchedEngine, SamplingParams
    g, cfg, model = tiny
    prompts, params = engine_case(cfg["vocab_size"])
    eng = BatchedEngine(model, num_pages=32, max_batch=2)
    greedy = eng.generate(prompts, 10)
    eng.stop_tokens = {greedy[1][3], greedy[3][6]}                          # different stop lengths: rows free up at different passes
    greedy = eng.generate(prompts, 10)
    assert len(greedy[1]) <= 4 and len({len(o) for o in greedy}) > 1
    one = eng.generate(prompts, 10, sampling=params)
    two = eng.generate(prompts, 10, sampling=params)
    assert one == two                                                       # seeded: two identical runs
    assert one[1] == greedy[1]                                              # temp = 0, penalty = 1: today's greedy tokens
    assert eng.generate(prompts, 10, sampling=SamplingParams()) == greedy
    assert any(a != b for a, b in zip(one, greedy))                         # (the records did something)
    assert all(0 <= t < cfg["vocab_size"] for o in one for t in o)
    assert model._batch_tail is None
    # a request's stream is its own: first or last in the queue of a one-slot engine
    solo = BatchedEngine(model, num_pages=32, max_batch=1, stop_tokens=eng.stop_tokens)
    first = solo.generate([prompts[0]] + prompts[1:], 10, sampling=[params[0]] + params[1:])
    last = solo.generate(prompts[1:] + [prompts[0]], 10, sampling=params[1:] + [params[0]])
    assert first[0] == last[-1] and first[1:] == last[:-1]


@pytest.mark.parametrize("kw", [dict(kv_dtype=torch.int8), dict(prefill_chunk=16), dict(share_prefix=True)])
def test_engine_variants_repeat_themselves(tiny, kw):
    from proxy_inference_engine_amd.engine import BatchedEngine
    g, cfg, model = tiny
    prompts, params = engine_case(cfg["vocab_size"])
    if kw.get("share_prefix"):
        prompts = [prompts[1][:66] + p for p in prompts]
    try:
        eng = BatchedEngine(model, num_pages=40, max_batch=2, **kw)
        one = eng.generate(prompts, 8, sampling=params)
        assert one == eng.generate(prompts, 8, sampling=params)
        assert [len(o) for o in one] == [8] * 5
        assert one[1] == eng.generate(prompts, 8)[1]                        # the plain request among them: today's tokens
    finally:
        model.enable_paged_kv(num_pages=16)                                 # (back to T pages for whoever uses the fixture next)


# ------------------------------------------------------------------ 6. refusals, each before any launch
def test_refusals(tiny):
    from proxy_inference_engine_amd import _ffi, hip_ops
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    from proxy_inference_engine_amd.tp import HipComm
    from tests.test_gpu_tp import CFG
    g, cfg, model = tiny
    lib = _ffi.load()
    model.clear_batch_tail()
    model.enable_paged_kv(num_pages=16)
    prompts = repeating_prompts(cfg["vocab_size"], [9, 20, 30], 3)
    caches, first = prefilled(model, prompts)
    model.step_batch(dev_ids(first), caches, graph=False)                   # (the B = 3 buffers exist from here on)
    bt = model.set_batch_tail(2)
    try:
        # more rows than records
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
        # misaligned workspace / table / ring: refused, and the tail that was set stays
        args = [_ffi.p(bt["table"]), 2, _ffi.p(bt["recent"]), _ffi.p(bt["ws"])]
        assert lib.pie_decoder_set_batch_tail(model._dec, args[0], 2, args[2], C.c_void_p(bt["ws"].data_ptr() + 4)) == -3
        assert lib.pie_decoder_set_batch_tail(model._dec, C.c_void_p(bt["table"].data_ptr() + 4), 2, args[2], args[3]) == -3
        assert lib.pie_decoder_set_batch_tail(model._dec, args[0], 2, C.c_void_p(bt["recent"].data_ptr() + 2), args[3]) == -3
        assert lib.pie_decoder_set_batch_tail(model._dec, args[0], 0, args[2], args[3]) == -2
        assert lib.pie_decoder_set_batch_tail(model._dec, args[0], 2, None, args[3]) == -1
        with pytest.raises(ValueError, match="rows_cap"):                   # (still armed with 2 rows)
            model.step_batch(dev_ids(first), caches, graph=False)
        lp = torch.zeros((2, 512), dtype=torch.float32, device="cuda")
        assert lib.pie_sample_rows(_ffi.p(lp), 2, 512, args[0], C.c_void_p(bt["ws"].data_ptr() + 4), _ffi.p(buf["next"]), None, None, _ffi.stream()) == -3
        assert lib.pie_sample_rows(_ffi.p(lp), 2, 1024 * 512 + 1, args[0], args[3], _ffi.p(buf["next"]), None, None, _ffi.stream()) == -2
    finally:
        model.clear_batch_tail()
    nxt, _, _ = model.step_batch(dev_ids(first), caches, graph=False)       # off again: the step takes three rows
    assert nxt.shape == (3,)
    # a tensor-parallel decoder's tail is vocabulary-parallel: the setter is refused
    w = po.synth_checkpoint(CFG, seed=72, dtype=DT, lm_head_gain=4.0)
    dev_w = {k: (codes_dev(v) if v.dtype == np.uint32 else to_dev(v, DT)) for k, v in w.items()}
    comm = HipComm(CFG["hidden_size"], backend="ipc")
    try:
        tp = Model(ModelArgs(**CFG), dev_w, tp=comm)
        assert lib.pie_decoder_set_batch_tail(tp._dec, _ffi.p(bt["table"]), 2, _ffi.p(bt["recent"]), _ffi.p(bt["ws"])) == -5
        assert b"pie_decoder_set_batch_tail" in lib.pie_last_error()
        assert lib.pie_decoder_set_batch_tail(tp._dec, None, 0, None, None) == -5
        with pytest.raises(RuntimeError):
            tp.set_batch_tail(2)
        del tp
    finally:
        comm.close()
