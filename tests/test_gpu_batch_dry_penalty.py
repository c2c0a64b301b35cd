"""-m gpu: the per-row DRY penalty in the multi-sequence passes against host orchestration per row: the unarmed pass, then
the single-row ops in the stated order -- pie_logits_penalty, pie_logits_bias, pie_logits_dry_penalty over the ids the row has been fed,
pie_logprobs_argmax(_masked), a one-row pie_sample.  The stand-alone op itself is pinned against tests/dry_penalty_reference.py by
tests/test_gpu_dry_penalty.py; here every comparison is exact as well, and every run asserts from the reference that the rule fired.
The prompts are a short pattern repeated, so a row's own tail repeats from its first token on."""
import numpy as np
import pytest
import torch

from tests import dry_penalty_reference as ref
from tests._util import to_bits
from tests.test_gpu_batch_edits import Req, make_model, pack, request, tiny  # noqa: F401  (tiny: the fixture)
from tests.test_gpu_batch_tail import dev_ids, f32_bits, prefilled, sample_one

pytestmark = pytest.mark.gpu
ZERO = (0.0, 1.75, 2, 1024, ())
# by request; the third holds a zero record.  allowed_length 1 on most: beside a mask, a repetition penalty and a sampler a run repeats whole
# sequences less often, and the rule still has to fire on a third of the armed rows
DRYS = [(0.8, 1.75, 1, 1024, ()), (1.5, 2.0, 1, 50, (3, 77)), ZERO, (0.8, 1.75, 2, 1024, ()), (2.0, 1.75, 1, 16, ())]


def pattern_prompts(V, lens, seed):
    """Prompt i: a random pattern of 3..7 ids repeated to lens[i] ids."""
    rng = np.random.default_rng(seed)
    return [np.tile(rng.integers(0, V, 3 + i % 5), n // 3 + 1)[:n].astype(np.int32).tolist() for i, n in enumerate(lens)]


class DReq(Req):
    """Req + the request's DRY penalty, run by the stand-alone op on the row alone over the ids it has been fed."""

    def __init__(self, base: Req, dry):
        super().__init__(base.V, base.fed, base.mask, base.bias, base.penalty, base.context, base.spec, base.seed, base.calls)
        self.dry, self.fired = dry, 0

    def tail(self, logits_row, fed_now):
        from proxy_inference_engine_amd import hip_ops
        self.fed += [int(t) for t in fed_now]
        row = logits_row.clone()
        if self.penalty != 1.0:
            hip_ops.logits_penalty(row, dev_ids(self.fed[-self.context:]), self.penalty)
        if self.bias is not None:
            hip_ops.logits_bias(row, dev_ids(self.bias[0]), torch.tensor(self.bias[1], dtype=torch.float32, device="cuda"))
        m, b, a, r, brk = self.dry
        if m != 0.0:
            self.fired += bool(ref.penalties(self.fed[-r:], self.V, m, b, a, brk))
            hip_ops.logits_dry_penalty(row, dev_ids(self.fed[-r:]), m, b, a, brk)
        if self.mask is not None:
            tok, lp = hip_ops.logprobs_argmax_masked(row, torch.from_numpy(pack(self.mask)).cuda())
        else:
            tok, lp = hip_ops.logprobs_argmax(row)
        tok = int(tok.item())
        if self.spec is not None:
            tok = sample_one(lp, self.spec, self.seed, self.calls)[0]
            self.calls += 1
        return tok, f32_bits(lp), to_bits(row)


def dreqs(V, prompts, with_edits):
    """Request i: DRYS[i % 5]; with_edits: request()'s kinds on top (mask + penalty + bias / mask + sampler / bias / nothing)."""
    return [DReq(request(V, i % 4, i, p, True, p[-1]) if with_edits else Req(V, p), DRYS[i % len(DRYS)]) for i, p in enumerate(prompts)]


def arm(model, rows_cap, reqs, with_edits, fed, rows=None):
    """Arms every per-row state the requests need and writes their rows; fed[i]: the ids request i has been fed so far."""
    rows = list(range(len(reqs))) if rows is None else rows
    bd = model.set_batch_dry_penalty(rows_cap)
    bd["recent"].fill_(-5)                                              # (what a cached ring may hold: the write below rebuilds the rows)
    model.write_batch_dry_penalty(rows, [r.dry for r in reqs], fed)
    if with_edits:
        model.set_batch_tail(rows_cap)
        model.write_batch_tail(rows, [r.record() for r in reqs], fed)
        model.set_batch_edits(rows_cap, masks=True, bias_cap=6)
        model.write_batch_edits(rows, masks=[None if r.mask is None else torch.from_numpy(r.mask) for r in reqs], biases=[r.bias for r in reqs])
    return bd


def disarm(model):
    model.clear_batch_dry_penalty(), model.clear_batch_edits(), model.clear_batch_tail()


def assert_fired(hosts, per_row):
    armed = [h for h in hosts if h.dry[0] != 0.0]
    fired = sum(h.fired for h in armed)
    print(f"DRY fired on {fired} of {per_row * len(armed)} armed rows")
    assert 3 * fired >= per_row * len(armed), (fired, per_row, len(armed))     # nothing passes vacuously


# ------------------------------------------------------------------ 1. the batched step
@pytest.mark.parametrize("with_edits", [False, True])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("B", [3, 7])              # the fused few-sequence form; the general form
def test_step_batch_equals_host_orchestration(tiny, B, graph, with_edits):
    g, cfg, model = tiny
    V, steps, swap_at = cfg["vocab_size"], 10, 5
    prompts = pattern_prompts(V, [9, 60, 30, 12, 7, 21, 33][:B], 3)        # (60: the sequence crosses a page boundary during the steps)
    disarm(model)
    model.enable_paged_kv(num_pages=48)
    # run B: nothing armed, the single-row ops per row on the host
    caches, first = prefilled(model, prompts)
    hosts, feed, want = dreqs(V, prompts, with_edits), list(first), []
    for st in range(steps):
        if st == swap_at:
            hosts[0].dry, hosts[1].dry = hosts[1].dry, hosts[0].dry
        _, _, logits = model.step_batch(dev_ids(feed), caches, graph=graph)
        rows = [h.tail(logits[i], [feed[i]]) for i, h in enumerate(hosts)]
        want.append(rows)
        feed = [r[0] for r in rows]
    assert_fired(hosts, steps)
    assert any(not np.array_equal(want[-1][i][2], to_bits(logits[i])) for i in range(B))     # the host edits did something
    assert np.array_equal(want[-1][2][2], to_bits(logits[2])) or with_edits                  # the zero record's row keeps every bit
    # run A: fresh caches, the same requests as rows of the armed state
    caches, first_a = prefilled(model, prompts)
    assert first_a == first
    reqs = dreqs(V, prompts, with_edits)
    fed = [list(p) for p in prompts]
    try:
        bd = arm(model, B, reqs, with_edits, fed)
        replays, feed = model.batch_graph_replays(), dev_ids(first)
        for st in range(steps):
            if st == swap_at:
                # rows 0 and 1 get new occupants' parameters: their records are rewritten and their rings REBUILT from the fed ids; every address stays
                reqs[0].dry, reqs[1].dry = reqs[1].dry, reqs[0].dry
                bd["recent"][:2] = 12345
                model.write_batch_dry_penalty([0, 1], [r.dry for r in reqs[:2]], fed[:2])
            nxt, lp, lg = model.step_batch(feed, caches, graph=graph)
            for f, t in zip(fed, feed.tolist()):
                f.append(t)
            assert nxt.tolist() == [r[0] for r in want[st]], st
            for i in range(B):
                assert np.array_equal(to_bits(lg[i]), want[st][i][2]), (st, i, "logits")
                assert np.array_equal(f32_bits(lp[i]), want[st][i][1]), (st, i, "logprobs")
            feed = nxt.clone()
        # eager, capture, then replays only -- through the rewritten records and rings as well
        assert model.batch_graph_replays() - replays == (steps - 2 if graph else 0)
        ring = bd["recent"].cpu().numpy()
        for i, f in enumerate(fed):                                       # every live row recorded its input ids, the zero record's row too
            assert all(ring[i, q & 1023] == f[q] for q in range(len(prompts[i]), len(f))), i
    finally:
        disarm(model)


# ------------------------------------------------------------------ 2. the launch table and the graph's key
@pytest.mark.parametrize("B", [3, 7])
def test_launches_per_step_follow_the_table(golden_dir, B):
    """One launch per pass; the fused few-sequence step (B = 3), whose lm_head epilogue partials the edit makes stale, one more (the
    partials) unless a batch tail had it recompute them already.  Nothing set: what it launched before.
        B = 7                       + 1
        B = 3, nothing else armed   + 2
        B = 3, a batch tail armed   + 1"""
    g, cfg, model = make_model(golden_dir)         # a decoder whose setters were never called
    V = cfg["vocab_size"]
    model.enable_paged_kv(num_pages=64)
    prompts = pattern_prompts(V, [5 + 2 * i for i in range(B)], 9)

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
            model.set_batch_dry_penalty(B)
            assert count() == base + (2 if B == 3 and not tailed else 1), (B, tailed)
            model.clear_batch_dry_penalty()
            assert count() == base, (B, tailed)
    finally:
        disarm(model)


def test_new_addresses_recapture_and_new_contents_replay(golden_dir):
    g, cfg, model = make_model(golden_dir)
    V, B = cfg["vocab_size"], 3
    model.enable_paged_kv(num_pages=32)
    prompts = pattern_prompts(V, [9, 20, 12], 4)
    caches, first = prefilled(model, prompts)
    feed, fed = dev_ids(first), [list(p) for p in prompts]

    def step(n):
        nonlocal feed
        before = model.batch_graph_replays()
        for _ in range(n):
            for f, t in zip(fed, feed.tolist()):
                f.append(t)
            feed = model.step_batch(feed, caches)[0].clone()
        return model.batch_graph_replays() - before

    try:
        bd = model.set_batch_dry_penalty(B)
        model.write_batch_dry_penalty([0, 1, 2], [DRYS[0], DRYS[1], None], fed)
        assert step(3) == 1                                                    # eager, capture, replay
        model.write_batch_dry_penalty([0, 1, 2], [DRYS[3], None, DRYS[4]], fed)   # new contents behind the same addresses
        assert step(2) == 2 and model.set_batch_dry_penalty(B)["records"].data_ptr() == bd["records"].data_ptr()
        assert step(1) == 1                                                    # set again with the same buffers: the same key
        other = model.set_batch_dry_penalty(B + 2)                             # another rows_cap: other buffers, another key
        assert other["records"].data_ptr() != bd["records"].data_ptr()
        model.write_batch_dry_penalty([0, 1, 2], [DRYS[3], None, DRYS[4]], fed)
        assert step(3) == 1                                                    # eager, capture, replay again
        model.clear_batch_dry_penalty()
        assert step(3) == 1                                                    # the unarmed key: eager, capture, replay
    finally:
        disarm(model)


# ------------------------------------------------------------------ 3. the prompt passes
@pytest.mark.parametrize("with_edits", [False, True])
@pytest.mark.parametrize("S", [3, 7])
def test_prompt_passes(tiny, S, with_edits):
    """prefill_batch and step_mixed with S output rows under mixed records, the third of them zero: a prompt's first token is chosen
    against its own prompt's window, a decoding row against everything it has been fed, and the row with the zero record keeps every
    bit of its logits.  The rows are the passes' output rows, decoding rows first (S = 3: one decoding row and two prompts, the zero record on
    a prompt; S = 7: three and four, the zero record on a decoding row)."""
    g, cfg, model = tiny
    V = cfg["vocab_size"]
    prompts = pattern_prompts(V, [9, 20, 12, 7, 21, 33, 15][:S], 5)
    nd = S // 2                                        # decoding rows of the mixed pass
    assert DRYS[2] == ZERO
    disarm(model)
    model.enable_paged_kv(num_pages=48)
    fresh = lambda n: [model.make_cache() for _ in range(n)]
    # host orchestration on the unarmed passes
    _, _, logits = model.prefill_batch(prompts, fresh(S))
    hosts = dreqs(V, prompts, with_edits)
    for h in hosts:
        h.fed = []
    want_pf = [h.tail(logits[i], prompts[i]) for i, h in enumerate(hosts)]
    assert_fired(hosts, 1)
    if not with_edits:
        assert np.array_equal(want_pf[2][2], to_bits(logits[2])) and not np.array_equal(want_pf[0][2], to_bits(logits[0]))
    dcs, dtoks = prefilled(model, prompts[:nd])
    _, _, logits = model.step_mixed(dev_ids(dtoks), dcs, prompts[nd:], fresh(S - nd))
    hosts = dreqs(V, prompts, with_edits)
    for h in hosts[nd:]:
        h.fed = []
    want_mx = [h.tail(logits[i], [dtoks[i]] if i < nd else prompts[i]) for i, h in enumerate(hosts)]
    try:
        reqs = dreqs(V, prompts, with_edits)
        bd = arm(model, S, reqs, with_edits, [list(p) for p in prompts])
        nxt, lp, lg = model.prefill_batch(prompts, fresh(S))
        for i in range(S):
            assert int(nxt[i]) == want_pf[i][0], i
            assert np.array_equal(f32_bits(lp[i]), want_pf[i][1]) and np.array_equal(to_bits(lg[i]), want_pf[i][2]), i
        dcs, dtoks2 = prefilled(model, prompts[:nd])
        assert dtoks2 == dtoks
        bd = arm(model, S, reqs, with_edits, [list(p) for p in prompts])
        nxt, lp, lg = model.step_mixed(dev_ids(dtoks), dcs, prompts[nd:], fresh(S - nd))
        for i in range(S):
            assert int(nxt[i]) == want_mx[i][0], i
            assert np.array_equal(f32_bits(lp[i]), want_mx[i][1]) and np.array_equal(to_bits(lg[i]), want_mx[i][2]), i
        ring = bd["recent"].cpu().numpy()
        for i in range(nd):                                               # a decoding row recorded its input at its position
            assert ring[i, len(prompts[i]) & 1023] == dtoks[i], i
    finally:
        disarm(model)


# ------------------------------------------------------------------ 4. BatchedEngine.generate
@pytest.mark.parametrize("kw", [dict(), dict(prefill_chunk=16), dict(share_prefix=True), dict(kv_dtype=torch.int8)])
def test_engine_generates_with_mixed_penalties(tiny, kw):
    """Every request of a mixed batch generates what it generates alone through the same engine.
    The passes of a mixed batch and of a request alone are not the same launches (other row counts, other chunk boundaries, int8 pages
    quantised in another order), and on periodic prompts the tiny model sits on near-ties: with NOTHING armed, 7 of 12 prompt seeds tried
    gave some request another token alone than in the batch in at least one of the four variants.  Seed 27 is one on which the unarmed
    engine agrees with itself in all four -- asserted first, as the precondition -- so a difference below is the DRY state's."""
    from proxy_inference_engine_amd.engine import BatchedEngine, SamplingParams
    g, cfg, model = tiny
    V, new = cfg["vocab_size"], 10
    disarm(model)
    prompts = pattern_prompts(V, [12, 70, 5, 33, 64], 27)
    if kw.get("share_prefix"):
        prompts = [prompts[1][:66] + p for p in prompts]
    params = [SamplingParams(dry_multiplier=0.8), SamplingParams(dry_multiplier=1.5, dry_base=2.0, dry_allowed_length=1, dry_range=50, dry_sequence_breakers=(3, 77)),
              SamplingParams(), SamplingParams(dry_multiplier=0.8, dry_allowed_length=3, frequency_penalty=0.5),
              SamplingParams(temp=0.8, top_k=5, seed=21, dry_multiplier=2.0, dry_range=16)]
    assert [sp.plain for sp in params] == [False, False, True, False, False]
    eng = BatchedEngine(model, num_pages=64, max_batch=3, **kw)
    plain = eng.generate(prompts, new)
    assert plain == [eng.generate([p], new)[0] for p in prompts]                        # the precondition: the unarmed engine is batch-invariant here
    out = eng.generate(prompts, new, sampling=params)
    assert model._batch_dry is None and model._batch_tail is None and model._batch_counts is None      # cleared on the way out
    assert [len(o) for o in out] == [new] * 5 and out == eng.generate(prompts, new, sampling=params)
    assert out[2] == plain[2]                                                           # the request without DRY: a run with nothing armed
    assert any(out[r] != plain[r] for r in (0, 1, 3))                                   # (the penalty did something)
    alone = [eng.generate([prompts[r]], new, sampling=params[r])[0] for r in range(5)]
    assert out == alone
    if kw.get("kv_dtype") is not None:
        model.enable_paged_kv(num_pages=16)                                             # (back to T pages for whoever uses the fixture next)


# ------------------------------------------------------------------ 5. refusals, each before any launch
def test_refusals(tiny):
    from proxy_inference_engine_amd import hip_ops
    g, cfg, model = tiny
    V = cfg["vocab_size"]
    disarm(model)
    model.enable_paged_kv(num_pages=16)
    prompts = pattern_prompts(V, [9, 20, 30], 3)
    caches, first = prefilled(model, prompts)
    model.step_batch(dev_ids(first), caches, graph=False)                   # (the B = 3 buffers exist from here on)
    bd = model.set_batch_dry_penalty(2)
    try:
        assert bd["records"].shape == (2, hip_ops.DRY_PENALTY_WORDS) and bd["breakers"].shape == (2, 64) and bd["recent"].shape == (2, 1024)
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
        for bad in ((-0.5, 1.75, 2, 1024, ()), (0.8, 0.0, 2, 1024, ()), (0.8, 1.75, 65, 1024, ()), (0.8, 1.75, 2, 1025, ()), (0.8, 1.75, 2, 1024, tuple(range(65)))):
            with pytest.raises(ValueError):
                model.write_batch_dry_penalty([0], [bad])
        with pytest.raises(ValueError):
            model.write_batch_dry_penalty([0, 1], [DRYS[0]])
        model.write_batch_dry_penalty([1], [DRYS[1]], [list(range(1030))])
        assert bd["records"][1].tolist()[2:] == [1, 50, 2, 0] and bd["breakers"][1].tolist()[:3] == [3, 77, 0]
        ring = bd["recent"][1].tolist()
        assert ring[:6] == [1024, 1025, 1026, 1027, 1028, 1029] and ring[6:] == list(range(6, 1024))   # the last 1024 fed ids, by position & 1023
        model.write_batch_dry_penalty([1], [None])
        assert bd["records"][1, :1].view(torch.float32).item() == 0.0
    finally:
        model.clear_batch_dry_penalty()
    nxt, _, _ = model.step_batch(dev_ids(first), caches, graph=False)       # off again: the step takes three rows
    assert nxt.shape == (3,)
    with pytest.raises(RuntimeError):
        model.write_batch_dry_penalty([0], [None])                          # nothing is armed
    with pytest.raises(ValueError):
        model.set_batch_dry_penalty(0)
