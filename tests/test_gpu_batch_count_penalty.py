"""-m gpu: per-row frequency and presence penalties in the multi-sequence passes against host orchestration per row: the
unarmed pass, then the single-row ops in the stated order -- pie_logits_penalty, pie_logits_bias, pie_logits_count_penalty_rows on that row
alone with state of its own, pie_logprobs_argmax(_masked), a one-row pie_sample.  The stand-alone op itself is pinned against
tests/count_penalty_reference.py by tests/test_gpu_count_penalty.py; here every comparison is exact as well, and the rows' counts are checked
against bincount(generated)."""
import numpy as np
import pytest
import torch

from tests._util import to_bits
from tests.count_penalty_reference import generated_counts
from tests.test_gpu_batch_edits import Req, make_model, pack, request, tiny  # noqa: F401  (tiny: the fixture)
from tests.test_gpu_batch_tail import dev_ids, f32_bits, prefilled, repeating_prompts, sample_one

pytestmark = pytest.mark.gpu
PAIRS = [(0.5, 0.0), (0.0, 1.5), (0.0, 0.0), (-1.0, -0.25), (2.0, 2.0)]     # by request; the third holds a zero record


class CReq(Req):
    """Req + the request's frequency / presence penalties, run by the stand-alone op on the row alone with a record and counts of its own."""

    def __init__(self, base: Req, fp, start: int):
        from proxy_inference_engine_amd import hip_ops
        super().__init__(base.V, base.fed, base.mask, base.bias, base.penalty, base.context, base.spec, base.seed, base.calls)
        self.fp, self.start, self.gen = fp, start, []
        self.rec = hip_ops.count_penalty_records([hip_ops.count_penalty_pack(*fp, start)], "cuda")
        self.cnt = torch.zeros((1, self.V), dtype=torch.int32, device="cuda")

    def set_fp(self, fp):
        from proxy_inference_engine_amd import hip_ops
        self.fp = fp
        self.rec[0, :2].copy_(hip_ops.count_penalty_records([hip_ops.count_penalty_pack(*fp)])[0, :2])

    def tail(self, logits_row, fed_now):
        from proxy_inference_engine_amd import hip_ops
        self.fed += [int(t) for t in fed_now]
        row = logits_row.clone().reshape(1, -1)
        if self.penalty != 1.0:
            hip_ops.logits_penalty(row[0], dev_ids(self.fed[-self.context:]), self.penalty)
        if self.bias is not None:
            hip_ops.logits_bias(row[0], dev_ids(self.bias[0]), torch.tensor(self.bias[1], dtype=torch.float32, device="cuda"))
        hip_ops.logits_count_penalty_rows(row, self.rec, self.cnt, dev_ids(self.fed[-1:]), dev_ids([len(self.fed)]))
        if self.mask is not None:
            tok, lp = hip_ops.logprobs_argmax_masked(row[0], torch.from_numpy(pack(self.mask)).cuda())
        else:
            tok, lp = hip_ops.logprobs_argmax(row[0])
        tok = int(tok.item())
        if self.spec is not None:
            tok = sample_one(lp, self.spec, self.seed, self.calls)[0]
            self.calls += 1
        self.gen.append(tok)
        return tok, f32_bits(lp), to_bits(row[0])


def creqs(V, prompts, with_edits, firsts=None):
    """Request i: PAIRS[i % 5]; with_edits: request()'s kinds on top (mask + penalty + bias / mask + sampler / bias / nothing)."""
    out = []
    for i, p in enumerate(prompts):
        base = request(V, i % 4, i, p, True, p[-1]) if with_edits else Req(V, p)
        out.append(CReq(base, PAIRS[i % len(PAIRS)], len(p)))
        if firsts is not None:
            out[-1].gen.append(int(firsts[i]))
    return out


def arm(model, rows_cap, reqs, with_edits, rows=None):
    """Arms every per-row state the requests need and writes their rows."""
    rows = list(range(len(reqs))) if rows is None else rows
    bc = model.set_batch_count_penalty(rows_cap)
    model.write_batch_count_penalty(rows, [(*r.fp, r.start) for r in reqs], [r.gen for r in reqs])
    if with_edits:
        model.set_batch_tail(rows_cap)
        model.write_batch_tail(rows, [r.record() for r in reqs], [r.fed for r in reqs])
        be = model.set_batch_edits(rows_cap, masks=True, bias_cap=6)
        model.write_batch_edits(rows, masks=[None if r.mask is None else torch.from_numpy(r.mask) for r in reqs], biases=[r.bias for r in reqs])
    return bc


def disarm(model):
    model.clear_batch_count_penalty(), model.clear_batch_edits(), model.clear_batch_tail()


# ------------------------------------------------------------------ 1. the batched step
@pytest.mark.parametrize("with_edits", [False, True])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("B", [3, 7])              # the fused few-sequence form; the general form
def test_step_batch_equals_host_orchestration(tiny, B, graph, with_edits):
    g, cfg, model = tiny
    V, steps, swap_at = cfg["vocab_size"], 10, 5
    prompts = repeating_prompts(V, [9, 60, 30, 12, 7, 21, 33][:B], 3)      # (60: the sequence crosses a page boundary during the steps)
    disarm(model)
    model.enable_paged_kv(num_pages=48)
    # run B: nothing armed, the single-row ops per row on the host
    caches, first = prefilled(model, prompts)
    hosts, feed, want = creqs(V, prompts, with_edits, first), list(first), []
    for st in range(steps):
        if st == swap_at:
            a, b = hosts[0].fp, hosts[1].fp
            hosts[0].set_fp(b), hosts[1].set_fp(a)
        _, _, logits = model.step_batch(dev_ids(feed), caches, graph=graph)
        rows = [h.tail(logits[i], [feed[i]]) for i, h in enumerate(hosts)]
        want.append(rows)
        feed = [r[0] for r in rows]
    assert any(not np.array_equal(want[-1][i][2], to_bits(logits[i])) for i in range(B))     # the host edits did something
    # run A: fresh caches, the same requests as rows of the armed state
    caches, first_a = prefilled(model, prompts)
    assert first_a == first
    reqs = creqs(V, prompts, with_edits, first)
    try:
        bc = arm(model, B, reqs, with_edits)
        replays, feed = model.batch_graph_replays(), dev_ids(first)
        for st in range(steps):
            if st == swap_at:
                # rows 0 and 1 get new occupants' parameters: their records are rewritten and their counts REBUILT from the generated ids
                # (the last of which is this step's input: counted here, not again by the pass); every address stays
                reqs[0].fp, reqs[1].fp = reqs[1].fp, reqs[0].fp
                before = bc["counts"][:2].clone()
                bc["counts"][:2] = 12345
                model.write_batch_count_penalty([0, 1], [(*r.fp, r.start) for r in reqs[:2]], [r.gen for r in reqs[:2]])
                assert torch.equal(bc["counts"][:2], before + torch.nn.functional.one_hot(feed[:2].long(), V).int())
            nxt, lp, lg = model.step_batch(feed, caches, graph=graph)
            assert nxt.tolist() == [r[0] for r in want[st]], st
            for i in range(B):
                assert np.array_equal(to_bits(lg[i]), want[st][i][2]), (st, i, "logits")
                assert np.array_equal(f32_bits(lp[i]), want[st][i][1]), (st, i, "logprobs")
                reqs[i].gen.append(int(nxt[i]))
            feed = nxt.clone()
        # eager, capture, then replays only -- through the rewritten records and counts as well
        assert model.batch_graph_replays() - replays == (steps - 2 if graph else 0)
        got = bc["counts"].cpu().numpy()
        for i, r in enumerate(reqs):
            # every generated token but the last (not fed yet) -- for the request with the zero record nothing at all
            want_c = generated_counts(r.gen[:-1], V) if r.fp != (0.0, 0.0) else np.zeros(V, np.int32)
            assert np.array_equal(got[i], want_c), i
            assert np.array_equal(hosts[i].cnt.cpu().numpy()[0], got[i]), i
    finally:
        disarm(model)


# ------------------------------------------------------------------ 2. the launch table
@pytest.mark.parametrize("B", [3, 7])
def test_launches_per_step_follow_the_table(golden_dir, B):
    """One launch per pass; the fused few-sequence step, whose lm_head epilogue partials the edit makes stale, one more (the partials)
    unless a batch tail or batch edits had it recompute them already.  Nothing set: what it launched before."""
    g, cfg, model = make_model(golden_dir)         # a decoder whose setters were never called
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

    try:
        for tailed in (False, True):
            if tailed:
                model.set_batch_tail(B)
            base = count()
            assert base > 0
            model.set_batch_count_penalty(B)
            assert count() == base + (2 if B == 3 and not tailed else 1), (B, tailed)
            model.clear_batch_count_penalty()
            assert count() == base, (B, tailed)
    finally:
        disarm(model)


# ------------------------------------------------------------------ 3. the prompt passes
@pytest.mark.parametrize("with_edits", [False, True])
@pytest.mark.parametrize("S", [3, 7])
def test_prompt_passes(tiny, S, with_edits):
    """prefill_batch and step_mixed with S output rows under mixed records, the third of them zero: a prompt's row is chosen against its
    record with nothing counted (its input is a prompt token), a decoding row counts its input, and the row with the zero record keeps
    every bit of its logits and of its counts.  The rows are the passes' output rows, decoding rows first (S = 3: one decoding row and two
    prompts, the zero record on a prompt; S = 7: three and four, the zero record on a decoding row)."""
    g, cfg, model = tiny
    V = cfg["vocab_size"]
    prompts = repeating_prompts(V, [9, 20, 12, 7, 21, 33, 15][:S], 5)
    nd = S // 2                                        # decoding rows of the mixed pass
    assert PAIRS[2] == (0.0, 0.0)
    disarm(model)
    model.enable_paged_kv(num_pages=48)
    fresh = lambda n: [model.make_cache() for _ in range(n)]

    def plain(bits_row, req):                          # the row without its frequency / presence step: what a zero record must leave
        keep, req.fp = req.fp, (0.0, 0.0)
        req.set_fp((0.0, 0.0))
        out = req.tail(bits_row, [])
        req.set_fp(keep)
        return out

    # host orchestration on the unarmed passes
    _, _, logits = model.prefill_batch(prompts, fresh(S))
    hosts = creqs(V, prompts, with_edits)
    for h in hosts:
        h.fed, h.cnt[0, :7] = [], 3                    # (prompt rows with counts already there: requests resumed in fresh caches)
    want_pf = [h.tail(logits[i], prompts[i]) for i, h in enumerate(hosts)]
    zero_pf = plain(logits[2], hosts[2])
    assert np.array_equal(zero_pf[2], want_pf[2][2]) and not np.array_equal(plain(logits[0], hosts[0])[2], want_pf[0][2])
    dcs, dtoks = prefilled(model, prompts[:nd])
    _, _, logits = model.step_mixed(dev_ids(dtoks), dcs, prompts[nd:], fresh(S - nd))
    hosts = creqs(V, prompts, with_edits, dtoks + [0] * (S - nd))
    for h in hosts[nd:]:
        h.fed, h.gen = [], []
    want_mx = [h.tail(logits[i], [dtoks[i]] if i < nd else prompts[i]) for i, h in enumerate(hosts)]
    try:
        reqs = creqs(V, prompts, with_edits)
        bc = arm(model, S, reqs, with_edits)
        bc["counts"][:S, :7] = 3
        nxt, lp, lg = model.prefill_batch(prompts, fresh(S))
        for i in range(S):
            assert int(nxt[i]) == want_pf[i][0], i
            assert np.array_equal(f32_bits(lp[i]), want_pf[i][1]) and np.array_equal(to_bits(lg[i]), want_pf[i][2]), i
        assert np.array_equal(to_bits(lg[2]), zero_pf[2])                                  # the zero record among penalised rows: bit-untouched
        got = bc["counts"].cpu().numpy()
        assert (got[:S, :7] == 3).all() and not got[:S, 7:].any()                          # nothing counted, the zero row's counts included
        dcs, dtoks2 = prefilled(model, prompts[:nd])
        assert dtoks2 == dtoks
        reqs = creqs(V, prompts, with_edits, dtoks + [0] * (S - nd))
        for r in reqs[nd:]:
            r.gen = []
        bc = arm(model, S, reqs, with_edits)
        nxt, lp, lg = model.step_mixed(dev_ids(dtoks), dcs, prompts[nd:], fresh(S - nd))
        for i in range(S):
            assert int(nxt[i]) == want_mx[i][0], i
            assert np.array_equal(f32_bits(lp[i]), want_mx[i][1]) and np.array_equal(to_bits(lg[i]), want_mx[i][2]), i
        got = bc["counts"].cpu().numpy()
        for i in range(S):                                                                  # a decoding row with penalties counted its input; nobody else
            counted = i < nd and reqs[i].fp != (0.0, 0.0)
            assert np.array_equal(got[i], generated_counts(dtoks[i:i + 1] if counted else [], V)), i
            assert np.array_equal(hosts[i].cnt.cpu().numpy()[0], got[i]), i
    finally:
        disarm(model)


# ------------------------------------------------------------------ 4. BatchedEngine.generate
@pytest.mark.parametrize("kw", [dict(), dict(prefill_chunk=16), dict(share_prefix=True)])
def test_engine_generates_with_mixed_penalties(tiny, kw):
    """Every request of a mixed batch generates what it generates alone through the same engine."""
    from proxy_inference_engine_amd.engine import BatchedEngine, SamplingParams
    g, cfg, model = tiny
    V, new = cfg["vocab_size"], 10
    disarm(model)
    prompts = repeating_prompts(V, [12, 70, 5, 33, 64], 11)
    if kw.get("share_prefix"):
        prompts = [prompts[1][:66] + p for p in prompts]
    params = [SamplingParams(frequency_penalty=1.0, presence_penalty=0.5), SamplingParams(presence_penalty=2.0), SamplingParams(),
              SamplingParams(frequency_penalty=-1.0, presence_penalty=-0.25), SamplingParams(temp=0.8, top_k=5, seed=21, frequency_penalty=2.0, presence_penalty=2.0)]
    assert [sp.plain for sp in params] == [False, False, True, False, False]
    eng = BatchedEngine(model, num_pages=64, max_batch=3, **kw)
    plain = eng.generate(prompts, new)
    out = eng.generate(prompts, new, sampling=params)
    assert model._batch_counts is None and model._batch_tail is None                    # cleared on the way out
    assert [len(o) for o in out] == [new] * 5 and out == eng.generate(prompts, new, sampling=params)
    assert out[2] == plain[2]                                                           # the request without penalties: a run with nothing armed
    for r in range(5):
        assert out[r][0] == plain[r][0] or r == 4, r                                    # a first token is chosen against empty counts
    assert any(out[r] != plain[r] for r in (0, 1, 3))                                   # (the penalties did something)
    alone = [eng.generate([prompts[r]], new, sampling=params[r])[0] for r in range(5)]
    assert out == alone


# ------------------------------------------------------------------ 5. refusals, each before any launch
def test_refusals(tiny):
    g, cfg, model = tiny
    V = cfg["vocab_size"]
    disarm(model)
    model.enable_paged_kv(num_pages=16)
    prompts = repeating_prompts(V, [9, 20, 30], 3)
    caches, first = prefilled(model, prompts)
    model.step_batch(dev_ids(first), caches, graph=False)                   # (the B = 3 buffers exist from here on)
    bc = model.set_batch_count_penalty(2)
    try:
        assert bc["records"].shape == (2, 4) and bc["counts"].shape == (2, V) and not bc["counts"].any()
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
        with pytest.raises(ValueError):
            model.write_batch_count_penalty([0], [(2.5, 0.0, 3)])
        with pytest.raises(ValueError):
            model.write_batch_count_penalty([0, 1], [(0.5, 0.0, 3)])
        model.write_batch_count_penalty([1], [(0.5, 0.25, 3)], [[7, 7, V + 1, -4, 9]])
        assert bc["records"][1].tolist()[2:] == [3, 7] and bc["counts"][1].cpu().numpy().tolist() == generated_counts([7, 7, 9], V).tolist()
        model.write_batch_count_penalty([1], [None])
        assert bc["records"][1].tolist() == [0, 0, 0, -1] and not bc["counts"].any()
    finally:
        model.clear_batch_count_penalty()
    nxt, _, _ = model.step_batch(dev_ids(first), caches, graph=False)       # off again: the step takes three rows
    assert nxt.shape == (3,)
    with pytest.raises(RuntimeError):
        model.write_batch_count_penalty([0], [None])                        # nothing is armed
    with pytest.raises(ValueError):
        model.set_batch_count_penalty(0)
