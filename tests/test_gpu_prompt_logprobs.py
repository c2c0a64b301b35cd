"""-m gpu: log-probabilities of prompt tokens -- the op against the composition it replaces (exact), the decoder's setting
on every prompt pass and KV binding, and both engines.

Exact comparisons: ids equal, values bit-equal.  Where the lm_head sees other row counts than the reference's (several blocks, chunks,
the varlen passes) values are held to  2 x c_max x eps x max|logits|,  c_max = 4 and eps from tests/_util.py: its logit bound, applied
once to the logit and once to the log-sum-exp."""
import json

import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests import prompt_logprobs_reference as pref
from tests import top_logprobs_reference as tref
from tests._util import EPS, codes_dev, to_dev
from tests.test_gpu_batch_tail import prefilled, repeating_prompts

pytestmark = pytest.mark.gpu
DT = "bfloat16"
C_MAX = 4.0
SENT_ID, SENT_VAL = tref.SENTINEL_ID, 123.0


def dev_ids(ids) -> torch.Tensor:
    return torch.tensor([int(i) for i in ids], dtype=torch.int32, device="cuda")


def bits_of(t: torch.Tensor) -> np.ndarray:
    return t.detach().contiguous().cpu().numpy().view(np.uint32).copy()


def sentinels(rows, n):
    return (torch.full((rows, n + 1), SENT_ID, dtype=torch.int32, device="cuda"), torch.full((rows, n + 1), SENT_VAL, dtype=torch.float32, device="cuda"))


def assert_same_records(got, want, what):
    assert got[0].cpu().tolist() == want[0].cpu().tolist(), what
    assert np.array_equal(bits_of(got[1]), bits_of(want[1])), what


# ------------------------------------------------------------------ 1. the op against the composition
def designed_rows(V: int, rows: int, dtype: torch.dtype) -> torch.Tensor:
    """[rows, V] logits in `dtype`: the rows at which the op can go wrong, cycled, between random ones."""
    rng = np.random.default_rng(V * 131 + rows)
    x = (rng.standard_normal((rows, V)) * 4.0).astype(np.float32)
    for r in range(rows):
        kind = r % 7
        if kind == 0:                                   # a row of equal logits: every rank is a tie, the ids come out ascending
            x[r] = 1.5
        elif kind == 1:                                 # -inf entries and fewer than n finite ones
            keep = rng.choice(V, size=min(3, V), replace=False)
            row = np.full(V, -np.inf, np.float32)
            row[keep] = x[r, keep]
            x[r] = row
        elif kind == 2 and V > 512:                     # equal maxima on both sides of the 512-id slice edge
            x[r, 511] = x[r, 512] = 40.0
            x[r, V - 1] = 40.0
        elif kind == 3 and V >= 3:                      # two distinct tiny logits under a large lse: their lp collide, the lower id wins
            x[r] = -50.0 - np.abs(x[r])
            a, b = sorted(rng.choice(V - 1, size=2, replace=False).tolist())
            x[r, V - 1], x[r, a], x[r, b] = 30000.0, 2.0 ** -12, 2.0 ** -11   # (both far below half an fp32 ulp at 3e4; the HIGHER id holds the larger logit)
        elif kind == 4 and V >= 2:                      # +0.0 and -0.0 among negative values
            x[r] = -1.0 - np.abs(x[r])
            x[r, V // 2], x[r, V // 3] = 0.0, -0.0
    return torch.from_numpy(x).to("cuda").to(dtype).contiguous()


def composition(logits, n, targets, count, out):
    """What the op replaces: pie_logprobs_argmax per row (no mask armed), then pie_top_logprobs over the fp32 rows."""
    from proxy_inference_engine_amd import hip_ops
    rows, V = logits.shape
    masks = torch.zeros((rows, (V + 31) // 32), dtype=torch.int32, device="cuda")
    _, lp = hip_ops.logprobs_argmax_rows_masked(logits.clone(), masks, torch.zeros(rows, dtype=torch.int32, device="cuda"))
    return hip_ops.top_logprobs(lp, n, tokens=targets, count=count, out=out), lp


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("V,rows", [(1, 37), (200, 37), (511, 37), (512, 37), (513, 37), (1000, 37), (513, 1), (128256, 3)])
def test_op_equals_the_composition(V, rows, dtype):
    """V = 1; fewer ids than partial tiles (empty tiles); the 512-id slice edge; V & 7 != 0; a real vocabulary."""
    from proxy_inference_engine_amd import hip_ops
    logits = designed_rows(V, rows, dtype)
    targets = dev_ids([(-1, 0, V - 1, V, (7 * r + 3) % V)[r % 5] for r in range(rows)])
    counts = [(3, 25, 0, -1)[r % 4] for r in range(rows)]
    for n in (1, 5, 20):
        ws = hip_ops.prompt_logprobs_workspace("cuda", rows, V, n)
        ws.fill_(-1)                                    # the workspace needs no initialisation: garbage must not show
        for count in (None, dev_ids(counts)):
            got = hip_ops.prompt_logprobs(logits, n, targets=targets, count=count, workspace=ws, out=sentinels(rows, n))
            want, lp = composition(logits, n, targets, count, sentinels(rows, n))
            assert_same_records(got, want, (V, rows, n, dtype, count is not None))
            if count is not None:                       # a skipped row keeps what was there
                skipped = [r for r, c in enumerate(counts) if c < 0]
                assert got[0][skipped].eq(SENT_ID).all() and got[1][skipped].eq(SENT_VAL).all()
        if rows > 1:                                    # a row alone is the row in its block
            one = hip_ops.prompt_logprobs(logits[4 % rows].contiguous(), n, targets=targets[4 % rows:4 % rows + 1].contiguous())
            full = hip_ops.prompt_logprobs(logits, n, targets=targets)
            assert_same_records((one[0][0], one[1][0]), (full[0][4 % rows], full[1][4 % rows]), (V, n, "one row"))
    none = hip_ops.prompt_logprobs(logits, 5)           # no targets: slot 0 is (-1, -inf)
    assert none[0][:, 0].eq(-1).all() and bits_of(none[1][:, 0]).tolist() == [0xFF800000] * rows
    if V >= 3 and rows > 3:                             # the designed collision really is one: equal lp from distinct logits, lower id first
        x, lpr = logits[3].float().cpu().numpy(), lp[3].cpu().numpy()
        a, b = np.flatnonzero((x > 0) & (x < 1))
        assert x[a] < x[b] and lpr[a] == lpr[b]
        ids = hip_ops.prompt_logprobs(logits, 5)[0][3, 1:4].tolist()
        assert ids == [V - 1, a, b]


# ------------------------------------------------------------------ the tiny golden model
def build_tiny(golden_dir):
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    g = np.load(golden_dir / "tiny_llama_w4_bf16.npz")
    cfg = json.loads(str(g["config_json"]))
    w = {k[2:]: g[k] for k in g.files if k.startswith("w:")}
    dev_w = {k: (codes_dev(v) if v.dtype == np.uint32 else to_dev(v, DT)) for k, v in w.items()}
    return w, cfg, Model(ModelArgs(**cfg), dev_w)


@pytest.fixture(scope="module")
def tiny(golden_dir):
    """The tiny int4 bf16 model on its own contiguous caches."""
    return build_tiny(golden_dir)


@pytest.fixture(scope="module")
def paged_tiny(golden_dir):
    """A second instance for the tests that switch the model to a page pool (enable_paged_kv is not undone)."""
    return build_tiny(golden_dir)


def make_cache(model, kind):
    from proxy_inference_engine_amd.cache import QuantizedKVCache, ReusableKVCache, RotatingKVCache
    if kind == "contiguous":
        return [ReusableKVCache() for _ in model.layers]
    if kind == "pages":
        return model.make_paged_cache(num_pages=8, max_blocks=4)
    if kind == "quantized":
        return [QuantizedKVCache(group_size=64, bits=8) for _ in model.layers]
    return [RotatingKVCache(32, keep=4) for _ in model.layers]     # max_kv_size larger than the prompt


def arm(model, rows_cap, n, block_rows, targets, counts):
    bufs = model.set_prompt_logprobs(rows_cap, n, block_rows)
    bufs["targets"].copy_(dev_ids(targets)), bufs["count"].copy_(dev_ids(counts))
    bufs["ids"].fill_(SENT_ID), bufs["vals"].fill_(SENT_VAL)
    return bufs


def scored_step(model, kind, prompt, n, block_rows):
    """model.step(prompt) on a fresh cache with the prompt's rows scored -> (records, token, logprobs bits)."""
    L = len(prompt)
    bufs = arm(model, L, n, block_rows, prompt[1:] + [0], [n] * (L - 1) + [-1])
    try:
        tok, lp, _ = model.step(dev_ids(prompt), make_cache(model, kind))
        return (bufs["ids"].clone(), bufs["vals"].clone()), int(tok.item()), bits_of(lp)
    finally:
        model.clear_prompt_logprobs()


def op_on_call(model, kind, prompt, n):
    """The op on model(ids)'s logits (a fresh cache of the same kind) -> (records, logits)."""
    from proxy_inference_engine_amd import hip_ops
    L = len(prompt)
    logits = model(dev_ids(prompt)[None], cache=make_cache(model, kind))[0].contiguous()
    rec = hip_ops.prompt_logprobs(logits, n, targets=dev_ids(prompt[1:] + [0]), count=dev_ids([n] * (L - 1) + [-1]), out=sentinels(L, n))
    return rec, logits


def test_setter_refusals(tiny):
    from proxy_inference_engine_amd import _ffi
    from tests.test_prompt_logprobs_host import check_setter_refusals
    w, cfg, model = tiny
    check_setter_refusals(_ffi.load(), model._dec, cfg["vocab_size"])
    for bad in ((0, 5, 16), (8, 0, 16), (8, 21, 16), (8, 5, 7), (8, 5, 1025), (65536, 5, 16)):
        with pytest.raises(ValueError, match="set_prompt_logprobs"):
            model.set_prompt_logprobs(*bad)
    prompt = repeating_prompts(cfg["vocab_size"], [20], 2)[0]
    bufs = arm(model, 8, 3, 16, [0] * 8, [-1] * 8)
    try:
        before = model.token.clone()
        with pytest.raises(ValueError, match="rows_cap"):                       # more rows than records: before any launch
            model.step(dev_ids(prompt), make_cache(model, "contiguous"))
        with pytest.raises(ValueError, match="rows_cap"):
            model(dev_ids(prompt)[None], cache=make_cache(model, "contiguous"))
        torch.cuda.synchronize()
        assert torch.equal(model.token, before) and bufs["ids"].eq(SENT_ID).all()
    finally:
        model.clear_prompt_logprobs()


@pytest.mark.parametrize("L", [20, 4])      # the batched path; the iterated path (fewer rows than PIE_KNOB_PREFILL_MIN)
def test_decoder_one_block_is_the_op_on_the_calls_logits(tiny, L):
    w, cfg, model = tiny
    prompt = repeating_prompts(cfg["vocab_size"], [L], 7)[0]
    n = 5
    plain_tok, plain_lp, _ = model.step(dev_ids(prompt), make_cache(model, "contiguous"))
    plain_tok, plain_lp = int(plain_tok.item()), bits_of(plain_lp)
    cache = make_cache(model, "contiguous")
    model.step(dev_ids(prompt), cache), model.step(None, cache)
    launches = model.graph_launches()
    got, tok, lp = scored_step(model, "contiguous", prompt, n, 32)
    want, _ = op_on_call(model, "contiguous", prompt, n)
    assert_same_records(got, want, L)
    assert got[0][L - 1].eq(SENT_ID).all() and (got[0][:L - 1, 0].cpu().tolist() == prompt[1:])     # the last row is left alone; slot 0 is the next prompt id
    assert tok == plain_tok and np.array_equal(lp, plain_lp)                  # the pass's own outputs do not notice
    cache = make_cache(model, "contiguous")
    model.step(dev_ids(prompt), cache), model.step(None, cache)
    assert model.graph_launches() == launches > 0                               # cleared: exactly the launches from before


def test_decoder_ignores_the_configured_tail_on_prompt_rows(tiny):
    """Raw model distribution: a configured sampler and penalty change neither the records nor, on the iterated path, what the rows before the last draw."""
    from proxy_inference_engine_amd import samplers
    w, cfg, model = tiny
    for L in (20, 4):
        prompt = repeating_prompts(cfg["vocab_size"], [L], 9)[0]
        want, _ = op_on_call(model, "contiguous", prompt, 3)
        try:
            samplers.seed(4)
            model.set_step_tail(sampler=("top_k", 0.8, 0.0, 5), repetition_penalty=1.3)
            plain_tok = int(model.step(dev_ids(prompt), make_cache(model, "contiguous"))[0].item())
            samplers.seed(4)
            model.set_step_tail(sampler=("top_k", 0.8, 0.0, 5), repetition_penalty=1.3)
            got, tok, _ = scored_step(model, "contiguous", prompt, 3, 32)
        finally:
            model.set_step_tail()
        assert_same_records(got, want, L)
        assert tok == plain_tok                                                  # one draw, for the last row, from the same stream position


def test_decoder_scores_a_prompt_of_embeddings(tiny):
    """pie_decoder_prefill_embeds: the rows of step_embeds(embed(ids)) get the records the rows of step(ids) get."""
    w, cfg, model = tiny
    prompt = repeating_prompts(cfg["vocab_size"], [20], 37)[0]
    want, _, _ = scored_step(model, "contiguous", prompt, 5, 32)
    L = len(prompt)
    bufs = arm(model, L, 5, 32, prompt[1:] + [0], [5] * (L - 1) + [-1])
    try:
        model.step_embeds(model.embed(dev_ids(prompt)), make_cache(model, "contiguous"), dev_ids(prompt))
        assert_same_records((bufs["ids"], bufs["vals"]), want, "embeds")
    finally:
        model.clear_prompt_logprobs()


def bound_of(logits_row) -> float:
    return 2 * C_MAX * EPS[DT] * float(np.abs(np.asarray(logits_row, np.float64)).max())


def assert_records_close(ids, vals, want_ids, want_vals, bounds, V, what):
    """Rows of records against reference rows: slot 0 and the k-th best VALUE within the row's bound (ids may swap at near-ties); each
    record's values non-increasing, its ids distinct and in range."""
    worst = 0.0
    for r, b in enumerate(bounds):
        best, want_best = vals[r, 1:].astype(np.float64), want_vals[r, 1:].astype(np.float64)
        e0, ek = abs(float(vals[r, 0]) - float(want_vals[r, 0])), float(np.abs(best - want_best).max())
        worst = max(worst, e0 / b, ek / b)
        assert ids[r, 0] == want_ids[r, 0] and e0 <= b, (what, r, vals[r, 0], want_vals[r, 0], b)
        assert ek <= b, (what, r, ek, b)
        assert (np.diff(best) <= 0).all(), (what, r)
        top = ids[r, 1:].tolist()
        assert len(set(top)) == len(top) and all(0 <= i < V for i in top), (what, r)
    print(f"{what}: {len(bounds)} rows, worst error {worst:.3f} of the bound")


def test_decoder_several_blocks_and_chunks(tiny, knobs):
    """L = 40 in chunks of 16, scored in blocks of 8: 8,8 | 8,8 | 8.  The reference's lm_head multiplies 16, 16 and 8 rows at a time."""
    w, cfg, model = tiny
    knobs("prefill_chunk", 16)
    L, n, V = 40, 5, cfg["vocab_size"]
    prompt = repeating_prompts(V, [L], 13)[0]
    got, _, _ = scored_step(model, "contiguous", prompt, n, 8)
    want, logits = op_on_call(model, "contiguous", prompt, n)
    lg = logits.float().cpu().numpy()
    assert got[0][L - 1].eq(SENT_ID).all()
    assert_records_close(got[0].cpu().numpy()[:L - 1], got[1].cpu().numpy()[:L - 1], want[0].cpu().numpy(), want[1].cpu().numpy(),
                         [bound_of(lg[r]) for r in range(L - 1)], V, "chunks")


@pytest.mark.parametrize("kind", ["pages", "quantized", "rotating"])
def test_decoder_on_every_kv_binding(tiny, kind):
    w, cfg, model = tiny
    prompt = repeating_prompts(cfg["vocab_size"], [20], 17)[0]
    got, _, _ = scored_step(model, kind, prompt, 5, 32)
    want, _ = op_on_call(model, kind, prompt, 5)
    assert_same_records(got, want, kind)


# ------------------------------------------------------------------ the varlen passes
@pytest.fixture(scope="module")
def oracle_rows(paged_tiny):
    """Oracle logits of the three prompts' every row, in the many-row regime the passes multiply in: computed once."""
    w, cfg, model = paged_tiny
    prompts = repeating_prompts(cfg["vocab_size"], [7, 12, 20], 19)
    po.set_qmm_min_rows(1)
    try:
        rows = []
        for p in prompts:
            orc = po.OracleLlama(cfg, w, DT)
            rows.append(np.asarray(orc.forward(np.asarray(p, np.int32), [po.OracleKVCache() for _ in orc.layers]), np.float32))
    finally:
        po.set_qmm_min_rows(6)
    return prompts, rows


def reference_rows(prompt, logits, n):
    """numpy records of a prompt's rows but the last, from the oracle's logits."""
    recs = [pref.reference(logits[r], n, target=prompt[r + 1]) for r in range(len(prompt) - 1)]
    return np.stack([r[0] for r in recs]), np.stack([r[1] for r in recs]).view(np.float32)


def test_varlen_passes_against_the_oracle(paged_tiny, oracle_rows):
    w, cfg, model = paged_tiny
    prompts, orc = oracle_rows
    V, n = cfg["vocab_size"], 5
    model.enable_paged_kv(num_pages=24)

    def targets_of(ps):
        t, c = [], []
        for p in ps:
            t += p[1:] + [0]
            c += [n] * (len(p) - 1) + [-1]
        return t, c

    def check(bufs, row0, ps, logits, what):
        r = row0
        for p, lg in zip(ps, logits):
            ids, vals = bufs["ids"][r:r + len(p)].cpu().numpy(), bufs["vals"][r:r + len(p)].cpu().numpy()
            want_ids, want_vals = reference_rows(p, lg, n)
            assert_records_close(ids[:-1], vals[:-1], want_ids, want_vals, [bound_of(lg[k]) for k in range(len(p) - 1)], V, what)
            assert (ids[-1] == SENT_ID).all()                                    # a prompt's last row
            r += len(p)
        assert bufs["ids"][r:].eq(SENT_ID).all() and bufs["ids"][:row0].eq(SENT_ID).all()     # decode rows, and rows beyond the pass's

    try:
        plain = model.prefill_batch(prompts, [model.make_cache() for _ in prompts])
        plain = (plain[0].tolist(), bits_of(plain[1]))
        t, c = targets_of(prompts)
        bufs = arm(model, 48, n, 16, t + [0] * (48 - len(t)), c + [-1] * (48 - len(c)))     # 39 rows: blocks of 16, 16 and 7
        nxt, lp, _ = model.prefill_batch(prompts, [model.make_cache() for _ in prompts])
        assert nxt.tolist() == plain[0] and np.array_equal(bits_of(lp), plain[1])        # the pass's own outputs do not notice
        check(bufs, 0, prompts, orc, "prefill_batch")
        model.clear_prompt_logprobs()
        # two decode rows and one fresh prompt
        dps = repeating_prompts(V, [9, 30], 23)
        dc, dtok = prefilled(model, dps)
        plain = model.step_mixed(dev_ids(dtok), dc, [prompts[1]], [model.make_cache()])
        plain = (plain[0].tolist(), bits_of(plain[1]))
        dc, dtok = prefilled(model, dps)
        t, c = targets_of([prompts[1]])
        bufs = arm(model, 48, n, 16, [0, 0] + t + [0] * (46 - len(t)), [n, n] + c + [-1] * (46 - len(c)))   # the decode rows' counts are not looked at
        nxt, lp, _ = model.step_mixed(dev_ids(dtok), dc, [prompts[1]], [model.make_cache()])
        assert nxt.tolist() == plain[0] and np.array_equal(bits_of(lp), plain[1])
        check(bufs, 2, [prompts[1]], [orc[1]], "step_mixed")
    finally:
        model.clear_prompt_logprobs()


# ------------------------------------------------------------------ the engines
def test_inference_engine_score_and_generate(tiny):
    from proxy_inference_engine_amd import InferenceEngine
    from proxy_inference_engine_amd.engine.inference_engine import prompt_maps
    w, cfg, model = tiny
    prompt = repeating_prompts(cfg["vocab_size"], [20], 29)[0]
    want, _ = op_on_call(model, "contiguous", prompt, 3)
    want_maps = prompt_maps(want[0].cpu().numpy(), want[1].cpu().numpy(), 3)
    eng = InferenceEngine(model=model)
    got = eng.score(prompt, top_logprobs=3)
    assert got == want_maps and got[0] is None and len(got) == len(prompt)
    assert all(prompt[j] in got[j] and len(got[j]) in (3, 4) for j in range(1, len(prompt)))
    own = eng.score(prompt, top_logprobs=0)                                     # the tokens' own log-probabilities alone
    assert [list(m) for m in own[1:]] == [[t] for t in prompt[1:]] and all(own[j][prompt[j]] == got[j][prompt[j]] for j in range(1, len(prompt)))
    assert InferenceEngine(model=model).score(prompt[:1]) == [None]
    plain = [t for t, _ in InferenceEngine(model=model).generate(prompt, max_completion_tokens=6)]
    eng = InferenceEngine(model=model)
    eng.score(prompt[:12], top_logprobs=1)                                      # a cached prefix of the next request: not reused by a scored one
    gen = eng.generate(prompt, max_completion_tokens=6, prompt_logprobs=3)
    first = next(gen)
    assert eng.prompt_logprobs == want_maps                                     # before the first yield
    assert [first[0]] + [t for t, _ in gen] == plain
    want_k, _ = op_on_call(model, "rotating", prompt, 3)                        # the engine's own cache kinds: a ring of max_kv_size rows
    assert InferenceEngine(model=model).score(prompt, top_logprobs=3, max_kv_size=32) == prompt_maps(want_k[0].cpu().numpy(), want_k[1].cpu().numpy(), 3)
    with pytest.raises(ValueError, match="prompt_logprobs"):
        InferenceEngine(model=model).score(prompt, top_logprobs=21)


def test_batched_engine_prompt_maps(paged_tiny):
    from proxy_inference_engine_amd import InferenceEngine
    from proxy_inference_engine_amd.engine import BatchedEngine
    w, cfg, model = paged_tiny
    V = cfg["vocab_size"]
    prompts = repeating_prompts(V, [12, 30, 5, 21], 31)
    wants = [2, None, 0, 5]
    alone, bounds = [], []
    for p, k in zip(prompts, wants):
        alone.append(None if k is None else InferenceEngine(model=model).score(p, top_logprobs=k))
        lg = model(dev_ids(p)[None], cache=make_cache(model, "contiguous"))[0].float().cpu().numpy()
        bounds.append([None] + [bound_of(lg[j - 1]) for j in range(1, len(p))])
    try:
        eng = BatchedEngine(model, num_pages=32, max_batch=4, prefill_chunk=8)
        plain = eng.generate(prompts, 6)
        out, maps = eng.generate(prompts, 6, prompt_logprobs=wants)
        assert out == plain and maps[1] is None
        out2, tok_maps, maps2 = eng.generate(prompts, 6, logprobs=True, top_logprobs=1, prompt_logprobs=wants)
        assert out2 == plain and maps2 == maps and [len(m) for m in tok_maps] == [6] * 4
        for i, (p, k) in enumerate(zip(prompts, wants)):
            if k is None:
                continue
            assert len(maps[i]) == len(p) and maps[i][0] is None
            for j in range(1, len(p)):
                m, a, b = maps[i][j], alone[i][j], bounds[i][j]
                assert p[j] in m and abs(m[p[j]] - a[p[j]]) <= b, (i, j, m, a, b)
                mv, av = list(m.values())[:k], list(a.values())[:k]
                assert len(mv) == len(av) and all(abs(x - y) <= b for x, y in zip(mv, av)), (i, j, m, a, b)
                assert all(x >= y for x, y in zip(mv, mv[1:])) and len(m) in (max(k, 1), k + 1)
        assert eng.generate(prompts, 6) == plain                                 # the arming was cleared
        with pytest.raises(ValueError, match="share_prefix"):
            BatchedEngine(model, num_pages=32, max_batch=4, share_prefix=True).generate(prompts, 2, prompt_logprobs=1)
    finally:
        model.clear_prompt_logprobs()
