"""-m gpu: greedy speculative decoding -- the drafter and the verify against their numpy restatements (exact), the
decoder's speculative pass on the tiny golden models (contiguous and paged caches), the engine end to end, the refusals, and the
untouched plain path.

Prompts are generated from seeds.  Wherever a token is compared with the oracle's, the seed was chosen on the CPU so that at every
generated position the oracle's top-two logit gap exceeds twice the max-abs bound assert_vec_close grants the dtype (margin_ok below);
the tests assert that condition again, so a seed that stops meeting it fails loudly instead of comparing tokens across a near-tie."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests import speculative_reference as ref
from tests._util import EPS, assert_vec_close, codes_dev, to_dev

pytestmark = pytest.mark.gpu
SENT = -77


def dev_ids(ids) -> torch.Tensor:
    return torch.tensor([int(i) for i in ids], dtype=torch.int32, device="cuda")


def bits_of(t: torch.Tensor) -> np.ndarray:
    return t.detach().contiguous().cpu().numpy().view(np.uint32).copy()


# ------------------------------------------------------------------ 1. the drafter against the reference, exact
@pytest.mark.parametrize("alphabet", [4, 50000])
@pytest.mark.parametrize("length", [1, 2, 63, 64, 65, 5000, 70001])
def test_ngram_draft_equals_the_reference(length, alphabet):
    """Lengths around one wave, beyond one workgroup's 2048 ids and (70001, with the grid sized for exactly that many) beyond one
    grid-stride; a 4-symbol alphabet matches at every n, 50000 symbols almost never."""
    from proxy_inference_engine_amd import hip_ops
    rng = np.random.default_rng(length * 7 + alphabet)
    ids = rng.integers(0, alphabet, length).astype(np.int32)
    if alphabet == 4 and length >= 64:                  # a period-3 tail: the copy must run into its own output
        ids[-7:] = np.resize(ids[-10:-7], 7)
    exact = dev_ids(ids)                                # cap == len
    padded = torch.cat([exact, exact[-8:].repeat(40)]) if length >= 8 else torch.cat([exact, exact.repeat(16)])   # beyond len: ids that WOULD match
    n_dev = dev_ids([length])
    ws = hip_ops.ngram_draft_workspace("cuda")
    ws.fill_(-1)                                        # no initialisation needed: garbage must not show
    for nmax, nmin in ((1, 1), (3, 1), (8, 3)):
        for k in (1, 7, 31):
            want = ref.ngram_draft(ids, nmax, nmin, k)
            for buf in (exact, padded):
                out = (torch.full((31,), SENT, dtype=torch.int32, device="cuda"), torch.full((1,), SENT, dtype=torch.int32, device="cuda"))
                draft, count = hip_ops.ngram_draft(buf, n_dev, nmax, nmin, k, workspace=ws, out=out)
                what = (length, alphabet, nmax, nmin, k, buf.numel())
                assert int(count.item()) == len(want), what
                assert draft[:len(want)].tolist() == want, what
                assert draft[len(want):].eq(SENT).all(), what      # no match: out_ids keeps its contents; a match writes k ids only
    if alphabet == 4 and length >= 64:
        assert len(ref.ngram_draft(ids, 3, 1, 31)) == 31           # the periodic tail drafted k ids, not 3


def test_ngram_draft_clamps_len_and_checks_arguments():
    from proxy_inference_engine_amd import _ffi, hip_ops
    ids = dev_ids([5, 1, 9, 5, 2, 8, 5])
    for n in (7, 8, 1 << 30):                           # len above cap acts as cap
        draft, count = hip_ops.ngram_draft(ids, dev_ids([n]), 1, 1, 2)
        assert (int(count.item()), draft.tolist()) == (2, [2, 8])
    draft, count = hip_ops.ngram_draft(ids, dev_ids([-3]), 1, 1, 2)       # below 0 acts as 0
    assert (int(count.item()), draft.tolist()) == (0, [-1, -1])
    draft, count = hip_ops.ngram_draft(ids, dev_ids([4]), 1, 1, 3)        # a prefix: [5, 1, 9, 5] -> the copy runs on into the draft
    assert (int(count.item()), draft.tolist()) == (3, [1, 9, 5])
    n = dev_ids([7])
    for nmax, nmin, k in ((0, 0, 3), (3, 0, 3), (2, 3, 3), (9, 1, 3), (3, 1, 0), (3, 1, 32)):
        with pytest.raises(ValueError, match="pie_ngram_draft"):
            hip_ops.ngram_draft(ids, n, nmax, nmin, k, out=(torch.zeros(40, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")))
    with pytest.raises(ValueError, match="ngram_draft"):
        hip_ops.ngram_draft(ids.long(), n, 3, 1, 3)
    lib, ws, out = _ffi.load(), hip_ops.ngram_draft_workspace("cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    args = lambda ids_p, ws_p, cap=7: (ids_p, _ffi.p(n), cap, 3, 1, 3, _ffi.p(out), _ffi.p(out[4:]), ws_p, _ffi.stream())   # noqa: E731
    assert lib.pie_ngram_draft(*args(_ffi.p(ids), C.c_void_p(ws.data_ptr() + 2))) == -3          # PIE_E_ALIGN
    assert lib.pie_ngram_draft(*args(C.c_void_p(ids.data_ptr() + 1), _ffi.p(ws))) == -3
    assert lib.pie_ngram_draft(*args(_ffi.p(ids), _ffi.p(ws), cap=0)) == -2                      # PIE_E_SHAPE
    assert lib.pie_ngram_draft(*args(_ffi.p(ids), _ffi.p(ws), cap=(1 << 27) + 1)) == -2
    assert lib.pie_ngram_draft(*args(None, _ffi.p(ws))) == -1                                    # PIE_E_ARG
    torch.cuda.synchronize()
    assert out.eq(0).all()                                                                       # each before any launch


# ------------------------------------------------------------------ 2. the verify, exact
def verify_rows(V: int, rows: int, dtype: torch.dtype) -> torch.Tensor:
    rng = np.random.default_rng(V * 31 + rows)
    x = (rng.standard_normal((rows, V)) * 3.0).astype(np.float32)
    return torch.from_numpy(x).to("cuda").to(dtype).contiguous()


def rows_alone(logits):
    """hip_ops.logprobs_argmax of every row alone: (tokens list, [logprobs bits per row])."""
    from proxy_inference_engine_amd import hip_ops
    toks, lps = [], []
    for r in range(logits.shape[0]):
        t, lp = hip_ops.logprobs_argmax(logits[r].contiguous())
        toks.append(int(t.item())), lps.append(lp)
    return toks, torch.stack(lps)


def check_verify(logits, draft, toks, lps, want_acc, what):
    from proxy_inference_engine_amd import hip_ops
    rows, V = logits.shape
    poison = torch.full((rows, V), 123.0, dtype=torch.float32, device="cuda")
    ws = hip_ops.spec_verify_workspace("cuda", rows)
    ws.fill_(-1)
    out = (torch.full((rows,), SENT, dtype=torch.int32, device="cuda"), torch.full((1,), SENT, dtype=torch.int32, device="cuda"))
    tokens, n = hip_ops.spec_verify(logits, dev_ids(draft), logprobs=poison, workspace=ws, out=out)
    n_acc, want_tokens = ref.accept(toks, draft)
    assert n_acc == want_acc, what                                     # the case is what it claims to be
    assert int(n.item()) == n_acc + 1 and tokens.tolist() == want_tokens, what
    assert torch.equal(poison[:n_acc + 1].view(torch.int32), lps[:n_acc + 1].view(torch.int32)), what     # written rows: logprobs_argmax's bits
    assert poison[n_acc + 1:].eq(123.0).all(), what                    # rows behind the accepted run: untouched
    tokens2, n2 = hip_ops.spec_verify(logits, dev_ids(draft))          # without logprobs: the same decision
    assert int(n2.item()) == n_acc + 1 and tokens2.tolist() == want_tokens, what


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("V", [1000, 32003, 128256])
def test_spec_verify_equals_the_rows_alone(V, dtype):
    """V & 7 != 0 and fewer ids than 256 tiles x 8; an odd vocabulary; a real one.  Per row count: drafts built from the rows' own argmax
    that accept 0, 1, rows - 2 and all; a duplicated maximum; draft ids -1 and V."""
    for rows in (2, 6, 8, 17, 32):
        logits = verify_rows(V, rows, dtype)
        r_dup = rows // 2                                              # a duplicated maximum in a row: the lower id wins
        lo, hi = 17, V - 5
        logits[r_dup, lo] = logits[r_dup, hi] = 60.0
        toks, lps = rows_alone(logits)
        assert toks[r_dup] == lo
        good = toks[:rows - 1]
        for acc in sorted({0, 1, rows - 2, rows - 1}):
            draft = list(good)
            if acc < rows - 1:
                draft[acc] = (good[acc] + 1) % V                       # the first wrong draft
            check_verify(logits, draft, toks, lps, acc, (V, rows, dtype, "accept", acc))
        if r_dup < rows - 1:                                           # a draft naming the higher id of the tie is rejected
            draft = list(good)
            draft[r_dup] = hi
            check_verify(logits, draft, toks, lps, r_dup, (V, rows, dtype, "tie"))
        for bad in (-1, V):                                            # never accepted, never an index
            for at in sorted({0, rows - 2}):
                draft = list(good)
                draft[at] = bad
                check_verify(logits, draft, toks, lps, at, (V, rows, dtype, "id", bad, at))


def test_spec_verify_checks_arguments():
    from proxy_inference_engine_amd import _ffi, hip_ops
    x = verify_rows(100, 4, torch.bfloat16)
    for rows in (1, 33):
        with pytest.raises(ValueError, match="spec_verify"):
            hip_ops.spec_verify(verify_rows(100, rows, torch.bfloat16), dev_ids([0] * (rows - 1)), workspace=hip_ops.spec_verify_workspace("cuda", 2))
    with pytest.raises(ValueError, match="draft"):
        hip_ops.spec_verify(x, dev_ids([0, 0]))
    with pytest.raises(ValueError, match="logits"):
        hip_ops.spec_verify(x.float(), dev_ids([0, 0, 0]))
    lib, ws, out, d = _ffi.load(), hip_ops.spec_verify_workspace("cuda", 4), torch.zeros(8, dtype=torch.int32, device="cuda"), dev_ids([0, 0, 0])
    args = lambda x_p, ws_p, rows=4, V=100, dt=_ffi.PIE_BF16: (x_p, rows, V, dt, _ffi.p(d), _ffi.p(out), _ffi.p(out[4:]), None, ws_p, _ffi.stream())   # noqa: E731
    assert lib.pie_spec_verify(*args(_ffi.p(x), C.c_void_p(ws.data_ptr() + 8))) == -3             # PIE_E_ALIGN
    assert lib.pie_spec_verify(*args(C.c_void_p(x.data_ptr() + 1), _ffi.p(ws))) == -3
    assert lib.pie_spec_verify(*args(_ffi.p(x), _ffi.p(ws), rows=1)) == -2 and lib.pie_spec_verify(*args(_ffi.p(x), _ffi.p(ws), V=0)) == -2
    assert lib.pie_spec_verify(*args(_ffi.p(x), _ffi.p(ws), dt=3)) == -1 and lib.pie_spec_verify(*args(None, _ffi.p(ws))) == -1
    torch.cuda.synchronize()
    assert out.eq(0).all()                                                                        # each before any launch


# ------------------------------------------------------------------ the tiny golden models and their oracle continuations
MODELS = {"tiny_llama_w4_bf16": None, "tiny_dense_f16_bias": None}


def load_tiny(golden_dir, name):
    """(cfg, dtype name, oracle, model) of a golden fixture, built once per session."""
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    if MODELS[name] is None:
        g = np.load(golden_dir / f"{name}.npz")
        dt = str(g["dtype"])
        cfg = json.loads(str(g["config_json"]))
        w = {k[2:]: g[k] for k in g.files if k.startswith("w:")}
        dev_w = {k: (codes_dev(v) if v.dtype == np.uint32 else to_dev(v, dt)) for k, v in w.items()}
        MODELS[name] = (cfg, dt, po.OracleLlama(cfg, w, dt), Model(ModelArgs(**cfg), dev_w))
    return MODELS[name]


def margin_ok(logits, dt) -> bool:
    """The oracle's top-two gap exceeds twice the max-abs bound assert_vec_close grants: the greedy token is comparable."""
    top = np.sort(logits)[-2:]
    return float(top[1] - top[0]) > 2 * 4.0 * EPS[dt] * float(np.abs(logits).max())


ORACLE_RUNS: dict = {}


def oracle_run(golden_dir, name, prompt, n):
    """The oracle's greedy continuation of `prompt`: (tokens [n], logits [n, V]) -- logits[i] chose tokens[i]; every position's margin
    is asserted.  Computed once per (model, prompt)."""
    key = (name, tuple(int(t) for t in prompt), n)
    if key not in ORACLE_RUNS:
        cfg, dt, orc, _ = load_tiny(golden_dir, name)
        cache = [po.OracleKVCache() for _ in orc.layers]
        lg = orc.forward(np.asarray(prompt), cache, last_only=True)
        toks, rows = [], []
        for i in range(n):
            assert margin_ok(lg, dt), f"{name}: position {i} of the oracle's continuation is a near-tie: choose another seed"
            toks.append(int(np.argmax(lg))), rows.append(lg)
            if i + 1 < n:
                lg = orc.forward(np.array([toks[-1]]), cache)[0]
        ORACLE_RUNS[key] = (toks, np.stack(rows))
    return ORACLE_RUNS[key]


def fresh_cache(model, kind):
    from proxy_inference_engine_amd.cache import ReusableKVCache
    if kind == "contiguous":
        return [ReusableKVCache() for _ in model.layers]
    return model.make_paged_cache(num_pages=8, max_blocks=1)          # a one-block table: every new page re-binds a longer one


# seeds chosen on the CPU (see the module docstring): prompt = default_rng(1000 * o + seed).integers(0, V, o)
STEP_SEEDS = {("tiny_llama_w4_bf16", 60): 5, ("tiny_llama_w4_bf16", 252): 10, ("tiny_dense_f16_bias", 60): 0, ("tiny_dense_f16_bias", 252): 0}
M_DRAFT, FURTHER = 7, 12


@pytest.mark.parametrize("kind", ["contiguous", "pages"])
@pytest.mark.parametrize("o", [60, 252])
@pytest.mark.parametrize("name", list(MODELS))
def test_spec_step_leaves_the_decoder_where_greedy_steps_would(golden_dir, name, o, kind):
    """o + m + 1 = 68 / 260 crosses a 64-row page boundary (and 256, the contiguous cache's growth step); o + n_acc + 1 stays below it
    when the first draft is wrong and crosses it too when all are right.  Drafts: the oracle's continuation, corrupted at 0, 2, last,
    and uncorrupted."""
    from proxy_inference_engine_amd import hip_ops
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    V, m = cfg["vocab_size"], M_DRAFT
    prompt = np.random.default_rng(1000 * o + STEP_SEEDS[(name, o)]).integers(0, V, o)
    cont, ologits = oracle_run(golden_dir, name, prompt, m + 1 + FURTHER + 1)
    for corrupt in (0, 2, m - 1, None):
        what = f"{name} o={o} {kind} corrupt={corrupt}"
        draft = cont[1:m + 1]
        if corrupt is not None:
            draft[corrupt] = (draft[corrupt] + 1) % V
        n_acc = m if corrupt is None else corrupt
        twin = fresh_cache(model, kind)                                  # first: the twin's calls move the model's device-side state
        model.step(dev_ids(prompt), twin)
        want_block = model(dev_ids([cont[0]] + draft)[None], cache=twin)[0].clone()
        cache = fresh_cache(model, kind)
        tok, _, _ = model.step(dev_ids(prompt), cache)
        assert int(tok.item()) == cont[0], what
        poison = model._spec_state()["logprobs"]
        poison.fill_(123.0)
        tokens, n, lps = model.spec_step(dev_ids(draft), cache)
        block = model.spec_logits(m + 1).clone()
        assert n == n_acc + 1 and tokens.tolist() == cont[1:n_acc + 2], what
        assert all(c.offset == o + n_acc + 1 for c in cache), what
        assert model.spec_tokens[n:m + 1].eq(-1).all() and poison[n:].eq(123.0).all(), what
        # the block is Model.__call__'s on the same ids at the same offset, bit for bit, and the rows' log-probabilities are the op's
        assert torch.equal(block.view(torch.int16), want_block.view(torch.int16)), what
        for r in range(n):
            assert torch.equal(lps[r].view(torch.int32), hip_ops.logprobs_argmax(block[r].contiguous())[1].view(torch.int32)), what
        # the ids by position and the history are whole up to the token about to be fed
        seq = list(prompt) + cont[:n_acc + 2]
        assert model.fed_ids[:len(seq)].tolist() == seq, what
        assert model.history[o:len(seq)].tolist() == cont[:n_acc + 2], what
        # plain steps right after: the last accepted token is fed back, and nothing reads the rejected drafts' rows
        for k in range(FURTHER):
            tok, lp, logits = model.step(None, cache)
            i = n_acc + 1 + k                                          # the position o + i was fed cont[i]
            assert_vec_close(logits.float().cpu().numpy(), ologits[i + 1], dt, what=f"{what} step {k}")
            assert int(tok.item()) == cont[i + 1], f"{what} step {k}"
        assert all(c.offset == o + n_acc + 1 + FURTHER for c in cache), what


# ------------------------------------------------------------------ end to end
# seeds chosen on the CPU: the schedule has a fully accepted pass, a partly rejected pass and a fallback step, and every one of the
# positions meets margin_ok
E2E_SEEDS = {"tiny_llama_w4_bf16": [3125, 5510], "tiny_dense_f16_bias": [94]}
E2E_TOKENS = 48


def e2e_prompt(seed, V):
    rng = np.random.default_rng(seed)
    per, reps = int(rng.integers(3, 12)), int(rng.integers(2, 6))
    base = rng.integers(0, V, per)
    return np.concatenate([np.tile(base, reps), rng.integers(0, V, int(rng.integers(0, 6)))])


@pytest.mark.parametrize("kind", ["contiguous", "pages"])
@pytest.mark.parametrize("name", list(MODELS))
def test_engine_generates_greedy_tokens_on_the_simulated_schedule(golden_dir, name, kind):
    from proxy_inference_engine_amd import InferenceEngine, SpeculativeParams
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    sp = SpeculativeParams(num_draft=7, ngram_max=3, ngram_min=1, min_draft=5)
    for seed in E2E_SEEDS[name]:
        prompt = e2e_prompt(seed, cfg["vocab_size"])
        cont, _ = oracle_run(golden_dir, name, prompt, E2E_TOKENS + 12)
        full = [int(t) for t in prompt] + cont
        want, schedule = ref.simulate(prompt, lambda s: full[len(s)], E2E_TOKENS, sp.num_draft, sp.ngram_max, sp.ngram_min, sp.min_draft, model.spec_min_rows)
        kinds = {("full" if e[2] == e[1] else "partial") if e[0] == "pass" else "step" for e in schedule}
        assert kinds == {"full", "partial", "step"}, (name, seed, schedule)

        def engine():
            eng = InferenceEngine(model=model)
            eng.prompt_cache.cache = fresh_cache(model, kind)
            eng.prepare_engine(prompt, temp=0)
            return eng

        plain = [t for t, _ in engine().generate(torch.from_numpy(prompt), max_completion_tokens=E2E_TOKENS)]
        assert plain == cont[:E2E_TOKENS], (name, seed)
        eng = engine()
        gen = eng.generate_step(torch.from_numpy(prompt), speculative=sp, top_logprobs=3)
        got, yielded = [], []
        while len(got) < E2E_TOKENS:
            tokens, rows = next(gen)
            assert rows.shape == (tokens.numel(), cfg["vocab_size"]) and rows.argmax(dim=1).tolist() == tokens.tolist()
            assert eng.top_record[0].shape == (tokens.numel(), 4) and eng.top_record[0][:, 0].tolist() == tokens.tolist()
            got += tokens.tolist()
            yielded.append(tokens.numel())
        assert got == want[:len(got)] == cont[:len(got)], (name, seed)
        done = schedule[:len(yielded) - 1]
        assert yielded[1:] == [e[2] + 1 if e[0] == "pass" else 1 for e in done], (name, seed)      # the exact (n_draft, n_acc) schedule
        passes = [e for e in done if e[0] == "pass"]
        assert eng.spec_stats == {"passes": len(passes), "steps": len(done) - len(passes), "drafted": sum(e[1] for e in passes),
                                  "accepted": sum(e[2] for e in passes)}
        assert eng.prompt_cache.computed_ids == full[:eng.prompt_cache.cache[0].offset]
        # generate(): the same tokens one by one, a log-probability map per token, the budget cut inside a run
        out = list(engine().generate(torch.from_numpy(prompt), speculative=sp, max_completion_tokens=E2E_TOKENS - 1, logprobs=True, top_logprobs=2))
        assert [t for t, _ in out] == cont[:E2E_TOKENS - 1]
        assert all(t in mp and len(mp) in (2, 3) and max(mp, key=mp.get) == t for t, mp in out)


# ------------------------------------------------------------------ refusals, by name
def test_refusals_by_name(golden_dir):
    from proxy_inference_engine_amd import _ffi, hip_ops
    from proxy_inference_engine_amd.cache import QuantizedKVCache, RotatingKVCache
    cfg, dt, orc, model = load_tiny(golden_dir, "tiny_llama_w4_bf16")
    V = cfg["vocab_size"]
    prompt = dev_ids(np.random.default_rng(5).integers(0, V, 20))
    draft = dev_ids([1] * 7)
    for cache, name in (([QuantizedKVCache(group_size=64, bits=8) for _ in model.layers], "QuantizedKVCache"),
                        ([RotatingKVCache(32, keep=4) for _ in model.layers], "RotatingKVCache")):
        model.step(prompt, cache)
        with pytest.raises(ValueError, match=name):
            model.spec_step(draft, cache)
    cache = fresh_cache(model, "contiguous")
    model.step(prompt, cache)
    for m in (4, 32):                                                  # 5 rows: below the many-row pass; 33 rows: above the verify
        with pytest.raises(ValueError, match="rows"):
            model.spec_step(dev_ids([1] * m), cache)
    tails = (dict(sampler=("top_k", 0.8, 0.0, 5)), dict(repetition_penalty=1.2), dict(token_mask=hip_ops.pack_token_mask(torch.ones(V, dtype=torch.bool), V)),
             dict(logit_bias=([1, 2], [0.5, -0.5])), dict(top_logprobs=3), dict(frequency_penalty=0.5, count_start=20))
    lib, st = _ffi.load(), model._spec_state()
    rec = st["rec"]

    def raw_call(n_draft):
        return lib.pie_decoder_spec_step(model._dec, _ffi.p(draft), n_draft, _ffi.p(rec[1:]), _ffi.p(rec[0:]), None, _ffi.p(st["ws"]), None, 0, None, _ffi.stream())

    try:
        for kw in tails:
            model.set_step_tail(**kw)
            with pytest.raises(ValueError, match="greedy and raw"):
                model.spec_step(draft, cache)
            assert raw_call(7) == -5, kw                               # PIE_E_STATE from the library too, before any launch
            model.set_step_tail()
        bufs = model.set_prompt_logprobs(8, 3, 16)
        bufs["count"].fill_(-1)
        assert raw_call(7) == -5
        model.clear_prompt_logprobs()
        assert raw_call(4) == -2 and raw_call(32) == -2 and raw_call(0) == -2      # PIE_E_SHAPE: row bounds
        assert int(lib.pie_decoder_spec_workspace_bytes(model._dec, 1)) == 0 and int(lib.pie_decoder_spec_workspace_bytes(model._dec, 33)) == 0
    finally:
        model.set_step_tail()
        model.clear_prompt_logprobs()
    before = all(c.offset == 20 for c in cache)
    tokens, n, _ = model.spec_step(draft, cache)                       # and after all that the pass still runs
    assert before and 1 <= n <= 8 and all(c.offset == 20 + n for c in cache)


def test_refusals_on_int8_pages_and_through_the_engine(golden_dir):
    from proxy_inference_engine_amd import InferenceEngine, SpeculativeParams
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    g = np.load(golden_dir / "tiny_llama_w4_bf16.npz")
    cfg = json.loads(str(g["config_json"]))
    w = {k[2:]: g[k] for k in g.files if k.startswith("w:")}
    model = Model(ModelArgs(**cfg), {k: (codes_dev(v) if v.dtype == np.uint32 else to_dev(v, "bfloat16")) for k, v in w.items()})
    model.enable_paged_kv(num_pages=8, max_blocks=2, kv_dtype=torch.int8)
    cache = model.make_cache()
    model.step(dev_ids(g["prompt"][:4]), cache)
    with pytest.raises(ValueError, match="int8 KV pages"):
        model.spec_step(dev_ids([1] * 7), cache)
    eng = InferenceEngine(model=model)
    eng.prepare_engine(g["prompt"], temp=0)
    with pytest.raises(ValueError, match="int8 KV pages"):
        next(eng.generate_step(torch.from_numpy(g["prompt"]), speculative=SpeculativeParams()))
    for kw, name in ((dict(kv_bits=8), "kv_bits"), (dict(max_kv_size=64), "max_kv_size")):
        with pytest.raises(ValueError, match=name):
            next(eng.generate_step(torch.from_numpy(g["prompt"]), speculative=SpeculativeParams(), **kw))


# ------------------------------------------------------------------ the untouched plain path
def test_plain_generation_is_the_same_before_and_after_a_speculative_one(golden_dir):
    from proxy_inference_engine_amd import InferenceEngine, SpeculativeParams
    cfg, dt, orc, model = load_tiny(golden_dir, "tiny_llama_w4_bf16")
    prompt = e2e_prompt(E2E_SEEDS["tiny_llama_w4_bf16"][0], cfg["vocab_size"])

    def plain():
        eng = InferenceEngine(model=model)
        eng.prompt_cache.cache = fresh_cache(model, "contiguous")
        eng.prepare_engine(prompt, temp=0)
        gen = eng.generate_step(torch.from_numpy(prompt))
        toks, bits = [], []
        for _ in range(24):
            t, lp = next(gen)
            toks.append(int(t.item())), bits.append(bits_of(lp))
        return toks, np.stack(bits), model.graph_launches()

    toks0, bits0, launches0 = plain()
    eng = InferenceEngine(model=model)
    eng.prompt_cache.cache = fresh_cache(model, "contiguous")
    eng.prepare_engine(prompt, temp=0)
    spec = [t for t, _ in eng.generate(torch.from_numpy(prompt), speculative=SpeculativeParams(), max_completion_tokens=24)]
    assert eng.spec_stats["passes"] >= 1
    toks1, bits1, launches1 = plain()
    assert launches0 > 0 and launches1 == launches0                    # the captured step's kernel count
    assert toks1 == toks0 == spec and np.array_equal(bits0, bits1)
