"""-m gpu: speculative decoding under a sampler, a repetition penalty and a logit bias -- the op against the rows alone
(exact), its argument checks, the decoder's pass under a configured tail against a block built only from existing ops (exact) with the
plain configured steps behind it, the engine through the stochastic path (deterministic with top_k = 1, really random with top-p), and
the untouched greedy and plain paths.

The random stream is the samplers' own (samplers._rng): one seed and one device-side call counter.  A test that calls hip_ops.sample to
restate a draw sets the counter to the stream position it restates and puts back the position the code under test left."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests import sampler_rows
from tests import spec_sampled_reference as sref
from tests import speculative_reference as ref
from tests._util import assert_vec_close
from tests.test_gpu_speculative import E2E_SEEDS, E2E_TOKENS, MODELS, bits_of, dev_ids, e2e_prompt, fresh_cache, load_tiny, oracle_run

pytestmark = pytest.mark.gpu
SENT = -77
SEED = 20240607


def stream():
    """(seed, counter) of the samplers' stream on the test device, under the tests' fixed seed."""
    from proxy_inference_engine_amd.samplers import _rng
    if _rng._hip_seed != SEED:
        _rng.seed(SEED)
    return _rng.hip_state(torch.device("cuda", torch.cuda.current_device()))


def set_position(c: int) -> None:
    stream()[1].copy_(torch.tensor([int(c), 0], dtype=torch.int64))


def position() -> list[int]:
    return stream()[1].tolist()


def draw_at(lp: torch.Tensor, c: int, spec, xtc=None) -> int:
    """hip_ops.sample of one row of log-probabilities at stream position c (the counter is left at c + 1)."""
    from proxy_inference_engine_amd import hip_ops
    set_position(c)
    return int(hip_ops.sample(lp.contiguous(), *spec, xtc=xtc).item())


# ------------------------------------------------------------------ 1. the op equals the rows alone
def op_settings():
    from proxy_inference_engine_amd import hip_ops
    return [(("categorical", 0.7, 0.0, 0), None), (("top_k", 1.0, 0.0, 5), None), (("top_p", 0.8, 0.9, 0), hip_ops.xtc_pack(0.6, 0.1, (3,))),
            (("min_p", 1.3, 0.05, 3), None)]


def op_rows(V: int, rows: int, dtype: torch.dtype) -> torch.Tensor:
    """Rows of logits [rows, V]: random ones and sampler_rows' designed families (exact ties, a sparse row of -inf, a one-hot row) in turn."""
    rng = np.random.default_rng(V * 31 + rows)
    makers = [None, lambda s: sampler_rows.quantized(V, s), lambda s: sampler_rows.sparse(V, 600, s), lambda s: sampler_rows.one_hot(V, s),
              lambda s: sampler_rows.wide_tie(V, s), None, lambda s: sampler_rows.topp_tie(V, s), lambda s: sampler_rows.sparse(V, 3, s)]
    out = []
    for r in range(rows):
        make = makers[r % len(makers)]
        out.append((rng.standard_normal(V) * 3.0).astype(np.float32) if make is None else make(r).lp)
    return torch.from_numpy(np.stack(out)).to("cuda").to(dtype).contiguous()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows", [2, 8, 32])
@pytest.mark.parametrize("V", [1000, 32003, 128256])
def test_spec_verify_sampled_equals_the_rows_alone(V, rows, dtype):
    """V & 7 != 0 and fewer ids than 256 tiles x 8; an odd vocabulary; a real one.  Per setting the rows' tokens come from hip_ops.sample of
    each row alone at {c + r, 0}; the drafts are those tokens corrupted at 0, 2, the last position and nowhere, and with an id outside
    [0, V).  One workspace, zeroed once, serves every call."""
    from proxy_inference_engine_amd import hip_ops
    logits = op_rows(V, rows, dtype)
    lps = torch.stack([hip_ops.logprobs_argmax(logits[r].contiguous())[1] for r in range(rows)])
    ws = hip_ops.spec_verify_sampled_workspace("cuda", rows, V)
    c = 0
    for si, (spec, xtc) in enumerate(op_settings()):
        c = c * 3 + 5 + si                                                   # a nonzero start, another one per setting
        toks = [draw_at(lps[r], p, spec, xtc) for r, p in enumerate(sref.stream_positions(c, rows))]
        good = toks[:rows - 1]
        drafts = []
        for at in sorted({0, 2, rows - 2} & set(range(rows - 1))) + [None]:
            d = list(good)
            if at is not None:
                d[at] = (good[at] + 1) % V
            drafts.append(d)
        for bad in (-1, V):
            d = list(good)
            d[min(1, rows - 2)] = bad
            drafts.append(d)
        for draft in drafts:
            what = (V, rows, dtype, spec[0], draft[:4])
            n_acc, want_tokens = sref.accept(toks, draft, V)
            poison = torch.full((rows, V), 123.0, dtype=torch.float32, device="cuda")
            out = (torch.full((rows,), SENT, dtype=torch.int32, device="cuda"), torch.full((1,), SENT, dtype=torch.int32, device="cuda"))
            set_position(c)
            tokens, n, got_lps = hip_ops.spec_verify_sampled(logits, dev_ids(draft), *spec, xtc=xtc, logprobs=poison, workspace=ws, out=out)
            assert int(n.item()) == n_acc + 1 and tokens.tolist() == want_tokens, what
            assert torch.equal(got_lps.view(torch.int32), lps.view(torch.int32)), what       # EVERY row: logprobs_argmax's bits
            assert position() == list(sref.counter_after(c, n_acc)), what


# ------------------------------------------------------------------ 2. the op's argument checks
def test_spec_verify_sampled_checks_arguments():
    from proxy_inference_engine_amd import _ffi, hip_ops
    x = torch.randn((4, 100), device="cuda").to(torch.bfloat16)
    with pytest.raises(ValueError, match="spec_verify_sampled"):
        hip_ops.spec_verify_sampled(torch.randn((33, 100), device="cuda").to(torch.bfloat16), dev_ids([0] * 32), "top_k", 1.0, 0.0, 5, workspace=torch.zeros(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="draft"):
        hip_ops.spec_verify_sampled(x, dev_ids([0, 0]), "top_k", 1.0, 0.0, 5)
    with pytest.raises(ValueError, match="logits"):
        hip_ops.spec_verify_sampled(x.float(), dev_ids([0, 0, 0]), "top_k", 1.0, 0.0, 5)
    with pytest.raises(ValueError, match="mode"):
        hip_ops.spec_verify_sampled(x, dev_ids([0, 0, 0]), "greedy", 1.0)
    for spec in (("top_k", 1.0, 0.0, 0), ("top_k", 1.0, 0.0, 100), ("top_p", 1.0, 1.0, 0), ("min_p", 1.0, 0.0, 1), ("categorical", 0.0, 0.0, 0)):
        with pytest.raises(ValueError, match="pie_spec_verify_sampled"):                         # pie_sample's parameter rules, under this op's name
            hip_ops.spec_verify_sampled(x, dev_ids([0, 0, 0]), *spec)
    lib = _ffi.load()
    assert int(lib.pie_spec_verify_sampled_workspace_bytes(1, 100)) == 0 and int(lib.pie_spec_verify_sampled_workspace_bytes(33, 100)) == 0
    assert int(lib.pie_spec_verify_sampled_workspace_bytes(4, 524289)) == 0 and int(lib.pie_spec_verify_sampled_workspace_bytes(4, 0)) == 0
    ws, out, d = hip_ops.spec_verify_sampled_workspace("cuda", 4, 100), torch.zeros(8, dtype=torch.int32, device="cuda"), dev_ids([0, 0, 0])
    lp = torch.full((4, 100), 123.0, dtype=torch.float32, device="cuda")
    seed, counter = stream()
    set_position(9)

    def call(x_p=None, ws_p=None, rows=4, V=100, dt=_ffi.PIE_BF16, mode=1, k=5, counter_p=None, lp_p=None):
        return lib.pie_spec_verify_sampled(_ffi.p(x) if x_p is None else x_p, rows, V, dt, _ffi.p(d), mode, 1.0, 0.0, k, seed,
                                           _ffi.p(counter) if counter_p is None else counter_p, None, _ffi.p(out), _ffi.p(out[4:]),
                                           _ffi.p(lp) if lp_p is None else lp_p, _ffi.p(ws) if ws_p is None else ws_p, _ffi.stream())

    assert call(ws_p=C.c_void_p(ws.data_ptr() + 8)) == -3 and call(x_p=C.c_void_p(x.data_ptr() + 1)) == -3      # PIE_E_ALIGN
    assert call(counter_p=C.c_void_p(counter.data_ptr() + 4)) == -3
    assert call(rows=1) == -2 and call(rows=33) == -2 and call(V=0) == -2 and call(V=524289) == -2             # PIE_E_SHAPE
    assert call(dt=3) == -1 and call(x_p=C.c_void_p(None)) == -1 and call(lp_p=C.c_void_p(None)) == -1          # PIE_E_ARG (logprobs is required)
    assert call(counter_p=C.c_void_p(None)) == -1 and call(mode=4) == -1 and call(k=100) == -1
    assert call(mode=-1) == -1                                                                                  # PIE_SAMPLE_GREEDY: use pie_spec_verify
    torch.cuda.synchronize()
    assert out.eq(0).all() and lp.eq(123.0).all() and position() == [9, 0] and ws.eq(0).all()                   # each before any launch
    assert call() == 0                                                                                          # and the same arguments, in range, run
    torch.cuda.synchronize()
    assert 1 <= int(out[4].item()) <= 4 and position() == [9 + int(out[4].item()), 0]


# ------------------------------------------------------------------ 3. the decoder's pass, teacher-forced
M_DRAFT, FURTHER, C0 = 7, 12, 11
BIAS = ([5, 17, 300, 17, 100000], [4.0, -3.0, 2.5, 9.0, 1.0])               # a duplicate id (the first entry holds it) and an id outside the vocabulary
TAILS = {
    "top_p+penalty+bias": dict(sampler=("top_p", 0.8, 0.9, 0), repetition_penalty=1.3, context_size=20, logit_bias=BIAS),
    "top_k+xtc": dict(sampler=("top_k", 1.0, 0.0, 8), xtc=(0.6, 0.1, (3,))),
    "greedy+penalty": dict(repetition_penalty=1.3, context_size=60),
}
PASS_SEEDS = {60: 1, 252: 2}


def process_row(row: torch.Tensor, window, tail) -> torch.Tensor:
    """One raw row under the tail's edits, by the ops: the repetition penalty over `window`, then the bias."""
    from proxy_inference_engine_amd import hip_ops
    row = row.clone().contiguous()
    if tail.get("repetition_penalty", 1.0) != 1.0:
        hip_ops.logits_penalty(row, dev_ids(window), tail["repetition_penalty"])
    if tail.get("logit_bias") is not None:
        hip_ops.logits_bias(row, dev_ids(tail["logit_bias"][0]), torch.tensor(tail["logit_bias"][1], dtype=torch.float32, device="cuda"))
    return row


def row_token(row: torch.Tensor, c: int, tail):
    """(token, log-probabilities) of one processed row drawn at stream position c (the argmax under the greedy sampler)."""
    from proxy_inference_engine_amd import hip_ops
    tok, lp = hip_ops.logprobs_argmax(row)
    if tail.get("sampler") is None:
        return int(tok.item()), lp
    xtc = None if tail.get("xtc") is None else hip_ops.xtc_pack(*tail["xtc"])
    return draw_at(lp, c, tail["sampler"], xtc), lp


def twin_pass(model, kind, prompt, fed, draft, tail, c):
    """What a pass over [fed] + draft at the prompt's end must leave, from existing ops only: Model.__call__ on a twin cache gives the raw
    block; per row the penalty over the rule's window, the bias, logprobs_argmax and hip_ops.sample at {c + r, 0}."""
    model.set_step_tail()
    twin = fresh_cache(model, kind)
    model(dev_ids(prompt)[None], cache=twin)
    raw = model(dev_ids([fed] + list(draft))[None], cache=twin)[0]
    o, ctx = len(prompt), tail.get("context_size", 60)
    block, lps, toks = [], [], []
    for r in range(len(draft) + 1):
        row = process_row(raw[r], sref.row_window(prompt, fed, draft, o, r, ctx), tail)
        tok, lp = row_token(row, c + r, tail)
        block.append(row), lps.append(lp), toks.append(tok)
    return torch.stack(block), torch.stack(lps), toks


def oracle_processed(row: np.ndarray, window, tail, dt: str) -> np.ndarray:
    """The oracle's logits of one position under the tail's edits, in numpy on storage bits (fp32 arithmetic, one rounding each)."""
    bits = po.to_bits(row, dt)
    if tail.get("repetition_penalty", 1.0) != 1.0:
        ids = np.unique([i for i in window if 0 <= i < bits.size]).astype(np.int64)
        s = po.from_bits(bits[ids], dt)
        bits[ids] = po.to_bits(np.where(s < 0, s * np.float32(tail["repetition_penalty"]), s / np.float32(tail["repetition_penalty"])).astype(np.float32), dt)
    seen = set()
    for i, b in zip(*tail.get("logit_bias", ((), ()))):
        if 0 <= i < bits.size and i not in seen:
            bits[i] = po.to_bits(np.array([po.from_bits(bits[i:i + 1], dt)[0] + np.float32(b)], np.float32), dt)[0]
        seen.add(i)
    return po.from_bits(bits, dt)


ORACLE_PROMPTS: dict = {}


def oracle_after_prompt(golden_dir, name, prompt):
    """The oracle's cache behind `prompt`, computed once per (model, prompt); callers deep-copy it."""
    key = (name, tuple(prompt))
    if key not in ORACLE_PROMPTS:
        orc = load_tiny(golden_dir, name)[2]
        cache = [po.OracleKVCache() for _ in orc.layers]
        orc.forward(np.asarray(prompt), cache, last_only=True)
        ORACLE_PROMPTS[key] = cache
    return copy.deepcopy(ORACLE_PROMPTS[key])


@pytest.mark.parametrize("tail_name", list(TAILS))
@pytest.mark.parametrize("kind", ["contiguous", "pages"])
@pytest.mark.parametrize("o", [60, 252])
@pytest.mark.parametrize("name", list(MODELS))
def test_spec_step_tail_equals_the_rows_alone_and_leaves_plain_steps_whole(golden_dir, name, o, kind, tail_name):
    """o + m + 1 = 68 / 260 crosses a 64-row page boundary (and 256, the contiguous cache's growth step)."""
    tail_pass_case(golden_dir, name, o, kind, tail_name, TAILS[tail_name], M_DRAFT)


# The edges of a row's penalty window (row r at position o + r covers max(0, o + r + 1 - context) .. o + r), which the cases above do not
# reach: a window of the row's own input alone, in the fewest rows a pass can have; one that begins at position 0 in every row of the
# largest pass; and the largest window, full, in front of positions >= 1024.
WINDOW_EDGES = {
    "context=1, 2 rows": (60, 1, dict(sampler=("top_p", 0.8, 0.9, 0), repetition_penalty=1.3, context_size=1)),
    "position + 1 < context, 32 rows": (60, 31, dict(repetition_penalty=1.3, context_size=100)),
    "context=1024 at positions >= 1024": (1030, M_DRAFT, dict(repetition_penalty=1.3, context_size=1024)),
}


@pytest.mark.parametrize("edge", list(WINDOW_EDGES))
def test_spec_step_tail_window_edges(golden_dir, knobs, edge):
    o, m, tail = WINDOW_EDGES[edge]
    if m + 1 < 6:
        knobs("prefill_min", m + 1)                                          # the many-row pass from 2 rows on
    tail_pass_case(golden_dir, "tiny_llama_w4_bf16", o, "contiguous", edge, tail, m)


def tail_pass_case(golden_dir, name, o, kind, tail_name, tail, m):
    """The agreeing continuation is built row by row (row r's token depends on the drafts before it only): m + 1 twin passes; then one
    twin pass per corrupted draft."""
    from proxy_inference_engine_amd import hip_ops
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    V = cfg["vocab_size"]
    draws = tail.get("sampler") is not None
    xtc = None if tail.get("xtc") is None else hip_ops.xtc_pack(*tail["xtc"])
    prompt = [int(t) for t in np.random.default_rng(1000 * o + PASS_SEEDS.get(o, 3)).integers(0, V, o)]
    ctx = tail.get("context_size", 60)
    try:
        # the prompt's own step: the last prompt row under the tail, drawn at C0
        model.set_step_tail()
        raw_last = model(dev_ids(prompt)[None], cache=fresh_cache(model, kind))[0, -1]
        fed, _ = row_token(process_row(raw_last, prompt[-ctx:], tail), C0, tail)
        c = C0 + 1 if draws else C0
        good = [0] * m
        for r in range(m + 1):
            toks = twin_pass(model, kind, prompt, fed, good, tail, c)[2]
            if r < m:
                good[r] = toks[r]
        assert toks[:m] == good                                             # the continuation agrees with itself
        for corrupt in (*sorted({0, min(2, m - 1), m - 1}), None):
            what = f"{name} o={o} {kind} {tail_name} corrupt={corrupt}"
            draft = list(good)
            if corrupt is not None:
                draft[corrupt] = (draft[corrupt] + 1) % V
            want_block, want_lps, want_toks = twin_pass(model, kind, prompt, fed, draft, tail, c)
            n_acc, want_out = sref.accept(want_toks, draft, V)
            assert n_acc == (m if corrupt is None else corrupt), what
            # the pass itself
            cache = fresh_cache(model, kind)
            model.set_step_tail(**tail)
            set_position(C0)
            tok, _, _ = model.step(dev_ids(prompt), cache)
            assert int(tok.item()) == fed and position() == [c, 0], what
            poison = model._spec_state()["logprobs"]
            poison.fill_(123.0)
            tokens, n, lps = model.spec_step_tail(dev_ids(draft), cache)
            assert n == n_acc + 1 and tokens.tolist() == want_out[:n], what
            assert model.spec_tokens[:m + 1].tolist() == want_out, what
            assert all(c_.offset == o + n for c_ in cache), what
            assert torch.equal(model.spec_logits(m + 1).view(torch.int16), want_block.view(torch.int16)), what       # the processed block, every row
            assert torch.equal(poison[:m + 1].view(torch.int32), want_lps.view(torch.int32)), what                  # the log-probabilities, every row
            assert lps.shape == (n, V) and poison[m + 1:].eq(123.0).all(), what
            assert position() == (list(sref.counter_after(c, n_acc)) if draws else [C0, 0]), what                   # the pass's own tail drew nothing
            seq = sref.recorded_ids(prompt, fed, want_out, o)
            assert model.fed_ids[:len(seq)].tolist() == seq, what
            assert model.history[o:len(seq)].tolist() == seq[o:], what
            # plain configured steps right behind it: their draws continue the stream, and nothing reads the rejected rows
            ocache = oracle_after_prompt(golden_dir, name, prompt)
            for t in seq[o:-1]:
                orc.forward(np.array([t]), ocache)
            for k in range(FURTHER):
                at = position()[0]
                tok, lp, logits = model.step(None, cache)
                got_tok, lp, logits = int(tok.item()), lp.clone(), logits.float().cpu().numpy()
                if draws:
                    assert position() == [at + 1, 0], f"{what} step {k}"
                    assert got_tok == draw_at(lp, at, tail["sampler"], xtc), f"{what} step {k}"       # (leaves the counter at at + 1 again)
                else:
                    assert got_tok == int(lp.argmax().item()) and position() == [C0, 0], f"{what} step {k}"
                raw = orc.forward(np.array([seq[-1]]), ocache)[0]
                assert_vec_close(logits, oracle_processed(raw, seq[-ctx:], tail, dt), dt, what=f"{what} step {k}")
                seq.append(got_tok)
            assert all(c_.offset == o + n + FURTHER for c_ in cache), what
            if tail.get("repetition_penalty", 1.0) != 1.0:                  # the penalty's launch records every step's input token
                assert model.fed_ids[:len(seq) - 1].tolist() == seq[:-1], what
    finally:
        model.set_step_tail()


# ------------------------------------------------------------------ 4. the engine, deterministic through the stochastic path
@pytest.mark.parametrize("kind", ["contiguous", "pages"])
@pytest.mark.parametrize("name", list(MODELS))
def test_engine_top_k_1_follows_the_oracle_on_the_simulated_schedule(golden_dir, name, kind):
    """temp = 1, top_k = 1 keeps a single id, so the draw is the argmax -- but every launch of the stochastic path runs."""
    from proxy_inference_engine_amd import InferenceEngine, SpeculativeParams
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    sp = SpeculativeParams(num_draft=7, ngram_max=3, ngram_min=1, min_draft=5, configured_tail=True)
    try:
        for seed in E2E_SEEDS[name]:
            prompt = e2e_prompt(seed, cfg["vocab_size"])
            cont, _ = oracle_run(golden_dir, name, prompt, E2E_TOKENS + 12)
            full = [int(t) for t in prompt] + cont
            want, schedule = ref.simulate(prompt, lambda s: full[len(s)], E2E_TOKENS, sp.num_draft, sp.ngram_max, sp.ngram_min, sp.min_draft, model.spec_min_rows)
            kinds = {("full" if e[2] == e[1] else "partial") if e[0] == "pass" else "step" for e in schedule}
            assert kinds == {"full", "partial", "step"}, (name, seed, schedule)
            eng = InferenceEngine(model=model)
            eng.prompt_cache.cache = fresh_cache(model, kind)
            eng.prepare_engine(prompt, temp=1.0, top_k=1)
            set_position(0)
            gen = eng.generate_step(torch.from_numpy(prompt), speculative=sp, top_logprobs=3)
            got, yielded = [], []
            while len(got) < E2E_TOKENS:
                tokens, rows = next(gen)
                assert rows.shape == (tokens.numel(), cfg["vocab_size"]) and rows.argmax(dim=1).tolist() == tokens.tolist()
                assert eng.top_record[0].shape == (tokens.numel(), 4) and eng.top_record[0][:, 0].tolist() == tokens.tolist()
                got += tokens.tolist()
                yielded.append(tokens.numel())
                assert position() == [len(got), 0], (name, seed)            # token j is draw j
            assert model.step_tail[0] == ("top_k", 1.0, 0.0, 1)             # the stochastic tail was really configured
            assert got == want[:len(got)] == cont[:len(got)], (name, seed)
            done = schedule[:len(yielded) - 1]
            assert yielded[1:] == [e[2] + 1 if e[0] == "pass" else 1 for e in done], (name, seed)
            passes = [e for e in done if e[0] == "pass"]
            assert eng.spec_stats == {"passes": len(passes), "steps": len(done) - len(passes), "drafted": sum(e[1] for e in passes),
                                      "accepted": sum(e[2] for e in passes)}
            assert eng.prompt_cache.computed_ids == full[:eng.prompt_cache.cache[0].offset]
    finally:
        model.set_step_tail()


# ------------------------------------------------------------------ 5. the engine, really random
RANDOM_SEEDS = {"tiny_llama_w4_bf16": 3125, "tiny_dense_f16_bias": 94}      # e2e_prompt seeds: tiled prompts


@pytest.mark.parametrize("penalty", [None, 1.2])
@pytest.mark.parametrize("name", list(MODELS))
def test_engine_random_draws_are_the_stream_positions_draws(golden_dir, name, penalty):
    """temp = 0.8, top_p = 0.9 under a fixed seed: yield j's token is hip_ops.sample of the yielded row at stream position j -- no oracle
    margin is needed -- and the yield sizes are the simulated schedule's for the tokens actually produced.  A pass runs as soon as a
    drawn token occurs earlier in the sequence (ngram_min = 1, and the overlapped copy always drafts num_draft ids): with these seeds and
    prompts that happens within the 40 tokens (the schedules are printed), which the last spec_stats assertion pins."""
    from proxy_inference_engine_amd import InferenceEngine, SpeculativeParams
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    sp = SpeculativeParams(num_draft=7, ngram_max=3, ngram_min=1, min_draft=5, configured_tail=True)
    spec = ("top_p", 0.8, 0.9, 0)
    request = dict(temp=0.8, top_p=0.9, **({} if penalty is None else {"repetition_penalty": penalty, "context_size": 20}))
    prompt = e2e_prompt(RANDOM_SEEDS[name], cfg["vocab_size"])
    n_tokens = 40
    try:
        eng = InferenceEngine(model=model)
        eng.prompt_cache.cache = fresh_cache(model, "contiguous")
        eng.prepare_engine(prompt, **request)
        set_position(0)
        gen = eng.generate_step(torch.from_numpy(prompt), speculative=sp)
        got, yielded = [], []
        while len(got) < n_tokens:
            tokens, rows = next(gen)
            assert rows.shape == (tokens.numel(), cfg["vocab_size"])
            here = position()
            assert here == [len(got) + tokens.numel(), 0], (name, penalty)
            for j, t in enumerate(tokens.tolist()):
                assert t == draw_at(rows[j].clone(), len(got) + j, spec), (name, penalty, len(got) + j)
            set_position(here[0])
            got += tokens.tolist()
            yielded.append(tokens.numel())
        full = [int(t) for t in prompt] + got
        _, schedule = ref.simulate(prompt, lambda s: full[len(s)], len(got), sp.num_draft, sp.ngram_max, sp.ngram_min, sp.min_draft, model.spec_min_rows)
        assert yielded[1:] == [e[2] + 1 if e[0] == "pass" else 1 for e in schedule], (name, penalty, schedule)
        passes = [e for e in schedule if e[0] == "pass"]
        assert eng.spec_stats == {"passes": len(passes), "steps": len(schedule) - len(passes), "drafted": sum(e[1] for e in passes),
                                  "accepted": sum(e[2] for e in passes)}
        print(f"{name} penalty={penalty}: schedule {schedule}")
        assert eng.spec_stats["passes"] >= 1, (name, penalty, got[:4])
        # generate(): the same tokens under the same seed, one by one, each with a map that holds the drawn token
        eng = InferenceEngine(model=model)
        eng.prompt_cache.cache = fresh_cache(model, "contiguous")
        eng.prepare_engine(prompt, **request)
        set_position(0)
        out = list(eng.generate(torch.from_numpy(prompt), speculative=sp, max_completion_tokens=n_tokens - 1, logprobs=True, top_logprobs=2))
        assert [t for t, _ in out] == got[:n_tokens - 1], (name, penalty)
        assert all(t in mp and len(mp) in (2, 3) for t, mp in out)
    finally:
        model.set_step_tail()


# ------------------------------------------------------------------ 6. the unchanged paths
def test_greedy_and_plain_paths_are_the_same_before_and_after(golden_dir):
    from proxy_inference_engine_amd import InferenceEngine, SpeculativeParams
    cfg, dt, orc, model = load_tiny(golden_dir, "tiny_llama_w4_bf16")
    V = cfg["vocab_size"]
    prompt = e2e_prompt(E2E_SEEDS["tiny_llama_w4_bf16"][0], V)
    request = dict(temp=0.8, top_p=0.9)

    def engine(**kw):
        eng = InferenceEngine(model=model)
        eng.prompt_cache.cache = fresh_cache(model, "contiguous")
        eng.prepare_engine(prompt, **kw)
        return eng

    def plain_sampled():
        set_position(3)
        gen = engine(**request).generate_step(torch.from_numpy(prompt))
        toks, bits = [], []
        for _ in range(16):
            t, lp = next(gen)
            toks.append(int(t.item())), bits.append(bits_of(lp))
        return toks, np.stack(bits), model.graph_launches()

    def greedy_pass():
        model.set_step_tail()
        cache = fresh_cache(model, "contiguous")
        tok, _, _ = model.step(dev_ids(prompt), cache)
        draft = dev_ids([int(tok.item())] * 7)
        tokens, n, lps = model.spec_step(draft, cache)
        return tokens.tolist(), n, bits_of(lps), bits_of(model.spec_logits(8).float())

    try:
        before = (plain_sampled(), greedy_pass())
        set_position(0)
        eng = engine(**request)
        out = [t for t, _ in eng.generate(torch.from_numpy(prompt), speculative=SpeculativeParams(configured_tail=True), max_completion_tokens=24)]
        assert len(out) == 24 and eng.spec_stats["passes"] >= 1
        after = (plain_sampled(), greedy_pass())
        for b, a in zip(before, after):
            assert len(b) == len(a)
            for x, y in zip(b, a):
                assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
        assert before[0][2] > 0
        # spec_step still refuses a configured tail, and the library's greedy entry too
        cache = fresh_cache(model, "contiguous")
        model.set_step_tail(sampler=("top_p", 0.8, 0.9, 0))
        model.step(dev_ids(prompt), cache)
        with pytest.raises(ValueError, match="greedy and raw"):
            model.spec_step(dev_ids([1] * 7), cache)
    finally:
        model.set_step_tail()


def test_tail_entry_refusals_by_name(golden_dir):
    from proxy_inference_engine_amd import _ffi, hip_ops
    from proxy_inference_engine_amd.cache import QuantizedKVCache, RotatingKVCache
    cfg, dt, orc, model = load_tiny(golden_dir, "tiny_llama_w4_bf16")
    V = cfg["vocab_size"]
    prompt, draft = dev_ids(np.random.default_rng(5).integers(0, V, 20)), dev_ids([1] * 7)
    lib, st = _ffi.load(), model._spec_state()
    rec = st["rec"]
    sampler = dict(sampler=("top_k", 0.8, 0.0, 5))
    try:
        model.set_step_tail(**sampler)
        for cache, name in (([QuantizedKVCache(group_size=64, bits=8) for _ in model.layers], "QuantizedKVCache"),
                            ([RotatingKVCache(32, keep=4) for _ in model.layers], "RotatingKVCache")):
            model.step(prompt, cache)
            with pytest.raises(ValueError, match=name):
                model.spec_step_tail(draft, cache)
        cache = fresh_cache(model, "contiguous")
        model.step(prompt, cache)
        for m in (4, 32):
            with pytest.raises(ValueError, match="rows"):
                model.spec_step_tail(dev_ids([1] * m), cache)
        tokens, n, _ = model.spec_step_tail(draft, cache)                   # (makes the tail workspace)
        assert 1 <= n <= 8 and all(c.offset == 20 + n for c in cache)

        def raw_call(n_draft, lp=st["logprobs"]):
            return lib.pie_decoder_spec_step_tail(model._dec, _ffi.p(draft), n_draft, _ffi.p(rec[1:]), _ffi.p(rec[0:]), _ffi.p(lp), _ffi.p(st["tail_ws"]), None, 0,
                                                  None, _ffi.stream())

        refused = ((dict(token_mask=hip_ops.pack_token_mask(torch.ones(V, dtype=torch.bool), V)), "token mask"), (dict(top_logprobs=3), "top_logprobs"),
                   (dict(frequency_penalty=0.5, count_start=20), "frequency / presence"), (dict(dry=(0.8, 1.75, 2, 64, ())), "DRY"))
        for kw, name in refused:
            model.set_step_tail(**sampler, **kw)
            with pytest.raises(ValueError, match=name):
                model.spec_step_tail(draft, cache)
            assert raw_call(7) == -5, kw                                    # PIE_E_STATE from the library too, before any launch
        model.set_step_tail()
        with pytest.raises(ValueError, match="spec_step"):                  # nothing configured: that pass is spec_step's
            model.spec_step_tail(draft, cache)
        assert raw_call(7) == -5
        model.set_step_tail(**sampler)
        bufs = model.set_prompt_logprobs(8, 3, 16)
        bufs["count"].fill_(-1)
        assert raw_call(7) == -5
        model.clear_prompt_logprobs()
        assert raw_call(7, lp=None) == -1                                   # logprobs_rows is required
        assert raw_call(4) == -2 and raw_call(32) == -2 and raw_call(0) == -2
        assert int(lib.pie_decoder_spec_tail_workspace_bytes(model._dec, 1)) == 0 and int(lib.pie_decoder_spec_tail_workspace_bytes(model._dec, 33)) == 0
        torch.cuda.synchronize()
        assert all(c.offset == 20 + n for c in cache)
    finally:
        model.set_step_tail()
        model.clear_prompt_logprobs()
