"""-m gpu: draft-model speculative decoding -- pie_spec_verify_draft against the float64 reference (decisions exact, values
to 1e-4 relative), its residual draw against hip_ops.sample (exact), its edge cases and argument checks, a chi-square test of the op's
first token against P on the device; then the decoder's pass and the engine on the tiny int4 model with a drafter of the same checkpoint
(high acceptance) and of its first layer alone (low acceptance), greedy against the oracle and sampled against the stream's bookkeeping,
the refusals by name and the untouched paths.

The target draws from the samplers' own stream (samplers._rng.hip_state), the drafter from samplers._rng.draft_state; draws the tests
restate use a scratch counter under the seed they restate, so neither stream moves."""
import json

import ctypes as C
import numpy as np
import pytest
import torch

from tests import spec_draft_reference as dref
from tests._util import assert_vec_close, codes_dev, to_dev
from tests.test_gpu_spec_sampled import position, process_row, set_position, stream
from tests.test_gpu_speculative import E2E_SEEDS, E2E_TOKENS, bits_of, dev_ids, e2e_prompt, fresh_cache, load_tiny, oracle_run

pytestmark = pytest.mark.gpu
SENT = -77
REL = 1e-4      # fp32 exp at |argument| <= 60 and a tree sum over <= 2^17 terms stay below about 2e-5 (the op's fp64 arithmetic is far inside)
SETTINGS = [("categorical", 0.7, 0.0, 0), ("top_k", 0.8, 0.0, 12), ("top_p", 0.8, 0.9, 0), ("min_p", 1.3, 0.05, 3)]


def draft_stream():
    from proxy_inference_engine_amd.samplers import _rng
    stream()
    return _rng.draft_state(torch.device("cuda", torch.cuda.current_device()))


def scratch(seed: int, c: int):
    """A stream of `seed` at position c that is nobody's: restating a draw moves no real counter."""
    return int(seed), torch.tensor([int(c), 0], dtype=torch.int64, device="cuda")


def kept_sets(lp: torch.Tensor, spec) -> np.ndarray:
    """The sampler's own kept_mask of every row of lp [rows, V], as bool."""
    from proxy_inference_engine_amd import hip_ops
    return np.stack([hip_ops.sample(lp[r].contiguous(), *spec, want_mask=True, rng=scratch(1, 0))[2][0].cpu().numpy().astype(bool) for r in range(lp.shape[0])])


def op_inputs(V: int, rows: int, dtype, gen_seed: int):
    """Target logits N(0, 2) in `dtype`, and the drafter's log-probabilities: the log-softmax of the same logits plus N(0, 1)."""
    g = torch.Generator(device="cpu").manual_seed(gen_seed)
    base = torch.randn((rows, V), generator=g) * 2.0
    logits = base.to(dtype).to("cuda").contiguous()
    q = torch.log_softmax((base[:rows - 1] + torch.randn((rows - 1, V), generator=g)).double(), dim=-1).float().to("cuda").contiguous()
    return logits, q


def reference(lp: torch.Tensor, q_lp: torch.Tensor, spec):
    """(P [rows, V], Q [rows - 1, V]) in float64 from the fp32 log-probabilities and the sampler's own kept sets."""
    kp, kq = kept_sets(lp, spec), kept_sets(q_lp, spec)
    lp_h, q_h = lp.cpu().numpy(), q_lp.cpu().numpy()
    P = np.stack([dref.dist(lp_h[r], kp[r], spec[1]) for r in range(lp_h.shape[0])])
    Q = np.stack([dref.dist(q_h[r], kq[r], spec[1]) for r in range(q_h.shape[0])])
    return P, Q, kp, kq


def prefix_from_record(rec: np.ndarray, draft, V: int) -> int:
    n = 0
    for i, d in enumerate(draft):
        if not 0 <= int(d) < V or not dref.accepts(rec[i, 0], rec[i, 1], rec[i, 2]):
            break
        n += 1
    return n


def check_call(logits, q_lp, draft, spec, c, ws, what):
    """One call at stream position c, checked against everything the header promises; returns (n_acc, tokens, record, residual)."""
    from proxy_inference_engine_amd import hip_ops
    rows, V = logits.shape
    seed, counter = stream()
    set_position(c)
    out = (torch.full((rows,), SENT, dtype=torch.int32, device="cuda"), torch.full((1,), SENT, dtype=torch.int32, device="cuda"))
    tokens, n, lp, rec, res = hip_ops.spec_verify_draft(logits, dev_ids(draft), q_lp, *spec, workspace=ws, out=out, want_record=True)
    n, tokens, rec_h = int(n.item()), tokens.tolist(), rec.cpu().numpy()
    n_acc = n - 1
    assert position() == [c + n, 0], what
    for r in range(rows):                                                   # every row: logprobs_argmax's bits
        assert torch.equal(lp[r].view(torch.int32), hip_ops.logprobs_argmax(logits[r].contiguous())[1].view(torch.int32)), what
    # decisions: exact
    assert [float(x) for x in rec_h[:, 2]] == [float(dref.accept_u(seed, c + i)) for i in range(rows - 1)], what
    assert n_acc == prefix_from_record(rec_h, draft, V), what
    assert tokens[:n_acc] == [int(d) for d in draft[:n_acc]] and tokens[n:] == [-1] * (rows - n) and 0 <= tokens[n_acc] < V, what
    # values: the float64 reference to 1e-4 relative
    P, Q, kp, kq = reference(lp, q_lp, spec)
    if spec[0] != "categorical":                                            # the filtered-out mass is at least 1 %: a forgotten mask shows
        full = np.exp(lp.cpu().numpy().astype(np.float64) * dref.inv_temp(spec[1]))
        assert all(1.0 - full[r][kp[r]].sum() / full[r].sum() >= 0.01 for r in range(rows)), what
    for i, d in enumerate(draft):
        if 0 <= int(d) < V:
            assert abs(rec_h[i, 0] - P[i, d]) <= REL * P[i, d] and abs(rec_h[i, 1] - Q[i, d]) <= REL * Q[i, d], (what, i)
        else:
            assert rec_h[i, 0] == 0.0 and rec_h[i, 1] == 0.0, (what, i)
    res_h = res.cpu().numpy()
    for i in range(rows - 1):
        want, got = dref.residual(P[i], Q[i]), res_h[i].astype(np.float64)
        clear = np.abs(P[i] - Q[i]) > REL * np.maximum(P[i], Q[i])          # where rounding cannot flip the sign of the difference
        assert np.array_equal(np.isneginf(got)[clear], np.isneginf(want)[clear]), (what, i)
        both = np.isfinite(got) & np.isfinite(want) & clear
        assert np.all(np.abs(np.exp(got[both]) - np.exp(want[both])) <= REL * np.exp(want[both])), (what, i)
        assert not np.isnan(got).any() and not np.isposinf(got).any(), (what, i)
    # the last token: the residual's draw, the row's ordinary draw behind an empty residual, the bonus token behind a full block
    if n_acc < rows - 1 and np.isfinite(res_h[n_acc]).any():
        want_last = int(hip_ops.sample(res[n_acc].contiguous(), "categorical", 1.0, rng=scratch(seed, c + n_acc)).item())
        assert np.isfinite(res_h[n_acc, tokens[n_acc]]), what              # a token of the residual's support
    else:
        want_last = int(hip_ops.sample(lp[n_acc].contiguous(), *spec, rng=scratch(seed, c + n_acc)).item())
    assert tokens[n_acc] == want_last, what
    return n_acc, tokens, rec_h, res_h


# ------------------------------------------------------------------ 1-5. the op
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows", [2, 8, 32])
@pytest.mark.parametrize("V", [1000, 4099, 128256])
def test_op_decisions_values_and_draws(V, rows, dtype):
    """V below 256 tiles x 8 and no multiple of 8; an odd vocabulary a little over eight 512-id tiles; a real one.  Per sampler setting:
    drafts drawn from Q under the drafter's stream (decisions, values, the residual's draw), then the same drafts with an id outside the
    vocabulary and an id outside Q's kept set.  One workspace, zeroed once, serves every call."""
    from proxy_inference_engine_amd import hip_ops
    logits, q_lp = op_inputs(V, rows, dtype, V * 7 + rows)
    ws = hip_ops.spec_verify_draft_workspace("cuda", rows, V)
    dseed, dcounter = draft_stream()
    c, seen = 0, set()
    for si, spec in enumerate(SETTINGS):
        c = c * 3 + 5 + si
        dcounter.copy_(torch.tensor([c, 0]))
        draft = hip_ops.sample(q_lp, *spec, rng=(dseed, dcounter)).tolist()
        what = (V, rows, dtype, spec[0])
        n_acc, _, rec, _ = check_call(logits, q_lp, draft, spec, c, ws, what)
        seen.add("full" if n_acc == rows - 1 else "refused")
        assert (rec[:, 1] > 0).all(), what                                  # a draft drawn from Q lies in Q's kept set
        at = min(1, rows - 2)
        if si < 2:                                                          # (one variant per setting keeps a case within seconds)
            bad = (-1, V)[si]
            d = list(draft)
            d[at] = bad
            n_bad, _, _, _ = check_call(logits, q_lp, d, spec, c + 100, ws, what + (bad,))
            assert n_bad <= at, what
        else:                                                               # an id the drafter's filter removed: Q = 0, refused
            kq = kept_sets(q_lp[at:at + 1], spec)[0]
            d = list(draft)
            d[at] = int(np.flatnonzero(~kq)[0])
            n_out, _, rec_out, _ = check_call(logits, q_lp, d, spec, c + 200, ws, what + ("outside Q",))
            assert n_out <= at and rec_out[at, 1] == 0.0, what
    assert "refused" in seen, (V, rows, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows", [2, 8, 32])
@pytest.mark.parametrize("V", [1000, 4099, 128256])
def test_op_accepts_every_draft_when_q_is_p(V, rows, dtype):
    """Q == P bit for bit: u q < p holds for every draft drawn from Q, out_n = rows, the last token is the last row's ordinary draw at
    {c + rows - 1, 0} and the counter ends at c + rows.  With an id outside the vocabulary the draft is refused, every residual entry
    is <= 0, and the last token falls back to the row's ordinary draw."""
    from proxy_inference_engine_amd import hip_ops
    logits, _ = op_inputs(V, rows, dtype, V * 11 + rows)
    lps = torch.stack([hip_ops.logprobs_argmax(logits[r].contiguous())[1] for r in range(rows)])
    q_lp = lps[:rows - 1].clone().contiguous()
    ws = hip_ops.spec_verify_draft_workspace("cuda", rows, V)
    seed, _ = stream()
    dseed, dcounter = draft_stream()
    for si, spec in enumerate(SETTINGS):
        c = 17 + 1000 * si
        what = (V, rows, dtype, spec[0])
        dcounter.copy_(torch.tensor([c, 0]))
        draft = hip_ops.sample(q_lp, *spec, rng=(dseed, dcounter)).tolist()
        n_acc, tokens, rec, res = check_call(logits, q_lp, draft, spec, c, ws, what)
        assert n_acc == rows - 1 and tokens[:rows - 1] == draft, what
        assert [float(x) for x in rec[:, 0]] == [float(x) for x in rec[:, 1]] and np.isneginf(res[:rows - 1]).all(), what
        assert tokens[rows - 1] == int(hip_ops.sample(lps[rows - 1].contiguous(), *spec, rng=scratch(seed, c + rows - 1)).item()), what
        at = rows - 2
        for bad in ((-1,), (), (), (V,))[si]:
            d = list(draft)
            d[at] = bad
            n_bad, tokens, _, res = check_call(logits, q_lp, d, spec, c + 50, ws, what + (bad,))
            assert n_bad == at and np.isneginf(res[at]).all(), what
            assert tokens[at] == int(hip_ops.sample(lps[at].contiguous(), *spec, rng=scratch(seed, c + 50 + at)).item()), what


def test_op_is_bit_identical_from_run_to_run():
    from proxy_inference_engine_amd import hip_ops
    logits, q_lp = op_inputs(128256, 8, torch.bfloat16, 99)
    ws = hip_ops.spec_verify_draft_workspace("cuda", 8, 128256)
    draft = dev_ids(hip_ops.sample(q_lp, "top_p", 0.8, 0.9, 0, rng=scratch(5, 0)).tolist())
    runs = []
    for _ in range(3):
        set_position(4)
        tokens, n, lp, rec, res = hip_ops.spec_verify_draft(logits, draft, q_lp, "top_p", 0.8, 0.9, 0, workspace=ws, want_record=True)
        runs.append((tokens.tolist(), int(n.item()), bits_of(rec), bits_of(res[:7])))
    for r in runs[1:]:
        assert r[0] == runs[0][0] and r[1] == runs[0][1] and np.array_equal(r[2], runs[0][2]) and np.array_equal(r[3], runs[0][3])


# ------------------------------------------------------------------ 6. chi-square on the device
def test_op_first_token_is_distributed_as_the_target():
    """The host test's inputs (tests/spec_draft_reference.py: V = 1000, top-k 12 at temp 0.8, 2000 trials) with rows = 2: every trial
    draws the draft with hip_ops.sample from Q under the drafter's seed; Pearson's chi-square of out_tokens[0] against P over P's support
    lies below the 1 - 1e-6 quantile for 11 degrees of freedom, and no token falls outside P's kept set."""
    from proxy_inference_engine_amd import hip_ops
    cin = dref.CHI2_INPUTS
    V, trials, spec = cin["V"], cin["trials"], ("top_k", cin["temp"], 0.0, cin["k"])
    lp_h, lq_h, _, _ = dref.chi2_inputs(2)
    logits = torch.from_numpy(np.stack([lp_h, lp_h])).to("cuda").to(torch.bfloat16).contiguous()
    q_lp = torch.from_numpy(lq_h[None]).to("cuda").contiguous()
    ws = hip_ops.spec_verify_draft_workspace("cuda", 2, V)
    lp = torch.empty((2, V), dtype=torch.float32, device="cuda")
    toks, ns = torch.full((trials, 2), SENT, dtype=torch.int32, device="cuda"), torch.zeros(trials, dtype=torch.int32, device="cuda")
    drafts = torch.zeros(trials, dtype=torch.int32, device="cuda")
    seed, counter = stream()
    dseed, dcounter = draft_stream()
    assert dseed != seed
    set_position(0)
    dcounter.zero_()
    for t in range(trials):
        drafts[t:t + 1].copy_(hip_ops.sample(q_lp, *spec, rng=(dseed, dcounter)))
        hip_ops.spec_verify_draft(logits, drafts[t:t + 1], q_lp, *spec, logprobs=lp, workspace=ws, out=(toks[t], ns[t:t + 1]))
    P, Q, kp, _ = reference(lp, q_lp, spec)
    first, ns_h = toks[:, 0].cpu().numpy(), ns.cpu().numpy()
    stat, dof, outside = dref.chi2_statistic(first, P[0])
    print(f"device chi2 = {stat:.2f} ({dof} dof); accepted {int((ns_h == 2).sum())} of {trials}; expected acceptance {np.minimum(P[0], Q[0]).sum():.3f}")
    assert dof == 11 and outside == 0 and kp[0][first].all()
    assert stat < dref.CHI2_BOUND_11
    assert position() == [int(ns_h.sum()), 0] and set(ns_h.tolist()) == {1, 2}
    # the same drafts under the wrong rule "always accept" would not pass: the statistic of the drafts themselves against P
    wrong, _, _ = dref.chi2_statistic(drafts.cpu().numpy(), P[0])
    assert wrong > dref.CHI2_BOUND_11


# ------------------------------------------------------------------ 7. argument checks
def test_op_checks_arguments():
    from proxy_inference_engine_amd import _ffi, hip_ops
    x = torch.randn((4, 100), device="cuda").to(torch.bfloat16)
    q = torch.log_softmax(torch.randn((3, 100), device="cuda"), dim=-1)
    d = dev_ids([0, 0, 0])
    with pytest.raises(ValueError, match="spec_verify_draft"):
        hip_ops.spec_verify_draft_workspace("cuda", 33, 100)
    with pytest.raises(ValueError, match="draft"):
        hip_ops.spec_verify_draft(x, dev_ids([0, 0]), q, "top_k", 1.0, 0.0, 5)
    with pytest.raises(ValueError, match="q_logprobs"):
        hip_ops.spec_verify_draft(x, d, q[:2].contiguous(), "top_k", 1.0, 0.0, 5)
    with pytest.raises(ValueError, match="q_logprobs"):
        hip_ops.spec_verify_draft(x, d, q.double(), "top_k", 1.0, 0.0, 5)
    with pytest.raises(ValueError, match="logits"):
        hip_ops.spec_verify_draft(x.float(), d, q, "top_k", 1.0, 0.0, 5)
    with pytest.raises(ValueError, match="mode"):
        hip_ops.spec_verify_draft(x, d, q, "greedy", 1.0)
    for spec in (("top_k", 1.0, 0.0, 0), ("top_k", 1.0, 0.0, 100), ("top_p", 1.0, 1.0, 0), ("min_p", 1.0, 0.0, 1), ("categorical", 0.0, 0.0, 0)):
        with pytest.raises(ValueError, match="pie_spec_verify_draft"):      # pie_sample's parameter rules, under this op's name
            hip_ops.spec_verify_draft(x, d, q, *spec)
    lib = _ffi.load()
    assert int(lib.pie_spec_verify_draft_workspace_bytes(1, 100)) == 0 and int(lib.pie_spec_verify_draft_workspace_bytes(33, 100)) == 0
    assert int(lib.pie_spec_verify_draft_workspace_bytes(4, 524289)) == 0 and int(lib.pie_spec_verify_draft_workspace_bytes(4, 0)) == 0
    ws, out = hip_ops.spec_verify_draft_workspace("cuda", 4, 100), torch.zeros(8, dtype=torch.int32, device="cuda")
    lp = torch.full((4, 100), 123.0, dtype=torch.float32, device="cuda")
    rec, res = torch.full((3, 3), 123.0, device="cuda"), torch.full((4, 100), 123.0, device="cuda")
    seed, counter = stream()
    set_position(9)
    null = C.c_void_p(None)

    def call(x_p=None, ws_p=None, rows=4, V=100, dt=_ffi.PIE_BF16, mode=1, k=5, counter_p=None, lp_p=None, q_p=None, d_p=None):
        return lib.pie_spec_verify_draft(_ffi.p(x) if x_p is None else x_p, rows, V, dt, _ffi.p(d) if d_p is None else d_p, _ffi.p(q) if q_p is None else q_p,
                                         mode, 1.0, 0.0, k, seed, _ffi.p(counter) if counter_p is None else counter_p, _ffi.p(out), _ffi.p(out[4:]),
                                         _ffi.p(lp) if lp_p is None else lp_p, _ffi.p(rec), _ffi.p(res), _ffi.p(ws) if ws_p is None else ws_p, _ffi.stream())

    assert call(ws_p=C.c_void_p(ws.data_ptr() + 8)) == -3 and call(x_p=C.c_void_p(x.data_ptr() + 1)) == -3      # PIE_E_ALIGN
    assert call(counter_p=C.c_void_p(counter.data_ptr() + 4)) == -3 and call(q_p=C.c_void_p(q.data_ptr() + 2)) == -3
    assert call(rows=1) == -2 and call(rows=33) == -2 and call(V=0) == -2 and call(V=524289) == -2             # PIE_E_SHAPE
    assert call(dt=3) == -1 and call(x_p=null) == -1 and call(lp_p=null) == -1 and call(q_p=null) == -1          # PIE_E_ARG
    assert call(d_p=null) == -1 and call(counter_p=null) == -1 and call(mode=4) == -1 and call(k=100) == -1
    assert call(mode=-1) == -1                                                                                  # PIE_SAMPLE_GREEDY: use pie_spec_verify
    torch.cuda.synchronize()
    assert out.eq(0).all() and lp.eq(123.0).all() and rec.eq(123.0).all() and res.eq(123.0).all() and position() == [9, 0] and ws.eq(0).all()
    assert call() == 0                                                                                          # and the same arguments, in range, run
    torch.cuda.synchronize()
    assert 1 <= int(out[4].item()) <= 4 and position() == [9 + int(out[4].item()), 0]


# ------------------------------------------------------------------ the tiny model and its two drafters
NAME = "tiny_llama_w4_bf16"
DRAFTERS: dict = {}
TAIL = dict(sampler=("top_p", 0.8, 0.9, 0), repetition_penalty=1.1, context_size=20, logit_bias=([5, 17, 300], [2.0, -3.0, 1.5]))
REQUEST = dict(temp=0.8, top_p=0.9, repetition_penalty=1.1, context_size=20, logit_bias={5: 2.0, 17: -3.0, 300: 1.5})


def load_drafter(golden_dir, layers: int | None):
    """A second Model of the tiny checkpoint (layers None: all of it), or of its first `layers` layers: one vocabulary, other predictions."""
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    if layers not in DRAFTERS:
        g = np.load(golden_dir / f"{NAME}.npz")
        cfg = json.loads(str(g["config_json"]))
        w = {k[2:]: g[k] for k in g.files if k.startswith("w:")}
        if layers is not None:
            cfg["num_hidden_layers"] = layers
            w = {k: v for k, v in w.items() if ".layers." not in k or int(k.split(".layers.")[1].split(".")[0]) < layers}
        DRAFTERS[layers] = Model(ModelArgs(**cfg), {k: (codes_dev(v) if v.dtype == np.uint32 else to_dev(v, str(g["dtype"]))) for k, v in w.items()})
    return DRAFTERS[layers]


def new_engine(model, prompt, kind="contiguous", **request):
    from proxy_inference_engine_amd import InferenceEngine
    eng = InferenceEngine(model=model)
    eng.prompt_cache.cache = fresh_cache(model, kind)
    eng.prepare_engine(prompt, **request)
    return eng


# ------------------------------------------------------------------ 8. greedy
GREEDY_STATS: dict = {}


@pytest.mark.parametrize("kind", ["contiguous", "pages"])
@pytest.mark.parametrize("layers", [None, 1])
def test_engine_greedy_tokens_are_the_oracles(golden_dir, layers, kind):
    from proxy_inference_engine_amd import SpeculativeParams
    cfg, dt, orc, model = load_tiny(golden_dir, NAME)
    d = load_drafter(golden_dir, layers)
    sp = SpeculativeParams(draft_model=d, num_draft=7)
    stats = {"passes": 0, "drafted": 0, "accepted": 0, "full": 0}
    try:
        for seed in E2E_SEEDS[NAME]:
            prompt = e2e_prompt(seed, cfg["vocab_size"])
            cont, _ = oracle_run(golden_dir, NAME, prompt, E2E_TOKENS + 12)      # (asserts the margin rule at every position)
            eng = new_engine(model, prompt, kind, temp=0)
            gen = eng.generate_step(torch.from_numpy(prompt), speculative=sp, top_logprobs=3)
            got, yielded = [], []
            while len(got) < E2E_TOKENS:
                tokens, rows = next(gen)
                assert rows.shape == (tokens.numel(), cfg["vocab_size"]) and rows.argmax(dim=1).tolist() == tokens.tolist()
                assert eng.top_record[0].shape == (tokens.numel(), 4) and eng.top_record[0][:, 0].tolist() == tokens.tolist()
                got += tokens.tolist()
                yielded.append(tokens.numel())
            assert got == cont[:len(got)], (layers, kind, seed)
            assert eng.spec_stats["passes"] == len(yielded) - 1 and eng.spec_stats["steps"] == 0
            assert eng.spec_stats["drafted"] == 7 * (len(yielded) - 1) and eng.spec_stats["accepted"] == sum(yielded[1:]) - (len(yielded) - 1)
            assert eng.prompt_cache.computed_ids == ([int(t) for t in prompt] + got)[:eng.prompt_cache.cache[0].offset]
            for key in ("passes", "drafted", "accepted"):
                stats[key] += eng.spec_stats[key]
            stats["full"] += sum(1 for y in yielded[1:] if y == 8)
            out = [t for t, _ in new_engine(model, prompt, kind, temp=0).generate(torch.from_numpy(prompt), speculative=sp, max_completion_tokens=E2E_TOKENS - 1)]
            assert out == cont[:E2E_TOKENS - 1], (layers, kind, seed)
        print(f"layers={layers} {kind}: {stats}")
        GREEDY_STATS[(layers, kind)] = stats
        if layers is None:
            assert stats["full"] >= 1, stats                                # the same checkpoint drafts what the target chooses
        else:
            assert stats["accepted"] < stats["drafted"], stats              # the one-layer drafter is wrong, and the tokens are still the oracle's
    finally:
        model.set_step_tail(), d.set_step_tail()


LONG_TOKENS = 128


@pytest.mark.parametrize("kind", ["contiguous", "pages"])
def test_engine_greedy_one_layer_drafter_is_accepted_and_rejected(golden_dir, kind):
    """The one-layer drafter's spec_stats must show both accepted and rejected drafts.  Within the end-to-end test's 48 tokens it shows
    none accepted: cut to its first layer the tiny checkpoint's argmax equals the target's greedy token at 0 of 60 teacher-forced
    positions of either prompt in the numpy oracle (0 of 658 drafts on the device).  Along the second prompt's continuation it first
    does at position 84 (71 of the next 316), so this run generates 128 tokens of that prompt.  The oracle's margin rule stops holding
    at position 80 there, so beyond the oracle's 60 asserted positions the comparator is the plain greedy loop on the same model under
    the same rule: tokens are compared up to the plain loop's first near-tie (margin_ok of its own logits), and behind it every yielded
    token must still be the argmax of its yielded row."""
    from proxy_inference_engine_amd import SpeculativeParams
    from tests.test_gpu_speculative import margin_ok
    cfg, dt, orc, model = load_tiny(golden_dir, NAME)
    d = load_drafter(golden_dir, 1)
    prompt = e2e_prompt(E2E_SEEDS[NAME][-1], cfg["vocab_size"])
    cont, _ = oracle_run(golden_dir, NAME, prompt, E2E_TOKENS + 12)
    try:
        gen = new_engine(model, prompt, kind, temp=0).generate_step(torch.from_numpy(prompt))
        plain, comparable = [], None
        for i in range(LONG_TOKENS):
            tok, _ = next(gen)
            if comparable is None and not margin_ok(model.logits.float().cpu().numpy(), dt):
                comparable = i                                              # token i itself is the near-tie's: the tokens before it are comparable
            plain.append(int(tok.item()))
        gen.close()
        comparable = LONG_TOKENS if comparable is None else comparable
        assert comparable >= len(cont) and plain[:len(cont)] == cont, comparable
        eng = new_engine(model, prompt, kind, temp=0)
        gen = eng.generate_step(torch.from_numpy(prompt), speculative=SpeculativeParams(draft_model=d, num_draft=7))
        got, yielded = [], []
        while len(got) < LONG_TOKENS:
            tokens, rows = next(gen)
            assert rows.argmax(dim=1).tolist() == tokens.tolist()
            got += tokens.tolist()
            yielded.append(tokens.numel())
        gen.close()
        stats = eng.spec_stats
        print(f"one-layer drafter, greedy, {kind}: {stats}; comparable with the plain loop up to token {comparable}; yields {yielded}")
        assert got[:comparable] == plain[:comparable], kind
        assert stats["passes"] == len(yielded) - 1 and stats["drafted"] == 7 * stats["passes"] and stats["accepted"] == sum(yielded[1:]) - stats["passes"]
        assert eng.prompt_cache.computed_ids == ([int(t) for t in prompt] + got)[:eng.prompt_cache.cache[0].offset]
        assert stats["accepted"] < stats["drafted"], stats
        assert stats["accepted"] > 0, stats
    finally:
        model.set_step_tail(), d.set_step_tail()


# ------------------------------------------------------------------ 9. sampled
def run_sampled(golden_dir, layers, kind, n_tokens, stop_after=None):
    """A sampled generation under TAIL from stream position 0, checked after every round; returns (engine, generator, tokens, yields)."""
    from proxy_inference_engine_amd import SpeculativeParams, hip_ops
    cfg, dt, orc, model = load_tiny(golden_dir, NAME)
    d = load_drafter(golden_dir, layers)
    prompt = e2e_prompt(E2E_SEEDS[NAME][0], cfg["vocab_size"])
    L = len(prompt)
    eng = new_engine(model, prompt, kind, **REQUEST)
    set_position(0)
    draft_stream()[1].zero_()
    gen = eng.generate_step(torch.from_numpy(prompt), speculative=SpeculativeParams(draft_model=d, num_draft=7))
    got, yielded = [], []
    while len(got) < n_tokens and (stop_after is None or len(yielded) <= stop_after):
        tokens, rows = next(gen)
        got += tokens.tolist()
        yielded.append(tokens.numel())
        what = (layers, kind, len(yielded))
        assert position() == [len(got), 0], what                            # the target's counter: c + out_n after every round
        assert all(c.offset == L + len(got) - 1 for c in eng.prompt_cache.cache), what
        seq = [int(t) for t in prompt] + got
        whole = len(seq) if len(yielded) > 1 else len(seq) - 1              # (a plain step records its token when it is fed, a pass at once)
        assert model.fed_ids[:whole].tolist() == seq[:whole] and model.history[L:len(seq)].tolist() == got, what
        for j, t in enumerate(tokens.tolist()):                             # every token lies in its row's kept set
            assert int(hip_ops.sample(rows[j].contiguous(), *TAIL["sampler"], want_mask=True, rng=scratch(1, 0))[2][0, t].item()) == 1, what
    return eng, gen, got, yielded


@pytest.mark.parametrize("kind", ["contiguous", "pages"])
@pytest.mark.parametrize("layers", [None, 1])
def test_engine_sampled_rounds_keep_the_books(golden_dir, layers, kind):
    cfg, dt, orc, model = load_tiny(golden_dir, NAME)
    d = load_drafter(golden_dir, layers)
    try:
        eng, gen, got, yielded = run_sampled(golden_dir, layers, kind, 40)
        gen.close()
        assert model.step_tail[0] == TAIL["sampler"] and d.step_tail[0] == TAIL["sampler"]
        assert eng.spec_stats["passes"] == len(yielded) - 1 and eng.spec_stats["accepted"] == sum(yielded[1:]) - (len(yielded) - 1)
        print(f"layers={layers} {kind}: yields {yielded}")
        _, gen2, again, yielded2 = run_sampled(golden_dir, layers, kind, 40)
        gen2.close()
        assert again == got and yielded2 == yielded                        # the same seed: the same tokens
    finally:
        model.set_step_tail(), d.set_step_tail()


def test_plain_steps_behind_a_pass_read_no_rejected_row(golden_dir):
    """12 plain configured steps behind the passes agree with the same positions of a twin cache fed the same ids in one raw call
    (processed row by row with the ops): nothing reads the K / V rows of rejected drafts."""
    cfg, dt, orc, model = load_tiny(golden_dir, NAME)
    d = load_drafter(golden_dir, 1)
    try:
        eng, gen, got, yielded = run_sampled(golden_dir, 1, "contiguous", 24)
        gen.close()
        assert any(y < 8 for y in yielded[1:])                              # there were rejected rows
        cache = eng.prompt_cache.cache
        prompt = [int(t) for t in e2e_prompt(E2E_SEEDS[NAME][0], cfg["vocab_size"])]
        seq, stepped = prompt + got, []
        for _ in range(12):
            tok, _, logits = model.step(None, cache)
            stepped.append((int(tok.item()), logits.float().cpu().numpy()))
            seq.append(stepped[-1][0])
        model.set_step_tail()
        raw = model(dev_ids(seq[:-1])[None], cache=fresh_cache(model, "contiguous"))[0]
        first = len(prompt) + len(got) - 1                                  # the position the first step fed
        for k, (tok, logits) in enumerate(stepped):
            pos = first + k
            want = process_row(raw[pos], seq[max(0, pos + 1 - TAIL["context_size"]):pos + 1], TAIL)
            assert_vec_close(logits, want.float().cpu().numpy(), dt, what=f"step {k}")
    finally:
        model.set_step_tail(), d.set_step_tail()


@pytest.mark.parametrize("layers,want_full", [(None, True), (1, False)])
def test_drafter_cache_is_whole_after_a_round(golden_dir, layers, want_full):
    """After a fully accepted round (the same-checkpoint drafter) and after a partly rejected one (the one-layer drafter): fed the pass's
    last token, the drafter's logits equal those of a fresh cache fed the whole sequence."""
    cfg, dt, orc, model = load_tiny(golden_dir, NAME)
    d = load_drafter(golden_dir, layers)
    try:
        _, gen, _, yielded = run_sampled(golden_dir, layers, "contiguous", 64)
        gen.close()
        rounds = [i for i, y in enumerate(yielded) if i > 0 and (y == 8) == want_full and (want_full or y < 8)]
        assert rounds, (layers, yielded)
        eng, gen, got, _ = run_sampled(golden_dir, layers, "contiguous", 10 ** 6, stop_after=rounds[0])
        gen.close()
        prompt = [int(t) for t in e2e_prompt(E2E_SEEDS[NAME][0], cfg["vocab_size"])]
        seq = prompt + got
        assert all(c.offset == len(seq) - 1 for c in eng._draft_cache)
        _, _, logits = d.step(dev_ids(seq[-1:]), eng._draft_cache)
        logits = logits.float().cpu().numpy()
        d.set_step_tail()
        _, _, want = d.step(dev_ids(seq), fresh_cache(d, "contiguous"))
        assert_vec_close(logits, want.float().cpu().numpy(), dt, what=f"layers={layers}")
    finally:
        model.set_step_tail(), d.set_step_tail()


# ------------------------------------------------------------------ 10. the untouched paths, on the same model objects
def test_plain_and_prompt_lookup_generations_are_the_same_before_and_after(golden_dir):
    from proxy_inference_engine_amd import SpeculativeParams
    cfg, dt, orc, model = load_tiny(golden_dir, NAME)
    d = load_drafter(golden_dir, None)
    prompt = e2e_prompt(E2E_SEEDS[NAME][0], cfg["vocab_size"])
    request = dict(temp=0.8, top_p=0.9)

    def generation(speculative=None, n=24):
        set_position(3)
        gen = new_engine(model, prompt, **request).generate_step(torch.from_numpy(prompt), speculative=speculative)
        toks, bits = [], []
        while len(toks) < n:
            t, lp = next(gen)
            toks += t.reshape(-1).tolist()
            bits.append(bits_of(lp.reshape(-1, cfg["vocab_size"])))
        return toks, np.concatenate(bits), model.graph_launches()

    try:
        before = (generation(), generation(SpeculativeParams(configured_tail=True)))
        set_position(0)
        eng = new_engine(model, prompt, **request)
        out = [t for t, _ in eng.generate(torch.from_numpy(prompt), speculative=SpeculativeParams(draft_model=d), max_completion_tokens=24)]
        assert len(out) == 24 and eng.spec_stats["passes"] >= 1 and eng.spec_stats["accepted"] >= 1
        after = (generation(), generation(SpeculativeParams(configured_tail=True)))
        for b, a in zip(before, after):
            assert b[0] == a[0] and np.array_equal(b[1], a[1]) and b[2] == a[2] > 0
    finally:
        model.set_step_tail(), d.set_step_tail()


# ------------------------------------------------------------------ refusals, by name
def test_refusals_by_name(golden_dir):
    from proxy_inference_engine_amd import InferenceEngine, SpeculativeParams, _ffi, hip_ops
    from proxy_inference_engine_amd.cache import QuantizedKVCache, RotatingKVCache
    from proxy_inference_engine_amd.samplers import _rng
    cfg, dt, orc, model = load_tiny(golden_dir, NAME)
    d = load_drafter(golden_dir, 1)
    V = cfg["vocab_size"]
    prompt, draft = dev_ids(np.random.default_rng(5).integers(0, V, 20)), dev_ids([1] * 7)
    q = torch.log_softmax(torch.randn((7, V), device="cuda"), dim=-1).contiguous()
    lib, st = _ffi.load(), model._spec_state()
    rec = st["rec"]
    sampler = dict(sampler=("top_k", 0.8, 0.0, 5))
    dseed = draft_stream()[0]
    try:
        model.set_step_tail(**sampler)
        for cache, name in (([QuantizedKVCache(group_size=64, bits=8) for _ in model.layers], "QuantizedKVCache"),
                            ([RotatingKVCache(32, keep=4) for _ in model.layers], "RotatingKVCache")):
            model.step(prompt, cache)
            with pytest.raises(ValueError, match=name):
                model.spec_step_draft(draft, q, cache, draft_seed=dseed)
        cache = fresh_cache(model, "contiguous")
        model.step(prompt, cache)
        for m in (4, 32):
            with pytest.raises(ValueError, match="rows"):
                model.spec_step_draft(dev_ids([1] * m), torch.zeros((m, V), device="cuda"), cache, draft_seed=dseed)
        with pytest.raises(ValueError, match="vocabulary mismatch"):
            model.spec_step_draft(draft, torch.zeros((7, V + 1), device="cuda"), cache, draft_seed=dseed)
        with pytest.raises(ValueError, match="the target's seed"):
            model.spec_step_draft(draft, q, cache, draft_seed=stream()[0])
        tokens, n, _ = model.spec_step_draft(draft, q, cache, draft_seed=dseed)      # (makes the workspace)
        assert 1 <= n <= 8 and all(c.offset == 20 + n for c in cache)

        def raw_call(n_draft, lp=st["logprobs"], q_p=q):
            return lib.pie_decoder_spec_step_draft(model._dec, _ffi.p(draft), n_draft, _ffi.p(q_p), _ffi.p(rec[1:]), _ffi.p(rec[0:]), _ffi.p(lp),
                                                   _ffi.p(st["draft_model_ws"]), None, 0, None, _ffi.stream())

        refused = ((dict(xtc=(0.6, 0.1, (3,))), "XTC"), (dict(token_mask=hip_ops.pack_token_mask(torch.ones(V, dtype=torch.bool), V)), "token mask"),
                   (dict(top_logprobs=3), "top_logprobs"), (dict(frequency_penalty=0.5, count_start=20), "frequency / presence"),
                   (dict(dry=(0.8, 1.75, 2, 64, ())), "DRY"))
        for kw, name in refused:
            model.set_step_tail(**sampler, **kw)
            with pytest.raises(ValueError, match=name):
                model.spec_step_draft(draft, q, cache, draft_seed=dseed)
            assert raw_call(7) == -5, kw                                    # PIE_E_STATE from the library too, before any launch
        for kw in ({}, dict(repetition_penalty=1.3)):                       # no stochastic sampler: a greedy draft is a point mass
            model.set_step_tail(**kw)
            with pytest.raises(ValueError, match="stochastic sampler"):
                model.spec_step_draft(draft, q, cache, draft_seed=dseed)
            assert raw_call(7) == -5
        model.set_step_tail(**sampler)
        bufs = model.set_prompt_logprobs(8, 3, 16)
        bufs["count"].fill_(-1)
        assert raw_call(7) == -5
        model.clear_prompt_logprobs()
        assert raw_call(7, lp=None) == -1 and raw_call(7, q_p=None) == -1
        assert raw_call(4) == -2 and raw_call(32) == -2 and raw_call(0) == -2
        assert int(lib.pie_decoder_spec_draft_workspace_bytes(model._dec, 1)) == 0 and int(lib.pie_decoder_spec_draft_workspace_bytes(model._dec, 33)) == 0
        torch.cuda.synchronize()
        assert all(c.offset == 20 + n for c in cache)
        # through the engine
        host_prompt = np.random.default_rng(5).integers(0, V, 20)
        sp = SpeculativeParams(draft_model=d)
        for request, kw, name in ((dict(temp=0.8, xtc_probability=0.5, xtc_threshold=0.1), {}, "XTC"), (dict(temp=0.8, frequency_penalty=0.5), {}, "frequency / presence"),
                                  (dict(temp=0.8, dry_multiplier=0.8), {}, "DRY"), (dict(temp=0.8, token_mask=torch.ones(V, dtype=torch.bool)), {}, "token mask"),
                                  (dict(temp=0.8), dict(kv_bits=8), "kv_bits"), (dict(temp=0.8), dict(max_kv_size=64), "max_kv_size")):
            with pytest.raises(ValueError, match=name):
                next(new_engine(model, host_prompt, **request).generate_step(torch.from_numpy(host_prompt), speculative=sp, **kw))
        with pytest.raises(ValueError, match="num_draft"):
            next(new_engine(model, host_prompt, temp=0.8).generate_step(torch.from_numpy(host_prompt), speculative=SpeculativeParams(draft_model=d, num_draft=3)))
        offset, _rng.DRAFT_SEED_OFFSET = _rng.DRAFT_SEED_OFFSET, 0           # a drafter under the target's seed is refused by the pass itself
        try:
            with pytest.raises(ValueError, match="the target's seed"):
                gen = new_engine(model, host_prompt, temp=0.8).generate_step(torch.from_numpy(host_prompt), speculative=sp)
                next(gen), next(gen)
        finally:
            _rng.DRAFT_SEED_OFFSET = offset
    finally:
        model.set_step_tail(), d.set_step_tail()
        model.clear_prompt_logprobs()


def test_refusal_on_int8_pages(golden_dir):
    from proxy_inference_engine_amd import SpeculativeParams
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    g = np.load(golden_dir / f"{NAME}.npz")
    cfg = json.loads(str(g["config_json"]))
    w = {k[2:]: g[k] for k in g.files if k.startswith("w:")}
    model = Model(ModelArgs(**cfg), {k: (codes_dev(v) if v.dtype == np.uint32 else to_dev(v, "bfloat16")) for k, v in w.items()})
    model.enable_paged_kv(num_pages=8, max_blocks=2, kv_dtype=torch.int8)
    cache = model.make_cache()
    model.step(dev_ids(g["prompt"][:4]), cache)
    try:
        model.set_step_tail(sampler=("top_k", 0.8, 0.0, 5))
        with pytest.raises(ValueError, match="int8 KV pages"):
            model.spec_step_draft(dev_ids([1] * 7), torch.zeros((7, cfg["vocab_size"]), device="cuda"), cache, draft_seed=draft_stream()[0])
        from proxy_inference_engine_amd import InferenceEngine
        eng = InferenceEngine(model=model)
        eng.prepare_engine(g["prompt"], temp=0.8)
        with pytest.raises(ValueError, match="int8 KV pages"):
            next(eng.generate_step(torch.from_numpy(g["prompt"]), speculative=SpeculativeParams(draft_model=load_drafter(golden_dir, 1))))
    finally:
        model.set_step_tail()
