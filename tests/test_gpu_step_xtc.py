"""-m gpu: XTC inside the decode step's configured tail against the host-orchestrated chain on the tiny golden int4
model: the unconfigured step's log-probabilities -> hip_ops.sample(xtc=) on the same seed.  Tokens, log-probabilities and logits are
compared exactly.  THRESHOLD lies below the second-largest probability of every compared step, so the reference removes at least one
id on each of them; every run asserts that from tests/xtc_reference.py."""
import numpy as np
import pytest
import torch

from tests import xtc_reference as ref
from tests._util import to_bits
from tests.test_gpu_step_edits import unconfigured_launches, vocab
from tests.test_gpu_step_tail import PROMPT, assert_runs_equal, dev_ids, f32_bits, tiny  # noqa: F401  (tiny: the fixture)

pytestmark = pytest.mark.gpu
STEPS = 16
THRESHOLD = 0.01
SPECIAL = (5, 900000)                       # one id of the vocabulary, one outside it
SPECS = {"categorical": ("categorical", 1.0, 0.0, 0), "top_k": ("top_k", 0.8, 0.0, 5), "top_p": ("top_p", 0.9, 0.9, 0), "min_p": ("min_p", 1.0, 0.1, 2)}
SEED = 12


def host_chain(model, prompt, steps, spec, probs, graph=True):
    """Per step: (token, logprobs bits, logits bits), and the ids the op removed, and the reference's count whatever the coin said."""
    from proxy_inference_engine_amd import hip_ops
    model.set_step_tail()
    cache, ids, out, removed, could = model.make_cache(), dev_ids(prompt), [], [], []
    for i in range(steps):
        _, lp, lg = model.step(ids, cache, graph=graph)
        tok, gone = hip_ops.sample(lp, *spec, xtc=hip_ops.xtc_pack(probs[i], THRESHOLD, SPECIAL), want_removed=True)
        could.append(int(ref.removed_set(lp.float().cpu().numpy().reshape(-1), THRESHOLD, SPECIAL).sum()))
        removed.append(int(gone.item()))
        out.append((int(tok.item()), f32_bits(lp), to_bits(lg).copy()))
        ids = tok.reshape(1).to(torch.int32).clone()
    return out, removed, could


def fused_chain(model, prompt, steps, spec, xtc, graph=True, each_step=None, **tail):
    model.set_step_tail(sampler=spec, xtc=xtc, **tail)
    cache, out = model.make_cache(), []
    for i in range(steps):
        if each_step is not None:
            each_step(i)
        tok, lp, lg = model.step(dev_ids(prompt) if i == 0 else None, cache, graph=graph)
        out.append((int(tok.item()), f32_bits(lp), to_bits(lg).copy()))
    return out


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("name", list(SPECS))
def test_step_with_xtc_matches_host_chain(tiny, name, graph):
    from proxy_inference_engine_amd import samplers
    g, cfg, model = tiny
    spec = SPECS[name]
    try:
        samplers.seed(SEED)
        host, removed, could = host_chain(model, PROMPT, STEPS, spec, [1.0] * STEPS, graph)
        print(f"{name}: removed per step {removed}")
        assert min(could) >= 1 and removed == could                   # the precondition: XTC bites on every compared step
        samplers.seed(SEED)
        fused = fused_chain(model, PROMPT, STEPS, spec, (1.0, THRESHOLD, SPECIAL), graph)
        assert model.step_xtc_record is not None
        assert_runs_equal(fused, host, f"{name}, graph {graph}")       # (the logprobs and logits: those before XTC)
        samplers.seed(SEED)
        plain = fused_chain(model, PROMPT, STEPS, spec, None, graph)
        assert model.step_xtc_record is None
        assert [f[0] for f in plain] != [f[0] for f in fused]
        samplers.seed(SEED)
        zero = fused_chain(model, PROMPT, STEPS, spec, (0.0, THRESHOLD, SPECIAL), graph)     # probability 0: off, nothing armed
        assert model.step_xtc_record is None
        assert_runs_equal(zero, plain, "probability 0")
    finally:
        model.set_step_tail()


def test_launch_budget_and_dropped_graphs(tiny):
    """With XTC the captured step has the same sampler's launches plus one; unset, today's count; setting or clearing XTC drops the
    captured graphs; a record without a sampler is a no-op."""
    from proxy_inference_engine_amd import _ffi, hip_ops
    g, cfg, model = tiny
    lib = _ffi.load()
    U = unconfigured_launches(model)
    assert U > 0
    try:
        for name, spec in SPECS.items():
            fused_chain(model, PROMPT, 3, spec, None)
            S = model.graph_launches()
            assert S - U == (5 if name in ("top_k", "top_p", "min_p") else 2), name
            model.set_step_tail(sampler=spec, xtc=(0.5, THRESHOLD, ()))
            assert model.graph_launches() == -1                       # setting it dropped the graphs
            fused_chain(model, PROMPT, 3, spec, (0.5, THRESHOLD, ()))
            assert model.graph_launches() == S + 1, name
            model.set_step_tail(sampler=spec, xtc=(0.25, 0.2, (3,)))   # new values: the same record, no new capture
            assert model.graph_launches() == S + 1
            model.set_step_tail(sampler=spec)
            assert model.graph_launches() == -1                       # clearing it dropped them too
            fused_chain(model, PROMPT, 3, spec, None)
            assert model.graph_launches() == S
        # a record without a sampler: the greedy step launches and returns what it always did
        model.set_step_tail()
        rec = hip_ops.xtc_records([hip_ops.xtc_pack(1.0, THRESHOLD)], "cuda")
        assert lib.pie_decoder_set_xtc(model._dec, _ffi.p(rec)) == 0
        cache = model.make_cache()
        toks = [int(model.step(dev_ids(g["prompt"].tolist()), cache)[0].item())] + [int(model.step(None, cache)[0].item()) for _ in range(len(g["tokens"]) - 1)]
        assert model.graph_launches() == U and toks == g["tokens"].tolist()
    finally:
        lib.pie_decoder_set_xtc(model._dec, None)
        model.set_step_tail()
    assert unconfigured_launches(model) == U


def test_new_probability_replays_the_captured_graph(tiny):
    """The record's probability is rewritten on the device between replays: the draws follow, and no graph is captured anew."""
    from proxy_inference_engine_amd import hip_ops, samplers
    g, cfg, model = tiny
    spec, half = SPECS["top_k"], STEPS // 2
    probs = [1.0] * half + [0.0] * (STEPS - half)
    seen = []

    def each_step(i):
        seen.append(model.graph_launches())
        if i == half:
            model.step_xtc_record.view(torch.float32)[0, hip_ops.XTC_PROBABILITY_WORD] = 0.0

    try:
        samplers.seed(SEED)
        host, removed, could = host_chain(model, PROMPT, STEPS, spec, probs)
        assert min(could) >= 1 and min(removed[:half]) >= 1 and removed[half:] == [0] * (STEPS - half)
        samplers.seed(SEED)
        fused = fused_chain(model, PROMPT, STEPS, spec, (1.0, THRESHOLD, SPECIAL), each_step=each_step)
        assert_runs_equal(fused, host, "probability rewritten")
        # step 0 is the prompt pass, step 1 captures; from then on the graph is there before each step (a dropped one reads -1), unchanged
        assert len(set(seen[2:])) == 1 and seen[2] > 0 and model.graph_launches() == seen[2], seen
        model.set_step_tail()                                         # (the model does not know that its record was rewritten behind it)
        samplers.seed(SEED)
        armed = fused_chain(model, PROMPT, STEPS, spec, (1.0, THRESHOLD, SPECIAL))
        assert [f[0] for f in armed[:half]] == [f[0] for f in fused[:half]] and [f[0] for f in armed] != [f[0] for f in fused]
    finally:
        model.set_step_tail()


def test_top_logprobs_record_is_the_one_before_xtc(tiny):
    from proxy_inference_engine_amd import hip_ops, samplers
    g, cfg, model = tiny
    spec = SPECS["categorical"]
    try:
        samplers.seed(SEED)
        host, removed, could = host_chain(model, PROMPT, 6, spec, [1.0] * 6)
        assert min(removed) >= 1
        samplers.seed(SEED)
        model.set_step_tail(sampler=spec, xtc=(1.0, THRESHOLD, SPECIAL), top_logprobs=3)
        cache = model.make_cache()
        for i in range(6):
            tok, lp, _ = model.step(dev_ids(PROMPT) if i == 0 else None, cache)
            ids, vals = (t.clone() for t in model.step_top_logprobs)
            want_ids, want_vals = hip_ops.top_logprobs(lp.reshape(1, -1), 3, tokens=tok.reshape(1).to(torch.int32))
            assert int(tok.item()) == host[i][0] and np.array_equal(f32_bits(lp), host[i][1])
            assert ids.tolist() == want_ids[0].tolist() and np.array_equal(f32_bits(vals), f32_bits(want_vals[0]))
            best = int(lp.reshape(-1).argmax().item())
            assert ids[1].item() == best and int(tok.item()) != best and torch.isfinite(vals).all()   # the record still names the id XTC hid from the draw
    finally:
        model.set_step_tail()


def test_refusals(tiny):
    import ctypes as C
    from oracle import pie_oracle as po
    from proxy_inference_engine_amd import _ffi, hip_ops
    from proxy_inference_engine_amd.cache import ReusableKVCache
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    from proxy_inference_engine_amd.tp import HipComm
    from tests._util import codes_dev, to_dev
    from tests.test_gpu_step_tail import DT
    from tests.test_gpu_tp import CFG
    g, cfg, model = tiny
    lib = _ffi.load()
    rec = hip_ops.xtc_records([hip_ops.xtc_pack(1.0, THRESHOLD)] * 2, "cuda")
    R = _ffi.p(rec)
    w = po.synth_checkpoint(CFG, seed=72, dtype=DT, lm_head_gain=4.0)
    dev_w = {k: (codes_dev(v) if v.dtype == np.uint32 else to_dev(v, DT)) for k, v in w.items()}
    comm = HipComm(CFG["hidden_size"], backend="ipc")
    try:
        tp = Model(ModelArgs(**CFG), dev_w, tp=comm)
        assert lib.pie_decoder_set_xtc(tp._dec, R) == -5 and b"pie_decoder_set_xtc" in lib.pie_last_error()
        assert lib.pie_decoder_set_xtc(tp._dec, None) == -5
        assert lib.pie_decoder_set_batch_xtc(tp._dec, R, 2) == -5 and b"pie_decoder_set_batch_xtc" in lib.pie_last_error()
        del tp
    finally:
        comm.close()
    odd = C.c_void_p(rec.data_ptr() + 2)
    assert lib.pie_decoder_set_xtc(model._dec, odd) == -3 and lib.pie_decoder_set_batch_xtc(model._dec, odd, 2) == -3
    assert lib.pie_decoder_set_batch_xtc(model._dec, R, 0) == -1
    with pytest.raises(ValueError):
        model.set_step_tail(sampler=SPECS["top_k"], xtc=(0.5, 0.6, ()))      # threshold outside (0, 0.5]
    with pytest.raises(ValueError):
        model.set_step_tail(sampler=SPECS["top_k"], xtc=(0.5, 0.1))
    model.set_step_tail()
    assert model.step_xtc_record is None
    # speculation refuses a set record by name, before any launch, and runs again once it is cleared
    st = model._spec_state()
    srec, draft = st["rec"], dev_ids([1] * 7)
    cache = [ReusableKVCache() for _ in model.layers]
    model.step(dev_ids(np.random.default_rng(5).integers(0, vocab(cfg), 20)), cache)
    raw_call = lambda: lib.pie_decoder_spec_step(model._dec, _ffi.p(draft), 7, _ffi.p(srec[1:]), _ffi.p(srec[0:]), None, _ffi.p(st["ws"]), None, 0, None, _ffi.stream())
    try:
        assert lib.pie_decoder_set_xtc(model._dec, R) == 0
        assert raw_call() == -5 and b"XTC" in lib.pie_last_error()
    finally:
        lib.pie_decoder_set_xtc(model._dec, None)
    tokens, n, _ = model.spec_step(draft, cache)
    assert 1 <= n <= 8 and all(c.offset == 20 + n for c in cache)
