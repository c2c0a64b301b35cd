"""No GPU: draft-model speculative decoding -- the float64 reference's rule reproduces the target's distribution (and two
wrong rules do not), the accept test's Philox index word, SpeculativeParams(draft_model=), check_speculative_draft's refusals by name, and
the new names in the binding table and the header."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import spec_draft_reference as dref
from tests.xtc_reference import COIN_IDX4


# ------------------------------------------------------------------ the rule reproduces P
def test_chi2_bound_is_the_quantile():
    from scipy.stats import chi2
    assert abs(chi2.ppf(1.0 - 1e-6, 11) - dref.CHI2_BOUND_11) < 0.01


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_reference_rule_reproduces_the_target_distribution(seed):
    """V = 1000, top-k 12 at temp 0.8, logits N(0, 2) for P and the same plus N(0, 1) for Q, 2000 numpy-drawn trials.  Pearson's
    chi-square of the first output token against P over P's support lies below the 1 - 1e-6 quantile for the exact rule; "always accept"
    (the tokens are Q's) and "redraw from P on refusal" (the accepted mass is counted twice) lie far above it."""
    _, _, P, Q = dref.chi2_inputs(seed)
    trials = dref.CHI2_INPUTS["trials"]
    assert abs(P.sum() - 1.0) < 1e-12 and abs(Q.sum() - 1.0) < 1e-12 and (P > 0).sum() == 12 and (Q > 0).sum() == 12
    stat, dof, outside = dref.chi2_statistic(dref.simulate_first_token(P, Q, trials, 100 + seed), P)
    print(f"seed {seed}: exact rule chi2 = {stat:.2f} ({dof} dof), smallest expected count {P[P > 0].min() * trials:.1f}, "
          f"acceptance probability {np.minimum(P, Q).sum():.3f}")
    assert dof == 11 and outside == 0 and stat < dref.CHI2_BOUND_11
    for rule in ("always", "redraw"):
        wrong, _, _ = dref.chi2_statistic(dref.simulate_first_token(P, Q, trials, 100 + seed, rule), P)
        print(f"seed {seed}: rule {rule!r} chi2 = {wrong:.1f}")
        assert wrong > dref.CHI2_BOUND_11, rule


def test_reference_dist_accept_and_residual_by_hand():
    lp = np.log(np.array([0.5, 0.25, 0.125, 0.125]))
    kept = np.array([True, True, False, True])
    p = dref.dist(lp, kept, 1.0)
    assert np.allclose(p, [0.5 / 0.875, 0.25 / 0.875, 0.0, 0.125 / 0.875]) and p[2] == 0.0
    assert np.allclose(dref.dist(lp, kept, 0.5), np.array([0.25, 0.0625, 0.0, 0.015625]) / 0.328125)
    assert not dref.dist(lp, np.zeros(4, dtype=bool), 1.0).any()            # a filter that kept nothing: zero everywhere
    # accept iff q > 0 and u * q < p
    assert dref.accepts(0.5, 0.25, 0.999) and dref.accepts(0.25, 0.5, 0.49) and not dref.accepts(0.25, 0.5, 0.5)
    assert not dref.accepts(0.5, 0.0, 0.0) and not dref.accepts(0.0, 0.5, 0.1)
    P = np.array([[0.5, 0.5, 0.0], [0.2, 0.3, 0.5], [1.0, 0.0, 0.0]])
    Q = np.array([[0.25, 0.75, 0.0], [0.6, 0.2, 0.2]])
    assert dref.accepted_prefix(P, Q, [0, 1], [0.9, 0.9]) == 2
    assert dref.accepted_prefix(P, Q, [1, 1], [0.9, 0.9]) == 0 and dref.accepted_prefix(P, Q, [1, 1], [0.6, 0.9]) == 2
    assert dref.accepted_prefix(P, Q, [0, 0], [0.9, 0.4]) == 1
    assert dref.accepted_prefix(P, Q, [-1, 1], [0.0, 0.0]) == 0 and dref.accepted_prefix(P, Q, [0, 3], [0.0, 0.0]) == 1   # never indexed
    assert dref.accepted_prefix(P, Q, [2, 1], [0.0, 0.0]) == 0               # outside Q's kept set
    r = dref.residual(P[1], Q[1])
    assert r[0] == -np.inf and np.allclose(np.exp(r[1:]), [0.1, 0.3])
    assert np.isneginf(dref.residual(P[0], P[0])).all()                      # Q == P: an empty residual


# ------------------------------------------------------------------ the stream layout
def test_accept_index_word_collides_with_nothing():
    assert dref.U_IDX4 == 0xFFFFFFFE and dref.U_IDX4 != COIN_IDX4
    for V in (1, 1000, 128256, 524288):
        assert dref.index_words_are_disjoint(V)
    u = [dref.accept_u(20240607, c) for c in range(64)]
    assert all(0.0 < float(x) <= 1.0 for x in u) and len(set(float(x) for x in u)) > 60
    from tests.xtc_reference import coin_u
    assert all(float(dref.accept_u(7, c)) != float(coin_u(7, c)) for c in range(16))   # another block than the coin's
    assert dref.draft_seed(5) == 5 + 0x9E3779B97F4A7C15 and dref.draft_seed(2 ** 64 - 1) == 0x9E3779B97F4A7C14


def test_draft_stream_is_not_the_targets():
    from proxy_inference_engine_amd.samplers import _rng
    assert _rng.DRAFT_SEED_OFFSET == dref.DRAFT_SEED_OFFSET
    _rng.seed(2 ** 64 - 3)
    dev = torch.device("cpu")
    (seed, counter), (dseed, dcounter) = _rng.hip_state(dev), _rng.draft_state(dev)
    assert dseed == dref.draft_seed(seed) != seed and dcounter.data_ptr() != counter.data_ptr()
    dcounter.fill_(9)
    _rng.seed(11)
    assert _rng.draft_state(dev)[0] == dref.draft_seed(11) and _rng.draft_state(dev)[1].tolist() == [0, 0]


# ------------------------------------------------------------------ SpeculativeParams(draft_model=)
class DraftStub:
    """What the checks look at: a vocabulary and the entry points' names."""

    def __init__(self, V=64):
        self.logprobs, self.history = torch.zeros(V), torch.zeros(16, dtype=torch.int32)

    def step(self, *a, **k):
        raise AssertionError("refused before any model call")

    set_step_tail = spec_step = spec_step_tail = spec_step_draft = step


def test_params_validation():
    from proxy_inference_engine_amd import SpeculativeParams
    assert SpeculativeParams().draft_model is None
    d = DraftStub()
    assert SpeculativeParams(draft_model=d).draft_model is d and SpeculativeParams(draft_model="some/checkpoint").draft_model == "some/checkpoint"
    assert SpeculativeParams(draft_model=d, num_draft=3, min_draft=5).num_draft == 3     # min_draft is ignored with a draft model
    assert SpeculativeParams(draft_model=d, num_draft=31).num_draft == 31
    for bad in (0, 32):
        with pytest.raises(ValueError, match="num_draft"):
            SpeculativeParams(draft_model=d, num_draft=bad)
    for bad in (object(), 3, True):
        with pytest.raises(ValueError, match="draft_model"):
            SpeculativeParams(draft_model=bad)
    with pytest.raises(ValueError, match="min_draft"):                                   # without one the old rule holds
        SpeculativeParams(num_draft=3, min_draft=5)


def draft_args(**kw):
    from proxy_inference_engine_amd.samplers import make_sampler
    args = dict(sampler=make_sampler(temp=0.8, top_p=0.9), processors=[], structuring_engine=None, pixel_values=None, kv_bits=None, max_kv_size=None,
                prompt_logprobs=None)
    args.update(kw)
    return args


def test_check_speculative_draft_plans_and_refusals_by_name():
    from proxy_inference_engine_amd.engine.inference_engine import check_speculative_draft
    from proxy_inference_engine_amd.logits_processors import (count_penalty_logits_processor, dry_logits_processor, make_logit_bias, make_token_mask,
                                                              repetition_penalty_logits_processor)
    from proxy_inference_engine_amd.samplers import make_sampler
    m, d = DraftStub(), DraftStub()
    plan = check_speculative_draft(m, d, *draft_args().values())
    assert plan["sampler"] == ("top_p", 0.8, 0.9, 0) and plan["repetition_penalty"] == 1.0 and plan["bias"] is None
    pen, bias = repetition_penalty_logits_processor(1.1, 20), make_logit_bias({3: 1.5})
    plan = check_speculative_draft(m, d, *draft_args(processors=[pen, bias]).values())
    assert (plan["repetition_penalty"], plan["context_size"]) == (1.1, 20) and plan["bias"] is bias
    assert check_speculative_draft(m, d, *draft_args(sampler=make_sampler(temp=0)).values()) is None       # greedy and raw: spec_step
    plan = check_speculative_draft(m, d, *draft_args(sampler=make_sampler(temp=0), processors=[pen]).values())
    assert plan["sampler"] is None and plan["repetition_penalty"] == 1.1                                   # greedy under a penalty: spec_step_tail

    class Pool:
        dtype = torch.int8

    cases = [(dict(structuring_engine=object()), "structuring engine"), (dict(pixel_values=torch.zeros(1)), "pixel_values"), (dict(kv_bits=8), "kv_bits"),
             (dict(max_kv_size=64), "max_kv_size"), (dict(prompt_logprobs=2), "prompt_logprobs"),
             (dict(sampler=make_sampler(temp=1.0, top_k=4, xtc_probability=0.5, xtc_threshold=0.1)), "XTC"),
             (dict(processors=[make_token_mask(torch.ones(64, dtype=torch.bool))]), "token mask"),
             (dict(processors=[count_penalty_logits_processor(0.5, 0.0)]), "frequency / presence"),
             (dict(processors=[dry_logits_processor(0.8, 1.75, 2, 64, ())]), "DRY"),
             (dict(processors=[lambda t, x: x]), "outside the fused tail plan"), (dict(sampler=lambda x: x), "outside the fused tail plan")]
    for kw, name in cases:
        with pytest.raises(ValueError, match=name):
            check_speculative_draft(m, d, *draft_args(**kw).values())
    tp_model, tp_draft, i8_model = DraftStub(), DraftStub(), DraftStub()
    tp_model.tp, tp_draft.tp, i8_model._page_pool = object(), object(), Pool()
    with pytest.raises(ValueError, match="tensor-parallel model"):
        check_speculative_draft(tp_model, d, *draft_args().values())
    with pytest.raises(ValueError, match="tensor-parallel draft model"):
        check_speculative_draft(m, tp_draft, *draft_args().values())
    with pytest.raises(ValueError, match="int8 KV pages"):
        check_speculative_draft(i8_model, d, *draft_args().values())
    with pytest.raises(ValueError, match="vocabulary mismatch"):
        check_speculative_draft(m, DraftStub(65), *draft_args().values())
    with pytest.raises(ValueError, match="the target itself"):
        check_speculative_draft(m, m, *draft_args().values())
    with pytest.raises(ValueError, match="no spec_step_draft"):
        check_speculative_draft(object(), d, *draft_args().values())


def test_refusals_reach_the_engine_before_any_model_call():
    from proxy_inference_engine_amd import InferenceEngine, SpeculativeParams
    prompt = list(range(10))
    sp = SpeculativeParams(draft_model=DraftStub())

    def engine(**request):
        eng = InferenceEngine(model=DraftStub())
        eng.prompt_cache.cache = []
        eng.prepare_engine(prompt, **request)
        return eng

    for request, kw, name in ((dict(temp=0.8, xtc_probability=0.5, xtc_threshold=0.1), {}, "XTC"), (dict(temp=0.8, frequency_penalty=0.5), {}, "frequency / presence"),
                              (dict(temp=0.8, dry_multiplier=0.8), {}, "DRY"), (dict(temp=0.8, token_mask=torch.ones(64, dtype=torch.bool)), {}, "token mask"),
                              (dict(temp=0.8), dict(kv_bits=8), "kv_bits"), (dict(temp=0.8), dict(max_kv_size=64), "max_kv_size"),
                              (dict(temp=0.8), dict(prompt_logprobs=2), "prompt_logprobs")):
        with pytest.raises(ValueError, match=name):
            next(engine(**request).generate_step(prompt, speculative=sp, **kw))
    with pytest.raises(ValueError, match="vocabulary mismatch"):
        next(engine(temp=0.8).generate_step(prompt, speculative=SpeculativeParams(draft_model=DraftStub(65))))


# ------------------------------------------------------------------ the names
def test_new_symbols_are_exported():
    from proxy_inference_engine_amd import _ffi, hip_ops
    from proxy_inference_engine_amd.engine import inference_engine
    from proxy_inference_engine_amd.models.llama import Model
    assert callable(inference_engine.check_speculative_draft)
    for name in ("spec_verify_draft", "spec_verify_draft_workspace"):
        assert callable(getattr(hip_ops, name))
    assert callable(Model.spec_step_draft)
    names = ("pie_spec_verify_draft", "pie_spec_verify_draft_workspace_bytes", "pie_decoder_spec_step_draft", "pie_decoder_spec_draft_workspace_bytes")
    header = (Path(__file__).resolve().parent.parent / "include" / "pie_hip.h").read_text()
    for name in names:
        assert name in _ffi.EXPORTS and name + "(" in header
