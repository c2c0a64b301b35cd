"""InferenceEngine: the decode hot loop on MI355X.

Host-side mirror of engine/inference_engine.py of the reference for the path SURVEY.md 8a names:
generate_step (:228-297), generate (:175-226), make_sampler (:299-317), make_processors (:319-335).
Out of scope here: the tokenizer / chat template, the PSE structuring engine (third-party,
absent) and the Interaction value objects -- `generate` works on token ids; the PSE hooks are optional
injected callables that default to identity.

Array type: torch.Tensor on the ROCm device instead of mx.array.
"""
from __future__ import annotations

from collections.abc import Callable, Generator, Iterator
from dataclasses import dataclass, field
from functools import partial

import torch

from .. import hip_ops
from ..cache import BaseCache, PromptCache, QuantizedKVCache, ReusableKVCache, RotatingKVCache
from ..cache.kv_cache import PagedKVCache
from ..cache.kv_cache.quantized import check_format as check_kv_format
from ..logits_processors import check_vocab, count_penalty_logits_processor, dry_logits_processor, make_logit_bias, make_token_automaton, make_token_mask, packed_token_mask, repetition_penalty_logits_processor
from ..models import load
from ..samplers import make_sampler

Sampler = Callable[[torch.Tensor], torch.Tensor]
LogitsProcessor = Callable[[object, torch.Tensor], torch.Tensor]
ModelOutput = tuple[int, dict]


def check_generate_mask(mask, n_heads: int | None = None) -> None:
    """generate_step(mask=array).  The reference forwards ONE array to the prompt pass and to every later single-token call
    (inference_engine.py:246-249), and mx.fast.scaled_dot_product_attention broadcasts it against scores [1, H, L, S] -- L = the prompt
    length, then 1; S growing by one per step.  The only arrays that broadcast against all of those are constant per head: shape
    (), (1,)*k or [.., H | 1, 1, 1].  Such a mask cannot change which keys a query sees: a boolean one must be all True (False hides EVERY
    key of a row: the softmax of an empty row is NaN upstream), an additive one shifts every score of a row by the same finite amount,
    which the softmax cancels.  Accepted and applied as what they are -- nothing; anything else is refused with the reason the reference
    itself would fail with (a broadcast error at the first decode step, or NaN logits)."""
    m = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(mask)
    shape = tuple(m.shape)
    if len(shape) > 4 or any(d != 1 for d in shape[-2:]) or (len(shape) == 4 and shape[0] != 1) or \
            (len(shape) >= 3 and shape[-3] != 1 and (n_heads is None or shape[-3] != n_heads)):
        raise ValueError(f"generate_step(mask=array of shape {shape}): one array is forwarded to the prompt pass and to every single-token step "
                         "(inference_engine.py:246-249), so it must broadcast against scores [1, H, L, S] for every L and S -- shape [.., H | 1, 1, 1]; "
                         "a [L, S] causal mask belongs to Model.__call__(inputs, mask=...) for one call")
    if m.dtype == torch.bool:
        if not bool(m.all()):
            raise ValueError("generate_step(mask=boolean array): a False entry hides every key of its rows (softmax of an empty row)")
    elif not bool(torch.isfinite(m.float()).all()):
        raise ValueError("generate_step(mask=additive array): a non-finite entry hides every key of its rows (softmax of an empty row)")


def fused_tail_spec(processors, sampler, structuring_engine=None, tensor_parallel: bool = False):
    """Whether one _inference call can end inside the decode step's configured tail (Model.set_step_tail), and with what:
    returns (sampler spec or None, repetition_penalty, context_size) -- set_step_tail's arguments -- or None for the host-orchestrated
    branches.  Fused: no structuring engine (its hooks are host callables), processors empty or exactly the one repetition-penalty
    processor with 1 <= context_size <= 1024 (context_size 0 means the whole history upstream, tokens[-0:]), a sampler that is greedy or
    carries a `hip_spec` (make_sampler's own closures), and a model that is not tensor-parallel (vocabulary-parallel tail).  A sampler
    under XTC (`hip_xtc` next to `hip_spec`) is fused like the same sampler without: fused_tail_plan passes its
    parameters on as plan["xtc"]."""
    if structuring_engine is not None or tensor_parallel:
        return None
    procs = list(processors or [])
    penalty, context_size = 1.0, 60
    if procs:
        if len(procs) != 1 or not hasattr(procs[0], "penalty") or not hasattr(procs[0], "context_size"):
            return None
        penalty, context_size = float(procs[0].penalty), int(procs[0].context_size)
        if not 1 <= context_size <= 1024:
            return None
    if getattr(sampler, "is_greedy", False):
        return None, penalty, context_size
    spec = getattr(sampler, "hip_spec", None)
    return None if spec is None else (tuple(spec), penalty, context_size)


def fused_tail_plan(processors, sampler, structuring_engine=None, tensor_parallel: bool = False):
    """fused_tail_spec with the tail's token mask and logit bias: whether one _inference call can end inside the decode
    step's configured tail, and with what -- a dict(sampler=spec or None, repetition_penalty, context_size, mask=the token-mask processor
    or None, bias=the logit-bias processor or None) -- plus counts=the frequency / presence processor and dry=the DRY
    processor when the request carries one -- or None for the host-orchestrated branches.  Fused: the processor list is a
    sub-sequence of (one token mask, one repetition penalty, one logit bias, one frequency / presence penalty, one DRY penalty) in that
    order -- the order the kernels define -- and
    fused_tail_spec's other conditions hold: no structuring engine, a repetition context of 1..1024, a greedy or `hip_spec` sampler,
    no tensor parallelism.  A token automaton's processor (make_token_automaton) is a kind of its own, in the mask's
    position: plan["automaton"] carries it, and a list that holds it together with a token mask is a ValueError -- the automaton writes
    the step's mask."""
    kinds = []
    for proc in list(processors or []):
        if hasattr(proc, "mask_fn") and hasattr(proc, "mask"):
            kinds.append("mask")
        elif hasattr(proc, "automaton"):
            kinds.append("automaton")
        elif hasattr(proc, "penalty") and hasattr(proc, "context_size"):
            kinds.append("penalty")
        elif hasattr(proc, "ids") and hasattr(proc, "values"):
            kinds.append("bias")
        elif hasattr(proc, "frequency_penalty") and hasattr(proc, "presence_penalty"):
            kinds.append("counts")
        elif hasattr(proc, "dry_multiplier"):
            kinds.append("dry")
        else:
            return None
    if "mask" in kinds and "automaton" in kinds:
        raise ValueError("a token mask and a token automaton are exclusive: the automaton derives the mask itself")
    order = [("mask", "penalty", "bias", "counts", "dry").index("mask" if k == "automaton" else k) for k in kinds]
    if any(b <= a for a, b in zip(order, order[1:])):  # out of order, or one kind twice
        return None
    by_kind = dict(zip(kinds, list(processors or [])))
    spec = fused_tail_spec([by_kind["penalty"]] if "penalty" in by_kind else [], sampler, structuring_engine, tensor_parallel)
    if spec is None:
        return None
    plan = dict(sampler=spec[0], repetition_penalty=spec[1], context_size=spec[2], mask=by_kind.get("mask"), bias=by_kind.get("bias"))
    if spec[0] is not None and getattr(sampler, "hip_xtc", None) is not None:  # XTC rides the sampler's launches
        plan["xtc"] = tuple(sampler.hip_xtc)
    for kind in ("counts", "dry", "automaton"):  # (a request without them gets the plan it always got)
        if kind in by_kind:
            plan[kind] = by_kind[kind]
    return plan


@dataclass(frozen=True)
class SpeculativeParams:
    """Greedy speculative decoding with prompt-lookup drafts (generate_step(speculative=...)): after every step or pass the
    drafter looks the sequence's last ngram_max .. ngram_min ids up in the sequence itself and copies the num_draft ids behind the latest
    occurrence of the longest suffix found; a draft of at least min_draft ids is verified in one many-row pass, anything shorter is one
    plain replayed step.  The tokens are exactly greedy decoding's.
    configured_tail: False -- speculation is greedy and raw, and anything else is refused.  True -- the request's sampler
    (any temperature, top-p / top-k / min-p, XTC), repetition penalty and logit bias run inside the passes: row r's token is drawn from the
    model's own processed distribution at the stream position the plain loop would have used for it, and a draft is accepted while it
    equals the draw -- exact for prompt-lookup drafts, which are point masses: token j of the generation is draw j of the seed from row
    j's own distribution.  (A pass's rows come from the many-row GEMMs and a step's from the GEMVs, so their logits may differ in the last
    bit, as in the greedy case: the plain loop draws the same tokens wherever no draw falls within that rounding of a boundary.)  A greedy
    request without processors takes the greedy path either way.
    batch_tail: configured_tail's analogue for BatchedEngine(speculative=...), which refuses configured_tail itself.  True --
    generate() admits requests whose SamplingParams set a sampler (temp, top_p, top_k, min_p, min_tokens_to_keep, seed, XTC), a
    repetition penalty and a logit_bias: every seat's record, ring, bias table and XTC record are applied to the 1 + m_s rows of its
    segment inside the one pass (Model.spec_step_batch_tail), by the same point-mass rule.  A token mask, a token automaton, frequency /
    presence penalties, DRY and log-probabilities stay refused there.  InferenceEngine refuses batch_tail=True by name.
    draft_model: None -- prompt-lookup drafts, as above.  A built `Model` of the target's vocabulary, or a checkpoint
    path (loaded once and kept on the engine) -- every round the draft model runs num_draft of its own replayed steps (num_draft =
    the target's spec_min_rows - 1 .. 31, so that the pass keeps its many-row form) and the target verifies them in one pass.  A greedy
    request accepts while the draft equals the target's greedy token: the tokens are the plain greedy loop's.  A sampled request (any
    temperature, top-p / top-k / min-p; repetition penalty and logit bias on the target) runs speculative sampling: the drafter draws
    under the request's (mode, temp, p, k) and a seed of its own, draft i is accepted with probability min(1, P_i / Q_i), and the token
    behind the accepted prefix comes from the residual max(0, P - Q) -- every token is distributed as the plain loop's, though it is no
    longer draw j of the seed.  min_draft, ngram_max, ngram_min and configured_tail are ignored with a draft model: every round drafts
    num_draft ids, and the request's sampler decides the path.
    grammar: True -- a request whose root processors hold a token automaton (make_token_automaton) is speculated too: the
    drafter knows the grammar -- a looked-up draft is cut at the first id the automaton forbids, and in a state that allows exactly one
    id that id is drafted, with no look-up and no second model -- and the pass masks every row in the state the drafts before it lead
    to (Model.spec_step_grammar).  A forced id is a point mass under any sampler, so it is always accepted; `spec_stats["forced"]` counts
    the drafted ids that came from the forced table.  What configured_tail=True admits is admitted beside the automaton; a request
    without an automaton behaves as under configured_tail=True.  Not available with a draft model."""
    num_draft: int = 7
    ngram_max: int = 3
    ngram_min: int = 1
    min_draft: int = 5
    configured_tail: bool = False
    batch_tail: bool = field(default=False, kw_only=True)   # (keyword-only: the positional order of the fields around it stays as it was)
    draft_model: object = None
    grammar: bool = False

    def __post_init__(self):
        if not 1 <= int(self.ngram_min) <= int(self.ngram_max) <= hip_ops.SPEC_MAX_NGRAM:
            raise ValueError(f"SpeculativeParams: 1 <= ngram_min <= ngram_max <= {hip_ops.SPEC_MAX_NGRAM}")
        if self.draft_model is not None:
            import os
            if not isinstance(self.draft_model, (str, os.PathLike)) and not all(hasattr(self.draft_model, a) for a in ("step", "set_step_tail", "history", "logprobs")):
                raise ValueError("SpeculativeParams: draft_model is None, a built Model or a checkpoint path")
            if not 1 <= int(self.num_draft) <= hip_ops.SPEC_MAX_ROWS - 1:
                raise ValueError(f"SpeculativeParams: 1 <= num_draft <= {hip_ops.SPEC_MAX_ROWS - 1} with a draft model")
        elif not 1 <= int(self.min_draft) <= int(self.num_draft) <= hip_ops.SPEC_MAX_ROWS - 1:
            raise ValueError(f"SpeculativeParams: 1 <= min_draft <= num_draft <= {hip_ops.SPEC_MAX_ROWS - 1}")
        if not isinstance(self.configured_tail, bool):
            raise ValueError("SpeculativeParams: configured_tail is a bool")
        if not isinstance(self.grammar, bool):
            raise ValueError("SpeculativeParams: grammar is a bool")
        if not isinstance(self.batch_tail, bool):
            raise ValueError("SpeculativeParams: batch_tail is a bool")
        if self.grammar and self.draft_model is not None:
            raise ValueError("SpeculativeParams: grammar is not available with a draft model")


def _speculative_environment(model, structuring_engine, pixel_values, kv_bits, max_kv_size, prompt_logprobs=None) -> list:
    """The (refused, name) rows every kind of speculation shares: it runs on one sequence's 16-bit cache, without host hooks."""
    return [(structuring_engine is not None, "a structuring engine"), (pixel_values is not None, "pixel_values"),
            (kv_bits is not None, "kv_bits"), (max_kv_size is not None, "max_kv_size"), (prompt_logprobs is not None, "prompt_logprobs"),
            (getattr(model, "tp", None) is not None, "a tensor-parallel model"),
            (getattr(getattr(model, "_page_pool", None), "dtype", None) == torch.int8, "int8 KV pages")]


def _refuse(what: str, rows) -> None:
    """ValueError for the first refused row: '`what` is not available with `name`'."""
    for bad, name in rows:
        if bad:
            raise ValueError(f"{what} is not available with {name}")


def _speculative_plan(what: str, model, sampler, processors, structuring_engine, refused_parts) -> dict:
    """The request's fused tail plan for a kind of speculation whose passes run a configured tail: ValueError when there is none, or
    when it holds one of refused_parts ((plan key, name) rows)."""
    plan = fused_tail_plan(processors, sampler, structuring_engine, getattr(model, "tp", None) is not None)
    if plan is None:
        raise ValueError(f"{what} is not available with a sampler or logits processors outside the fused tail plan "
                         "(make_sampler's samplers; one repetition penalty with a context of 1..1024, one logit bias)")
    _refuse(what, ((plan.get(key) is not None, name) for key, name in refused_parts))
    return plan


_PASS_REFUSED_PARTS = (("mask", "a token mask"), ("automaton", "a token automaton"), ("counts", "frequency / presence penalties"), ("dry", "a DRY penalty"))


def check_speculative(model, sampler, processors, structuring_engine, pixel_values, kv_bits, max_kv_size) -> None:
    """What generate_step(speculative=...) refuses, each by name: speculation here is greedy and raw, on one sequence's 16-bit cache."""
    _refuse("speculative decoding", [(not getattr(sampler, "is_greedy", False), "a non-greedy sampler (temp > 0)"),
                                     (any(hasattr(p, "automaton") for p in processors or []), "a token automaton"), (bool(processors), "logits processors")]
            + _speculative_environment(model, structuring_engine, pixel_values, kv_bits, max_kv_size))
    if not hasattr(model, "spec_step"):
        raise ValueError("speculative decoding is not available with this model (no spec_step)")


def check_speculative_tail(model, sampler, processors, structuring_engine, pixel_values, kv_bits, max_kv_size, prompt_logprobs=None) -> dict:
    """What generate_step(speculative=SpeculativeParams(configured_tail=True)) refuses, each by name, and the fused tail
    plan of what it accepts: a greedy or `hip_spec` sampler (XTC included), the repetition penalty and the logit bias.  A token mask,
    frequency / presence penalties and DRY stay out of the passes, like everything check_speculative refuses besides the sampler and the
    processors."""
    _refuse("speculative decoding", _speculative_environment(model, structuring_engine, pixel_values, kv_bits, max_kv_size, prompt_logprobs))
    plan = _speculative_plan("speculative decoding under a configured tail", model, sampler, processors, structuring_engine, _PASS_REFUSED_PARTS)
    if not hasattr(model, "spec_step_tail") or not hasattr(model, "set_step_tail"):
        raise ValueError("speculative decoding under a configured tail is not available with this model (no spec_step_tail)")
    return plan


_GRAMMAR_REFUSED_PARTS = tuple(row for row in _PASS_REFUSED_PARTS if row[0] != "automaton")


def check_speculative_grammar(model, sampler, processors, structuring_engine, pixel_values, kv_bits, max_kv_size, prompt_logprobs=None) -> dict:
    """What generate_step(speculative=SpeculativeParams(grammar=True)) refuses for a request that carries a token automaton, each by name
    (DESIGN.md 23), and the fused tail plan of what it accepts: what check_speculative_tail accepts, plus the automaton.  A token mask,
    frequency / presence penalties and DRY stay out of the passes, like everything _speculative_environment refuses."""
    _refuse("speculative decoding", _speculative_environment(model, structuring_engine, pixel_values, kv_bits, max_kv_size, prompt_logprobs))
    plan = _speculative_plan("speculative decoding under a token automaton", model, sampler, processors, structuring_engine, _GRAMMAR_REFUSED_PARTS)
    if plan.get("automaton") is None:
        raise ValueError("speculative decoding under a token automaton: the request carries no token automaton (check_speculative_tail's path)")
    if not hasattr(model, "spec_step_grammar") or not hasattr(model, "set_step_tail"):
        raise ValueError("speculative decoding under a token automaton is not available with this model (no spec_step_grammar)")
    return plan


def check_speculative_draft(model, draft_model, sampler, processors, structuring_engine, pixel_values, kv_bits, max_kv_size, prompt_logprobs=None):
    """What generate_step(speculative=SpeculativeParams(draft_model=...)) refuses, each by name, and the fused tail plan of
    what it accepts -- None for a greedy request without processors, whose passes are Model.spec_step's.  Besides what
    check_speculative_tail refuses: XTC (its coin changes the target's distribution from call to call), a draft model of another
    vocabulary, a tensor-parallel draft model."""
    what = "speculative decoding with a draft model"
    rows = _speculative_environment(model, structuring_engine, pixel_values, kv_bits, max_kv_size, prompt_logprobs)
    rows.insert(-1, (getattr(draft_model, "tp", None) is not None, "a tensor-parallel draft model"))  # (the KV pages' row stays the last)
    _refuse(what, rows)
    if not hasattr(model, "spec_step_draft") or not hasattr(model, "set_step_tail"):
        raise ValueError("speculative decoding with a draft model is not available with this model (no spec_step_draft)")
    if not all(hasattr(draft_model, a) for a in ("step", "set_step_tail", "history", "logprobs")):
        raise ValueError("speculative decoding with a draft model is not available with this draft model (no step / set_step_tail)")
    if draft_model is model:
        raise ValueError("speculative decoding with a draft model: the draft model is the target itself (build a second Model; the two keep separate caches and streams)")
    v_t, v_d = int(model.logprobs.numel()), int(draft_model.logprobs.numel())
    if v_t != v_d:
        raise ValueError(f"speculative decoding with a draft model: a vocabulary mismatch (the target has {v_t} ids, the draft model {v_d})")
    if getattr(sampler, "is_greedy", False) and not processors:
        return None
    return _speculative_plan(what, model, sampler, processors, structuring_engine, (("xtc", "XTC"),) + _PASS_REFUSED_PARTS)


def _speculative_request_plan(model, draft_model, sp: SpeculativeParams, samplers: dict, logits_processors: dict, structuring_engine,
                              pixel_values, kv_bits, max_kv_size):
    """Which of the three checks a generate_step(speculative=sp) request goes through, and the plan its passes run under (None: greedy
    and raw).  draft_model: sp.draft_model as a built Model, or None."""
    sampler, root = samplers["root"], logits_processors.get("root") or []
    if draft_model is not None:
        return check_speculative_draft(model, draft_model, sampler, root, structuring_engine, pixel_values, kv_bits, max_kv_size)
    all_procs = [p for ps in logits_processors.values() for p in ps]
    if sp.grammar and any(hasattr(p, "automaton") for p in root):
        return check_speculative_grammar(model, sampler, root, structuring_engine, pixel_values, kv_bits, max_kv_size)
    if (sp.configured_tail or sp.grammar) and not (getattr(sampler, "is_greedy", False) and not all_procs):
        return check_speculative_tail(model, sampler, root, structuring_engine, pixel_values, kv_bits, max_kv_size)
    # (a greedy request without processors under configured_tail=True: the greedy path)
    check_speculative(model, sampler, all_procs, structuring_engine, pixel_values, kv_bits, max_kv_size)
    return None


def _forced_ids(automaton, state: int, draft: list[int]) -> int:
    """How many ids of `draft`, walked from `state`, are the forced id of the state they were drafted in (TokenAutomaton.forced())."""
    forced, n = automaton.forced(), 0
    for t in draft:
        if not 0 <= state < automaton.n_states:
            break
        n += int(forced[state, 0] == t)
        state = automaton.step(state, t)
    return n


def _check_generate_args(model, pixel_values, mask, kv_bits, kv_group_size, max_kv_size, top_logprobs, prompt_logprobs, speculative) -> None:
    """What generate_step refuses in its arguments, before it touches the prompt cache or the model."""
    scored = prompt_logprobs is not None
    if speculative is not None and getattr(speculative, "batch_tail", False):
        raise ValueError("speculative decoding is not available with batch_tail (BatchedEngine's passes; the single sequence's is configured_tail)")
    if speculative is not None and scored:
        raise ValueError("speculative decoding is not available with prompt_logprobs")
    if scored and not 0 <= int(prompt_logprobs) <= hip_ops.TOP_LOGPROBS_MAX:
        raise ValueError(f"prompt_logprobs must be 0..{hip_ops.TOP_LOGPROBS_MAX}")
    if scored and getattr(model, "tp", None) is not None:
        raise ValueError("prompt_logprobs: not available on a tensor-parallel model")
    if top_logprobs is not None and not 0 <= int(top_logprobs) <= hip_ops.TOP_LOGPROBS_MAX:
        raise ValueError(f"top_logprobs must be 0..{hip_ops.TOP_LOGPROBS_MAX}")
    if kv_bits is not None:
        check_kv_format(kv_group_size, kv_bits)
    if max_kv_size is not None:
        RotatingKVCache(max_kv_size, keep=4)  # ValueError for a window that cannot hold the 4 sink rows plus one
        if getattr(model, "_page_pool", None) is not None:
            raise ValueError("max_kv_size: a rotating KV cache runs on contiguous buffers, not on the model's KV pages")
        if getattr(model, "tp", None) is not None:
            raise ValueError("max_kv_size: a rotating KV cache is not available on a tensor-parallel model")
    if mask is not None and not (isinstance(mask, str) and mask == "causal"):
        check_generate_mask(mask, getattr(getattr(model, "args", None), "num_attention_heads", None))
    if pixel_values is not None and not hasattr(model, "get_input_embeddings"):
        raise TypeError("pixel_values need a VLM ensemble (models/intern/ensemble.py: Model) as the engine's model")


class InferenceEngine:
    """One model, one PromptCache, not re-entrant -- like the reference (server/app.py:23,35)."""

    def __init__(self, model_path: str | None = None, *, model=None, stop_tokens=(), structuring_engine=None):
        """model_path: local checkpoint directory (models/utils.py layout).  `model=` injects an already built
        proxy_inference_engine_amd.models.llama.Model (synthetic checkpoints, tests, benchmarks)."""
        if model is None:
            if model_path is None:
                raise ValueError("InferenceEngine needs a model_path or a model")
            llm = load(model_path)
            model, self.hf_tokenizer, self.tokenizer_config = llm.model, llm.hf_tokenizer, llm.tokenizer_config
        else:
            self.hf_tokenizer, self.tokenizer_config = None, {}
        self.model = model
        self.prompt_cache = PromptCache()
        self.stop_tokens = set(int(t) for t in stop_tokens)
        self.structuring_engine = structuring_engine  # optional PSE-like object (inference_engine.py:37-41)
        self.samplers: dict[str, Sampler] = {}
        self.logits_processors: dict[str, list[LogitsProcessor]] = {}
        self._draft_models: dict = {}   # SpeculativeParams(draft_model=path): the checkpoints loaded so far, by path
        self._draft_cache = None        # the draft model's KV caches of the running request

    def _draft_model(self, sp):
        """SpeculativeParams.draft_model as a built Model: a checkpoint path is loaded once and kept."""
        dm = sp.draft_model
        if hasattr(dm, "step"):
            return dm
        key = str(dm)
        if key not in self._draft_models:
            self._draft_models[key] = load(key).model
        return self._draft_models[key]

    # ------------------------------------------------------------------ samplers / processors
    def make_sampler(self, **kwargs) -> Sampler:
        """inference_engine.py:299-317.  NB the reference's default is temp=1.0 (sampling); greedy needs temp=0.
        xtc_probability > 0 with xtc_threshold in (0, 0.5]: the draw runs under XTC; xtc_special_tokens (at most 16 ids)
        defaults to the engine's stop tokens, so XTC never removes the end of a sequence."""
        special = kwargs.get("xtc_special_tokens")
        sampler = make_sampler(temp=kwargs.get("temp", 1.0), top_p=kwargs.get("top_p", 1.0), top_k=kwargs.get("top_k", -1),
                               min_p=kwargs.get("min_p", 0.0), min_tokens_to_keep=kwargs.get("min_tokens_to_keep", 1),
                               xtc_probability=kwargs.get("xtc_probability") or 0.0, xtc_threshold=kwargs.get("xtc_threshold") or 0.0,
                               xtc_special_tokens=sorted(self.stop_tokens) if special is None else special)
        if self.structuring_engine is None:
            return sampler
        wrapped = lambda x: self.structuring_engine.sample(x, sampler)  # noqa: E731
        return wrapped

    def make_processors(self, **kwargs) -> list[LogitsProcessor]:
        """inference_engine.py:319-335: [PSE process_logits] + optional repetition penalty; around it the two processors DESIGN.md 12
        defines -- [token mask] in front (where the PSE's masking stands), [logit bias] behind (logit_processor_factory.cpp's order).
        token_mask: packed words, a bool mask or a callable tokens -> mask (make_token_mask); logit_bias: {token id: bias}.
        token_automaton: a TokenAutomaton, where the token mask stands and exclusive with it -- a grammar whose state
        lives on the device wherever the request takes the fused plan.
        frequency_penalty / presence_penalty (each -2.0 .. 2.0): one processor behind the bias, over the counts of the
        request's generated tokens.
        dry_multiplier != 0 (with dry_base, dry_allowed_length, dry_range, dry_sequence_breakers = token ids): the DRY
        processor behind the count penalty."""
        procs: list[LogitsProcessor] = []
        if self.structuring_engine is not None:
            procs.append(self.structuring_engine.process_logits)
        if kwargs.get("token_mask") is not None and kwargs.get("token_automaton") is not None:
            raise ValueError("make_processors: token_mask and token_automaton are exclusive")
        if kwargs.get("token_mask") is not None:
            procs.append(make_token_mask(kwargs["token_mask"]))
        if kwargs.get("token_automaton") is not None:
            procs.append(make_token_automaton(kwargs["token_automaton"]))
        if kwargs.get("repetition_penalty", 1.0) != 1.0:
            procs.append(repetition_penalty_logits_processor(float(kwargs.get("repetition_penalty", 1.0)),
                                                             int(kwargs.get("context_size", 60))))
        if kwargs.get("logit_bias"):
            procs.append(make_logit_bias(kwargs["logit_bias"]))
        freq, pres = hip_ops.check_count_penalties(kwargs.get("frequency_penalty") or 0.0, kwargs.get("presence_penalty") or 0.0, "make_processors")
        if freq != 0.0 or pres != 0.0:
            procs.append(count_penalty_logits_processor(freq, pres))
        dry = hip_ops.check_dry(kwargs.get("dry_multiplier") or 0.0, kwargs.get("dry_base", 1.75), kwargs.get("dry_allowed_length", 2),
                                kwargs.get("dry_range", 1024), kwargs.get("dry_sequence_breakers") or (), "make_processors")
        if dry[0] != 0.0:
            procs.append(dry_logits_processor(dry[0], dry[1], dry[2], dry[3], dry[4]))
        return procs

    def prepare_engine(self, prompt_ids, **inference_kwargs):
        """The sampler / processor half of prepare_engine (inference_engine.py:47-94); tokenisation and the
        state machine are outside this build, so `prompt_ids` are already token ids."""
        self.prompt_cache.load_cached_prompt(prompt_ids)
        self.samplers["root"] = self.make_sampler(**inference_kwargs)
        self.logits_processors["root"] = self.make_processors(**inference_kwargs)
        return prompt_ids

    # ------------------------------------------------------------------ the hot loop
    def generate_step(self, prompt_ids, pixel_values=None, mask=None, kv_bits: int | None = None, kv_group_size: int = 64,
                      quantized_kv_start: int = 0, max_kv_size: int | None = None,
                      top_logprobs: int | None = None, prompt_logprobs: int | None = None,
                      speculative: SpeculativeParams | None = None) -> Iterator[tuple[torch.Tensor, torch.Tensor]]:
        """Yields (next_token_id[1] int32, logprobs[V] fp32) per step, forever (inference_engine.py:228-297).
        Prefill of the non-cached prompt suffix, then one forward per token; all device work is queued
        asynchronously, the consumer synchronises when it reads a token (generate() does, like `.tolist()` :202).
        kv_bits (4 / 8; None = 16-bit KV), kv_group_size, quantized_kv_start: mlx_lm's KV quantization -- before a model call the
        prompt cache's layers become QuantizedKVCache once they hold more than quantized_kv_start positions (BaseCache.maybe_quantize,
        cache/kv_cache/__init__.py:240-266).
        max_kv_size (mlx_lm's name): the prompt cache becomes RotatingKVCache(max_kv_size, keep=4) per layer -- memory and step cost
        bounded by the window; kv_bits then has no effect (a rotating cache stays 16-bit, as in the reference).  A prompt cache of
        another kind or size is replaced by fresh rings (and back to the model's own caches when max_kv_size is None).
        top_logprobs (None: off, else 0..20): every step also leaves `self.top_record` = (ids int32 [n + 1], vals fp32 [n + 1]) on the
        device -- hip_ops.top_logprobs of the yielded logprobs with the yielded token in slot 0, valid until the next step:
        written inside the replayed step where the request takes the fused plan, by the op on the host-orchestrated branches.
        prompt_logprobs (None: off, else 0..20): the prompt's own tokens are scored inside the prompt pass (Model.set_prompt_logprobs;
        DESIGN.md 16) and `self.prompt_logprobs` holds their maps before the first yield -- entry 0 None, entry j the map of prompt token j
        under the raw model distribution: the best prompt_logprobs pairs, then the token itself when absent.  Such a request processes its
        whole prompt: the prompt cache's common prefix is not reused for it.
        speculative (None: exactly the path above): greedy speculative decoding -- each yield is then (tokens [m] int32,
        logprobs [m, V] fp32), the m >= 1 tokens one verify pass accepted (or the one token of a plain step) with their rows'
        log-probabilities, the same tokens the plain loop yields one by one; `self.spec_stats` counts passes, steps, drafted and accepted
        ids.  With top_logprobs, `self.top_record` holds one record per yielded token ([m, n + 1]).  Greedy and raw only: a non-greedy
        sampler, logits processors, a structuring engine, pixel_values, kv_bits, max_kv_size, prompt_logprobs, a tensor-parallel model
        and int8 KV pages are refused by name.  SpeculativeParams(configured_tail=True) lifts the first two for what the
        fused tail plan holds besides a token mask, counts and DRY: the request's sampler, repetition penalty and logit bias run inside
        the passes, token j is draw j of the samplers' seed from row j's distribution, and the yielded rows are the processed
        log-probabilities."""
        _check_generate_args(self.model, pixel_values, mask, kv_bits, kv_group_size, max_kv_size, top_logprobs, prompt_logprobs, speculative)
        scored = prompt_logprobs is not None
        self.prompt_logprobs = self.top_record = None
        if "root" not in self.samplers:
            self.prepare_engine(prompt_ids, temp=0)
        spec_plan = None
        if speculative is not None:
            spec_plan = _speculative_request_plan(self.model, None if speculative.draft_model is None else self._draft_model(speculative), speculative,
                                                  self.samplers, self.logits_processors, self.structuring_engine, pixel_values, kv_bits, max_kv_size)
        self._select_prompt_cache(prompt_ids, max_kv_size, scored)
        todo = self.prompt_cache(prompt_ids)                                   # :277
        host_ids = [int(t) for t in (todo.tolist() if isinstance(todo, torch.Tensor) else todo)]
        if speculative is not None and speculative.draft_model is not None:
            yield from self._speculative_draft_steps([int(t) for t in prompt_ids], host_ids, speculative, top_logprobs, spec_plan)
            return
        if speculative is not None:
            yield from self._speculative_steps(host_ids, speculative, top_logprobs, spec_plan)
            return
        # what every step of this request is called with; host_top: [(ids, vals), workspace] of the host-orchestrated branches' top-n record
        request = dict(pixel_values=pixel_values, kv_quant=None if kv_bits is None else (quantized_kv_start, kv_group_size, kv_bits),
                       top_logprobs=top_logprobs, count_start=len(prompt_ids), host_top=[])
        if scored and len(host_ids) > 1:
            lm = getattr(self.model, "language_model", self.model)
            bufs = lm.set_prompt_logprobs(len(host_ids), max(int(prompt_logprobs), 1))
            targets, counts = prompt_targets(host_ids, int(prompt_logprobs))
            bufs["targets"].copy_(torch.tensor(targets, dtype=torch.int32))
            bufs["count"].copy_(torch.tensor(counts, dtype=torch.int32))
            try:
                next_token, logprobs = self._inference(torch.tensor(host_ids, dtype=torch.int32), False, **request)
            finally:
                lm.clear_prompt_logprobs()
            self.prompt_logprobs = prompt_maps(bufs["ids"].cpu().numpy(), bufs["vals"].cpu().numpy(), int(prompt_logprobs))
        else:
            if scored:
                self.prompt_logprobs = [None]
            next_token, logprobs = self._inference(torch.tensor(host_ids, dtype=torch.int32), False, **request)   # :278 (host ids: no read-back)
        while True:
            yield next_token, logprobs
            next_token, logprobs = self._inference(next_token, True, **request)   # :288

    def _select_prompt_cache(self, prompt_ids, max_kv_size: int | None, scored: bool) -> None:
        """The prompt cache a request runs on -- the one it finds, or fresh caches of the kind it asks for -- and the request's start for
        the processors that keep state of their own."""
        cur = self.prompt_cache.cache
        ring = bool(cur) and isinstance(cur[0], RotatingKVCache)
        if cur and (scored or ring != (max_kv_size is not None) or (ring and cur[0].max_size != max_kv_size)):
            self.prompt_cache.cache, self.prompt_cache.computed_ids = [], []  # another cache kind: nothing of it is reusable; a scored prompt: every row is computed
        if len(self.prompt_cache.cache) == 0:
            if max_kv_size is not None:
                self.prompt_cache.cache = BaseCache.make_kv_cache(self.model, max_kv_size=max_kv_size)
            else:
                self.prompt_cache.create_kv_cache(self.model)                  # :274-275
        for procs in self.logits_processors.values():
            for proc in procs:
                if (hasattr(proc, "frequency_penalty") or hasattr(proc, "automaton")) and hasattr(proc, "reset"):
                    proc.reset(len(prompt_ids))  # the prompt cache may be reused across requests, the counts and an automaton's walk may not: this request's start

    def _inference(self, ids: torch.Tensor, fed_back: bool, *, pixel_values, kv_quant, top_logprobs, count_start, host_top: list) -> tuple[torch.Tensor, torch.Tensor]:
        """One forward + tail.  fed_back: `ids` is the token the previous call returned (still in the decoder's
        device-side state), so nothing has to be copied or read back.  The state, its sampler and processors and the plan are resolved
        here, per call: a structuring engine changes state per token, and prepare_engine may run between two steps."""
        self.top_record = None
        state = "root"
        if self.structuring_engine is not None:
            state = self.structuring_engine.get_current_state() or "root"
            if state not in self.logits_processors:
                state = "root"
        sampler = self.samplers[state]
        procs = self.logits_processors.get(state) or []
        if kv_quant is not None:
            self._maybe_quantize(*kv_quant)
        model = self.model
        plan = fused_tail_plan(procs, sampler, self.structuring_engine, getattr(model, "tp", None) is not None) if hasattr(model, "set_step_tail") else None
        offset = int(self.prompt_cache.cache[0].offset) if self.prompt_cache.cache else 0
        if plan is None or offset + int(ids.numel()) > model.fed_ids.numel():
            self._apply_tail_plan(None)  # the host-orchestrated branches run on Model.step's documented greedy tail
            tok, logprobs = self._host_tail(ids, fed_back, pixel_values, sampler, procs)
            if top_logprobs is not None:  # their top-n record comes from the op (the fused plan's is written inside the step)
                self._record_top(host_top, top_logprobs, tok.reshape(1).to(torch.int32), logprobs.reshape(1, -1), 1)
                self.top_record = (self.top_record[0][0], self.top_record[1][0])
            return tok, logprobs
        # The whole tail inside the step: mask, penalty, bias, log-softmax and the draw ride the replayed graph; the
        # drawn token is fed back on the device, so a fed-back step passes nothing, whatever the sampler
        mask = plan["mask"]
        vocab = getattr(model, "language_model", model).logprobs.numel()
        words = None
        if mask is not None:
            check_vocab(mask, vocab)
            words = mask.mask  # (static host words: set_step_tail refuses a mask that allows no token when it uploads them)
        recorded = mask is not None and mask.mask_fn is not None
        if recorded:
            # a grammar's mask depends on the tokens so far, this row's input included (the processors run after :255): the one
            # read-back of the fed-back token such a request pays per step, then a 16 KB upload into the replayed graph's buffer
            self.prompt_cache.update(ids)
            words = packed_token_mask(mask.mask_fn(self.prompt_cache.computed_ids), vocab)
        # count_start: the request's first call starts zero counts, from the prompt's end on
        self._apply_tail_plan(plan, offset, first=not fed_back, count_start=None if fed_back else count_start, token_mask=words,
                              **({} if top_logprobs is None else {"top_logprobs": int(top_logprobs)}))
        if plan.get("automaton") is not None and not fed_back:
            # the request's first call: the start state, in stream order.  From here on the state moves on the device by the
            # token each step feeds back: nothing is read back and no mask is uploaded
            model.reset_step_automaton()
        if pixel_values is not None and not fed_back:
            embeds = model.get_input_embeddings(ids.reshape(1, -1), pixel_values)
            tok, logprobs, _ = model.step_embeds(embeds, self.prompt_cache.cache, ids)
        else:
            tok, logprobs, _ = model.step(None if fed_back else ids, self.prompt_cache.cache)
        if not recorded:
            self.prompt_cache.update(ids)                              # :255 (device ids resolve lazily)
        if top_logprobs is not None:
            self.top_record = model.step_top_logprobs
        return tok, logprobs

    def _apply_tail_plan(self, plan: dict | None, offset: int = 0, first: bool = True, count_start: int | None = None, **step_parts) -> None:
        """Configures the model's step tail (Model.set_step_tail) with a fused tail plan's parts -- a part the plan lacks is not passed,
        so the setter's default switches it off -- and the caller's step_parts; plan None: the documented greedy tail, where the model
        has a configurable one.  first, over a reused prefix of `offset` cached positions: the prefix's ids may predate this
        configuration (fed back unrecorded, loaded from disk), so the fed ids a tail reads are written again from the prompt cache's,
        which may already hold this call's own ids behind them."""
        model = self.model
        if plan is None:
            if hasattr(model, "set_step_tail"):
                model.set_step_tail()
            return
        bias, counts, dry = plan["bias"], plan.get("counts"), plan.get("dry")
        window = max(plan["context_size"] if plan["repetition_penalty"] != 1.0 else 0, 0 if dry is None else dry.dry_range)  # the fed ids a tail reads
        if window and first and offset > 0:
            seen = self.prompt_cache.computed_ids[offset - min(offset, window):offset]
            model.fed_ids[offset - len(seen):offset].copy_(torch.tensor(seen, dtype=torch.int32))
        parts = dict(sampler=plan["sampler"], repetition_penalty=plan["repetition_penalty"], context_size=plan["context_size"],
                     logit_bias=None if bias is None else (bias.ids, bias.values))
        if counts is not None:  # (a request without them passes nothing: set_step_tail's defaults switch them off)
            parts.update(frequency_penalty=counts.frequency_penalty, presence_penalty=counts.presence_penalty, count_start=count_start)
        if dry is not None:
            parts["dry"] = (dry.dry_multiplier, dry.dry_base, dry.dry_allowed_length, dry.dry_range, dry.dry_sequence_breakers)
        if plan.get("xtc") is not None:
            parts["xtc"] = plan["xtc"]
        if plan.get("automaton") is not None:
            parts["token_automaton"] = plan["automaton"].automaton
        model.set_step_tail(**parts, **step_parts)

    def _invoke(self, ids: torch.Tensor, fed_back: bool, pixel_values, procs, greedy: bool):
        """The model call of a host-orchestrated step: (token, logprobs) from the fused step where no processor wants the logits,
        else the raw logits of the last row [1, V]."""
        model, cache = self.model, self.prompt_cache.cache
        if pixel_values is not None and not fed_back:
            # the prompt of a VLM request (:246-252): text embeddings with the image features scattered in, through the
            # text tower.  The reference passes pixel_values on every later step too, where a single new token holds
            # no image token and the vision tower's output is discarded (ensemble.py:62-91); those steps skip it here.
            embeds = model.get_input_embeddings(ids.reshape(1, -1), pixel_values)
            if not procs:
                return model.step_embeds(embeds, cache)[:2]
            return model.language_model(None, cache=cache, inputs_embeds=embeds)[:, -1, :]
        if not procs:
            # fused step: hipGraph replay for L == 1, log-softmax (+ greedy argmax) in the HIP tail, no host sync; only a greedy
            # step finds the token it is fed on the device
            return model.step(None if (fed_back and greedy) else ids, cache)[:2]
        return model(ids[None], cache=cache)[:, -1, :]                         # :252, :254

    def _host_tail(self, ids: torch.Tensor, fed_back: bool, pixel_values, sampler, procs) -> tuple[torch.Tensor, torch.Tensor]:
        """A step outside the fused plan: the model call, then the processors, the log-softmax and the sampler from the host."""
        greedy_sampler = getattr(sampler, "is_greedy", False)
        out = self._invoke(ids, fed_back, pixel_values, procs, greedy_sampler)
        self.prompt_cache.update(ids)                                          # :255 (device ids resolve lazily)
        if procs:
            last = out
            for proc in procs:                                                 # :257-266
                last = proc(self.prompt_cache.computed_ids, last)
            tok, logprobs = hip_ops.logprobs_argmax(last)                      # :268-269 + greedy argmax, HIP tail
        else:
            tok, logprobs = out
        if greedy_sampler:
            return tok, logprobs
        drawn = sampler(logprobs[None])                                        # :271
        # stochastic sampler without processors: drawn on the device; the token tensor feeds the next step without a read-back
        return (drawn if procs else drawn.reshape(1).to(torch.int32)), logprobs

    def _record_top(self, host_top: list, top_logprobs: int | None, tokens_dev: torch.Tensor, rows: torch.Tensor, max_rows: int) -> None:
        """The top-n records of a yield, from the host: one hip_ops.top_logprobs call over the yielded rows [m <= max_rows, V], record r =
        token r's, left on `self.top_record` as [m, n + 1].  host_top keeps this generation's own record and workspace, made once: a
        yield allocates nothing."""
        if top_logprobs is None:
            return
        n, m = max(int(top_logprobs), 1), rows.shape[0]
        if not host_top:
            host_top.append((torch.full((max_rows, n + 1), -1, dtype=torch.int32, device=rows.device),
                             torch.full((max_rows, n + 1), float("-inf"), dtype=torch.float32, device=rows.device)))
            host_top.append(hip_ops.top_logprobs_workspace(rows.device, max_rows, rows.shape[1], n))
        ids, vals = hip_ops.top_logprobs(rows, n, tokens=tokens_dev[:m].contiguous(), workspace=host_top[1], out=(host_top[0][0][:m], host_top[0][1][:m]))
        self.top_record = (ids[:, :int(top_logprobs) + 1], vals[:, :int(top_logprobs) + 1])

    def _speculative_prologue(self, host_ids: list[int], plan: dict | None, top_logprobs: int | None):
        """What both speculative loops begin with: the plan's tail on the target (its passes and its plain steps run under it), fresh
        `spec_stats`, the generation's top-n recorder, and the prompt's suffix as one plain step.  Returns (token, rows [1, V], record)."""
        model, cache = self.model, self.prompt_cache.cache
        offset = int(cache[0].offset) if cache else 0
        if plan is not None and offset + len(host_ids) > model.fed_ids.numel():
            raise ValueError("speculative decoding: the prompt runs past the model's id history")
        self._apply_tail_plan(plan, offset)  # (plan None: the documented greedy tail: the passes refuse anything else)
        self.spec_stats = {"passes": 0, "steps": 0, "drafted": 0, "accepted": 0}
        if plan is not None and plan.get("automaton") is not None:  # (only check_speculative_grammar's plans hold one)
            model.reset_step_automaton()  # the request's start state, in stream order, as _inference's first call
            self.spec_stats["forced"] = 0
        record = partial(self._record_top, [], top_logprobs, max_rows=hip_ops.SPEC_MAX_ROWS)  # record(tokens on the device, rows)
        ids = torch.tensor(host_ids, dtype=torch.int32)
        tok, logprobs, _ = model.step(ids, cache)
        self.prompt_cache.update(ids)
        return tok, logprobs[None], record

    def _speculative_pass_done(self, fed: int, tokens: list[int], drafted: int, n: int) -> None:
        """A verify pass's accounting.  The prompt cache receives the ids whose K / V rows the cache now holds: the fed-back token and the
        accepted drafts, not the token behind them."""
        self.prompt_cache.update([fed] + tokens[:-1])
        self.spec_stats["passes"] += 1
        self.spec_stats["drafted"] += drafted
        self.spec_stats["accepted"] += n - 1

    def _speculative_steps(self, host_ids: list[int], sp: SpeculativeParams, top_logprobs: int | None, plan: dict | None = None):
        """generate_step's loop under speculative decoding.  The prompt's suffix is one plain step; behind it, and behind every
        later step or pass, ONE drafter launch is queued, and its count comes back in the read-back the loop pays anyway: the tokens
        (Model.spec_read).  count >= min_draft (and enough rows for the many-row pass): a verify pass over count + 1 rows, whose accepted
        tokens are the next yield; otherwise one replayed step.  prompt_cache.update receives the ids whose K / V rows the cache now holds:
        the fed-back token and the accepted drafts.
        plan (check_speculative_tail's): the steps are the ordinary configured replayed step and the passes
        Model.spec_step_tail under the plan's sampler / XTC / repetition penalty / logit bias; both draw from one stream position, so
        token j of the generation is draw j of the seed whichever produced it.
        A plan that holds an automaton (check_speculative_grammar's): the drafter's launch is followed by the grammar's, the
        passes are Model.spec_step_grammar and the steps the ordinary step under the automaton.  The automaton's state is followed on the
        host from the tokens the loop reads anyway, only to count the forced ids of a draft: nothing more is read back."""
        model, cache = self.model, self.prompt_cache.cache
        automaton = None if plan is None or plan.get("automaton") is None else plan["automaton"].automaton
        spec_pass = model.spec_step if plan is None else model.spec_step_tail if automaton is None else model.spec_step_grammar
        drafter = (int(sp.ngram_max), int(sp.ngram_min), int(sp.num_draft)) + (() if automaton is None else (True,))
        floor = max(int(sp.min_draft), int(getattr(model, "spec_min_rows", 6)) - 1)
        _, rows, record = self._speculative_prologue(host_ids, plan, top_logprobs)
        model.draft(*drafter)
        state = None if automaton is None else automaton.start
        while True:
            tokens, count = model.spec_read()
            record(model.spec_tokens, rows)
            yield torch.tensor(tokens, dtype=torch.int32), rows
            fed = tokens[-1]
            if automaton is not None:
                state = automaton.walk(tokens, state)  # the device-side state the draft started from
            if count >= floor:
                if automaton is not None:
                    self.spec_stats["forced"] += _forced_ids(automaton, state, model.spec_read_draft())
                _, n, rows = spec_pass(model.spec_draft[:count], cache, then_draft=drafter)
                self._speculative_pass_done(fed, model.spec_read()[0], count, n)
            else:
                _, logprobs, _ = model.step(None, cache)
                self.prompt_cache.update([fed])
                model.draft(*drafter)
                rows = logprobs[None]
                self.spec_stats["steps"] += 1

    def _speculative_draft_steps(self, prompt_ids: list[int], host_ids: list[int], sp: SpeculativeParams, top_logprobs: int | None, plan: dict | None):
        """generate_step's loop with a draft model.  The draft model gets ReusableKVCaches of its own and the WHOLE prompt (no
        prefix reuse for it); the target's prompt suffix is one plain step.  A round: the drafter is fed the current token and replays
        num_draft of its configured steps back to back, no host synchronisation in between -- its drafts are its own device-side history,
        and behind every step its bound log-probabilities are copied, device to device in stream order, into a row of one [31, V] block;
        one target pass (Model.spec_step_draft under a stochastic sampler, spec_step / spec_step_tail for a greedy request); the one
        record read-back; the drafter's caches trimmed to the accepted offset -- the rows behind it are overwritten before anything
        attends to them -- or, when every draft was accepted, the drafter fed the last draft, whose K / V rows it never produced.
        The drafter draws under the request's (mode, temp, p, k) and samplers._rng.draft_state's seed, never under the target's."""
        from ..samplers import _rng
        model, cache, d = self.model, self.prompt_cache.cache, self._draft_model(sp)
        k, min_rows = int(sp.num_draft), int(model.spec_min_rows)
        if not min_rows - 1 <= k <= hip_ops.SPEC_MAX_ROWS - 1:
            raise ValueError(f"speculative decoding with a draft model: num_draft is {min_rows - 1}..{hip_ops.SPEC_MAX_ROWS - 1} (the pass keeps at least {min_rows} rows), got {k}")
        limit = min(model.fed_ids.numel(), d.fed_ids.numel(), d.history.numel())
        if len(prompt_ids) > limit:
            raise ValueError("speculative decoding: the prompt runs past the model's id history")
        sampler = None if plan is None else plan["sampler"]
        draft_seed = None
        if sampler is not None:  # one sampler setting for both sides, two streams
            draft_seed, draft_counter = _rng.draft_state(d.device)
            d.set_step_tail(sampler=sampler, rng=(draft_seed, draft_counter))
            q_rows = torch.empty((hip_ops.SPEC_MAX_ROWS - 1, d.logprobs.numel()), dtype=torch.float32, device=d.device)
        else:
            d.set_step_tail()
        self._draft_cache = dcache = [ReusableKVCache() for _ in d.layers]
        d.step(torch.tensor(prompt_ids, dtype=torch.int32), dcache)  # (its own choice behind the prompt is not used: the target's is fed)
        tok, rows, record = self._speculative_prologue(host_ids, plan, top_logprobs)
        record(tok, rows)
        tokens = [int(tok)]
        while True:
            yield torch.tensor(tokens, dtype=torch.int32), rows
            fed, o = tokens[-1], int(cache[0].offset)
            if o != int(dcache[0].offset):
                raise RuntimeError("speculative decoding: the draft model's cache left the target's offset")
            if o + k + 1 > limit:
                raise ValueError("speculative decoding: the round would run past the model's id history")
            d.step(torch.tensor([fed], dtype=torch.int32), dcache)
            for i in range(k):
                if i:
                    d.step(None, dcache)
                if sampler is not None:
                    q_rows[i].copy_(d.logprobs)
            draft = d.history[o + 1:o + 1 + k]
            if sampler is not None:
                _, n, rows = model.spec_step_draft(draft, q_rows, cache, draft_seed=draft_seed)
            elif plan is not None:
                _, n, rows = model.spec_step_tail(draft, cache)
            else:
                _, n, rows = model.spec_step(draft, cache)
            tokens = model.spec_read()[0]
            self._speculative_pass_done(fed, tokens, k, n)
            if n == k + 1:
                d.step(torch.tensor(tokens[-2:-1], dtype=torch.int32), dcache)  # the last draft: accepted, and not yet in the drafter's cache
            else:
                for c in dcache:
                    c.trim(k - n)  # offset o + k -> o + n
            record(model.spec_tokens, rows)

    def score(self, prompt_ids, top_logprobs: int = 0, **kv) -> list:
        """The log-probabilities of a prompt's own tokens (`echo`, perplexity, ranking): runs the prompt only and returns a list as long as
        the prompt -- entry 0 None, entry j the {id: logprob} map of prompt token j given the tokens before it: the best top_logprobs
        pairs, then the token itself when absent.  kv: generate_step's KV arguments (kv_bits, kv_group_size, quantized_kv_start, max_kv_size)."""
        step = self.generate_step(prompt_ids, prompt_logprobs=int(top_logprobs), **kv)
        next(step)
        step.close()
        return self.prompt_logprobs

    def _maybe_quantize(self, quantized_start: int, group_size: int, bits: int) -> None:
        """BaseCache.maybe_quantize (cache/kv_cache/__init__.py:240-266) on the prompt cache's layers."""
        cache = self.prompt_cache.cache
        if cache and isinstance(cache[0], PagedKVCache):
            raise ValueError("kv_bits: the quantized KV cache runs on contiguous caches, not on KV pages")
        if cache and isinstance(cache[0], ReusableKVCache) and cache[0].offset > quantized_start:
            for i in range(len(cache)):
                cache[i] = QuantizedKVCache.from_cache(cache[i], group_size=group_size, bits=bits)

    def generate(self, prompt_ids, **inference_kwargs) -> Generator[ModelOutput, None, str]:
        """Stop-token / max_completion_tokens loop (inference_engine.py:175-226).  Yields (token_id, logprobs_map);
        the generator's return value is the stop reason ("stop" | "length" | "tool_calls")."""
        max_completion_tokens = inference_kwargs.get("max_completion_tokens", -1)
        collect_logprobs = inference_kwargs.get("logprobs", False)
        top_logprobs: int = int(inference_kwargs.get("top_logprobs", 0) or 0)
        if collect_logprobs and not 0 <= top_logprobs <= hip_ops.TOP_LOGPROBS_MAX:
            raise ValueError(f"top_logprobs must be 0..{hip_ops.TOP_LOGPROBS_MAX}")   # the reference request model's bound
        logprobs_map: dict[int, float] = {}
        stop_reason = "stop"
        token_count = 0
        kv = {k: inference_kwargs[k] for k in ("kv_bits", "kv_group_size", "quantized_kv_start", "max_kv_size") if inference_kwargs.get(k) is not None}
        if collect_logprobs:
            kv["top_logprobs"] = top_logprobs
        if inference_kwargs.get("prompt_logprobs") is not None:  # the prompt's maps are on `self.prompt_logprobs` before the first yield
            kv["prompt_logprobs"] = int(inference_kwargs["prompt_logprobs"])
        if inference_kwargs.get("speculative") is not None:  # (a request without it passes nothing: exactly the plain loop)
            kv["speculative"] = inference_kwargs["speculative"]
        for new_tokens, new_logprobs in self.generate_step(prompt_ids, **kv):
            budget = max_completion_tokens - token_count if max_completion_tokens > 0 else new_tokens.numel()  # a pass may yield more than is left
            token_count += new_tokens.numel()
            maps = None
            if collect_logprobs and self.top_record[0].dim() == 2:
                # a speculative pass: one read of its [m, n + 1] records, one map per accepted token
                token_ids, maps = records_to_maps(*self.top_record, top_logprobs)
            elif collect_logprobs:
                # one read per token: the (n + 1)-pair record, whose slot 0 is the token itself
                token_ids, logprobs_map = record_to_map(*self.top_record, top_logprobs)
            else:
                token_ids = new_tokens.tolist()
            stopped = False
            for i, token_id in enumerate(token_ids[:budget]):
                if token_id in self.stop_tokens:
                    stopped = True
                    break
                if maps is not None:
                    logprobs_map = maps[i]
                yield token_id, logprobs_map
            if stopped:
                # the reference `break`s only the inner loop and keeps generating (inference_engine.py:204-206);
                # that is an endless loop once a stop token appears, so the outer loop ends here instead
                break
            if self.structuring_engine is not None and self.structuring_engine.has_reached_accept_state:
                stop_reason = "tool_calls"
                break
            if max_completion_tokens > 0 and token_count >= max_completion_tokens:
                stop_reason = "length"
                break
        return stop_reason


def record_to_map(ids: torch.Tensor, vals: torch.Tensor, top_k: int) -> tuple[list[int], dict[int, float]]:
    """One top-n record (hip_ops.top_logprobs; device or host) -> ([token], {id: logprob}): the best top_k pairs by decreasing
    log-probability (ties: lowest id first), then the chosen token of slot 0 when absent.  One read-back of 2 (n + 1) words."""
    tokens, maps = records_to_maps(ids.reshape(1, -1), vals.reshape(1, -1), top_k)
    return tokens, maps[0]


def records_to_maps(ids: torch.Tensor, vals: torch.Tensor, top_k: int) -> tuple[list[int], list[dict[int, float]]]:
    """record_to_map for the [m, n + 1] records of a speculative pass: ([token per row], [map per row]), one read-back for all rows."""
    import numpy as np
    m = ids.shape[0]
    words = torch.cat([ids.reshape(-1), vals.reshape(-1).view(torch.int32)]).cpu().numpy()
    h_ids, h_vals = words[:words.size // 2].reshape(m, -1), words[words.size // 2:].view(np.float32).reshape(m, -1)
    rows = [host_record_to_map(h_ids[r], h_vals[r], top_k) for r in range(m)]
    return [t[0][0] for t in rows], [t[1] for t in rows]


def host_record_to_map(ids, vals, top_k: int) -> tuple[list[int], dict[int, float]]:
    """record_to_map for a record already on the host (numpy int32 [n + 1], float32 [n + 1])."""
    out = {int(i): float(v) for i, v in zip(ids[1:1 + top_k], vals[1:1 + top_k]) if i >= 0}
    token = int(ids[0])
    if token not in out:
        out[token] = float(vals[0])
    return [token], out


def prompt_targets(prompt_ids, top_k: int) -> tuple[list[int], list[int]]:
    """What the host writes for the rows of one prompt (Model.set_prompt_logprobs): targets[i] = the id that follows row i, counts[i] =
    top_k -- and for the last row, which nothing follows, (0, -1): its record is left alone."""
    ids = [int(t) for t in prompt_ids]
    return ids[1:] + [0], [int(top_k)] * (len(ids) - 1) + [-1]


def prompt_maps(ids, vals, top_k: int) -> list:
    """The records of a prompt's rows on the host (numpy int32 / float32 [L, n + 1]) -> [None, map of token 1, ..., map of token L - 1]:
    row j - 1 scores token j."""
    return [None] + [host_record_to_map(ids[r], vals[r], top_k)[1] for r in range(len(ids) - 1)]


def get_top_logprobs(logprobs: torch.Tensor, top_k: int) -> dict[int, float]:
    """engine/utils.py:4-48: the top_k (token -> logprob) pairs, sorted by decreasing logprob."""
    if top_k == 0:
        return {}
    if logprobs.dim() == 2:
        logprobs = logprobs.squeeze(0)
    elif logprobs.dim() != 1:
        raise ValueError(f"Expected 1D or 2D array, got {logprobs.dim()}D")
    top_k = min(top_k, logprobs.shape[0])
    if logprobs.shape[0] == 0:
        return {}
    vals, idx = torch.topk(logprobs, top_k)
    return {int(i): float(v) for i, v in zip(idx.tolist(), vals.tolist())}
