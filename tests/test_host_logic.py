"""CPU: host-side mirrors of the reference's cache / prompt-cache / sampler logic behave like the oracle's
restatement (and therefore like cache/kv_cache/reusable.py, cache/prompt_cache.py, samplers/__init__.py)."""
import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from proxy_inference_engine_amd.cache import PromptCache, ReusableKVCache
from proxy_inference_engine_amd.logits_processors import make_repetition_penalty
from proxy_inference_engine_amd.models.base import create_attention_mask, create_causal_mask
from proxy_inference_engine_amd.models.llama import ModelArgs
from proxy_inference_engine_amd.samplers import make_sampler


def test_reusable_cache_capacity_sequence_matches_oracle():
    ref, mine = po.OracleKVCache(), ReusableKVCache()
    k = np.ones((1, 2, 128, 8), np.float32)
    ref.update_and_fetch(k, k)
    mine.update_and_fetch(torch.ones(1, 2, 128, 8), torch.ones(1, 2, 128, 8))
    one = torch.full((1, 2, 1, 8), 2.0)
    for _ in range(1100):
        ref.update_and_fetch(one.numpy(), one.numpy())
        kk, vv = mine.update_and_fetch(one, one)
        assert (mine.offset, mine.capacity) == (ref.offset, ref.keys.shape[2])
    assert kk.shape[2] == mine.offset and np.array_equal(mine.keys.numpy(), ref.keys)
    assert mine.trim(28) == 28 and mine.offset == 1200 and mine.is_trimmable() and mine.to_quantized() is mine
    # reserve()/advance() = the two halves of update_and_fetch used by the fused decoder
    c = ReusableKVCache()
    c.reserve(300, 2, 8, torch.float32, "cpu")
    assert c.capacity == 512 and c.offset == 0
    c.advance(300)
    c.reserve(300, 2, 8, torch.float32, "cpu")
    assert c.capacity == 768
    capped = ReusableKVCache(max_capacity=256)
    capped.reserve(200, 1, 8, torch.float32, "cpu")
    capped.advance(200)
    with pytest.raises(RuntimeError):
        capped.reserve(100, 1, 8, torch.float32, "cpu")


@pytest.mark.parametrize("chunks", [(520, 300), (700, 400), (255, 2, 300), (256, 300), (100, 1, 1, 700, 5, 900)])
def test_reusable_cache_growth_at_unaligned_offsets_matches_oracle(chunks):
    """reusable.py:125-129: growing at an offset that is not a multiple of `step` first slices the buffers to the offset, so the
    new capacity is computed from the offset (520 then 300 tokens -> 1024, not 1280).  Both halves of the product's API."""
    ref, mine, split = po.OracleKVCache(), ReusableKVCache(), ReusableKVCache()
    for n in chunks:
        ref.update_and_fetch(np.ones((1, 2, n, 8), np.float32), np.ones((1, 2, n, 8), np.float32))
        mine.update_and_fetch(torch.ones(1, 2, n, 8), torch.ones(1, 2, n, 8))
        split.reserve(n, 2, 8, torch.float32, "cpu")
        split.advance(n)
        assert (mine.offset, mine.capacity) == (ref.offset, ref.keys.shape[2])
        assert (split.offset, split.capacity) == (ref.offset, ref.keys.shape[2])
    if chunks == (520, 300):
        assert mine.capacity == 1024


def test_prompt_cache_history_is_cut_on_reuse():
    """A -> B -> A: after B diverged at k the caches hold B beyond k; the history must say so (deviation from
    prompt_cache.py:52-76, which keeps A + B[k:] and would let the third request reuse B's rows as A's)."""
    pc = PromptCache()
    pc.cache = [ReusableKVCache()]
    A, B = list(range(100, 140)), list(range(100, 120)) + list(range(500, 530))
    one = lambda n: torch.ones(1, 1, n, 8)

    def request(ids):
        todo = pc(torch.tensor(ids))
        pc.cache[0].update_and_fetch(one(len(todo)), one(len(todo)))
        pc.update(todo)
        return len(todo)

    assert request(A) == 40 and pc.computed_ids == A
    assert request(B) == 30 and pc.computed_ids == B and pc.cache[0].offset == 50
    assert request(A) == 20 and pc.computed_ids == A and pc.cache[0].offset == 40      # the reference would process 1 token here


def test_prompt_cache_lcp_matches_oracle():
    ref, mine = po.OraclePromptCache(), PromptCache()
    ref.cache, mine.cache = [po.OracleKVCache()], [ReusableKVCache()]
    k = np.ones((1, 2, 128, 8), np.float32)
    ref.cache[0].update_and_fetch(k, k)
    mine.cache[0].update_and_fetch(torch.ones(1, 2, 128, 8), torch.ones(1, 2, 128, 8))
    ref.update(np.arange(128)); mine.update(torch.arange(128))
    for prompt in (np.arange(128), np.concatenate([np.arange(50), np.arange(900, 1200)]), np.array([999, 1, 2]), np.arange(3)):
        a, b = ref(prompt), mine(torch.from_numpy(prompt))
        assert list(a) == list(b.tolist())
        assert (mine.cache[0].offset, mine.cache[0].capacity) == (ref.cache[0].offset, ref.cache[0].keys.shape[2])
    assert PromptCache()(torch.arange(5)).tolist() == [0, 1, 2, 3, 4]     # nothing cached yet


def test_sampler_and_processor_conventions():
    assert not getattr(make_sampler(temp=0.7, top_p=0.9), "is_greedy", False)
    assert getattr(make_sampler(temp=0), "is_greedy", False)
    with pytest.raises(ValueError):
        make_repetition_penalty(-1.0)
    proc = make_repetition_penalty(2.0, context_size=3)
    logits = torch.tensor([[1.0, -1.0, 4.0, -4.0, 8.0]])
    out = proc([4, 0, 1, 2, 3], logits.clone())                         # only the last 3 tokens count
    assert out.tolist() == [[1.0, -2.0, 2.0, -8.0, 8.0]]


def test_masks_and_model_args():
    m = create_causal_mask(3, offset=2)
    assert m.shape == (3, 5) and m[0].tolist() == [0, 0, 0, -1e9, -1e9] and m[2].tolist() == [0, 0, 0, 0, 0]
    assert np.array_equal(m.numpy().astype(np.float32), po.causal_mask(3, 2, "float32"))
    assert create_attention_mask(torch.zeros(1, 1, 8)) is None          # L == 1: no mask (models/base.py:39-53)
    a = ModelArgs(model_type="llama", hidden_size=64, num_hidden_layers=1, intermediate_size=128, num_attention_heads=2,
                  rms_norm_eps=1e-5, vocab_size=10, some_unknown_key=1)
    assert a.tie_word_embeddings is True and a.rope_theta == 10000 and not hasattr(a, "some_unknown_key")


def _ref_sets(logprobs, temp, top_p=0.0, min_p=0.0, keep=1, top_k=-1):
    """Numpy restatement of which vocabulary ids the reference's filters leave drawable (samplers/{top_p,min_p,top_k}.py)."""
    x = logprobs.astype(np.float64) / temp
    if 0 < top_p < 1.0:
        p = np.exp(x - x.max()); p /= p.sum()
        order = np.argsort(p, kind="stable")
        cum = np.cumsum(p[order].astype(np.float32))
        return set(order[cum > np.float32(1 - top_p)].tolist())
    if min_p != 0.0:
        order = np.argsort(-x, kind="stable")
        kept = x[order] >= x[order][0] + np.log(min_p)
        kept[:keep] = True
        return set(order[kept].tolist())
    if top_k > 0:
        return set(np.argsort(-x, kind="stable")[:top_k].tolist())
    return set(range(len(x)))


def _ref_kept32(logprobs, temp, top_p=0.0, min_p=0.0, keep=1, top_k=-1):
    """The reference's filters in the reference's own precision, as a bool mask [V] (top-p: the kernel's exact rule, _topp_sets).
    x = fp32(lp) * fp32(1 / temp); min-p keeps x >= fp32(max + fp32(log(min_p))) together with the first `keep` ids of the stable
    descending order; top-k keeps the first k ids of a stable sort on (-x, index) -- ties go to the lowest vocabulary index, the
    product's documented rule where mx.argpartition leaves the choice open."""
    x = np.asarray(logprobs, np.float32) * np.float32(1.0 / temp)
    V = x.shape[0]
    if 0 < top_p < 1.0:
        return _topp_sets(x, top_p)[0]
    kept = np.zeros(V, bool)
    if min_p != 0.0:
        kept = x >= np.float32(x.max() + np.float32(np.log(min_p)))
        kept[np.argsort(-x, kind="stable")[:keep]] = True
        return kept
    if top_k > 0:
        kept[np.argsort(-x, kind="stable")[:top_k]] = True
        return kept
    return np.ones(V, bool)


def _topp_sets(x, top_p):
    """Top-p over x = the already scaled fp32 values -> (exact, ref, margin, v).
    exact: the kernel's rule.  Tie classes merged, masses exp(x - max) in float64: v is the smallest value with
      mass{x < v} <= fp32(1 - top_p) * total < mass{x <= v};  kept = {x >= v}  (empty when no value qualifies).
    margin: the distance of the target from the nearer end of v's interval, as a fraction of the total mass.
    ref: the reference's set -- fp32 softmax, stable ascending sort, sequential fp32 cumsum, keep cum > fp32(1 - top_p) (as _ref_sets)."""
    x = np.asarray(x, np.float32)
    xd = x.astype(np.float64)
    fin = np.isfinite(xd)
    m = xd[fin].max() if fin.any() else 0.0
    w = np.where(fin, np.exp(xd - m), 0.0)
    total = w.sum()
    target = float(np.float32(1.0 - top_p)) * total
    vals, inv = np.unique(x, return_inverse=True)                 # ascending classes (-inf first)
    mass = np.bincount(inv.reshape(-1), weights=w, minlength=len(vals))
    hi = np.cumsum(mass)
    lo = hi - mass
    c = np.nonzero((lo <= target) & (target < hi))[0]
    if len(c):
        v = vals[c[0]]
        exact = x >= v
        margin = min(target - lo[c[0]], hi[c[0]] - target) / total
    else:
        v, exact, margin = np.float32(np.inf), np.zeros(x.shape[0], bool), 0.0
    p = (w / total).astype(np.float32) if total > 0 else np.zeros(x.shape[0], np.float32)
    order = np.argsort(p, kind="stable")
    cum = np.cumsum(p[order], dtype=np.float32)
    ref = np.zeros(x.shape[0], bool)
    ref[order[cum > np.float32(1 - top_p)]] = True
    return exact, ref, margin, v


def _topp_relations(x, top_p, exact, ref):
    """The two top-p sets of _topp_sets differ only by (a) ids of the tie class at v -- the kernel keeps the whole class, the sorted
    cumulative sum splits it -- and (b) ids whose exact ascending cumulative mass lies within the fp32 cumsum's rounding of
    1 - top_p: |fp32 cumsum_i - cum_i| <= (i + 4) * 2^-23 * cum_i for the i-th partial sum (i roundings of the running sum, a few of
    the fp32 softmax).  Returns the ids that break both."""
    x = np.asarray(x, np.float32)
    v = _topp_sets(x, top_p)[3]
    xd = x.astype(np.float64)
    fin = np.isfinite(xd)
    w = np.where(fin, np.exp(xd - (xd[fin].max() if fin.any() else 0.0)), 0.0)
    if w.sum() == 0:                                                  # all -inf: both sets are empty
        return np.nonzero(exact ^ ref)[0].tolist()
    p = w / w.sum()
    order = np.argsort(p.astype(np.float32), kind="stable")
    cum = np.cumsum(p[order])
    pos = np.empty_like(order)
    pos[order] = np.arange(len(order))
    bad = []
    for i in np.nonzero(exact ^ ref)[0]:
        if x[i] == v:
            continue
        j = pos[i]
        if abs(cum[j] - float(np.float32(1 - top_p))) <= (j + 5) * 2.0 ** -23 * cum[j] + 2.0 ** -24:
            continue
        bad.append(int(i))
    return bad


@pytest.mark.parametrize("kw", [dict(top_p=0.6), dict(top_p=0.95), dict(min_p=0.1), dict(min_p=0.3, min_tokens_to_keep=4),
                                dict(top_k=5), dict()])
def test_sampler_reference_keep_sets_and_distribution(kw):
    """tests/sampler_reference.py (the reference's samplers/*.py restated with torch ops, the comparator of the HIP kernels): every draw lies
    in the set the reference's filter keeps (numpy restatement above), every kept token with non-negligible mass is drawn, and the empirical
    frequencies follow the renormalised probabilities (total variation < 0.05 over 4000 draws)."""
    from tests import sampler_reference as sr
    rng = np.random.default_rng(11)
    V, temp = 64, 0.8
    logits = rng.standard_normal(V).astype(np.float32) * 2.0
    logprobs = logits - np.log(np.exp(logits.astype(np.float64)).sum()).astype(np.float32)
    sampler = sr.make_sampler(temp=temp, **kw)
    sr.seed(1234)
    x = torch.from_numpy(logprobs)[None].repeat(4000, 1)                # 4000 independent rows, one call
    draws = sampler(x).numpy()
    assert draws.shape == (4000,) and draws.dtype == np.int32
    allowed = _ref_sets(logprobs, temp, kw.get("top_p", 0.0), kw.get("min_p", 0.0), kw.get("min_tokens_to_keep", 1), kw.get("top_k", -1))
    assert set(draws.tolist()) <= allowed
    p = np.exp(logprobs.astype(np.float64) / temp)
    mask = np.zeros(V, bool); mask[list(allowed)] = True
    p = np.where(mask, p, 0.0); p /= p.sum()
    freq = np.bincount(draws, minlength=V) / 4000.0
    assert 0.5 * np.abs(freq - p).sum() < 0.05
    assert all(freq[i] > 0 for i in allowed if p[i] > 0.01)
    sr.seed(1234)
    assert np.array_equal(sampler(x).numpy(), draws)                   # seed() restarts the stream


def test_stochastic_sampler_argument_errors_and_no_host_path():
    x = torch.zeros((1, 16))
    with pytest.raises(ValueError):
        make_sampler(temp=1.0, top_k=16)(x)                             # top_k must be < vocab (top_k.py:20-24)
    with pytest.raises(ValueError):
        make_sampler(temp=1.0, min_p=1.5)(x)                            # min_p.py:33-36
    with pytest.raises(ValueError):
        make_sampler(temp=1.0, min_p=0.1, min_tokens_to_keep=0)(x)      # min_p.py:37-40
    # the product has no CPU path: a host tensor is refused by every stochastic branch, not sampled by torch
    for kw in (dict(top_p=0.6), dict(min_p=0.1), dict(top_k=5), dict()):
        with pytest.raises(ValueError, match="device tensors"):
            make_sampler(temp=1.0, **kw)(x)


def test_prompt_cache_persistence_round_trip(tmp_path):
    """cache_prompt / load_cached_prompt (prompt_cache.py:78-125) through BaseCache.save_cache / load_cache
    (kv_cache/__init__.py:163-210): file named by sha256 of the id list, arrays "<layer>.<0|1>", metadata
    "0.<i>" / "1.computed_ids" / "2.<i>"; a request with the same ids then re-processes exactly one token."""
    from safetensors import safe_open
    pc = PromptCache(directory=tmp_path, cache=[ReusableKVCache() for _ in range(3)])
    ids = list(range(40, 50))
    for i, c in enumerate(pc.cache):
        c.update_and_fetch(torch.full((1, 2, 10, 8), float(i + 1)), torch.full((1, 2, 10, 8), -float(i + 1)))
    pc.update(ids)
    pc.cache_prompt()
    files = list(tmp_path.glob("*.safetensors"))
    assert len(files) == 1 and files[0].stem == PromptCache._compute_prompt_hash(ids)
    with safe_open(str(files[0]), framework="pt") as f:
        assert sorted(f.keys()) == ["0.0", "0.1", "1.0", "1.1", "2.0", "2.1"]
        assert f.metadata()["1.computed_ids"] == str(ids).replace("'", "") and f.metadata()["2.1"] == "ReusableKVCache"
    fresh = PromptCache(directory=tmp_path)
    fresh.load_cached_prompt(list(range(7)))                            # no such file: nothing happens
    assert fresh.cache == [] and fresh.computed_ids == []
    fresh.load_cached_prompt(ids)
    assert fresh.computed_ids == ids and len(fresh.cache) == 3
    assert fresh.cache[2].offset == 256                                 # the reference quirk: offset = saved capacity ...
    assert torch.equal(fresh.cache[1].keys.cpu(), pc.cache[1].keys.cpu()) and float(fresh.cache[2].values[0, 0, 9, 0]) == -3.0
    todo = fresh(ids)                                                   # ... until the prefix match trims it
    assert list(todo) == ids[-1:] and fresh.cache[0].offset == 9


def test_reference_import_paths_resolve_to_the_same_modules():
    """Code written against the reference imports `proxy_inference_engine.<module>` (src/proxy_inference_engine/...): every
    such path must give the very module object of the implementation (shared sampler RNG state, one loaded library)."""
    import importlib
    for m in ("engine.inference_engine", "samplers", "samplers.top_p", "samplers.min_p", "samplers.top_k", "samplers.categorical",
              "cache", "cache.prompt_cache", "cache.kv_cache", "cache.kv_cache.reusable", "logits_processors",
              "logits_processors.repetition", "models", "models.base", "models.utils", "models.llama", "models.llama.language",
              "models.llama.utils", "pie_core"):
        assert importlib.import_module(f"proxy_inference_engine.{m}") is importlib.import_module(f"proxy_inference_engine_amd.{m}"), m
    from proxy_inference_engine import InferenceEngine, pie_core
    from proxy_inference_engine.engine.inference_engine import InferenceEngine as IE2
    assert InferenceEngine is IE2 and pie_core.hello() == "pie_core \u2713"
    with pytest.raises(ImportError):
        importlib.import_module("proxy_inference_engine.server")       # the HTTP server is out of scope: absent, not stubbed


def test_oracle_forward_from_input_embeddings_equals_forward_from_ids():
    """`h = inputs_embeds` (models/intern/language.py:155-158): feeding the oracle the embedding rows of the ids must give
    exactly the logits of feeding the ids."""
    cfg = {"model_type": "llama", "hidden_size": 128, "num_hidden_layers": 2, "intermediate_size": 256, "num_attention_heads": 4,
           "num_key_value_heads": 2, "rms_norm_eps": 1e-5, "vocab_size": 320, "rope_theta": 10000.0, "tie_word_embeddings": True,
           "quantization": {"group_size": 64, "bits": 4}}
    w = po.synth_checkpoint(cfg, seed=2, dtype="bfloat16")
    orc = po.OracleLlama(cfg, w, "bfloat16")
    ids = np.random.default_rng(0).integers(0, 320, 9)
    a = orc.forward(ids, [po.OracleKVCache() for _ in orc.layers])
    rows = po.dequantize(w["model.embed_tokens.weight"], w["model.embed_tokens.scales"], w["model.embed_tokens.biases"], dtype="bfloat16")[ids]
    b = orc.forward(None, [po.OracleKVCache() for _ in orc.layers], inputs_embeds=rows)
    assert np.array_equal(a, b)


def test_generate_step_mask_arrays_that_the_reference_loop_can_carry():
    """generate_step forwards ONE mask array to the prompt pass and to every single-token step (inference_engine.py:246-249): only arrays that are
    constant per head broadcast against every [1, H, L, S]; those cannot hide a key, so they are accepted (and change nothing); the rest is
    refused with the reason."""
    from proxy_inference_engine_amd.engine.inference_engine import check_generate_mask
    for ok in (torch.zeros(()), torch.zeros(1, 1), torch.full((1, 1, 1, 1), -3.5), torch.ones(1, 4, 1, 1, dtype=torch.bool), torch.zeros(4, 1, 1), np.zeros((1, 1), np.float32)):
        check_generate_mask(ok, 4)
    for bad, why in ((torch.zeros(12, 12), "broadcast"), (torch.zeros(1, 1, 1, 9), "broadcast"), (torch.zeros(2, 1, 1, 1), "broadcast"),
                     (torch.zeros(1, 3, 1, 1), "broadcast"), (torch.zeros(1, 1, dtype=torch.bool), "hides every key"),
                     (torch.full((1, 1), float("-inf")), "hides every key")):
        with pytest.raises(ValueError, match=why):
            check_generate_mask(bad, 4)


# ------------------------------------------------------------------ the fp32 restatement of the sampler filters on designed rows
def _modes(row):
    """(mode name, keyword arguments of _ref_kept32 / make_sampler) for every branch of make_sampler on a designed row."""
    return [("top_k", dict(top_k=row.top_k)), ("top_p", dict(top_p=row.top_p)), ("min_p", dict(min_p=row.min_p)),
            ("min_p_keep", dict(min_p=row.min_p, keep=row.keep)), ("categorical", dict())]


def _unique_answer(x, mode, kw):
    """True when the reference's own definition leaves no choice to its sort order (no tie across the boundary, a top-p crossing
    far from every step of the cumulative sum)."""
    xs = np.sort(x)[::-1]
    if mode == "top_k":
        k = kw["top_k"]
        return xs[k - 1] > xs[k] or xs[k] == -np.inf
    if mode.startswith("min_p"):
        keep = kw.get("keep", 1)
        thr = np.float32(xs[0] + np.float32(np.log(kw["min_p"])))
        return keep >= len(xs) or xs[keep - 1] > xs[keep] or xs[keep] >= thr or xs[keep] == -np.inf
    if mode == "top_p":
        exact, ref, margin, _ = _topp_sets(x, kw["top_p"])
        if not np.array_equal(exact, ref) or margin < 1e-4:
            return False
        p = np.exp(x.astype(np.float64) - x.max())
        cum = np.cumsum(np.sort(p / p.sum()))
        return np.min(np.abs(cum - (1 - kw["top_p"]))) > 1e-4 and len(np.unique(x[exact])) == int(exact.sum())
    return True


def test_fp32_restatement_agrees_with_the_torch_reference_on_designed_rows():
    """_ref_kept32 (the filters in fp32, ties by index) against tests/sampler_reference.py's op-for-op torch restatement, on every designed
    row and branch where the reference's answer is unique; compared on the finite ids (the torch filters mark the drawable ids)."""
    from tests import sampler_reference as sr
    from tests.sampler_rows import families
    compared = 0
    for V in (64, 513, 4099, 32000):
        for row in families(V, seed=V):
            if not np.isfinite(row.lp).any():
                continue
            x = row.lp * np.float32(1.0 / row.temp)
            for mode, kw in _modes(row):
                if not _unique_answer(x, mode, kw):
                    continue
                mine = _ref_kept32(row.lp, row.temp, **kw) & np.isfinite(x)
                tkw = dict(kw)
                if "keep" in tkw:
                    tkw["min_tokens_to_keep"] = tkw.pop("keep")
                theirs = sr.kept_mask(torch.from_numpy(row.lp)[None], row.temp, **tkw)[0].numpy()
                assert np.array_equal(mine, theirs), (V, row.name, mode, np.nonzero(mine ^ theirs)[0][:8])
                compared += 1
    assert compared >= 120, compared


def test_top_p_exact_rule_and_reference_set_differ_only_at_the_threshold():
    """The kernel's top-p rule keeps the whole tie class at the threshold value v; the reference's sorted fp32 cumsum keeps part of it
    (a deliberate difference, csrc/sampler.hip's header) and rounds as it goes.  On every designed row the two sets differ only by
    that tie class and by ids within the cumsum's rounding of 1 - top_p; on the designed top-p tie they differ by exactly half the class."""
    from tests.sampler_rows import families, topp_tie
    for V in (64, 513, 4099, 32000, 128256):
        for row in families(V, seed=V + 1):
            for top_p in (row.top_p, 0.3, 0.95):
                x = row.lp * np.float32(1.0 / row.temp)
                exact, ref, _, _ = _topp_sets(x, top_p)
                assert _topp_relations(x, top_p, exact, ref) == [], (V, row.name, top_p)
    for V in (64, 4099, 152064):
        row = topp_tie(V, seed=3)
        exact, ref, margin, v = _topp_sets(row.lp, row.top_p)
        tie = row.notes["tie"]
        assert margin > 0.1 and v == row.lp[tie[0]]
        assert set(np.nonzero(exact)[0]) == set(tie) | set(row.notes["big"])
        assert set(np.nonzero(exact & ~ref)[0]) == set(tie[:3]) and not (ref & ~exact).any()   # stable ascending: the last 3 stay


def test_fp32_scaling_merges_what_float64_keeps_apart():
    """At temp 3.0 fp32(x * fp32(1/3)) maps two adjacent log-probs to one value: in the reference's precision they tie at the top-k
    boundary (the lower index is kept), while the float64 comparator _ref_sets still orders them (it keeps the larger, higher index)."""
    from tests.sampler_rows import merged_by_temp
    for V in (64, 4099, 128256):
        row = merged_by_temp(V, seed=V)
        lo, hi = row.notes["lo"], row.notes["hi"]
        assert row.lp[hi] > row.lp[lo] and np.float32(row.lp[hi] * np.float32(1 / 3.0)) == np.float32(row.lp[lo] * np.float32(1 / 3.0))
        k32 = _ref_kept32(row.lp, row.temp, top_k=row.top_k)
        k64 = _ref_sets(row.lp, row.temp, top_k=row.top_k)
        assert k32[lo] and not k32[hi] and hi in k64 and lo not in k64 and int(k32.sum()) == row.top_k


def test_designed_rows_are_what_they_claim():
    """The generator's rows (tests/sampler_rows.py) have the structure the kernel tests rely on."""
    from tests import sampler_rows as R
    for V in (4099, 128256, R.V_MAX):
        w = R.wide_tie(V, seed=1)
        tie, x = w.notes["tie"], w.lp
        assert len(tie) >= 36 and len(np.unique(tie // R.SLICE)) >= 8 and (x[tie] == x[tie[0]]).all()
        assert int((x > x[tie[0]]).sum()) == 20 and 20 < w.top_k < 20 + len(tie)
        assert any(t % 2 == 0 and t + 1 in set(tie.tolist()) for t in tie)          # ids one kernel thread owns together
        last = R.wide_tie(V, seed=1, last_slice=True)
        assert (last.notes["tie"] // R.SLICE == (V - 1) // R.SLICE).all() or V - (V - 1) // R.SLICE * R.SLICE < 40
        for n in (1, 3, 600):
            sp = R.sparse(V, n, seed=2)
            fin = np.isfinite(sp.lp)
            assert int(fin.sum()) == n and sp.top_k > n and not fin[R.SLICE:2 * R.SLICE].any()
        q = R.quantized(V, seed=3)
        assert len(np.unique(q.lp)) < 4096                                          # bf16: a few thousand values at most
        assert np.sort(q.lp)[::-1][q.top_k - 1] == np.sort(q.lp)[::-1][q.top_k]     # k inside a tie class
    assert R.VOCABS[-1] == R.V_MAX == 524288
