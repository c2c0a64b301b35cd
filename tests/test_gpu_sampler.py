"""-m gpu: the fused HIP sampler (csrc/sampler.hip, pie_sample) against the reference's sort-based definitions.

samplers/{top_p,min_p,top_k,categorical}.py of the reference filter with argsort / cumsum / argpartition and draw with
mx.random.categorical; the product restates them as one sort-free kernel.  Pinned here: the KEPT SET of every branch equals the numpy
restatement of the reference's definition (tests/test_host_logic.py: _ref_sets) id for id; every draw lies in it; the empirical
distribution follows the renormalised probabilities; seeding restarts the stream and the device-side call counter advances it."""
import numpy as np
import pytest
import torch

from tests import sampler_rows as R
from tests.test_host_logic import _ref_kept32, _ref_sets, _topp_relations, _topp_sets

pytestmark = pytest.mark.gpu

CASES = [dict(top_p=0.6), dict(top_p=0.95), dict(top_p=0.05), dict(min_p=0.1), dict(min_p=0.3, min_tokens_to_keep=4), dict(min_p=0.9, min_tokens_to_keep=7),
         dict(top_k=1), dict(top_k=5), dict(top_k=50), dict()]


def _logprobs(rng, V, scale=2.0):
    logits = (rng.standard_normal(V) * scale).astype(np.float32)
    return logits - np.float32(np.log(np.exp(logits.astype(np.float64)).sum()))


def _mode(kw):
    if "top_p" in kw:
        return "top_p", kw["top_p"], 0
    if "min_p" in kw:
        return "min_p", kw["min_p"], kw.get("min_tokens_to_keep", 1)
    if "top_k" in kw:
        return "top_k", 0.0, kw["top_k"]
    return "categorical", 0.0, 0


@pytest.mark.parametrize("kw", CASES)
@pytest.mark.parametrize("V,temp", [(64, 0.8), (1000, 1.0), (4099, 0.7), (128256, 1.0)])
def test_kept_set_equals_the_references_definition(kw, V, temp):
    from proxy_inference_engine_amd import hip_ops
    rng = np.random.default_rng(V + int(temp * 10) + len(kw))
    lp = _logprobs(rng, V, 3.0 if V > 10000 else 2.0)
    mode, p, k = _mode(kw)
    tokens, kept, mask = hip_ops.sample(torch.from_numpy(lp).cuda(), mode, temp, p=p, k=k, want_mask=True)
    want = _ref_sets(lp, temp, kw.get("top_p", 0.0), kw.get("min_p", 0.0), kw.get("min_tokens_to_keep", 1), kw.get("top_k", -1))
    got = set(np.nonzero(mask[0].cpu().numpy())[0].tolist())
    if mode == "top_p" and got != want:
        # the reference's cumulative sum is a sequential fp32 sum over the sorted row; the kernel's is exact: the sets may differ by the ids
        # whose cumulative mass is within that rounding of 1 - top_p -- at most a handful of boundary ids, contiguous in the sorted order
        x = lp.astype(np.float64) / temp
        pr = np.exp(x - x.max())
        pr /= pr.sum()
        order = np.argsort(pr, kind="stable")
        cum = np.cumsum(pr[order])
        diff = got ^ want
        pos = {int(i): j for j, i in enumerate(order)}
        assert len(diff) <= 3 and all(abs(cum[pos[i]] - (1 - kw["top_p"])) < 2e-5 for i in diff), (len(diff), sorted(diff)[:5])
    else:
        assert got == want, (len(got), len(want), sorted(got ^ want)[:8])
    assert int(kept.item()) == len(got) and int(tokens.item()) in got


@pytest.mark.parametrize("kw", [dict(top_p=0.6), dict(min_p=0.1), dict(top_k=5), dict()])
def test_distribution_seed_and_counter(kw):
    from proxy_inference_engine_amd import samplers
    from proxy_inference_engine_amd.samplers import make_sampler
    rng = np.random.default_rng(11)
    V, temp, rows = 64, 0.8, 4000
    lp = _logprobs(rng, V)
    sampler = make_sampler(temp=temp, **kw)
    x = torch.from_numpy(lp)[None].repeat(rows, 1).cuda()
    samplers.seed(1234)
    draws = sampler(x)
    assert draws.is_cuda and draws.dtype == torch.int32 and draws.shape == (rows,)
    draws = draws.cpu().numpy()
    allowed = _ref_sets(lp, temp, kw.get("top_p", 0.0), kw.get("min_p", 0.0), kw.get("min_tokens_to_keep", 1), kw.get("top_k", -1))
    assert set(draws.tolist()) <= allowed
    p = np.exp(lp.astype(np.float64) / temp)
    mask = np.zeros(V, bool)
    mask[list(allowed)] = True
    p = np.where(mask, p, 0.0)
    p /= p.sum()
    freq = np.bincount(draws, minlength=V) / rows
    assert 0.5 * np.abs(freq - p).sum() < 0.05
    assert all(freq[i] > 0 for i in allowed if p[i] > 0.01)
    again = sampler(x).cpu().numpy()                  # the device-side call counter moved on: a different draw
    assert not np.array_equal(again, draws)
    samplers.seed(1234)                               # seed() restarts the stream
    assert np.array_equal(sampler(x).cpu().numpy(), draws)
    assert np.array_equal(sampler(x).cpu().numpy(), again)


def test_argument_errors_follow_the_reference():
    from proxy_inference_engine_amd.samplers import make_sampler
    x = torch.zeros((1, 16), device="cuda")
    with pytest.raises(ValueError):
        make_sampler(temp=1.0, top_k=16)(x)           # top_k must be < vocab (top_k.py:20-24)
    with pytest.raises(ValueError):
        make_sampler(temp=1.0, min_p=1.5)(x)          # min_p.py:33-36
    with pytest.raises(ValueError):
        make_sampler(temp=1.0, min_p=0.1, min_tokens_to_keep=0)(x)


# ------------------------------------------------------------------ designed rows: ties, masks, slices, temperatures (tests/sampler_rows.py)
_BIG = (151936, 152064, R.V_MAX)
_DESIGNED = [(V, n) for i, V in enumerate(R.VOCABS) for n in R.names(V)
             if V not in _BIG or n in ("quantized", "wide_tie", "wide_tie_last_slice", "sparse600", "all_inf")]


def _kernel_modes(row):
    """(hip_ops.sample mode, p, k, _ref_kept32 keywords) for every branch make_sampler can pick."""
    out = [("top_p", row.top_p, 0, dict(top_p=row.top_p)), ("min_p", row.min_p, 1, dict(min_p=row.min_p)),
           ("min_p", row.min_p, row.keep, dict(min_p=row.min_p, keep=row.keep)), ("categorical", 0.0, 0, dict())]
    if row.V > 1:
        out.insert(0, ("top_k", 0.0, row.top_k, dict(top_k=row.top_k)))
    return out


def _check_kept(row, mode, p, k, kw, mask, kept, token):
    """The kernel's kept mask against the fp32 restatement, id for id; the count and the draw against the mask."""
    x = row.lp * np.float32(1.0 / row.temp)
    what = (row.V, row.name, mode, p, k)
    if not np.isfinite(x).any():                                      # all -inf: only a valid id is asked for
        assert 0 <= token < row.V, what
        return
    if mode == "top_p":
        exact, ref, margin, v = _topp_sets(x, p)
        if not np.array_equal(mask, exact):
            # the kernel's fixed-point masses (2^-40 of the largest, truncated) may move the crossing only when the target lies within
            # V * 2^-40 + a few fp32 ulps of exp of a class end: then the neighbouring class is as right
            vals = np.unique(x)
            j = int(np.searchsorted(vals, v))
            alts = [x >= vals[i] for i in (j - 1, j + 1) if 0 <= i < len(vals)]
            assert margin < 1e-6 and any(np.array_equal(mask, a) for a in alts), (what, margin, np.nonzero(mask ^ exact)[0][:8])
        assert _topp_relations(x, p, mask, ref) == [], what
    else:
        want = _ref_kept32(row.lp, row.temp, **kw)
        assert np.array_equal(mask, want), (what, int(mask.sum()), int(want.sum()), np.nonzero(mask ^ want)[0][:8])
    assert kept == int(mask.sum()), what
    assert mask[token] and np.isfinite(x[token]), (what, token)


@pytest.mark.parametrize("V,name", _DESIGNED, ids=[f"{V}-{n}" for V, n in _DESIGNED])
def test_kept_sets_on_designed_rows(V, name):
    """Every branch on every designed row: the kept mask equals the fp32 restatement (top-p: the kernel's exact rule, and the set
    relations to the reference's cumsum set hold), kept_count is its size, the draw lies in it and never on a -inf id."""
    from proxy_inference_engine_amd import hip_ops
    row = R.make(name, V, seed=R.VOCABS.index(V))
    x = torch.from_numpy(row.lp).cuda()
    for mode, p, k, kw in _kernel_modes(row):
        tokens, kept, mask = hip_ops.sample(x, mode, row.temp, p=p, k=k, want_mask=True)
        _check_kept(row, mode, p, k, kw, mask[0].cpu().numpy().astype(bool), int(kept.item()), int(tokens.item()))


@pytest.mark.parametrize("V", [2, 513, 128256])
@pytest.mark.parametrize("temp", R.TEMPS)
def test_kept_sets_at_every_temperature(V, temp):
    """The tie-heavy rows at the four temperatures: fp32(lp * fp32(1 / temp)) is what the filters compare."""
    from proxy_inference_engine_amd import hip_ops
    rows = [R.quantized(V, seed=5, temp=temp)] + ([R.wide_tie(V, seed=5, temp=temp), R.topp_tie(V, seed=5, temp=temp)] if V >= 64 else [])
    for row in rows:
        x = torch.from_numpy(row.lp).cuda()
        for mode, p, k, kw in _kernel_modes(row):
            tokens, kept, mask = hip_ops.sample(x, mode, row.temp, p=p, k=k, want_mask=True)
            _check_kept(row, mode, p, k, kw, mask[0].cpu().numpy().astype(bool), int(kept.item()), int(tokens.item()))


def test_temperature_merge_is_a_tie_in_fp32():
    """merged_by_temp: two adjacent log-probs become one value at temp 3.0; top-k keeps the LOWER index of the pair (the float64
    comparator would keep the other one)."""
    from proxy_inference_engine_amd import hip_ops
    for V in (513, 128256):
        row = R.merged_by_temp(V, seed=9)
        _, _, mask = hip_ops.sample(torch.from_numpy(row.lp).cuda(), "top_k", row.temp, k=row.top_k, want_mask=True)
        m = mask[0].cpu().numpy().astype(bool)
        assert m[row.notes["lo"]] and not m[row.notes["hi"]] and int(m.sum()) == row.top_k


def test_all_inf_rows_return_a_valid_id_and_oversize_vocabularies_are_refused():
    from proxy_inference_engine_amd import hip_ops, samplers
    from proxy_inference_engine_amd.samplers import _rng
    for V in (2, 513, 128256):
        x = torch.full((2, V), float("-inf"), device="cuda")
        for mode, p, k in (("top_k", 0.0, 1), ("top_p", 0.9, 0), ("min_p", 0.1, 1), ("min_p", 0.1, 2), ("categorical", 0.0, 0)):
            t = hip_ops.sample(x, mode, 1.0, p=p, k=k).cpu().numpy()
            assert ((0 <= t) & (t < V)).all(), (V, mode, t)
    samplers.seed(5)
    _, counter = _rng.hip_state(torch.device("cuda", torch.cuda.current_device()))
    before = counter.cpu().tolist()
    with pytest.raises(ValueError):
        hip_ops.sample(torch.zeros((1, R.V_MAX + 1), device="cuda"), "categorical", 1.0)
    assert counter.cpu().tolist() == before                          # nothing was launched
    t = hip_ops.sample(torch.zeros((1, R.V_MAX), device="cuda"), "categorical", 1.0)
    assert 0 <= int(t.item()) < R.V_MAX and counter.cpu().tolist()[0] == before[0] + 1


# ------------------------------------------------------------------ batches of different rows
_BATCH_FAMILIES = ["quantized", "wide_tie", "sparse3", "one_hot", "uniform", "topp_tie", "sparse600", "wide_tie_last_slice", "all_inf",
                   "merged_by_temp", "sparse1"]


@pytest.mark.parametrize("B", [3, 32])
def test_batch_rows_equal_each_row_alone(B):
    """[B, 128256] rows of different families in one call: each row's kept mask and count equal the same row sampled alone, bit for bit
    (the per-row workspace, the row's own maximum and its own tie tables)."""
    from proxy_inference_engine_amd import hip_ops
    V = 128256
    rows = [R.make(_BATCH_FAMILIES[i % len(_BATCH_FAMILIES)], V, seed=i).lp for i in range(B)]
    x = torch.from_numpy(np.stack(rows)).cuda()
    for mode, p, k in (("top_k", 0.0, 37), ("top_p", 0.775, 0), ("min_p", 0.1, 25), ("min_p", 0.2, 1), ("categorical", 0.0, 0)):
        _, kept, mask = hip_ops.sample(x, mode, 0.7, p=p, k=k, want_mask=True)
        kept, mask = kept.cpu().numpy(), mask.cpu().numpy()
        for i in range(B):
            _, k1, m1 = hip_ops.sample(x[i], mode, 0.7, p=p, k=k, want_mask=True)
            assert np.array_equal(mask[i], m1[0].cpu().numpy()) and kept[i] == int(k1.item()), (mode, i)


def test_identical_rows_in_one_call_draw_independently():
    """16 pairs of identical rows per call, 25 calls: the fraction of pairs that draw the same id is sum p^2 of the kept set's
    renormalised probabilities (binomial, 6 sigma), not 1 (rows in lockstep)."""
    from proxy_inference_engine_amd import hip_ops, samplers
    V = 128256
    lp = np.full(V, -30.0, np.float32)
    ids = np.arange(8) * 15013 + 7
    lp[ids] = np.log(np.array([8, 6, 5, 4, 3, 2, 1, 1], np.float64) / 30).astype(np.float32)
    x = torch.from_numpy(lp)[None].repeat(32, 1).cuda()
    samplers.seed(77)
    same = n = 0
    for _ in range(25):
        t = hip_ops.sample(x, "top_k", 1.0, k=6).cpu().numpy()
        same += int((t[0::2] == t[1::2]).sum())
        n += 16
    pk = np.exp(np.sort(lp[ids].astype(np.float64))[::-1][:6])
    pk /= pk.sum()
    s2 = float((pk ** 2).sum())
    assert abs(same / n - s2) < 6 * np.sqrt(s2 * (1 - s2) / n), (same / n, s2)


# ------------------------------------------------------------------ distributions across workgroups (chi-square, seeded)
def _chi2_pvalue(counts, probs):
    counts = np.asarray(counts, np.float64)
    expect = np.asarray(probs, np.float64) / np.sum(probs) * counts.sum()
    stat = float(((counts - expect) ** 2 / expect).sum())
    df = len(counts) - 1
    return float(torch.special.gammaincc(torch.tensor(df / 2.0, dtype=torch.float64), torch.tensor(stat / 2.0, dtype=torch.float64))), stat


def _draws(x, mode, temp, calls, p=0.0, k=0):
    from proxy_inference_engine_amd import hip_ops
    return np.concatenate([hip_ops.sample(x, mode, temp, p=p, k=k).cpu().numpy() for _ in range(calls)])


def test_top_k_distribution_over_250_workgroups():
    """top_k = 250 at V = 128256: the kept ids lie one per 512-id slice (250 workgroups meet in the 64-bit atomic max) with graded
    probabilities (ratio 20); 65536 draws follow them (chi-square, p > 1e-6)."""
    from proxy_inference_engine_amd import samplers
    V, k = 128256, 250
    rng = np.random.default_rng(250)
    ids = np.arange(k) * R.SLICE + rng.integers(0, R.SLICE, k)
    lp = np.full(V, -40.0, np.float32)
    lp[ids] = np.linspace(0.0, -3.0, k).astype(np.float32)[rng.permutation(k)]
    samplers.seed(250)
    d = _draws(torch.from_numpy(lp)[None].repeat(512, 1).cuda(), "top_k", 1.0, 128, k=k)
    assert np.isin(d, ids).all()
    pos = {int(i): j for j, i in enumerate(ids)}
    counts = np.bincount([pos[int(t)] for t in d], minlength=k)
    pv, stat = _chi2_pvalue(counts, np.exp(lp[ids].astype(np.float64)))
    assert pv > 1e-6, (pv, stat)


def test_categorical_distribution_with_mass_in_distant_slices():
    """categorical at V = 4099 (9 slices, the last one 3 ids wide): the mass on five ids in slices 0, 2, 4, 6, 8, the rest -inf."""
    from proxy_inference_engine_amd import samplers
    V = 4099
    ids = np.array([3, 1100, 2050, 3583, 4098])
    lp = np.full(V, -np.inf, np.float32)
    lp[ids] = np.log(np.array([0.3, 0.05, 0.25, 0.1, 0.3])).astype(np.float32)
    samplers.seed(4099)
    d = _draws(torch.from_numpy(lp)[None].repeat(16384, 1).cuda(), "categorical", 0.7, 4)
    assert np.isin(d, ids).all()
    counts = np.array([(d == i).sum() for i in ids])
    pv, stat = _chi2_pvalue(counts, np.exp(lp[ids].astype(np.float64) / 0.7))
    assert pv > 1e-6, (pv, stat, counts)


def test_draws_inside_a_top_k_tie_class_are_uniform():
    """A class of 40 equal maxima spread over the row, with (even, odd) neighbours that one thread owns together; top_k keeps the
    lowest-index part of it, and every kept tie is drawn equally often (chi-square against uniform, p > 1e-6)."""
    from proxy_inference_engine_amd import hip_ops, samplers
    V = 128256
    rng = np.random.default_rng(40)
    pairs = np.array([1000, 1001, 20002, 20003, 30004, 30005])
    tie = np.unique(np.concatenate([pairs, rng.choice(np.setdiff1d(np.arange(V), pairs), 34, replace=False)]))
    k = int(np.searchsorted(tie, pairs.max())) + 1 + 2
    lp = np.full(V, -12.0, np.float32)
    lp[tie] = 0.0
    x = torch.from_numpy(lp)[None].repeat(512, 1).cuda()
    _, _, mask = hip_ops.sample(x[:1], "top_k", 1.0, k=k, want_mask=True)
    assert np.array_equal(np.nonzero(mask[0].cpu().numpy())[0], tie[:k])
    samplers.seed(40)
    d = _draws(x, "top_k", 1.0, 128, k=k)
    assert np.isin(d, tie[:k]).all()
    counts = np.array([(d == i).sum() for i in tie[:k]])
    pv, stat = _chi2_pvalue(counts, np.ones(k))
    assert pv > 1e-6, (pv, stat, counts)


# ------------------------------------------------------------------ state between calls: the workspace, the counter, a captured graph
def _fresh(fn):
    """fn() on workspaces the cache has never seen (the reused ones are put back afterwards)."""
    from proxy_inference_engine_amd import hip_ops
    saved = dict(hip_ops._sample_ws)
    hip_ops._sample_ws.clear()
    try:
        return fn()
    finally:
        hip_ops._sample_ws.clear()
        hip_ops._sample_ws.update(saved)


def test_reused_workspace_equals_a_fresh_one():
    """One (rows, V) workspace through: a row whose max is ~0, min-p on a row whose max is ~-20 (the previous call's maximum must have
    been cleared), top-p, categorical -- each call equals the same call (same seed, same counter) on a fresh workspace.  Then more than
    8 other (rows, V) keys clear the cache, and the sequence is checked again."""
    from proxy_inference_engine_amd import hip_ops, samplers
    V = 50257
    a = R.quantized(V, seed=1).lp
    b = (R.wide_tie(V, seed=2).lp - np.float32(20.0) - R.wide_tie(V, seed=2).lp.max()).astype(np.float32)
    c = R.topp_tie(V, seed=3).lp
    seq = [(a, "top_k", 0.0, 50), (b, "min_p", 0.3, 1), (b, "min_p", 0.3, 25), (c, "top_p", 0.775, 0), (a, "categorical", 0.0, 0)]

    def run(x, mode, p, k):
        return [t.cpu().numpy() for t in hip_ops.sample(torch.from_numpy(np.stack([x, x])).cuda(), mode, 1.0, p=p, k=k, want_mask=True)]

    for _ in range(2):
        for x, mode, p, k in seq:
            samplers.seed(31)
            got = run(x, mode, p, k)
            samplers.seed(31)
            want = _fresh(lambda: run(x, mode, p, k))
            for g, w in zip(got, want):
                assert np.array_equal(g, w), mode
            if mode == "min_p" and k == 1:
                assert np.array_equal(got[2][0].astype(bool), _ref_kept32(x, 1.0, min_p=p))
        for n in range(10):                                           # > 8 distinct keys: _sample_ws is cleared on the way
            hip_ops.sample(torch.zeros((1 + n % 2, 600 + n), device="cuda"), "categorical", 1.0)


def test_captured_graph_replays_draw_fresh_numbers_and_follow_seed():
    """make_sampler(top_p) captured in a torch.cuda.graph on one stream (eager warm-up first): every replay's draws lie in the exact kept
    set and differ from the previous replay's (the device-side call counter advances inside the graph); after samplers.seed(s) five
    replays reproduce five eager calls made after the same seed(s)."""
    from proxy_inference_engine_amd import samplers
    from proxy_inference_engine_amd.samplers import make_sampler
    V = 32000
    row = R.topp_tie(V, seed=6)
    x = torch.from_numpy(row.lp)[None].repeat(64, 1).cuda()
    sampler = make_sampler(temp=1.0, top_p=row.top_p)
    allowed = _topp_sets(row.lp, row.top_p)[0]
    samplers.seed(99)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            sampler(x)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = sampler(x)
    prev = None
    for _ in range(4):
        g.replay()
        t = out.cpu().numpy()
        assert allowed[t].all()
        assert prev is None or not np.array_equal(t, prev)
        prev = t
    samplers.seed(99)
    eager = [sampler(x).cpu().numpy() for _ in range(5)]
    samplers.seed(99)
    replays = []
    for _ in range(5):
        g.replay()
        replays.append(out.cpu().numpy())
    for e, r in zip(eager, replays):
        assert np.array_equal(e, r)
    assert not np.array_equal(eager[0], eager[1])


# ------------------------------------------------------------------ engine level
def test_batched_engine_sampler_rows_draw_from_their_own_top_k(golden_dir):
    """BatchedEngine(sampler=make_sampler(temp=0.8, top_k=5)) behind a recording wrapper: every row of every [B, V] block the sampler
    was given draws one of THAT row's top 5 (ties by index), never another row's."""
    import json
    from proxy_inference_engine_amd.engine import BatchedEngine
    from proxy_inference_engine_amd.samplers import make_sampler
    from tests.test_gpu_decode import build
    g = np.load(golden_dir / "tiny_llama_w4_bf16.npz")
    cfg = json.loads(str(g["config_json"]))
    model = build(cfg, {k[2:]: g[k] for k in g.files if k.startswith("w:")})
    base, calls = make_sampler(temp=0.8, top_k=5), []

    def recording(lp):
        t = base(lp)
        calls.append((lp.detach().float().reshape(-1, lp.shape[-1]).cpu().numpy(), t.detach().reshape(-1).cpu().numpy()))
        return t

    rng = np.random.default_rng(8)
    prompts = [rng.integers(0, cfg["vocab_size"], int(n)).tolist() for n in rng.integers(3, 40, 6)]
    out = BatchedEngine(model, num_pages=16, max_batch=4, sampler=recording).generate(prompts, 5)
    assert [len(t) for t in out] == [5] * 6
    assert sum(len(t) for _, t in calls) >= 30 and any(len(t) > 1 for _, t in calls)
    for lp, t in calls:
        assert lp.shape[0] == len(t)
        for i, tok in enumerate(t.tolist()):
            assert _ref_kept32(lp[i], 0.8, top_k=5)[tok], (i, tok)
