"""-m gpu: batched speculation under per-request samplers, repetition penalties and logit biases -- the segmented sampled
verify against the rows alone, bit for bit, from existing one-row ops only (hip_ops.logits_penalty over the reference window,
logits_bias, logprobs_argmax, hip_ops.sample at stream position calls + j); its independence of row order and neighbours;
Model.spec_step_batch_tail on the tiny golden models against the raw rows the greedy entry leaves on twin caches; the engine with
deterministic and with random draws; the untouched paths; the refusals at all three layers.

A random draw is restated with hip_ops.sample(rng=(seed, counter)): a private counter tensor, so the samplers' own stream is not touched."""
from unittest import mock

import numpy as np
import pytest
import torch

from tests import spec_batch_reference as sb
from tests import spec_batch_tail_reference as tr
from tests.test_gpu_spec_batch import SP_KW, e2e_case, private_pool
from tests.test_gpu_speculative import MODELS, SENT, bits_of, dev_ids, load_tiny

pytestmark = pytest.mark.gpu
CALLS_WORD = 3       # pie_row_tail as int64 words: mode | inv_temp, thr | k, seed | calls | penalty | context_size


def seat(spec=None, seed=0, calls=0, penalty=1.0, context=60, bias=None, xtc=None) -> dict:
    return dict(spec=spec, seed=seed, calls=calls, penalty=penalty, context=context, bias=bias, xtc=xtc)


def record_of(st):
    from proxy_inference_engine_amd import hip_ops
    mode, temp, p, k = st["spec"] or (None, 1.0, 0.0, 0)
    return hip_ops.row_tail_pack(mode, temp, p, k, seed=st["seed"], calls=st["calls"], penalty=st["penalty"], context_size=st["context"])


def expected_row(raw: torch.Tensor, window: list, st: dict, j: int):
    """(token, logprobs fp32 [V], processed logits [V]) of one row alone, from existing ops only."""
    from proxy_inference_engine_amd import hip_ops
    x = raw.clone().contiguous()
    if st["penalty"] != 1.0:
        hip_ops.logits_penalty(x, dev_ids(window), st["penalty"])
    if st["bias"] is not None:
        hip_ops.logits_bias(x, dev_ids(st["bias"][0]), torch.tensor(st["bias"][1], dtype=torch.float32, device="cuda"))
    tok, lp = hip_ops.logprobs_argmax(x)
    t = int(tok.item())
    if st["spec"] is not None:
        counter = torch.tensor([st["calls"] + j, 0], dtype=torch.int64, device="cuda")
        t = int(hip_ops.sample(lp, *st["spec"], xtc=None if st["xtc"] is None else hip_ops.xtc_pack(*st["xtc"]), rng=(st["seed"], counter)).item())
    return t, lp, x


def expected_segment(raw_rows, ring, pos0: int, st: dict, token: int, V: int, make_draft):
    """Row by row: (fed ids, drafts, tokens, logprobs, processed logits, rows specified).  make_draft(j, t_j) = draft j given the
    reference token of row j; fed[j + 1] = that draft, 0 in its place when it lies outside the vocabulary (the rows behind it are then
    outside the contract)."""
    fed, drafts, toks, lps, xs, specified = [int(token)], [], [], [], [], 0
    ok = True
    for j in range(raw_rows.shape[0]):
        t, lp, x = expected_row(raw_rows[j], tr.window(ring, fed, pos0, j, st["context"]), st, j)
        toks.append(t), lps.append(lp), xs.append(x)
        specified += ok
        if j + 1 < raw_rows.shape[0]:
            d = int(make_draft(j, t))
            drafts.append(d)
            ok = ok and 0 <= d < V
            fed.append(d if 0 <= d < V else 0)
    return dict(fed=fed, drafts=drafts, toks=toks, lps=lps, xs=xs, specified=specified)


def run_op(segs: list, V: int, dtype, ws=None, cap: int = 40):
    """pie_spec_verify_rows_sampled over `segs` in the given order: seg = dict(raw [rows, V] or None (idle), ring np [1024], pos0, seat,
    exp (expected_segment's), len0).  Returns per segment what the op left: tokens [8], n, logprobs rows, logits rows, ring, calls, ids row, len."""
    from proxy_inference_engine_amd import hip_ops
    B = len(segs)
    rows = [0 if g["raw"] is None else g["raw"].shape[0] for g in segs]
    seg_first = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    N = int(seg_first[-1])
    logits = torch.cat([g["raw"] for g in segs if g["raw"] is not None]).contiguous().clone()
    fed = [t for g in segs if g["raw"] is not None for t in g["exp"]["fed"]]
    drafts = np.full((B, 7), SENT, np.int32)
    for s, g in enumerate(segs):
        if g["raw"] is not None:
            drafts[s, :len(g["exp"]["drafts"])] = g["exp"]["drafts"]
    table = hip_ops.row_tail_table([record_of(g["seat"]) for g in segs], "cuda")
    rings = torch.from_numpy(np.stack([g["ring"] for g in segs]).astype(np.int32)).cuda()
    any_bias, any_xtc = any(g["seat"]["bias"] for g in segs), any(g["seat"]["xtc"] for g in segs)
    bias = None
    if any_bias:
        bcap = max(len(g["seat"]["bias"][0]) for g in segs if g["seat"]["bias"])
        b_ids, b_vals, b_n = np.full((B, bcap), 1, np.int32), np.full((B, bcap), 99.0, np.float32), np.zeros(B, np.int32)
        for s, g in enumerate(segs):
            if g["seat"]["bias"]:
                k = len(g["seat"]["bias"][0])
                b_ids[s, :k], b_vals[s, :k], b_n[s] = g["seat"]["bias"][0], g["seat"]["bias"][1], k
        bias = tuple(torch.from_numpy(a).cuda() for a in (b_ids, b_vals, b_n))
    xtc = hip_ops.xtc_records([hip_ops.xtc_pack(*g["seat"]["xtc"]) if g["seat"]["xtc"] else hip_ops.xtc_pack() for g in segs], "cuda") if any_xtc else None
    ids = torch.full((B, cap), SENT, dtype=torch.int32, device="cuda")
    lens = dev_ids([g["len0"] for g in segs])
    out = (torch.full((B, 8), SENT, dtype=torch.int32, device="cuda"), torch.full((B,), SENT, dtype=torch.int32, device="cuda"),
           torch.full((N, V), 123.0, dtype=torch.float32, device="cuda"))
    if ws is None:
        ws = hip_ops.spec_verify_rows_sampled_workspace("cuda", N, V)
    tokens, n, logprobs = hip_ops.spec_verify_rows_sampled(logits, torch.from_numpy(seg_first).cuda(), dev_ids(fed), torch.from_numpy(drafts).cuda(),
                                                           dev_ids([g["pos0"] for g in segs]), table, rings, bias=bias, xtc=xtc, ids=ids, lengths=lens,
                                                           workspace=ws, out=out)
    torch.cuda.synchronize()
    got = []
    for s in range(B):
        r0, r1 = int(seg_first[s]), int(seg_first[s + 1])
        got.append(dict(tokens=tokens[s].tolist(), n=int(n[s]), lp=logprobs[r0:r1], x=logits[r0:r1], ring=rings[s].cpu().numpy(), calls=int(table[s, CALLS_WORD]),
                        ids=ids[s].tolist(), len=int(lens[s])))
    return got, seg_first, fed


def check_segment(g: dict, got: dict, V: int, cap: int, what):
    """One segment of run_op's result against its expectation: everything bit for bit."""
    if g["raw"] is None:
        assert got["n"] == 0 and got["tokens"] == [-1] * 8 and got["calls"] == g["seat"]["calls"] and np.array_equal(got["ring"], g["ring"]), what
        assert got["len"] == g["len0"] and all(t == SENT for t in got["ids"]), what
        return
    e = g["exp"]
    (n, toks), = tr.accept_rows(e["toks"], [0, len(e["toks"])], [e["drafts"]], V)
    assert got["n"] == n and got["tokens"] == (toks + [-1] * 8)[:8], (what, got["tokens"], toks)
    for j in range(e["specified"]):
        assert np.array_equal(bits_of(got["lp"][j]), bits_of(e["lps"][j])), (what, "logprobs of row", j)
        assert torch.equal(got["x"][j].view(torch.int16), e["xs"][j].view(torch.int16)), (what, "processed logits of row", j)
    draws = g["seat"]["spec"] is not None
    want_ring, want_calls = tr.commit(g["ring"][None], [g["seat"]["calls"]], [draws], e["fed"], [0, len(e["fed"])], [g["pos0"]], [n])
    assert got["calls"] == want_calls[0] == g["seat"]["calls"] + (n if draws else 0), what
    assert np.array_equal(got["ring"], want_ring[0]) and int((got["ring"] != g["ring"]).sum()) <= n, what   # n committed slots, every other one as it was
    L = g["len0"]
    assert got["len"] == min(L + n, cap) and got["ids"][L:min(L + n, cap)] == toks[:max(0, min(n, cap - L))], what
    assert all(t == SENT for t in got["ids"][:L] + got["ids"][min(L + n, cap):]), what


# ------------------------------------------------------------------ 1. the op against the rows alone, bit for bit
SEG_ROWS = [1, 2, 8, 1, 0]                                               # and an idle slot
KINDS = ["greedy", "greedy_pen", "top_p_pen_bias", "top_k_xtc"]
POS_CASES = [(0, 60), (37, 60), (1020, 1024), (37, 1)]                   # pos0 0; below context_size; the segment's slots wrap onto positions row 0 still reads; a window of the row's own input alone
VARIANTS = ["all", "rej0", "mid", "oov"]


def op_segments(V: int, dtype, case: int, variant: str, order=None):
    """The five segments of a case: seat kinds rotated by the case over the segments, ids chosen so that whatever is read from a wrong
    place changes a logit -- eight ids that occur at ring positions 0..7 only, a sentinel id that occurs in unwritten slots only, and per
    segment a hot set of three ids that carry every row's largest logits and are what its tokens, hence its drafts, repeat."""
    pos0, context = POS_CASES[case]
    rng = np.random.default_rng(V * 7 + case)
    perm = rng.permutation(V)
    uniq8, sent_id, pool = perm[:8], int(perm[8]), perm[24:]
    segs = []
    for s, rows in enumerate(SEG_ROWS):
        H = [int(h) for h in perm[9 + 3 * s:12 + 3 * s]]
        kind = KINDS[(s + case) % 4]
        st = {"greedy": seat(seed=11 + s, calls=5, context=context),
              "greedy_pen": seat(seed=11 + s, calls=5, penalty=1.3, context=context),
              "top_p_pen_bias": seat(("top_p", 0.8, 0.9, 0), seed=977 + s, calls=2 ** 32 - 3, penalty=1.3, context=context,
                                     bias=([H[2], H[0], H[2], V + 5, int(pool[0])], [-1.5, 0.75, 3.0, 1.0, 0.25])),
              "top_k_xtc": seat(("top_k", 1.0, 0.0, 4), seed=31337 + s, calls=41, context=context, xtc=(0.9, 0.1, (H[1],)))}[kind]
        ring = np.full(tr.RING, sent_id, np.int64)
        for q in range(pos0):
            ring[q] = uniq8[q] if q < 8 else pool[int(rng.integers(1, len(pool)))]
        raw = None
        if rows:
            x = (rng.standard_normal((rows, V)) * 2.0).astype(np.float32)
            for k, h in enumerate(H):
                x[:, h] = 14.0 + 1.5 * k + 0.125 * rng.standard_normal(rows)   # (penalised, still above every other id)
            raw = torch.from_numpy(x).to("cuda").to(dtype).contiguous()
        g = dict(raw=raw, ring=ring, pos0=pos0, seat=st, len0=[5, 9, 33, 7, 12][s], kind=kind, exp=None)
        if rows:
            wrong = lambda t: (t + 1) % V
            corrupt = {"all": {}, "rej0": {0: wrong}, "mid": {3: wrong} if rows == 8 else {}, "oov": {2: lambda t: V + 3} if rows == 8 else {0: lambda t: -2}}[variant]
            g["exp"] = expected_segment(raw, ring, pos0, st, H[0], V, lambda j, t: corrupt[j](t) if j in corrupt else t)
        segs.append(g)
    return segs


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("V", [1003, 4099, 32000])
def test_the_op_equals_the_rows_alone(V, dtype):
    """V & 7 != 0 below 2048, an odd V near 4100, and 32000.  Segments of 1, 2, 8 and 1 rows and an idle slot; the four seat kinds move
    over them with the pos0 case.  One workspace, zeroed once, serves every call."""
    from proxy_inference_engine_amd import hip_ops
    ws = hip_ops.spec_verify_rows_sampled_workspace("cuda", sum(SEG_ROWS), V)
    for case in range(len(POS_CASES)):
        for variant in VARIANTS:
            segs = op_segments(V, dtype, case, variant)
            got, _, _ = run_op(segs, V, dtype, ws)
            n = [o["n"] for o in got]
            want_n = {"all": [1, 2, 8, 1, 0], "rej0": [1, 1, 1, 1, 0], "mid": [1, 2, 4, 1, 0], "oov": [1, 1, 3, 1, 0]}[variant]
            assert n == want_n, (V, dtype, case, variant, n)              # the cases are what they claim to be
            for s, (g, o) in enumerate(zip(segs, got)):
                check_segment(g, o, V, 40, (V, dtype, case, variant, s, g["kind"]))
            if variant == "all":                                           # the drafts repeat ids: a later row's window holds them, and they were penalised there
                e = segs[2]["exp"]
                assert len(set(e["fed"])) < len(e["fed"])


# ------------------------------------------------------------------ 2. independence of order and neighbours
def test_a_seat_does_not_depend_on_its_row_or_its_neighbours():
    V, dtype = 4099, torch.bfloat16
    segs = op_segments(V, dtype, 1, "all")
    first, _, _ = run_op(segs, V, dtype)
    other = op_segments(V, dtype, 2, "rej0")[2]                            # another seat, with other parameters, at another position
    order = [2, 4, 0, 3, 1]
    second, _, _ = run_op([other] + [segs[i] for i in order], V, dtype)
    for k, i in enumerate(order, 1):
        a, b = first[i], second[k]
        assert (a["tokens"], a["n"], a["calls"], a["ids"], a["len"]) == (b["tokens"], b["n"], b["calls"], b["ids"], b["len"]), i
        assert np.array_equal(a["ring"], b["ring"]) and torch.equal(a["x"].view(torch.int16), b["x"].view(torch.int16)), i
        assert np.array_equal(bits_of(a["lp"]), bits_of(b["lp"])), i
    check_segment(other, second[0], V, 40, "the neighbour")


# ------------------------------------------------------------------ 3. Model.spec_step_batch_tail on the tiny golden models
OFFSETS, COUNTS = (5, 60, 252), (0, 3, 7)                                # 252 + 8 rows cross a 64-row page boundary


def model_seats(V):
    return [seat(seed=3, calls=0, penalty=1.25, context=60),
            seat(("top_p", 0.8, 0.9, 0), seed=2024, calls=5, penalty=1.2, context=60, bias=([7, 3, 7, V + 2], [1.5, -0.5, 9.0, 2.0])),
            seat(("top_k", 1.0, 0.0, 4), seed=99, calls=11, penalty=1.1, context=300, xtc=(0.8, 0.1, (1,)))]


def arm(model, seats, prompts):
    B = len(seats)
    model.set_batch_tail(B)
    model.write_batch_tail(list(range(B)), [record_of(st) for st in seats], [list(p) for p in prompts])
    if any(st["bias"] for st in seats):
        model.set_batch_edits(B, masks=False, bias_cap=max(len(st["bias"][0]) for st in seats if st["bias"]))
        model.write_batch_edits(list(range(B)), biases=[st["bias"] for st in seats])
    if any(st["xtc"] for st in seats):
        model.set_batch_xtc(B)
        model.write_batch_xtc(list(range(B)), [st["xtc"] for st in seats])


def disarm(model):
    model.clear_batch_tail(), model.clear_batch_edits(), model.clear_batch_xtc()


def prefilled(model, pool, prompts):
    caches = [model.make_paged_cache(pool, max_blocks=8) for _ in prompts]
    first = [int(model.step(dev_ids(p), c)[0].item()) for p, c in zip(prompts, caches)]
    return caches, first


def release(caches):
    for c in caches:
        c[0].page_manager.release()


@pytest.mark.parametrize("name", list(MODELS))
def test_spec_step_batch_tail_equals_the_ops_over_the_greedy_entrys_rows(golden_dir, name):
    from proxy_inference_engine_amd import hip_ops
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    V = cfg["vocab_size"]
    prompts = [[int(t) for t in np.random.default_rng(4400 + o).integers(0, V, o)] for o in OFFSETS]
    seats = model_seats(V)
    rings = []
    for p in prompts:
        ring = np.zeros(tr.RING, np.int64)                                 # what write_batch_tail leaves: the prompt by position, zeros elsewhere
        ring[:len(p)] = p
        rings.append(ring)
    pool = private_pool(model, 24)
    seg_first = np.concatenate([[0], np.cumsum([1 + m for m in COUNTS])])
    N = int(seg_first[-1])

    def raw_rows(drafts):
        """The raw logits [N, V] the greedy entry leaves for this call, on a twin of the caches."""
        caches, first = prefilled(model, pool, prompts)
        model.spec_step_batch(dev_ids(first), caches, drafts, list(COUNTS))
        raw = model._spec_batch_ws.view(model.dtype)[:N * V].view(N, V).clone()
        release(caches)
        return first, raw

    def expected(first, raw, drafts):
        host = drafts.tolist()
        return [expected_segment(raw[seg_first[s]:seg_first[s + 1]], rings[s], OFFSETS[s], seats[s], first[s], V, lambda j, t, s=s: host[s][j]) for s in range(3)]

    # drafts that are the reference tokens: row j's raw logits depend on the drafts before it only, so round j settles draft j
    drafts = torch.zeros((3, 7), dtype=torch.int32, device="cuda")
    for j in range(max(COUNTS)):
        first, raw = raw_rows(drafts)
        exp = expected(first, raw, drafts)
        for s, m in enumerate(COUNTS):
            if j < m:
                drafts[s, j] = exp[s]["toks"][j]
    drafts[2, 4] = (int(drafts[2, 4]) + 1) % V                             # seat 2: rejected in the middle; seat 1: all accepted
    first, raw = raw_rows(drafts)
    exp = expected(first, raw, drafts)
    want = [tr.accept_rows(e["toks"], [0, len(e["toks"])], [e["drafts"]], V)[0] for e in exp]
    assert [w[0] for w in want] == [1, 4, 5]

    caches, first_b = prefilled(model, pool, prompts)                      # the twin the tail entry runs on
    assert first_b == first
    cap = 300
    seq_ids = torch.full((3, cap), SENT, dtype=torch.int32, device="cuda")
    for s, (p, f) in enumerate(zip(prompts, first)):
        seq_ids[s, :len(p) + 1] = dev_ids(list(p) + [f])
    seq_len = dev_ids([len(p) + 1 for p in prompts])
    try:
        arm(model, seats, prompts)
        n, toks, _ = model.spec_step_batch_tail(dev_ids(first), caches, drafts, list(COUNTS), seq_ids, seq_len)
        last = model.spec_batch_last
        assert n == [w[0] for w in want] and toks == [w[1] for w in want]
        assert last["n"].tolist() == n and last["seg_first"].tolist() == seg_first.tolist()
        for s, e in enumerate(exp):
            r0 = int(seg_first[s])
            for j in range(len(e["toks"])):
                assert np.array_equal(bits_of(last["logprobs"][r0 + j]), bits_of(e["lps"][j])), (name, s, j)
                assert torch.equal(last["logits"][r0 + j].view(torch.int16), e["xs"][j].view(torch.int16)), (name, s, j)
            assert all(c.offset == OFFSETS[s] + n[s] for c in caches[s])
            seq = prompts[s] + [first[s]] + toks[s]
            assert int(seq_len[s]) == len(seq) and seq_ids[s, :len(seq)].tolist() == seq and seq_ids[s, len(seq):].eq(SENT).all()
        bt = model._batch_tail
        draws = [st["spec"] is not None for st in seats]
        want_rings, want_calls = tr.commit(np.stack(rings), [st["calls"] for st in seats], draws, [t for e in exp for t in e["fed"]], seg_first, OFFSETS, n)
        assert bt["table"][:3, CALLS_WORD].tolist() == want_calls and np.array_equal(bt["recent"][:3].cpu().numpy(), want_rings)
        # a plain step under the same armed tail: its tokens are the rows-alone tokens at calls + n -- the stream is whole -- and it
        # recorded its inputs behind the ids the pass committed -- the ring is whole
        tok = dev_ids([t[-1] for t in toks])
        nxt, logprobs, _ = model.step_batch(tok, caches)
        for s, st in enumerate(seats):
            t = int(nxt[s])
            if st["spec"] is not None:
                counter = torch.tensor([want_calls[s], 0], dtype=torch.int64, device="cuda")
                assert t == int(hip_ops.sample(logprobs[s].clone(), *st["spec"], xtc=None if st["xtc"] is None else hip_ops.xtc_pack(*st["xtc"]), rng=(st["seed"], counter)).item()), (name, s)
            else:
                assert t == int(logprobs[s].argmax())
            want_rings[s, (OFFSETS[s] + n[s]) & (tr.RING - 1)] = toks[s][-1]
        assert np.array_equal(bt["recent"][:3].cpu().numpy(), want_rings)
        assert bt["table"][:3, CALLS_WORD].tolist() == [c + d for c, d in zip(want_calls, draws)]
    finally:
        disarm(model)
    release(caches)
    assert pool.get_num_free_pages() == pool.size()


# ------------------------------------------------------------------ 4. the engine, deterministic draws: the oracle's greedy continuations
def counted(model, name):
    """mock.patch.object context that counts the calls of a Model entry and lets them through."""
    real = getattr(model, name)
    calls = []

    def wrapped(*a, **kw):
        out = real(*a, **kw)
        calls.append(out)
        return out
    return mock.patch.object(model, name, wrapped), calls


@pytest.mark.parametrize("name", list(MODELS))
def test_engine_with_top_k_1_generates_the_oracle_tokens_on_the_simulated_schedule(golden_dir, name):
    from proxy_inference_engine_amd import SpeculativeParams
    from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine, SamplingParams
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    sp = SpeculativeParams(batch_tail=True, **SP_KW)
    prompts, conts, next_token, n = e2e_case(golden_dir, name, False)
    want, schedule = sb.simulate_batch(prompts, next_token, n, 2, (), sp.num_draft, sp.ngram_max, sp.ngram_min, sp.min_draft)
    assert want == conts
    sampling = [SamplingParams(temp=1.0, top_k=1, seed=5), SamplingParams(), SamplingParams(temp=1.0, top_k=1, seed=6)][:len(prompts)]
    eng = BatchedEngine(model, num_pages=64, max_batch=2, speculative=sp)
    patch, calls = counted(model, "spec_step_batch_tail")
    with patch:
        got = eng.generate(prompts, n, sampling=sampling)
    assert got == conts, name
    assert eng.spec_stats == sb.stats_of(schedule) and eng.spec_stats["accepted"] > 0 and len(calls) == eng.spec_stats["passes"] >= 1
    assert eng.pool.get_num_free_pages() == eng.pool.size()


# ------------------------------------------------------------------ 5. the engine, random draws: token j is draw j of the request's seed from its own row
@pytest.mark.parametrize("name", list(MODELS))
def test_engine_with_random_draws_yields_draw_j_of_every_seed(golden_dir, name):
    from proxy_inference_engine_amd import SpeculativeParams, hip_ops
    from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine, SamplingParams
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    V = cfg["vocab_size"]
    sp = SpeculativeParams(batch_tail=True, num_draft=7, ngram_max=3, ngram_min=1, min_draft=2)
    prompts, _, _, _ = e2e_case(golden_dir, name, False)
    new = 40
    sampling = [SamplingParams(temp=0.8, top_p=0.9, seed=700 + i, repetition_penalty=1.1, logit_bias={int(prompts[i][0]): 2.0, 5: -1.0}) for i in range(len(prompts))]
    rows: dict = {}                                                        # sequence -> the log-probability rows that yielded its tokens, in order
    passes = []

    def keep(cache, lps):
        rows.setdefault(id(cache[0].page_manager), []).extend(lp.clone() for lp in lps)

    real = {k: getattr(model, k) for k in ("spec_step_batch_tail", "step_batch", "prefill_batch", "step_mixed")}

    def spec_tail(tokens, caches, drafts, counts, *a, **kw):
        n, toks, nxt = real["spec_step_batch_tail"](tokens, caches, drafts, counts, *a, **kw)
        last = model.spec_batch_last
        first = last["seg_first"].tolist()
        for s, c in enumerate(caches):
            keep(c, [last["logprobs"][first[s] + i] for i in range(n[s])])
        passes.append((list(counts), list(n)))
        return n, toks, nxt

    def step_batch(tokens, caches, *a, **kw):
        out = real["step_batch"](tokens, caches, *a, **kw)
        for s, c in enumerate(caches):
            keep(c, [out[1][s]])
        return out

    def prefill_batch(ps, caches):
        out = real["prefill_batch"](ps, caches)
        for s, c in enumerate(caches):
            keep(c, [out[1][s]])
        return out

    def step_mixed(tokens, dcaches, ps, pcaches):
        out = real["step_mixed"](tokens, dcaches, ps, pcaches)
        for s, c in enumerate(list(dcaches) + list(pcaches)):
            keep(c, [out[1][s]])
        return out

    eng = BatchedEngine(model, num_pages=64, max_batch=4, speculative=sp)
    with mock.patch.multiple(model, spec_step_batch_tail=spec_tail, step_batch=step_batch, prefill_batch=prefill_batch, step_mixed=step_mixed):
        got = eng.generate(prompts, new, sampling=sampling)
    assert len(rows) == len(prompts) and all(len(g) == new for g in got)
    for i, (lps, g) in enumerate(zip(rows.values(), got)):                  # every request was admitted at once: sequences appear in request order
        assert len(lps) >= new
        spec = sampling[i].hip_spec()
        for j in range(new):
            counter = torch.tensor([j, 0], dtype=torch.int64, device="cuda")
            assert g[j] == int(hip_ops.sample(lps[j], *spec, rng=(700 + i, counter)).item()), (name, i, j)
    fulls = [list(p) + g for p, g in zip(prompts, got)]
    next_token = lambda seq: next((f[len(seq)] for f in fulls if len(f) > len(seq) and f[:len(seq)] == list(seq)), -1)   # noqa: E731  (-1: the token behind max_new_tokens, cut whatever it is)
    want, schedule = sb.simulate_batch(prompts, next_token, new, 4, (), sp.num_draft, sp.ngram_max, sp.ngram_min, sp.min_draft)
    assert want == got and eng.spec_stats == sb.stats_of(schedule)
    assert passes == [(e[2], e[3]) for e in schedule if e[0] == "pass"]


# ------------------------------------------------------------------ 6. the untouched paths
def test_other_paths_are_the_same_before_and_after_a_batch_tail_generation(golden_dir):
    from proxy_inference_engine_amd import SpeculativeParams
    from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine, SamplingParams
    name = "tiny_llama_w4_bf16"
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    prompts, conts, _, _ = e2e_case(golden_dir, name, False)
    sampling = [SamplingParams(temp=0.9, top_p=0.8, seed=40 + i, repetition_penalty=1.15, logit_bias={3: 1.0}) for i in range(len(prompts))]

    def others():
        plain = BatchedEngine(model, num_pages=64, max_batch=4).generate(prompts, 24, sampling=sampling)
        launches = model.batch_graph_launches()
        greedy = BatchedEngine(model, num_pages=64, max_batch=4, speculative=SpeculativeParams(**SP_KW)).generate(prompts, 24)
        return plain, greedy, launches

    before = others()
    eng = BatchedEngine(model, num_pages=64, max_batch=4, speculative=SpeculativeParams(batch_tail=True, **SP_KW))
    tailed = eng.generate(prompts, 24, sampling=sampling)
    assert eng.spec_stats["passes"] + eng.spec_stats["steps"] >= 1 and len(tailed) == len(prompts)
    after = others()
    assert after == before and before[2] > 0 and before[1] == [c[:24] for c in conts]
    assert model._batch_tail is None and model._batch_edits is None and model._batch_xtc is None


# ------------------------------------------------------------------ 7. refusals by name, at all three layers; nothing has moved
def test_refusals_by_name(golden_dir):
    from proxy_inference_engine_amd import SpeculativeParams, _ffi, hip_ops
    from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine, SamplingParams
    cfg, dt, orc, model = load_tiny(golden_dir, "tiny_llama_w4_bf16")
    V = cfg["vocab_size"]
    # the op
    segs = op_segments(1003, torch.bfloat16, 1, "all")
    lib = _ffi.load()
    assert int(lib.pie_spec_verify_rows_sampled_workspace_bytes(0, 1003)) == 0 and int(lib.pie_spec_verify_rows_sampled_workspace_bytes(4, 524289)) == 0
    x = segs[2]["raw"].clone()
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")   # noqa: E731
    table, ring = hip_ops.row_tail_table([hip_ops.row_tail_pack()], "cuda"), i32(1, 1024)
    good = dict(logits=x, seg_first=dev_ids([0, 8]), fed=i32(8), drafts=i32(1, 7), pos0=i32(1), table=table, recent_ids=ring)
    for bad, msg in ((dict(fed=i32(7)), "fed"), (dict(pos0=i32(2)), "pos0"), (dict(recent_ids=i32(1, 512)), "recent_ids"), (dict(logits=x.float()), "logits"),
                     (dict(bias=(i32(1, 4), torch.zeros((1, 3), device="cuda"), i32(1))), "bias"), (dict(ids=i32(1, 9)), "ids and lengths"),
                     (dict(workspace=torch.zeros(8, dtype=torch.int64, device="cuda")), "workspace")):
        with pytest.raises(ValueError, match=msg):
            hip_ops.spec_verify_rows_sampled(**{**good, **bad})
    ws = hip_ops.spec_verify_rows_sampled_workspace("cuda", 8, 1003)
    out, lp = i32(10), torch.zeros((8, 1003), device="cuda")
    call = lambda logits_p, B=1, dtype=_ffi.PIE_BF16, bias_cap=0: lib.pie_spec_verify_rows_sampled(   # noqa: E731
        logits_p, 8, 1003, dtype, _ffi.p(good["seg_first"]), B, _ffi.p(good["fed"]), _ffi.p(good["drafts"]), 7, _ffi.p(good["pos0"]), _ffi.p(table), _ffi.p(ring),
        None, None, None, bias_cap, None, _ffi.p(out), _ffi.p(out[8:]), _ffi.p(lp), None, None, 0, _ffi.p(ws), _ffi.stream())
    assert call(None) == -1 and call(_ffi.p(x), dtype=99) == -1 and call(_ffi.p(x), bias_cap=3) == -1 and call(_ffi.p(x), B=0) == -2
    assert call(_ffi.C.c_void_p(x.data_ptr() + 1)) == -3
    assert "pie_spec_verify_rows_sampled" in lib.pie_last_error().decode()
    # the Model entry and the library behind it
    pool = private_pool(model, 8)
    caches = [model.make_paged_cache(pool, max_blocks=4) for _ in range(2)]
    for c in caches:
        model.step(dev_ids([3, 4, 5, 6]), c)
    tok, drafts = dev_ids([1, 2]), torch.zeros((2, 7), dtype=torch.int32, device="cuda")
    run = lambda: model.spec_step_batch_tail(tok, caches, drafts, [1, 1])   # noqa: E731
    with pytest.raises(ValueError, match="no batch tail is set"):
        run()
    try:
        model.set_batch_tail(2)
        model.write_batch_tail([0, 1], [hip_ops.row_tail_pack("top_k", 1.0, 0.0, 3, seed=1, calls=9)] * 2)
        for arm_, clear, msg in ((lambda: model.set_batch_edits(2, masks=True, bias_cap=2), model.clear_batch_edits, "a mask part of the batch logits edits"),
                                 (lambda: model.set_batch_count_penalty(2), model.clear_batch_count_penalty, "a batch count penalty"),
                                 (lambda: model.set_batch_dry_penalty(2), model.clear_batch_dry_penalty, "a batch DRY penalty"),
                                 (lambda: model.set_batch_automata(2, 64), model.clear_batch_automata, "batch token automata"),
                                 (lambda: model.set_batch_top_logprobs(2, 3), model.clear_batch_top_logprobs, "top log-probabilities"),
                                 (lambda: model.set_prompt_logprobs(8, 3, 16)["count"].fill_(-1), model.clear_prompt_logprobs, "prompt scoring")):
            try:
                arm_()
                with pytest.raises(ValueError, match=msg):
                    run()
            finally:
                clear()
        with pytest.raises(ValueError, match="a batch tail"):              # the greedy entry keeps refusing it
            model.spec_step_batch(tok, caches, drafts, [1, 1])
        model.set_batch_tail(1)                                            # fewer seats than sequences: the library's own check
        with pytest.raises(Exception, match="rows_cap"):
            run()
        model.set_batch_tail(2)
        i8 = private_pool(model, 4)
        i8.dtype = torch.int8
        seq8 = [model.make_paged_cache(i8, max_blocks=2)]
        seq8[0][0].page_manager.advance(1)
        with pytest.raises(ValueError, match="int8 KV pages"):
            model.spec_step_batch_tail(tok[:1], seq8, drafts, [1])
        assert all(c.offset == 4 for cs in caches for c in cs)             # nothing moved: the caches ...
        assert model._batch_tail["table"][:2, CALLS_WORD].tolist() == [9, 9]   # ... and the seats' streams
        n, toks, _ = run()                                                  # and after all that the pass still runs
        assert [c[0].offset for c in caches] == [4 + n[0], 4 + n[1]] and model._batch_tail["table"][:2, CALLS_WORD].tolist() == [9 + n[0], 9 + n[1]]
    finally:
        disarm(model)
    release(caches)
    # the engines
    eng = BatchedEngine(model, num_pages=16, max_batch=2, speculative=SpeculativeParams(batch_tail=True, **SP_KW))
    for gen, msg in ((dict(sampling=SamplingParams(token_mask=[1, 2])), "a token mask"), (dict(sampling=SamplingParams(frequency_penalty=0.5)), "frequency / presence"),
                     (dict(sampling=SamplingParams(dry_multiplier=0.8)), "DRY"), (dict(logprobs=True), "`logprobs`"), (dict(prompt_logprobs=0), "`prompt_logprobs`")):
        with pytest.raises(ValueError, match=msg):
            eng.generate([[1, 2, 3], [4, 5]], 4, **gen)
    assert eng.pool.get_num_free_pages() == eng.pool.size() and model._batch_tail is None
    with pytest.raises(ValueError, match="configured_tail"):
        BatchedEngine(model, speculative=SpeculativeParams(batch_tail=True, configured_tail=True))
    plain = BatchedEngine(model, num_pages=16, max_batch=2, speculative=SpeculativeParams(**SP_KW))
    with pytest.raises(ValueError, match="not plain"):
        plain.generate([[1, 2, 3], [4, 5]], 4, sampling=SamplingParams(temp=0.7))
