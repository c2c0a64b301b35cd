"""Batched speculation on the GPU: the per-row drafter, the paged verify attention and the segmented verify at op level
against their references; Model.spec_step_batch and BatchedEngine(speculative=...) against the oracle's greedy continuations of the tiny
golden models; the untouched plain path.

Prompt seeds were chosen on the CPU, with the oracle alone: every position of every continuation used here meets margin_ok (the top-two
gap exceeds what the kernels' rounding can move), and the batch schedules simulate_batch derives from the continuations hold every kind
of pass the tests name -- asserted again below, on the simulation, before anything runs."""
import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests import spec_batch_reference as sb
from tests import speculative_reference as ref
from tests._util import POISON, TORCH_DT, assert_dot_close, assert_vec_close, kv_history, marker_rows, plant_needles, sdpa_f64, to_bits, to_dev
from tests.test_gpu_speculative import E2E_SEEDS, MODELS, SENT, STEP_SEEDS, dev_ids, e2e_prompt, load_tiny, oracle_run, rows_alone, verify_rows

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. the per-row drafter: the reference per row, and pie_ngram_draft's bits
LENGTHS = [0, 1, 2, 63, 64, 65, 5000]


@pytest.mark.parametrize("alphabet", [4, 50000])
@pytest.mark.parametrize("B", [1, 3, 32])
def test_ngram_draft_rows_equals_the_reference_per_row(B, alphabet):
    """One call holds rows of every length (B = 32: all of them, several times; B = 3: 65, 0, 5000; B = 1: 5000), under lengths above the
    capacity and below zero too; a row is what ngram_draft returns for it alone."""
    from proxy_inference_engine_amd import hip_ops
    rng = np.random.default_rng(B * 13 + alphabet)
    cap = 5008
    lens = {1: [5000], 3: [65, 0, 5000]}.get(B) or [LENGTHS[i % len(LENGTHS)] for i in range(B - 2)] + [cap + 9, -4]
    ids = rng.integers(0, alphabet, (B, cap)).astype(np.int32)
    if alphabet == 4:
        ids[-1 if B == 1 else 2, 4993:5000] = np.resize(ids[-1 if B == 1 else 2, 4990:4993], 7)   # a period-3 tail: the copy runs into its own output
    d_ids, d_len = torch.from_numpy(ids).cuda(), dev_ids(lens)
    for nmax, nmin, k in ((1, 1, 1), (3, 1, 7), (8, 3, 31)):
        out = (torch.full((B, k), SENT, dtype=torch.int32, device="cuda"), torch.full((B,), SENT, dtype=torch.int32, device="cuda"))
        ws = hip_ops.ngram_draft_rows_workspace("cuda", B)
        ws.fill_(-1)                                                   # no initialisation needed: garbage must not show
        drafts, counts = hip_ops.ngram_draft_rows(d_ids, d_len, nmax, nmin, k, workspace=ws, out=out)
        for s in range(B):
            what = (B, alphabet, nmax, nmin, k, s, lens[s])
            want = ref.ngram_draft(ids[s, :max(0, min(lens[s], cap))], nmax, nmin, k)
            assert int(counts[s]) == len(want) and drafts[s, :len(want)].tolist() == want, what
            assert drafts[s, len(want):].eq(SENT).all(), what          # no match: the row keeps its contents
            alone = hip_ops.ngram_draft(d_ids[s], d_len[s:s + 1], nmax, nmin, k, out=(torch.full((k,), SENT, dtype=torch.int32, device="cuda"),
                                                                                      torch.full((1,), SENT, dtype=torch.int32, device="cuda")))
            assert torch.equal(alone[0], drafts[s]) and int(alone[1]) == int(counts[s]), what


def test_ngram_draft_rows_checks_arguments():
    from proxy_inference_engine_amd import _ffi, hip_ops
    ids, n = torch.zeros((2, 9), dtype=torch.int32, device="cuda"), dev_ids([9, 9])
    for nmax, nmin, k in ((0, 0, 3), (2, 3, 3), (9, 1, 3), (3, 1, 0), (3, 1, 32)):
        with pytest.raises(ValueError, match="pie_ngram_draft_rows"):
            hip_ops.ngram_draft_rows(ids, n, nmax, nmin, k, out=(torch.zeros((2, k), dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")))
    with pytest.raises(ValueError, match="ngram_draft_rows"):
        hip_ops.ngram_draft_rows(ids[0], n, 3, 1, 3)
    lib = _ffi.load()
    assert int(lib.pie_ngram_draft_rows_workspace_bytes(0)) == 0 and int(lib.pie_ngram_draft_rows_workspace_bytes(4097)) == 0


# ------------------------------------------------------------------ 2. the paged verify attention against float64, one query row at a time
HKV, MAX_BLOCKS, N_PAGES = 2, 8, 40
SEG_ROWS = (1, 2, 8)                     # three sequences, and an idle slot behind them
FIRST_CTX = [(65, 64, 1), (200, 1, 63), (1, 63, 64), (64, 200, 65), (63, 65, 200), (1, 64, 300)]   # first-row contexts of the three segments


def attn_case(rng, D, rep, dt, first, splits):
    """(q, slab, tables, row_seq, row_ctx, seg_first, references): every sequence on shuffled pages of a pool that is NaN wherever nothing
    is referenced and behind every context; markers on both sides of every split edge of the segment's longest row; the K of every later
    draft row aligned with the query of the row before it and its V loud, so a row that sees its successor fails."""
    Hq = HKV * rep
    seg_first, row_seq, row_ctx = sb.form_rows([c - 1 for c in first], [r - 1 for r in SEG_ROWS])
    seg_first, N = seg_first + [seg_first[-1]], seg_first[-1]          # the idle slot
    q = po.round_T(rng.standard_normal((N, Hq, D), dtype=np.float32), dt)
    pool = np.full((N_PAGES, 2, HKV, 64, D), np.nan, np.float32)
    pages = rng.permutation(N_PAGES)
    tables = np.zeros((len(SEG_ROWS) + 1, MAX_BLOCKS), np.int32)
    want = np.zeros((N, Hq, D), np.float64)
    at = 0
    for s, (c0, rows) in enumerate(zip(first, SEG_ROWS)):
        T = c0 + rows - 1
        own = list(range(c0, T))                                       # the positions of the rows behind the first: successors of some row
        k, v = kv_history(rng, HKV, T, D, dt, sorted(set(marker_rows(T, [(T, splits)]) + own)), strong=own)
        for i, p in enumerate(own):                                    # position c0 + i is the first one row i must not see
            plant_needles(k, q[seg_first[s] + i], [p], T, rep, dt, rng)
        n_blocks = (T + 63) // 64
        mine = pages[at:at + n_blocks]
        at += n_blocks
        tables[s, :n_blocks] = mine
        tables[s, n_blocks:] = pages[-1]                               # an unreferenced page: NaN throughout
        pad = np.full((HKV, n_blocks * 64, D), np.nan, np.float32)
        pad[:, :T] = k
        pool[mine, 0] = pad.reshape(HKV, n_blocks, 64, D).transpose(1, 0, 2, 3)
        pad[:, :T] = v
        pool[mine, 1] = pad.reshape(HKV, n_blocks, 64, D).transpose(1, 0, 2, 3)
        for i in range(rows):
            r = seg_first[s] + i
            want[r] = sdpa_f64(q[r][:, None], k, v, 1.0 / np.sqrt(D), c0 + i)[:, 0]
    assert at < N_PAGES
    return q, pool, tables, row_seq, row_ctx, seg_first, want


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("rep", [1, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_paged_attn_verify_equals_float64_row_by_row(D, rep, dt):
    from proxy_inference_engine_amd import hip_ops
    auto = hip_ops.paged_attn_verify_splits(len(SEG_ROWS) + 1, HKV, MAX_BLOCKS)
    assert auto == MAX_BLOCKS                                          # 307 attended positions in 8 splits: every split is active in the last case
    rng = np.random.default_rng(D * 100 + rep * 10 + len(dt))
    for first in FIRST_CTX:
        for splits in (0, 1, 3):
            q, pool, tables, row_seq, row_ctx, seg_first, want = attn_case(rng, D, rep, dt, first, splits or auto)
            dev = lambda x: torch.from_numpy(np.asarray(x, np.int32)).cuda()
            out = hip_ops.paged_attn_verify(to_dev(po.to_bits(q, dt), dt), to_dev(po.to_bits(pool, dt), dt), N_PAGES, dev(tables), dev(row_seq), dev(row_ctx),
                                            dev(seg_first), HKV, 1.0 / np.sqrt(D), splits=splits)
            got = po.from_bits(to_bits(out), dt)
            assert np.isfinite(got).all(), (D, rep, dt, first, splits)
            for r in range(len(row_ctx)):
                assert_dot_close(got[r], po.round_T(want[r], dt), dt, what=f"D={D} rep={rep} {dt} first={first} splits={splits} row {r} (ctx {row_ctx[r]})")


def test_paged_attn_verify_clamps_device_indices_and_checks_arguments():
    """Context lengths beyond the table, a sequence index and page ids out of range, segments that overlap or run past N: nothing may
    become a wild address (the outputs are then unspecified, but finite or NaN values of the pool -- the launch completes)."""
    from proxy_inference_engine_amd import _ffi, hip_ops
    D, Hq, N = 64, 4, 10
    q = torch.randn((N, Hq, D), device="cuda").to(torch.bfloat16)
    slab = torch.randn((4, 2, HKV, 64, D), device="cuda").to(torch.bfloat16)
    dev = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")
    tables = dev([[0, 1], [1 << 30, -5], [3, 2]])
    out = hip_ops.paged_attn_verify(q, slab, 4, tables, dev([0, 7, -3, 1, 1, 1, 2, 2, 2, 2]), dev([1 << 30, -9, 5, 100, 129, 1 << 20, 0, 1, 2, 3]),
                                    dev([0, 3, -2, 99]), HKV, 0.125)
    torch.cuda.synchronize()
    assert out.shape == q.shape
    good = (dev([0] * N), dev([1] * N), dev([0, 1, 2, N]))
    with pytest.raises(ValueError, match="splits"):
        hip_ops.paged_attn_verify(q, slab, 4, tables, *good, HKV, 0.125, splits=33)
    lib = _ffi.load()
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    call = lambda q_p, D_=D, Hkv=HKV: lib.pie_paged_attn_verify(q_p, _ffi.p(slab), 4, _ffi.p(tables), 2, _ffi.p(good[0]), _ffi.p(good[1]), _ffi.p(good[2]), N, 3, Hq, Hkv, D_,   # noqa: E731
                                                                0.125, _ffi.PIE_BF16, 0, _ffi.p(out), _ffi.p(ws), _ffi.stream())
    assert call(None) == -1 and call(_ffi.p(q), 96) == -2 and call(_ffi.p(q), D, 3) == -2 and call(_ffi.C.c_void_p(q.data_ptr() + 2)) == -3
    assert int(lib.pie_paged_attn_verify_workspace_bytes(0, Hq, D, 1)) == 0 and int(lib.pie_paged_attn_verify_workspace_bytes(N, Hq, D, 33)) == 0


# ------------------------------------------------------------------ 3. the segmented verify: pie_spec_verify per segment, exact
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("V", [1000, 32003])
def test_spec_verify_rows_equals_spec_verify_per_segment(V, dtype):
    from proxy_inference_engine_amd import hip_ops
    seg_rows = [1, 4, 8, 0, 2, 8, 8, 5]                                # one-row segments, an idle slot, full ones
    seg_first = np.concatenate([[0], np.cumsum(seg_rows)]).astype(np.int32)
    N, B = int(seg_first[-1]), len(seg_rows)
    logits = verify_rows(V, N, dtype)
    toks, _ = rows_alone(logits)
    drafts = np.full((B, 7), SENT, np.int32)
    want = []
    for s, rows in enumerate(seg_rows):
        r0 = int(seg_first[s])
        good = toks[r0:r0 + rows - 1] if rows else []
        d = list(good)
        if s == 2:
            d[0] = (d[0] + 1) % V                                      # wrong at 0
        if s == 5:
            d[3] = (d[3] + 1) % V                                      # wrong in the middle
        if s == 6:
            d[5] = V + 3                                               # an id out of range: never accepted, never an index
        if s == 7:
            d[1] = -2
        drafts[s, :len(d)] = d
        if rows >= 2:                                                  # pie_spec_verify on the segment alone
            t, n = hip_ops.spec_verify(logits[r0:r0 + rows].contiguous(), dev_ids(d))
            want.append((int(n.item()), t.tolist()))
        elif rows == 1:                                                # pie_logprobs_argmax of the row alone
            want.append((1, [int(hip_ops.logprobs_argmax(logits[r0].contiguous())[0].item())]))
        else:
            want.append((0, []))
    assert [w[0] for w in want] == [1, 4, 1, 0, 2, 4, 6, 2]            # the cases are what they claim to be
    cap = 40
    ids = torch.full((B, cap), SENT, dtype=torch.int32, device="cuda")
    lens = dev_ids([5, 9, 33, 7, 0, 38, 39, 12])                       # 38 + 4 and 39 + 6 run past the capacity: clamped
    out = (torch.full((B, 8), SENT, dtype=torch.int32, device="cuda"), torch.full((B,), SENT, dtype=torch.int32, device="cuda"))
    tokens, n = hip_ops.spec_verify_rows(logits, torch.from_numpy(seg_first).cuda(), torch.from_numpy(drafts).cuda(), ids=ids, lengths=lens, out=out)
    for s, (wn, wt) in enumerate(want):
        assert int(n[s]) == wn and tokens[s].tolist() == (wt + [-1] * 8)[:8], (V, dtype, s)
        L = [5, 9, 33, 7, 0, 38, 39, 12][s]
        assert int(lens[s]) == min(L + wn, cap) and ids[s, L:min(L + wn, cap)].tolist() == wt[:max(0, min(wn, cap - L))], (V, dtype, s)
        assert ids[s, :L].eq(SENT).all() and ids[s, min(L + wn, cap):].eq(SENT).all(), (V, dtype, s)
    tokens2, n2 = hip_ops.spec_verify_rows(logits, torch.from_numpy(seg_first).cuda(), torch.from_numpy(drafts).cuda())   # without ids: the same decision
    assert torch.equal(tokens2, tokens) and torch.equal(n2, n)
    with pytest.raises(ValueError, match="ids and lengths"):
        hip_ops.spec_verify_rows(logits, torch.from_numpy(seg_first).cuda(), torch.from_numpy(drafts).cuda(), ids=ids)


# ------------------------------------------------------------------ 4. Model.spec_step_batch against the oracle's greedy continuations
OFFSETS, COUNTS, FURTHER = (5, 60, 252), (0, 3, 7), 12                 # 252 + 8 rows cross a page; 60 + 4 rows end exactly on one
OFFSET5_SEEDS = {"tiny_llama_w4_bf16": 52, "tiny_dense_f16_bias": 0}   # chosen on the CPU like STEP_SEEDS, with the same recipe


def private_pool(model, num_pages):
    from proxy_inference_engine_amd.cache.kv_cache.paged import PageAllocator
    return PageAllocator(num_pages, model.n_kv_heads, model.head_dim, dtype=model.dtype, device=model.device, num_layers=len(model.layers))


@pytest.mark.parametrize("name", list(MODELS))
def test_spec_step_batch_leaves_every_sequence_where_greedy_steps_would(golden_dir, name):
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    V = cfg["vocab_size"]
    seeds = [OFFSET5_SEEDS[name]] + [STEP_SEEDS[(name, o)] for o in OFFSETS[1:]]
    prompts = [np.random.default_rng(1000 * o + sd).integers(0, V, o) for o, sd in zip(OFFSETS, seeds)]
    runs = [oracle_run(golden_dir, name, p, 7 + 1 + FURTHER + 1) for p in prompts]
    for corrupt in (0, 2, None):
        what = f"{name} corrupt={corrupt}"
        pool = private_pool(model, 16)
        caches = [model.make_paged_cache(pool, max_blocks=8) for _ in prompts]
        first = [int(model.step(dev_ids(p), c)[0].item()) for p, c in zip(prompts, caches)]
        assert first == [r[0][0] for r in runs], what
        drafts = torch.full((3, 7), SENT, dtype=torch.int32, device="cuda")
        n_acc = []
        for s, (m, (cont, _)) in enumerate(zip(COUNTS, runs)):
            d = cont[1:m + 1]
            if corrupt is not None and corrupt < m:
                d[corrupt] = (d[corrupt] + 1) % V
            drafts[s, :m] = dev_ids(d) if m else drafts[s, :0]
            n_acc.append(m if corrupt is None or corrupt >= m else corrupt)
        cap = 300
        seq_ids = torch.full((3, cap), SENT, dtype=torch.int32, device="cuda")
        for s, (p, f) in enumerate(zip(prompts, first)):
            seq_ids[s, :len(p) + 1] = dev_ids(list(p) + [f])
        seq_len = dev_ids([len(p) + 1 for p in prompts])
        nxt_drafts = torch.full((3, 7), SENT, dtype=torch.int32, device="cuda")
        n, toks, nxt = model.spec_step_batch(dev_ids(first), caches, drafts, list(COUNTS), seq_ids, seq_len, then_draft=(3, 1, 7, nxt_drafts))
        assert n == [a + 1 for a in n_acc], what
        for s, (cont, _) in enumerate(runs):
            assert toks[s] == cont[1:n_acc[s] + 2], (what, s)
            assert all(c.offset == OFFSETS[s] + n[s] for c in caches[s]), (what, s)
            seq = list(prompts[s]) + cont[:n_acc[s] + 2]               # the seat's ids are whole up to the token about to be fed ...
            assert int(seq_len[s]) == len(seq) and seq_ids[s, :len(seq)].tolist() == seq and seq_ids[s, len(seq):].eq(SENT).all(), (what, s)
            want_draft = ref.ngram_draft(seq, 3, 1, 7)                 # ... and the next draft was made from them
            assert nxt[s] == len(want_draft) and nxt_drafts[s, :len(want_draft)].tolist() == want_draft, (what, s)
        assert model.spec_batch_last["n"].tolist() == n and [model.spec_batch_last["tokens"][s, :n[s]].tolist() for s in range(3)] == toks
        # plain steps right after: the last accepted token is fed back, and nothing reads the rejected drafts' rows
        tok = dev_ids([t[-1] for t in toks])
        for k in range(FURTHER):
            tok, _, logits = model.step_batch(tok, caches)
            for s, (cont, ologits) in enumerate(runs):
                i = n_acc[s] + 1 + k                                   # position offset + i was fed cont[i]
                assert_vec_close(logits[s].float().cpu().numpy(), ologits[i + 1], dt, what=f"{what} seq {s} step {k}")
                assert int(tok[s]) == cont[i + 1], f"{what} seq {s} step {k}"
            tok = tok.clone()
        for c in caches:
            c[0].page_manager.release()
        assert pool.get_num_free_pages() == pool.size()


def test_spec_step_batch_refusals_by_name(golden_dir):
    cfg, dt, orc, model = load_tiny(golden_dir, "tiny_llama_w4_bf16")
    pool = private_pool(model, 8)
    caches = [model.make_paged_cache(pool, max_blocks=4) for _ in range(2)]
    for c in caches:
        model.step(dev_ids([3, 4, 5, 6]), c)
    tok, drafts = dev_ids([1, 2]), torch.zeros((2, 7), dtype=torch.int32, device="cuda")
    for counts, name in (([8, 0], "count"), ([1], "one count per sequence"), ([-1, 2], "count")):
        with pytest.raises(ValueError, match=name):
            model.spec_step_batch(tok, caches, drafts, counts)
    with pytest.raises(ValueError, match="seq_ids and seq_len"):
        model.spec_step_batch(tok, caches, drafts, [1, 1], seq_ids=torch.zeros((2, 9), dtype=torch.int32, device="cuda"))
    try:
        model.set_batch_top_logprobs(2, 3)
        with pytest.raises(ValueError, match="top log-probabilities"):
            model.spec_step_batch(tok, caches, drafts, [1, 1])
        model.clear_batch_top_logprobs()
        model.set_batch_tail(2)
        with pytest.raises(ValueError, match="a batch tail"):
            model.spec_step_batch(tok, caches, drafts, [1, 1])
        model.clear_batch_tail()
        bufs = model.set_prompt_logprobs(8, 3, 16)
        bufs["count"].fill_(-1)
        with pytest.raises(ValueError, match="prompt scoring"):
            model.spec_step_batch(tok, caches, drafts, [1, 1])
    finally:
        model.clear_batch_top_logprobs(), model.clear_batch_tail(), model.clear_prompt_logprobs()
    i8 = private_pool(model, 4)
    i8.dtype = torch.int8                                              # what the check branches on (real int8 pools: tests/test_gpu_paged.py)
    seq8 = [model.make_paged_cache(i8, max_blocks=2)]
    seq8[0][0].page_manager.advance(1)
    with pytest.raises(ValueError, match="int8 KV pages"):
        model.spec_step_batch(tok[:1], seq8, drafts, [1])
    assert all(c.offset == 4 for cs in caches for c in cs)             # nothing moved
    n, toks, _ = model.spec_step_batch(tok, caches, drafts, [1, 0])    # and after all that the pass still runs
    assert len(n) == 2 and all(1 <= k <= 2 for k in n) and [c[0].offset for c in caches] == [4 + n[0], 4 + n[1]]


# ------------------------------------------------------------------ 5. the engine end to end
SP_KW = dict(num_draft=7, ngram_max=3, ngram_min=1, min_draft=5)
E2E_TOKENS = 48
BATCH_SEEDS = {"tiny_llama_w4_bf16": E2E_SEEDS["tiny_llama_w4_bf16"], "tiny_dense_f16_bias": E2E_SEEDS["tiny_dense_f16_bias"] + [95]}   # (95: found like the others)
PLAIN_SEEDS = {"tiny_llama_w4_bf16": 53, "tiny_dense_f16_bias": 1}     # a prompt that repeats nothing: default_rng(777000 + seed), 24 ids
PREFIX_SEEDS = {"tiny_llama_w4_bf16": 454, "tiny_dense_f16_bias": 18}  # 64 shared ids in front of every prompt: default_rng(424200 + seed)
PREFIX_TOKENS = 24
ORACLES: dict = {}


def continuation(golden_dir, name, prompt, n):
    """oracle_run's tokens without the device model: the oracle's greedy continuation, every position's margin asserted."""
    import json
    from tests.test_gpu_speculative import margin_ok
    if name not in ORACLES:
        g = np.load(golden_dir / f"{name}.npz")
        ORACLES[name] = (json.loads(str(g["config_json"])), str(g["dtype"]), {k[2:]: g[k] for k in g.files if k.startswith("w:")})
        ORACLES[name] += (po.OracleLlama(ORACLES[name][0], ORACLES[name][2], ORACLES[name][1]),)
    cfg, dt, _, orc = ORACLES[name]
    cache = [po.OracleKVCache() for _ in orc.layers]
    lg = orc.forward(np.asarray(prompt), cache, last_only=True)
    toks = []
    for i in range(n):
        assert margin_ok(lg, dt), f"{name}: position {i} of the oracle's continuation is a near-tie: choose another seed"
        toks.append(int(np.argmax(lg)))
        if i + 1 < n:
            lg = orc.forward(np.array([toks[-1]]), cache)[0]
    return toks


def e2e_case(golden_dir, name, prefix: bool):
    """(prompts, the oracle's continuations, next-token function) of the three prompts of a model, behind a shared page of ids or not."""
    g = np.load(golden_dir / f"{name}.npz")
    import json
    V = json.loads(str(g["config_json"]))["vocab_size"]
    prompts = [[int(t) for t in e2e_prompt(sd, V)] for sd in BATCH_SEEDS[name]] + [[int(t) for t in np.random.default_rng(777000 + PLAIN_SEEDS[name]).integers(0, V, 24)]]
    prompts = prompts[-3:]
    n = E2E_TOKENS
    if prefix:
        pre = [int(t) for t in np.random.default_rng(424200 + PREFIX_SEEDS[name]).integers(0, V, 64)]
        prompts, n = [pre + p for p in prompts], PREFIX_TOKENS
    conts = [continuation(golden_dir, name, p, n + 12) for p in prompts]
    fulls = [p + c for p, c in zip(prompts, conts)]

    def next_token(seq):
        return next(f[len(seq)] for f in fulls if f[:len(seq)] == list(seq))
    return prompts, [c[:n] for c in conts], next_token, n


def schedule_kinds(schedule) -> set:
    passes = [e for e in schedule if e[0] == "pass"]
    rows = [(m, n) for e in passes for m, n in zip(e[2], e[3])]
    kinds = {"step"} if any(e[0] == "step" for e in schedule) else set()
    kinds |= {"unequal"} if any(0 in e[2] and max(e[2]) > 0 for e in passes) else set()
    kinds |= {"full"} if any(m and n == m + 1 for m, n in rows) else set()
    return kinds | ({"partial"} if any(m and n < m + 1 for m, n in rows) else set())


@pytest.mark.parametrize("kw", [dict(max_batch=2), dict(max_batch=4, share_prefix=True)], ids=["two_seats", "shared_prefix"])
@pytest.mark.parametrize("name", list(MODELS))
def test_engine_generates_the_oracle_tokens_on_the_simulated_schedule(golden_dir, name, kw):
    from proxy_inference_engine_amd import SpeculativeParams
    from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    sp = SpeculativeParams(**SP_KW)
    prompts, conts, next_token, n = e2e_case(golden_dir, name, bool(kw.get("share_prefix")))
    want, schedule = sb.simulate_batch(prompts, next_token, n, kw["max_batch"], (), sp.num_draft, sp.ngram_max, sp.ngram_min, sp.min_draft)
    assert want == conts
    if not kw.get("share_prefix"):                                    # a pass with unequal m_s and an m_s = 0 row, a full run, a partial one, an all-zero iteration
        assert schedule_kinds(schedule) == {"step", "unequal", "full", "partial"}, schedule
    plain = BatchedEngine(model, num_pages=64, **kw).generate(prompts, n)
    eng = BatchedEngine(model, num_pages=64, speculative=sp, **kw)
    got = eng.generate(prompts, n)
    assert got == plain == conts, (name, kw)
    assert eng.spec_stats == sb.stats_of(schedule), (name, kw, schedule)
    assert (eng.shared_pages > 0) == bool(kw.get("share_prefix"))
    assert eng.pool.get_num_free_pages() == eng.pool.size()           # the pages taken for rejected rows came back too


# ------------------------------------------------------------------ 6. the untouched plain path
def test_plain_generation_is_the_same_before_and_after_a_speculative_one(golden_dir):
    from proxy_inference_engine_amd import SpeculativeParams
    from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine
    name = "tiny_llama_w4_bf16"
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    prompts, conts, _, n = e2e_case(golden_dir, name, False)

    def plain():
        eng = BatchedEngine(model, num_pages=64, max_batch=4)
        out = eng.generate(prompts, 24)
        return out, model.batch_graph_launches()

    out0, launches0 = plain()
    eng = BatchedEngine(model, num_pages=64, max_batch=4, speculative=SpeculativeParams(**SP_KW))
    spec = eng.generate(prompts, 24)
    assert eng.spec_stats["passes"] >= 1
    out1, launches1 = plain()
    assert launches0 > 0 and launches1 == launches0                    # the captured step's kernel count
    assert out1 == out0 == spec == [c[:24] for c in conts]
