"""Batched speculation on 16-bit pages through the MFMA verify attention: the kernel against float64, one query row at a
time, on the VALU kernel's cases; its clamps and refusals; Model.spec_step_batch[_tail](mfma_verify=True) against the pass without the
flag on twin caches; BatchedEngine(speculative=SpeculativeParams(mfma_verify=True)) against the engine without speculation."""
import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests._util import assert_dot_close, assert_vec_close, to_bits, to_dev
from tests.test_gpu_spec_batch import (BATCH_SEEDS, COUNTS, FIRST_CTX, FURTHER, HKV, MAX_BLOCKS, N_PAGES, OFFSET5_SEEDS, OFFSETS, PLAIN_SEEDS, SEG_ROWS, SP_KW,
                                       attn_case, private_pool)
from tests.test_gpu_spec_batch_tail import arm, disarm, prefilled, release, seat
from tests.test_gpu_speculative import MODELS, SENT, STEP_SEEDS, dev_ids, e2e_prompt, load_tiny

pytestmark = pytest.mark.gpu
MAX_FRAC = 0.02                                                        # assert_dot_close's default, the VALU kernel's limit on these cases


# ------------------------------------------------------------------ 1. the kernel against float64, one query row at a time
@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("rep", [1, 4, 5, 8])                          # 8-row segments: C = 8, 32, 40, 64 columns
@pytest.mark.parametrize("D", [64, 128])
def test_paged_attn_verify_mfma_equals_float64_row_by_row(D, rep, dt):
    from proxy_inference_engine_amd import hip_ops
    auto = hip_ops.paged_attn_verify_mfma_splits(len(SEG_ROWS) + 1, HKV, MAX_BLOCKS)
    assert auto == MAX_BLOCKS                                          # 307 attended positions in 8 splits: every split is active in the 300 case
    rng = np.random.default_rng(D * 100 + rep * 10 + len(dt))
    dev = lambda x: torch.from_numpy(np.asarray(x, np.int32)).cuda()   # noqa: E731
    fracs = []
    for first in FIRST_CTX:
        for splits in (0, 1, 3):
            q, pool, tables, row_seq, row_ctx, seg_first, want = attn_case(rng, D, rep, dt, first, splits or auto)
            out = hip_ops.paged_attn_verify_mfma(to_dev(po.to_bits(q, dt), dt), to_dev(po.to_bits(pool, dt), dt), N_PAGES, dev(tables), dev(row_seq), dev(row_ctx),
                                                 dev(seg_first), HKV, 1.0 / np.sqrt(D), splits=splits)
            got = po.from_bits(to_bits(out), dt)
            assert np.isfinite(got).all(), (D, rep, dt, first, splits)
            for r in range(len(row_ctx)):
                fracs.append(assert_dot_close(got[r], po.round_T(want[r], dt), dt, max_frac=1.0, what=f"D={D} rep={rep} {dt} first={first} splits={splits} row {r} (ctx {row_ctx[r]})"))
    print(f"differing share D={D} rep={rep} {dt}: mean {np.mean(fracs):.4f} max {np.max(fracs):.4f}")
    assert np.max(fracs) <= MAX_FRAC, f"{np.max(fracs):.4%} of a row's elements differ (limit {MAX_FRAC:.2%})"


# ------------------------------------------------------------------ 2. clamps and refusals
def test_paged_attn_verify_mfma_clamps_device_indices_and_checks_arguments():
    """The inputs of test_paged_attn_verify_clamps_device_indices_and_checks_arguments: nothing becomes a wild address, the launch completes;
    bad arguments are refused with pie_paged_attn_verify's codes."""
    from proxy_inference_engine_amd import _ffi, hip_ops
    D, Hq, N = 64, 4, 10
    q = torch.randn((N, Hq, D), device="cuda").to(torch.bfloat16)
    slab = torch.randn((4, 2, HKV, 64, D), device="cuda").to(torch.bfloat16)
    dev = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")  # noqa: E731
    tables = dev([[0, 1], [1 << 30, -5], [3, 2]])
    out = hip_ops.paged_attn_verify_mfma(q, slab, 4, tables, dev([0, 7, -3, 1, 1, 1, 2, 2, 2, 2]), dev([1 << 30, -9, 5, 100, 129, 1 << 20, 0, 1, 2, 3]),
                                         dev([0, 3, -2, 99]), HKV, 0.125)
    torch.cuda.synchronize()
    assert out.shape == q.shape
    good = (dev([0] * N), dev([1] * N), dev([0, 1, 2, N]))
    with pytest.raises(ValueError, match="splits"):
        hip_ops.paged_attn_verify_mfma(q, slab, 4, tables, *good, HKV, 0.125, splits=33)
    lib = _ffi.load()
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    call = lambda q_p, D_=D, Hkv=HKV: lib.pie_paged_attn_verify_mfma(q_p, _ffi.p(slab), 4, _ffi.p(tables), 2, _ffi.p(good[0]), _ffi.p(good[1]), _ffi.p(good[2]), N, 3, Hq,   # noqa: E731
                                                                     Hkv, D_, 0.125, _ffi.PIE_BF16, 0, _ffi.p(out), _ffi.p(ws), _ffi.stream())
    assert call(None) == -1 and call(_ffi.p(q), 96) == -2 and call(_ffi.p(q), D, 3) == -2 and call(_ffi.C.c_void_p(q.data_ptr() + 2)) == -3
    assert b"pie_paged_attn_verify_mfma" in lib.pie_last_error()


# ------------------------------------------------------------------ 3. the pass on the tiny golden models, against the pass without the flag
def spec_prompts(name, V):
    seeds = [OFFSET5_SEEDS[name]] + [STEP_SEEDS[(name, o)] for o in OFFSETS[1:]]
    return [[int(t) for t in np.random.default_rng(1000 * o + sd).integers(0, V, o)] for o, sd in zip(OFFSETS, seeds)]


@pytest.mark.parametrize("name", list(MODELS))
def test_spec_step_batch_with_the_flag_ends_where_the_pass_without_it_does(golden_dir, name):
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    V, prompts = cfg["vocab_size"], spec_prompts(name, cfg["vocab_size"])
    pool = private_pool(model, 40)
    twin, first = prefilled(model, pool, prompts)                      # plain greedy steps: the tokens every pass must end on
    plain, tok = [first], dev_ids(first)
    for _ in range(8 + FURTHER):
        tok = model.step_batch(tok, twin)[0].clone()
        plain.append(tok.tolist())
    plain = np.asarray(plain).T                                        # [sequence, position]
    release(twin)
    for corrupt in (2, None):
        drafts, n_acc = torch.full((3, 7), SENT, dtype=torch.int32, device="cuda"), []
        for s, m in enumerate(COUNTS):
            d = plain[s, 1:m + 1].tolist()
            if corrupt is not None and corrupt < m:
                d[corrupt] = (d[corrupt] + 1) % V
            drafts[s, :m] = dev_ids(d) if m else drafts[s, :0]
            n_acc.append(m if corrupt is None or corrupt >= m else corrupt)
        runs = {}
        for flag in (False, True):
            caches, first_b = prefilled(model, pool, prompts)
            assert first_b == first
            n, toks, _ = model.spec_step_batch(dev_ids(first), caches, drafts, list(COUNTS), mfma_verify=flag)
            assert n == [a + 1 for a in n_acc] and [c[0].offset for c in caches] == [o + k for o, k in zip(OFFSETS, n)], (name, corrupt, flag, n)
            assert toks == [plain[s, 1:n[s] + 1].tolist() for s in range(3)], (name, corrupt, flag)
            tok, logits = dev_ids([t[-1] for t in toks]), []
            for k in range(FURTHER):                                   # plain steps right after: nothing reads the rejected rows
                tok, _, lg = model.step_batch(tok, caches)
                tok = tok.clone()
                assert tok.tolist() == [plain[s, n_acc[s] + 2 + k] for s in range(3)], (name, corrupt, flag, k)
                logits.append(lg.float().cpu().numpy().copy())
            runs[flag] = logits
            release(caches)
        for k in range(FURTHER):
            for s in range(3):
                assert_vec_close(runs[True][k][s], runs[False][k][s], dt, what=f"{name} corrupt={corrupt} seq {s} step {k}")
    assert pool.get_num_free_pages() == pool.size()


def test_spec_step_batch_tail_with_the_flag_draws_the_tokens_of_the_pass_without_it(golden_dir):
    name = "tiny_llama_w4_bf16"
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    V, prompts = cfg["vocab_size"], spec_prompts(name, cfg["vocab_size"])
    seats = [seat(("top_p", 0.8, 0.9, 0), seed=2024 + s, calls=3 * s) for s in range(3)]
    pool = private_pool(model, 24)
    drafts = torch.zeros((3, 7), dtype=torch.int32, device="cuda")

    def run(flag):
        caches, first = prefilled(model, pool, prompts)
        arm(model, seats, prompts)                                     # (every run from the same records, rings and stream positions)
        try:
            n, toks, _ = model.spec_step_batch_tail(dev_ids(first), caches, drafts, list(COUNTS), mfma_verify=flag)
            return n, toks, [c[0].offset for c in caches]
        finally:
            disarm(model), release(caches)

    for j in range(max(COUNTS)):                                       # row j's draw depends on the drafts before it only: round j settles draft j
        toks = run(False)[1]
        for s, m in enumerate(COUNTS):
            if j < m:
                drafts[s, j] = toks[s][j]
    drafts[2, 4] = (int(drafts[2, 4]) + 1) % V                         # seat 2: rejected in the middle; seat 1: all accepted
    want = run(False)
    assert want[0] == [1, 4, 5]
    assert run(True) == want


# ------------------------------------------------------------------ 4. the engine
@pytest.mark.parametrize("name", list(MODELS))
def test_engine_with_the_flag_generates_the_tokens_of_the_plain_engine(golden_dir, name):
    from proxy_inference_engine_amd import SpeculativeParams
    from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    V, n = cfg["vocab_size"], 48
    prompts = ([[int(t) for t in e2e_prompt(sd, V)] for sd in BATCH_SEEDS[name]] + [[int(t) for t in np.random.default_rng(777000 + PLAIN_SEEDS[name]).integers(0, V, 24)]])[-3:]
    kw = dict(num_pages=64, max_batch=2)
    plain = BatchedEngine(model, **kw).generate(prompts, n)
    eng = BatchedEngine(model, speculative=SpeculativeParams(mfma_verify=True, **SP_KW), **kw)
    assert eng.generate(prompts, n) == plain and eng.spec_stats["accepted"] > 0, (name, eng.spec_stats)
    assert eng.pool.get_num_free_pages() == eng.pool.size()
    assert BatchedEngine(model, **kw).generate(prompts, n) == plain   # the plain path, before and after
