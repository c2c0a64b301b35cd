"""Batched speculation on int8 KV pages: the MFMA verify attention against float64 on the dequantised codes, one query row
at a time; Model.spec_step_batch(int8_pages=True) against the oracle's quantiser and against plain steps on a twin int8 pool;
BatchedEngine(kv_dtype=torch.int8, speculative=SpeculativeParams(int8_pages=True)) against the same engine without speculation."""
import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests import spec_batch_reference as sb
from tests._util import assert_dot_close, assert_vec_close, marker_rows, page_run_markers, sdpa_f64, to_bits, to_dev
from tests.test_gpu_spec_batch import BATCH_SEEDS, COUNTS, FURTHER, OFFSET5_SEEDS, OFFSETS, PLAIN_SEEDS, SP_KW
from tests.test_gpu_speculative import MODELS, SENT, STEP_SEEDS, dev_ids, e2e_prompt, load_tiny

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ 1. the kernel against float64, one query row at a time
HKV, MAX_BLOCKS, N_PAGES = 2, 8, 40
SEG_ROWS = (1, 2, 8)                                                   # three sequences, and an idle slot behind them
FIRST_CTX = [(300, 31, 1), (32, 200, 33), (63, 64, 65)]                # first-row contexts: key-block, page and split edges; 8 active splits at 300
MAX_FRAC = 0.03                                                        # the int8 decode-attention test's share (measured: DESIGN.md 26)


def i8_case(rng, D, rep, dt, first, *, seg_rows=SEG_ROWS, hkv=HKV, max_blocks=MAX_BLOCKS, n_pages=N_PAGES, splits=None, details=None, page_bytes=None):
    """(q, slab bytes, tables, row_seq, row_ctx, seg_first, want): shuffled pages, a distinct fp16 K and V scale per (page, head) over four
    octaves (drawn with repeats once the pool has more than 240 of them); unreferenced pages hold code -128 under NaN scales, positions
    behind a context -128; the K codes of every later draft row align with the query of the row before it under a loud V, so a row that
    sees its successor fails.
    splits (the long cases, tests/page_attn_long_cases.py): attn_case's long markers in codes (i8_markers), on pages whose K scale is lifted
    to 1/64 and more, where the aligned codes do not clip.  details: a list that receives every segment's (k, v, c0, rows, markers, pages)."""
    from proxy_inference_engine_amd import _ffi
    Hq, pb = hkv * rep, page_bytes or int(_ffi.load().pie_page_i8_bytes(hkv, D))
    seg_first, row_seq, row_ctx = sb.form_rows([c - 1 for c in first], [r - 1 for r in seg_rows])
    seg_first, N = seg_first + [seg_first[-1]], seg_first[-1]
    q = po.round_T(rng.standard_normal((N, Hq, D), dtype=np.float32), dt)
    draw = (lambda: rng.permutation(240)[:n_pages * hkv].reshape(n_pages, hkv)) if n_pages * hkv <= 240 else (lambda: rng.integers(0, 240, (n_pages, hkv)))
    ksc, vsc = ((unit * (16 + draw())).astype(np.float16) for unit in (2.0 ** -12, 2.0 ** -11))   # 1/256 .. 1/16, 1/128 .. 1/8
    codes = np.full((n_pages, 2, hkv, 64, D), -128, np.int8)
    scales = np.full((n_pages, 2, hkv), np.nan, np.float16)
    pages, at = rng.permutation(n_pages), 0
    tables = np.full((len(seg_rows) + 1, max_blocks), pages[-1], np.int32)   # behind a sequence's pages: an unreferenced one
    want = np.zeros((N, Hq, D), np.float64)
    for s, (c0, rows) in enumerate(zip(first, seg_rows)):
        T = c0 + rows - 1
        nb = (T + 63) // 64
        mine = pages[at:at + nb]
        at += nb
        tables[s, :nb] = mine
        marks = [m for m in sorted(set(marker_rows(T, [(T, splits)]) + page_run_markers(T, splits) + [c0 - 1])) if m < c0] if splits else []
        lift_k_scales(ksc, mine[sorted({m // 64 for m in marks + list(range(c0, T))})] if splits else [])
        scales[mine, 0], scales[mine, 1] = ksc[mine], vsc[mine]
        sd = np.sign(rng.standard_normal((hkv, 1, D)))                 # V: one sign per dim, so no mixture of rows cancels
        k8 = np.clip(np.rint(rng.standard_normal((hkv, nb * 64, D)) * 40), -127, 127)
        v8 = np.clip(np.rint(sd * (50 + 25 * rng.standard_normal((hkv, nb * 64, D)))), -127, 127)
        for i, p in enumerate(range(c0, T)):                           # position c0 + i is the first one row i must not see
            for g in range(hkv):
                qh = q[seg_first[s] + i, g * rep + i % rep].astype(np.float64)
                k8[g, p] = np.clip(np.rint((np.log(T) + 6) * np.sqrt(D) / (qh @ qh) * qh / np.float64(ksc[mine[p // 64], g])), -127, 127)
                v8[g, p] = -127 * sd[g, 0]
        i8_markers(k8, v8, q[seg_first[s]:seg_first[s] + rows], marks, c0, T, rep, ksc[mine], sd)
        k8[:, T:], v8[:, T:] = -128, -128
        codes[mine, 0] = k8.reshape(hkv, nb, 64, D).transpose(1, 0, 2, 3).astype(np.int8)
        codes[mine, 1] = v8.reshape(hkv, nb, 64, D).transpose(1, 0, 2, 3).astype(np.int8)
        per_pos = np.repeat(mine, 64)[:T]
        k = po.kv_i8_dequantize(k8[:, :T].transpose(1, 0, 2), ksc[per_pos]).transpose(1, 0, 2)   # the codes actually in the pages
        v = po.kv_i8_dequantize(v8[:, :T].transpose(1, 0, 2), vsc[per_pos]).transpose(1, 0, 2)
        for i in range(rows):
            want[seg_first[s] + i] = sdpa_f64(q[seg_first[s] + i][:, None], k, v, 1.0 / np.sqrt(D), c0 + i)[:, 0]
        if details is not None:
            details.append((k, v, c0, rows, marks, (k8[:, :T], v8[:, :T], ksc[mine], vsc[mine])))
    slab = np.zeros((n_pages, pb), np.uint8)
    slab[:, :2 * hkv * 64 * D] = codes.reshape(n_pages, -1).view(np.uint8)
    slab[:, 2 * hkv * 64 * D:2 * hkv * 64 * D + 4 * hkv] = scales.reshape(n_pages, -1).view(np.uint8)
    return q, slab, tables, row_seq, row_ctx, seg_first, want


def lift_k_scales(ksc, page_ids):
    """The K scales of the pages that hold a long case's markers: 1/32 + a quarter of the drawn one (exact in fp16, still distinct), so
    that codes aligned with a query reach a score of ln T without clipping at 127."""
    if len(page_ids):
        ksc[page_ids] = (np.float32(2.0 ** -5) + ksc[page_ids].astype(np.float32) / 4).astype(np.float16)


def i8_markers(k8, v8, q, marks, c0, T, rep, ksc, sd, bump=1.0, own_bump=2.0):
    """needle_markers of tests/test_gpu_spec_batch.py in codes, under each page's scale: marker i's K codes aligned with the query of row
    (i // rep) % rows, head i % rep, scored ~ln T + bump, its V codes 60 .. 117 of the dims' signs, -127 (against the sign) in dim 7 i % D; once there are
    markers, position c0 + j (its V stays -127) is aligned with row j's query (ln T + own_bump) and with row j + 1's, whose own it is."""
    hkv, _, D = k8.shape

    def aligned(row, g, i, b):
        qh = q[row, g * rep + i % rep].astype(np.float64)
        return (np.log(T) + b) * np.sqrt(D) / (qh @ qh) * qh

    for i, p in enumerate(marks + (list(range(c0, T)) if marks else [])):
        for g in range(hkv):
            kp = aligned((i // rep) % q.shape[0], g, i, bump) if p < c0 else aligned(p - c0, g, i, own_bump) + aligned(p - c0 + 1, g, i + 1, bump)
            k8[g, p] = np.clip(np.rint(kp / np.float64(ksc[p // 64, g])), -127, 127)
            if p < c0:
                v8[g, p] = (60 + 3 * (i % 20)) * sd[g, 0]
                v8[g, p, 7 * i % D] = -127 * sd[g, 0, 7 * i % D]


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("rep", [1, 4, 5, 8])                          # 8-row segments: C = 8, 32, 40, 64 columns
@pytest.mark.parametrize("D", [64, 128])
def test_paged_attn_verify_i8_equals_float64_row_by_row(D, rep, dt):
    from proxy_inference_engine_amd import hip_ops
    assert hip_ops.paged_attn_verify_i8_splits(len(SEG_ROWS) + 1, HKV, MAX_BLOCKS) == MAX_BLOCKS
    rng = np.random.default_rng(D * 100 + rep * 10 + len(dt))
    dev = lambda x: torch.from_numpy(np.asarray(x, np.int32)).cuda()   # noqa: E731
    fracs = []
    for first in FIRST_CTX:
        q, slab, tables, row_seq, row_ctx, seg_first, want = i8_case(rng, D, rep, dt, first)
        args = (to_dev(po.to_bits(q, dt), dt), torch.from_numpy(slab).cuda(), N_PAGES, dev(tables), dev(row_seq), dev(row_ctx), dev(seg_first), HKV, 1.0 / np.sqrt(D))
        for splits in (0, 3, 1):
            got = po.from_bits(to_bits(hip_ops.paged_attn_verify_i8(*args, splits=splits)), dt)
            assert np.isfinite(got).all(), (D, rep, dt, first, splits)
            for r in range(len(row_ctx)):
                fracs.append(assert_dot_close(got[r], po.round_T(want[r], dt), dt, max_frac=1.0, what=f"D={D} rep={rep} {dt} first={first} splits={splits} row {r}"))
    print(f"differing share D={D} rep={rep} {dt}: mean {np.mean(fracs):.4f} max {np.max(fracs):.4f}")
    assert np.max(fracs) <= MAX_FRAC, f"{np.max(fracs):.4%} of a row's elements differ (limit {MAX_FRAC:.2%})"


def test_paged_attn_verify_i8_clamps_device_indices_and_checks_arguments():
    """Context lengths beyond the table, a sequence index and page ids out of range, segments that overlap or run past N: nothing becomes
    a wild address; bad arguments are refused with paged_attn_verify's codes, and a slab below n_pages int8 pages with PIE_E_SHAPE."""
    from proxy_inference_engine_amd import _ffi, hip_ops
    D, Hq, N = 64, 4, 10
    lib = _ffi.load()
    pb = int(lib.pie_page_i8_bytes(HKV, D))
    q = torch.randn((N, Hq, D), device="cuda").to(torch.bfloat16)
    slab = torch.randint(-127, 128, (4, pb), device="cuda").to(torch.int8)
    slab[:, 2 * HKV * 64 * D:] = 0
    slab.view(torch.float16)[:, HKV * 64 * D:HKV * 64 * D + 2 * HKV] = 0.03125
    dev = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")  # noqa: E731
    tables = dev([[0, 1], [1 << 30, -5], [3, 2]])
    out = hip_ops.paged_attn_verify_i8(q, slab, 4, tables, dev([0, 7, -3, 1, 1, 1, 2, 2, 2, 2]), dev([1 << 30, -9, 5, 100, 129, 1 << 20, 0, 1, 2, 3]),
                                       dev([0, 3, -2, 99]), HKV, 0.125)
    torch.cuda.synchronize()
    assert out.shape == q.shape
    good = (dev([0] * N), dev([1] * N), dev([0, 1, 2, N]))
    with pytest.raises(ValueError, match="splits"):
        hip_ops.paged_attn_verify_i8(q, slab, 4, tables, *good, HKV, 0.125, splits=33)
    with pytest.raises(ValueError, match="smaller than n_pages int8 pages"):
        hip_ops.paged_attn_verify_i8(q, slab, 5, tables, *good, HKV, 0.125)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    call = lambda q_p, D_=D, Hkv=HKV: lib.pie_paged_attn_verify_i8(q_p, _ffi.p(slab), 4, slab.numel(), _ffi.p(tables), 2, _ffi.p(good[0]), _ffi.p(good[1]),   # noqa: E731
                                                                   _ffi.p(good[2]), N, 3, Hq, Hkv, D_, 0.125, _ffi.PIE_BF16, 0, _ffi.p(out), _ffi.p(ws), _ffi.stream())
    assert call(None) == -1 and call(_ffi.p(q), 96) == -2 and call(_ffi.p(q), D, 3) == -2 and call(_ffi.C.c_void_p(q.data_ptr() + 2)) == -3


# ------------------------------------------------------------------ 2. the pass on the tiny golden models, int8 pools
def amax_scales(model, prompts, steps):
    """(k, v) float16 [n_layers, n_kv_heads]: amax * 1.25 / 127 of the K / V rows of a T-page run of the prompts and `steps` greedy steps."""
    model.enable_paged_kv(num_pages=64)
    caches = [model.make_cache() for _ in prompts]
    tok = model.prefill_batch([[int(t) for t in p] for p in prompts], caches)[0].clone()
    for _ in range(steps):
        tok = model.step_batch(tok, caches, graph=False)[0].clone()
    amax = np.stack([np.stack([np.max([np.abs(c[l].state[w].float().cpu().numpy()).max(axis=(0, 2, 3)) for c in caches], axis=0) for l in range(len(model.layers))])
                     for w in range(2)])
    for c in caches:
        c[0].page_manager.release()
    return tuple(torch.from_numpy((amax[w] * 1.25 / 127).astype(np.float16)) for w in range(2))


@pytest.mark.parametrize("name", list(MODELS))
def test_spec_step_batch_on_int8_pages_ends_where_plain_int8_steps_would(golden_dir, name):
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    V, Hkv = cfg["vocab_size"], cfg["num_key_value_heads"]
    seeds = [OFFSET5_SEEDS[name]] + [STEP_SEEDS[(name, o)] for o in OFFSETS[1:]]
    prompts = [[int(t) for t in np.random.default_rng(1000 * o + sd).integers(0, V, o)] for o, sd in zip(OFFSETS, seeds)]
    ks, vs = amax_scales(model, prompts, 8 + FURTHER)
    try:
        pool = model.enable_paged_kv(num_pages=32, kv_dtype=torch.int8, kv_scales=(ks, vs))
        twin = [model.make_cache() for _ in prompts]                   # plain steps on a twin of every sequence: tokens and logits
        tok = model.prefill_batch(prompts, twin)[0].clone()
        plain, plain_logits = [tok.tolist()], []
        for _ in range(8 + FURTHER):
            tok, _, lg = model.step_batch(tok, twin, graph=False)
            tok = tok.clone()
            plain.append(tok.tolist()), plain_logits.append(lg.float().cpu().numpy().copy())
        plain = np.asarray(plain).T                                    # [sequence, position]: plain[s, i] is fed at offset + i
        for corrupt in (2, None):
            caches = [model.make_cache() for _ in prompts]
            first = model.prefill_batch(prompts, caches)[0].clone()
            assert first.tolist() == plain[:, 0].tolist()
            drafts, n_acc = torch.full((3, 7), SENT, dtype=torch.int32, device="cuda"), []
            for s, m in enumerate(COUNTS):
                d = plain[s, 1:m + 1].tolist()
                if corrupt is not None and corrupt < m:
                    d[corrupt] = (d[corrupt] + 1) % V
                drafts[s, :m] = dev_ids(d) if m else drafts[s, :0]
                n_acc.append(m if corrupt is None or corrupt >= m else corrupt)
            with pytest.raises(ValueError, match="not available on int8 KV pages"):
                model.spec_step_batch(first, caches, drafts, list(COUNTS))
            n, toks, _ = model.spec_step_batch(first, caches, drafts, list(COUNTS), int8_pages=True)
            assert n == [a + 1 for a in n_acc] and [c[0].offset for c in caches] == [o + k for o, k in zip(OFFSETS, n)], (name, corrupt, n)
            for s, m in enumerate(COUNTS):
                assert toks[s] == plain[s, 1:n[s] + 1].tolist(), (name, corrupt, s)
                # layer 0 of every row the pass wrote, rejected ones included: the oracle's rows under the oracle's quantiser, bit for bit
                fed = prompts[s] + [int(first[s])] + drafts[s, :m].tolist()
                oc = [po.OracleKVCache() for _ in orc.layers]
                orc.forward(np.asarray(fed), oc, last_only=True)
                ids = caches[s][0].page_manager.pages
                for p in range(OFFSETS[s], OFFSETS[s] + 1 + m):
                    page = pool.get_page(int(ids[p // 64]))
                    assert np.array_equal(page.key_cache()[p % 64].cpu().numpy(), po.kv_i8_quantize(oc[0].keys[0, :, p], ks[0].numpy())), (name, s, p)
                    assert np.array_equal(page.value_cache()[p % 64].cpu().numpy(), po.kv_i8_quantize(oc[0].values[0, :, p], vs[0].numpy())), (name, s, p)
            tok = dev_ids([t[-1] for t in toks])
            for k in range(FURTHER):                                   # plain steps right after: nothing reads the rejected rows
                tok, _, logits = model.step_batch(tok, caches, graph=False)
                tok = tok.clone()
                for s in range(3):
                    i = n_acc[s] + 1 + k
                    assert_vec_close(logits[s].float().cpu().numpy(), plain_logits[i][s], dt, c_max=24.0, c_rms=16.0, what=f"{name} corrupt={corrupt} seq {s} step {k}")
                    assert int(tok[s]) == plain[s, i + 1], (name, corrupt, s, k)
            for c in caches:
                c[0].page_manager.release()
    finally:
        model.enable_paged_kv(num_pages=8)                             # back to T pages


@pytest.mark.parametrize("name", list(MODELS))
def test_engine_on_int8_pages_generates_the_tokens_of_the_plain_int8_engine(golden_dir, name):
    from proxy_inference_engine_amd import SpeculativeParams
    from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine, SamplingParams
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    V, n = cfg["vocab_size"], 48
    prompts = ([[int(t) for t in e2e_prompt(sd, V)] for sd in BATCH_SEEDS[name]] + [[int(t) for t in np.random.default_rng(777000 + PLAIN_SEEDS[name]).integers(0, V, 24)]])[-3:]
    kw = dict(num_pages=64, max_batch=2, kv_dtype=torch.int8, kv_scales=amax_scales(model, prompts, n))
    try:
        plain = BatchedEngine(model, **kw).generate(prompts, n)
        with pytest.raises(ValueError, match="int8 KV pages"):
            BatchedEngine(model, speculative=SpeculativeParams(**SP_KW), **kw)
        eng = BatchedEngine(model, speculative=SpeculativeParams(int8_pages=True, **SP_KW), **kw)
        assert eng.generate(prompts, n) == plain and eng.spec_stats["accepted"] > 0, (name, eng.spec_stats)
        assert eng.pool.get_num_free_pages() == eng.pool.size()
        assert BatchedEngine(model, **kw).generate(prompts, n) == plain   # the plain int8 path, before and after a speculative run
        sampled = SamplingParams(temp=0.8, top_p=0.9, seed=1234)
        want = BatchedEngine(model, **kw).generate(prompts, n, sampling=sampled)
        tail = BatchedEngine(model, speculative=SpeculativeParams(int8_pages=True, batch_tail=True, **SP_KW), **kw)
        assert tail.generate(prompts, n, sampling=sampled) == want and tail.spec_stats["passes"] >= 1, (name, tail.spec_stats)
    finally:
        model.enable_paged_kv(num_pages=8)
