"""Chunked prefill and shared prefixes on int8 KV pages: the kernel against float64; the pass and the engine against one token per step."""
import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests._util import EPS, assert_dot_close, assert_vec_close, marker_rows, page_run_markers, sdpa_f64, to_bits, to_dev
from tests.test_gpu_spec_batch_i8 import amax_scales, i8_markers, lift_k_scales
from tests.test_gpu_speculative import MODELS, dev_ids, e2e_prompt, load_tiny

pytestmark = pytest.mark.gpu

HKV = 2
PAIRS = [(1, 64), (31, 1), (33, 63), (70, 100), (64, 200)]   # (rows, cached): tile edges at 32 / 64 rows, offsets at key-block and page edges
MAX_FRAC = 0.03                                               # the int8 decode-attention test's share (measured: DESIGN.md 27)


def chunk_case(rng, D, rep, dt, pairs, *, hkv=HKV, long=False, details=None, page_bytes=None):
    """(q, slab, tables, chunks, want), built as i8_case of test_gpu_spec_batch_i8 builds its data (a row that sees its successor fails).
    Row 0 of the batch belongs to no chunk.  long (tests/page_attn_long_cases.py): i8_case's long markers among the cached positions, as
    for 32 splits of them; details: a list that receives every chunk's (k, v, P, M, markers, (K codes, V codes, K scales, V scales))."""
    from proxy_inference_engine_amd import _ffi
    Hq, pb = hkv * rep, page_bytes or int(_ffi.load().pie_page_i8_bytes(hkv, D))
    blocks = [(m + p + 63) // 64 for m, p in pairs]
    n_pages, mb, N = sum(blocks) + 3, max(blocks), 1 + sum(m for m, _ in pairs)
    q = po.round_T(rng.standard_normal((N, Hq, D), dtype=np.float32), dt)
    ksc, vsc = ((unit * (16 + rng.integers(0, 240, (n_pages, hkv)))).astype(np.float16) for unit in (2.0 ** -12, 2.0 ** -11))   # 1/256 .. 1/16, 1/128 .. 1/8
    codes = np.full((n_pages, 2, hkv, 64, D), -128, np.int8)
    scales = np.full((n_pages, 2, hkv), np.nan, np.float16)
    pages, at, first = rng.permutation(n_pages), 0, 1
    tables = np.full((len(pairs), mb), pages[-1], np.int32)            # behind a sequence's pages: an unreferenced one
    want, chunks = np.zeros((N, Hq, D), np.float64), []
    for s, ((M, P), nb) in enumerate(zip(pairs, blocks)):
        T = P + M
        mine, at = pages[at:at + nb], at + nb
        tables[s, :nb] = mine
        marks = sorted(set(marker_rows(P + 1, [(P + 1, 32)]) + page_run_markers(P + 1, 32))) if long else []
        lift_k_scales(ksc, mine[sorted({m // 64 for m in marks + list(range(P + 1, T))})] if long else [])
        scales[mine, 0], scales[mine, 1] = ksc[mine], vsc[mine]
        sd = np.sign(rng.standard_normal((hkv, 1, D)))                 # V: one sign per dim
        k8 = np.clip(np.rint(rng.standard_normal((hkv, nb * 64, D)) * 40), -127, 127)
        v8 = np.clip(np.rint(sd * (50 + 25 * rng.standard_normal((hkv, nb * 64, D)))), -127, 127)
        for i, p in enumerate(range(P + 1, T)):                        # position P + 1 + i is the first one row i must not see
            for g in range(hkv):
                qh = q[first + i, g * rep + i % rep].astype(np.float64)
                k8[g, p] = np.clip(np.rint((np.log(T) + 6) * np.sqrt(D) / (qh @ qh) * qh / np.float64(ksc[mine[p // 64], g])), -127, 127)
                v8[g, p] = -127 * sd[g, 0]
        i8_markers(k8, v8, q[first:first + M], marks, P + 1, T, rep, ksc[mine], sd)
        k8[:, T:], v8[:, T:] = -128, -128
        codes[mine, 0] = k8.reshape(hkv, nb, 64, D).transpose(1, 0, 2, 3).astype(np.int8)
        codes[mine, 1] = v8.reshape(hkv, nb, 64, D).transpose(1, 0, 2, 3).astype(np.int8)
        per_pos = np.repeat(mine, 64)[:T]
        k = po.kv_i8_dequantize(k8[:, :T].transpose(1, 0, 2), ksc[per_pos]).transpose(1, 0, 2)   # the codes actually in the pages
        v = po.kv_i8_dequantize(v8[:, :T].transpose(1, 0, 2), vsc[per_pos]).transpose(1, 0, 2)
        for i in range(M):
            want[first + i] = sdpa_f64(q[first + i][:, None], k, v, 1.0 / np.sqrt(D), P + i + 1)[:, 0]
        if details is not None:
            details.append((k, v, P, M, marks, (k8[:, :T], v8[:, :T], ksc[mine], vsc[mine])))
        chunks, first = chunks + [[first, M, P, s]], first + M
    slab = np.zeros((n_pages, pb), np.uint8)
    slab[:, :2 * hkv * 64 * D] = codes.reshape(n_pages, -1).view(np.uint8)
    slab[:, 2 * hkv * 64 * D:2 * hkv * 64 * D + 4 * hkv] = scales.reshape(n_pages, -1).view(np.uint8)
    return q, slab, tables, chunks, want


def run_case(D, rep, dt, pairs, seed):
    """ONE call for all chunks; every chunk row against float64 -> the rows' differing shares."""
    from proxy_inference_engine_amd import hip_ops
    q, slab, tables, chunks, want = chunk_case(np.random.default_rng(seed), D, rep, dt, pairs)
    got = po.from_bits(to_bits(hip_ops.prefill_attn_i8(to_dev(po.to_bits(q, dt), dt), torch.from_numpy(slab).cuda(), len(slab), torch.from_numpy(tables).cuda(),
                                                       chunks, HKV, 1.0 / np.sqrt(D))), dt)
    assert np.isfinite(got).all() and not got[0].any(), (D, rep, dt)   # (row 0 is outside every chunk: left zero)
    return [assert_dot_close(got[r], po.round_T(want[r], dt), dt, max_frac=1.0, what=f"D={D} rep={rep} {dt} row {r}") for r in range(1, len(q))]


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("rep", [1, 4, 5, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_prefill_attn_i8_equals_float64_row_by_row(knobs, D, rep, dt):
    fracs = run_case(D, rep, dt, PAIRS, D * 100 + rep * 10 + len(dt))
    if rep <= 4:                                                       # the form of two 32-row tiles per workgroup, which these sizes do not pick
        knobs("prefill_qt", 2)
        fracs += run_case(D, rep, dt, PAIRS, D * 100 + rep * 10 + len(dt) + 1)
    print(f"differing share D={D} rep={rep} {dt}: mean {np.mean(fracs):.4f} max {np.max(fracs):.4f}")
    assert np.max(fracs) <= MAX_FRAC, f"{np.max(fracs):.4%} of a row's elements differ (limit {MAX_FRAC:.2%})"


def test_prefill_attn_i8_takes_more_chunks_than_one_launch_holds():
    assert np.max(run_case(128, 4, "bfloat16", [(1, 1 + 5 * j) for j in range(33)], 33)) <= MAX_FRAC


def test_prefill_attn_i8_clamps_page_ids_and_refuses_bad_chunks_and_arguments():
    """Page ids out of range are clamped; a chunk outside the batch, its block table or the tables' sequences is refused by name."""
    from proxy_inference_engine_amd import _ffi, hip_ops
    D, Hq, N = 64, 4, 40
    lib = _ffi.load()
    pb, q = int(lib.pie_page_i8_bytes(HKV, D)), torch.randn((N, Hq, D), device="cuda").to(torch.bfloat16)
    slab = torch.randint(-127, 128, (4, pb), device="cuda").to(torch.int8)
    slab[:, 2 * HKV * 64 * D:] = 0
    slab.view(torch.float16)[:, HKV * 64 * D:HKV * 64 * D + 2 * HKV] = 0.03125
    tables = torch.tensor([[0, 1], [1 << 30, -5]], dtype=torch.int32, device="cuda")
    out = hip_ops.prefill_attn_i8(q, slab, 4, tables, [[0, 40, 70, 1]], HKV, 0.125)
    torch.cuda.synchronize()
    assert out.shape == q.shape and bool(torch.isfinite(out.float()).all())
    for bad in ([1, 40, 1, 0], [-1, 2, 1, 0], [0, 0, 1, 0], [0, 2, 0, 0], [0, 2, 1, 2], [0, 2, 1, -1], [0, 2, 127, 0]):
        with pytest.raises(ValueError, match="a chunk is"):
            hip_ops.prefill_attn_i8(q, slab, 4, tables, [[0, 1, 1, 0], bad], HKV, 0.125)
    with pytest.raises(ValueError, match="smaller than n_pages int8 pages"):
        hip_ops.prefill_attn_i8(q, slab, 5, tables, [[0, 1, 1, 0]], HKV, 0.125)
    ch = np.asarray([[0, 1, 1, 0]], np.int32)
    call = lambda q_p, D_=D, Hkv=HKV: lib.pie_prefill_attn_i8(q_p, _ffi.p(slab), 4, slab.numel(), _ffi.p(tables), 2, 2, ch.ctypes.data, 1, N, Hq, Hkv, D_,   # noqa: E731
                                                              _ffi.PIE_BF16, 0.125, _ffi.p(out), _ffi.stream())
    assert call(None) == -1 and call(_ffi.p(q), 96) == -2 and call(_ffi.p(q), D, 3) == -2 and call(_ffi.C.c_void_p(q.data_ptr() + 2)) == -3


# ------------------------------------------------------------------ the pass and the engine on the tiny golden models, int8 pools
BOUND, FURTHER = dict(c_max=24.0, c_rms=16.0), 4   # test_gpu_spec_batch_i8's int8-page bound for a pass against plain steps


def one_per_step(model, fresh, rest, n):
    """The twin procedure: `fresh` as a whole prompt, `rest` one token per step_batch step, then n - 1 greedy steps -> (cache, n tokens, n logits)."""
    c = model.make_cache()
    tok, _, lg = model.prefill_batch([fresh], [c])
    for t in rest:
        tok, _, lg = model.step_batch(dev_ids([t]), [c], graph=False)
    toks, lgs = [int(tok[0])], [lg[0].float().cpu().numpy().copy()]
    for _ in range(n - 1):
        tok, _, lg = model.step_batch(dev_ids(toks[-1:]), [c], graph=False)
        toks.append(int(tok[0])), lgs.append(lg[0].float().cpu().numpy().copy())
    return c, toks, lgs


@pytest.mark.parametrize("name", list(MODELS))
def test_step_mixed_on_int8_pages_ends_where_one_token_per_step_would(golden_dir, name):
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    V = cfg["vocab_size"]
    rng = np.random.default_rng(len(name))
    prompt, side, shared = ([int(t) for t in rng.integers(0, V, n)] for n in (77, 9, 64))
    tails = [[int(t) for t in rng.integers(0, V, n)] for n in (5, 37)]
    ks, vs = amax_scales(model, [prompt, side, shared + tails[0], shared + tails[1]], 1 + FURTHER)
    try:
        pool = model.enable_paged_kv(num_pages=32, kv_dtype=torch.int8, kv_scales=(ks, vs))

        def check(cache, fed, first, twin):   # layer-0 codes of the rows from `first` on against the oracle's quantiser; then greedy steps against the twin
            oc = [po.OracleKVCache() for _ in orc.layers]
            orc.forward(np.asarray(fed), oc, last_only=True)
            ids = cache[0].page_manager.pages
            for p in range(first, len(fed)):
                page = pool.get_page(int(ids[p // 64]))
                assert np.array_equal(page.key_cache()[p % 64].cpu().numpy(), po.kv_i8_quantize(oc[0].keys[0, :, p], ks[0].numpy())), (name, p)
                assert np.array_equal(page.value_cache()[p % 64].cpu().numpy(), po.kv_i8_quantize(oc[0].values[0, :, p], vs[0].numpy())), (name, p)
            tok = twin[1][0]
            for k in range(1, 1 + FURTHER):
                nxt, _, lg = model.step_batch(dev_ids([tok]), [cache], graph=False)
                assert_vec_close(lg[0].float().cpu().numpy(), twin[2][k], dt, what=f"{name} step {k}", **BOUND)
                tok = int(nxt[0])
                assert tok == twin[1][k], (name, k)

        # (a) a fresh 20-token prompt, then chunks of 50 and 7 rows, the second alongside two decode rows
        twin = one_per_step(model, prompt[:20], prompt[20:], 1 + FURTHER)
        c, d = model.make_cache(), [model.make_cache(), model.make_cache()]
        model.prefill_batch([prompt[:20]], [c])
        dtok = model.prefill_batch([side, side], d)[0].clone()
        with pytest.raises(ValueError, match="a prompt that continues a cached prefix reads T pages"):
            model.step_mixed(None, [], [prompt[20:70]], [c])
        model.step_mixed(None, [], [prompt[20:70]], [c], int8_pages=True)
        nxt, _, lg = model.step_mixed(dtok, d, [prompt[70:]], [c], int8_pages=True)
        assert nxt.shape[0] == 3 and int(nxt[2]) == twin[1][0], name
        assert_vec_close(lg[2].float().cpu().numpy(), twin[2][0], dt, what=f"{name} chunked", **BOUND)
        check(c, prompt, 20, twin)
        # (b) two suffixes behind a forked 64-token prefix page
        twins = [one_per_step(model, shared, t, 1 + FURTHER) for t in tails]
        root = model.make_cache()
        model.prefill_batch([shared], [root])
        forks = [[type(root[0])(seq, i) for i in range(len(root))] for seq in (root[0].page_manager.fork(), root[0].page_manager.fork())]
        nxt, _, lg = model.step_mixed(None, [], tails, forks, int8_pages=True)
        for s in range(2):
            assert int(nxt[s]) == twins[s][1][0], (name, s)
            assert_vec_close(lg[s].float().cpu().numpy(), twins[s][2][0], dt, what=f"{name} suffix {s}", **BOUND)
            check(forks[s], shared + tails[s], 64, twins[s])
    finally:
        model.enable_paged_kv(num_pages=8)                             # back to T pages


def test_engine_with_int8_chunks_generates_the_tokens_of_one_token_per_step(golden_dir):
    from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine
    name, n = "tiny_dense_f16_bias", 8   # (f16: the int8-page bound is 2^-11-fine, so prompts with the margin exist; none of 30 had it on the bf16 model)
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    cands = [[int(t) for t in np.tile(e2e_prompt(sd, cfg["vocab_size"]), 3)][:56] for sd in range(100, 130)]   # (18 .. 56 tokens)
    kw = dict(num_pages=64, max_batch=1, kv_dtype=torch.int8, kv_scales=amax_scales(model, cands, n))
    try:
        model.enable_paged_kv(num_pages=64, kv_dtype=torch.int8, kv_scales=kw["kv_scales"])
        prompts, want, seen = [], [], 0
        for p in cands:                                                # prompts whose twin top-2 margin exceeds the int8-page bound at every generated token
            c, toks, lgs = one_per_step(model, p[:16], p[16:], n)
            c[0].page_manager.release()
            seen += 1
            if all(np.sort(lg)[-1] - np.sort(lg)[-2] > 2 * BOUND["c_max"] * EPS[dt] * np.abs(lg).max() for lg in lgs):
                prompts.append(p), want.append(toks)
            if len(prompts) == 3:
                break
        print(f"engine prompts: {seen} candidates tried for 3 ({seen - len(prompts)} replaced)")
        assert len(prompts) == 3, f"{len(prompts)} of {seen} candidates have the margin"
        plain = BatchedEngine(model, **kw).generate(prompts, n)
        eng = BatchedEngine(model, prefill_chunk=16, int8_chunks=True, **kw)
        assert eng.prefill_chunk == 16 and eng.generate(prompts, n) == want
        assert eng.pool.get_num_free_pages() == eng.pool.size()
        assert BatchedEngine(model, **kw).generate(prompts, n) == plain   # the plain int8 path, before and after
    finally:
        model.enable_paged_kv(num_pages=8)
