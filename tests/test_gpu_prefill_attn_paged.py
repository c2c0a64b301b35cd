"""Chunked prefill and shared prefixes on 16-bit KV pages in one split-KV launch: the kernel against float64 one row at a
time, bit for bit against the per-chunk prompt attention at one split, its clamps and refusals; Model.step_mixed(batched_chunks=True)
against the pass without the flag."""
import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests._util import assert_dot_close, assert_vec_close, sdpa_f64, to_bits, to_dev
from tests.test_gpu_prefill_attn_i8 import HKV, PAIRS, chunk_case
from tests.test_gpu_spec_batch import private_pool
from tests.test_gpu_speculative import MODELS, load_tiny

pytestmark = pytest.mark.gpu
MAX_FRAC = 0.02   # assert_dot_close's default: the limit test_gpu_spec_batch_mfma.py holds the other T-page MFMA kernel to
# Two cells whose rows have 128 / 256 elements exceed it with 3 / 7 of them: there the unchanged k_prefill_attn (run_loop below, the same rows)
# shows the same 3 / 128 and 7 / 256 (measured), and the cell is allowed twice that figure
LOOP_SHOWS = {(64, 1, "float16"): 3 / 128, (128, 1, "float16"): 7 / 256}


def paged_case(rng, D, rep, dt, pairs):
    """chunk_case's chunks with T values in T pages: every chunk's K / V (its dequantised codes, rounded to T) laid into the pages its table
    names, NaN in every unreferenced page and behind a chunk's last position -> (q, pool, tables, chunks, want, per-chunk (k, v))."""
    det = []
    q, slab, tables, chunks, _ = chunk_case(rng, D, rep, dt, pairs, details=det)
    pool = np.full((len(slab), 2, HKV, 64, D), np.nan, np.float32)
    want, kvs = np.zeros(q.shape, np.float64), []
    for (first, M, P, s), (k, v, *_) in zip(chunks, det):
        k, v = po.round_T(k, dt), po.round_T(v, dt)                    # [HKV, P + M, D]
        for t in range(P + M):
            pool[tables[s, t // 64], 0, :, t % 64], pool[tables[s, t // 64], 1, :, t % 64] = k[:, t], v[:, t]
        for i in range(M):
            want[first + i] = sdpa_f64(q[first + i][:, None], k, v, 1.0 / np.sqrt(D), P + i + 1)[:, 0]
        kvs.append((k, v))
    return q, pool, tables, chunks, want, kvs


def run_paged(case, D, dt, splits):
    from proxy_inference_engine_amd import hip_ops
    q, pool, tables, chunks = case[:4]
    return hip_ops.prefill_attn_paged(to_dev(po.to_bits(q, dt), dt), to_dev(po.to_bits(pool, dt), dt), len(pool), torch.from_numpy(tables).cuda(), chunks, HKV,
                                      1.0 / np.sqrt(D), splits=splits)


def run_loop(case, D, dt):
    """The per-chunk form: pie_sdpa_prefill (k_prefill_attn) once per chunk on the chunk's K / V laid out contiguously, offset = P."""
    from proxy_inference_engine_amd import _ffi
    q, _, _, chunks, _, kvs = case
    qd = to_dev(po.to_bits(q, dt), dt)
    out = torch.zeros_like(qd)
    Hq = q.shape[1]
    for (first, M, P, _), (k, v) in zip(chunks, kvs):
        kd, vd = (to_dev(po.to_bits(x, dt), dt) for x in (k, v))
        _ffi.check(_ffi.load().pie_sdpa_prefill(qd[first:].data_ptr(), _ffi.p(kd), _ffi.p(vd), Hq, HKV, M, P, k.shape[1], D, 1.0 / np.sqrt(D),
                                                _ffi.dtype_code(qd.dtype), out[first:].data_ptr(), _ffi.stream()))
    return out


def row_fracs(out, case, dt, what):
    got, (q, want) = po.from_bits(to_bits(out), dt), (case[0], case[4])
    assert np.isfinite(got).all() and not got[0].any(), what           # (row 0 is outside every chunk: left zero)
    return [assert_dot_close(got[r], po.round_T(want[r], dt), dt, max_frac=1.0, what=f"{what} row {r}") for r in range(1, len(q))]


@pytest.mark.parametrize("splits", [1, 3])   # 3: the (31, 1) chunk has one page (two empty splits), the (64, 200) chunk five (uneven; the last holds the causal edge)
@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("rep", [1, 4, 5, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_prefill_attn_paged_equals_float64_row_by_row(knobs, D, rep, dt, splits):
    fracs = []
    for qt in ((0, 2) if rep <= 4 else (0,)):                          # 2: the form of two 32-row tiles per workgroup, which these sizes do not pick
        if qt:
            knobs("prefill_qt", qt)
        case = paged_case(np.random.default_rng(D * 100 + rep * 10 + len(dt) + qt), D, rep, dt, PAIRS)
        fracs += row_fracs(run_paged(case, D, dt, splits), case, dt, f"D={D} rep={rep} {dt} splits={splits} qt={qt}")
    print(f"differing share D={D} rep={rep} {dt} splits={splits}: mean {np.mean(fracs):.4f} max {np.max(fracs):.4f}")
    limit = 2 * LOOP_SHOWS[D, rep, dt] if (D, rep, dt) in LOOP_SHOWS else MAX_FRAC
    assert np.max(fracs) <= limit, f"{np.max(fracs):.4%} of a row's elements differ (limit {limit:.2%})"


@pytest.mark.parametrize("D,rep,dt", [(128, 4, "bfloat16"), (64, 5, "float16")])
def test_one_split_is_bit_identical_to_the_per_chunk_launches(D, rep, dt):
    case = paged_case(np.random.default_rng(7 + D), D, rep, dt, PAIRS)
    assert torch.equal(run_paged(case, D, dt, 1).view(torch.int16), run_loop(case, D, dt).view(torch.int16))


@pytest.mark.parametrize("splits", [1, 2])
def test_prefill_attn_paged_takes_more_chunks_than_one_launch_holds(splits):
    case = paged_case(np.random.default_rng(33), 128, 4, "bfloat16", [(1, 1 + 5 * j) for j in range(33)])
    assert np.max(row_fracs(run_paged(case, 128, "bfloat16", splits), case, "bfloat16", f"33 chunks splits={splits}")) <= MAX_FRAC


def test_prefill_attn_paged_clamps_page_ids_and_refuses_bad_chunks_and_arguments():
    """Page ids out of range are clamped; what pie_prefill_attn_i8 refuses is refused with its codes, and so are a short slab and splits without a workspace."""
    from proxy_inference_engine_amd import _ffi, hip_ops
    D, Hq, N = 64, 4, 40
    lib = _ffi.load()
    q = torch.randn((N, Hq, D), device="cuda").to(torch.bfloat16)
    slab = torch.randn((4, 2, HKV, 64, D), device="cuda").to(torch.bfloat16)
    tables = torch.tensor([[0, 1], [1 << 30, -5]], dtype=torch.int32, device="cuda")
    for splits in (1, 2):
        out = hip_ops.prefill_attn_paged(q, slab, 4, tables, [[0, 40, 70, 1]], HKV, 0.125, splits=splits)
        torch.cuda.synchronize()
        assert out.shape == q.shape and bool(torch.isfinite(out.float()).all())
    for bad in ([1, 40, 1, 0], [-1, 2, 1, 0], [0, 0, 1, 0], [0, 2, 0, 0], [0, 2, 1, 2], [0, 2, 1, -1], [0, 2, 127, 0]):
        with pytest.raises(ValueError, match="a chunk is"):
            hip_ops.prefill_attn_paged(q, slab, 4, tables, [[0, 1, 1, 0], bad], HKV, 0.125)
    with pytest.raises(ValueError, match="smaller than n_pages T pages"):
        hip_ops.prefill_attn_paged(q, slab, 5, tables, [[0, 1, 1, 0]], HKV, 0.125)
    ch = np.asarray([[0, 1, 1, 0]], np.int32)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    call = lambda q_p, D_=D, Hkv=HKV, splits=0, ws_p=_ffi.p(ws): lib.pie_prefill_attn_paged(   # noqa: E731
        q_p, _ffi.p(slab), 4, slab.numel() * 2, _ffi.p(tables), 2, 2, ch.ctypes.data, 1, N, Hq, Hkv, D_, _ffi.PIE_BF16, 0.125, splits, _ffi.p(out), ws_p, _ffi.stream())
    assert call(None) == -1 and call(_ffi.p(q), 96) == -2 and call(_ffi.p(q), D, 3) == -2 and call(_ffi.C.c_void_p(q.data_ptr() + 2)) == -3
    assert call(_ffi.p(q), splits=2, ws_p=None) == -1 and b"pie_prefill_attn_paged" in lib.pie_last_error()
    assert call(_ffi.p(q), splits=33) == -1 and call(_ffi.p(q)) == 0


# ------------------------------------------------------------------ the pass on the tiny golden models: the flag against no flag, same pool
def mixed_passes(model, pool, cfg, **kw):
    """A fresh 20-token prompt, then chunks of 50 and 7 rows, the second beside two decode rows and a fresh prompt; then two suffixes behind a
    forked 64-token page -> [(tokens, logits)] of the two passes that carry chunks' last rows."""
    V, rng = cfg["vocab_size"], np.random.default_rng(30)
    prompt, side, fresh, shared = ([int(t) for t in rng.integers(0, V, n)] for n in (77, 9, 11, 64))
    tails = [[int(t) for t in rng.integers(0, V, n)] for n in (5, 37)]
    new = lambda: model.make_paged_cache(pool, max_blocks=8)           # noqa: E731
    c, cf, d, root = new(), new(), [new(), new()], new()
    model.prefill_batch([prompt[:20]], [c])
    dtok = model.prefill_batch([side, side], d)[0].clone()
    model.step_mixed(None, [], [prompt[20:70]], [c], **kw)
    nxt, _, lg = model.step_mixed(dtok, d, [prompt[70:], fresh], [c, cf], **kw)   # rows: two decoding, the chunk's last, the fresh prompt's last
    outs = [(nxt.tolist(), lg.clone())]
    model.prefill_batch([shared], [root])
    forks = [[type(root[0])(seq, i) for i in range(len(root))] for seq in (root[0].page_manager.fork(), root[0].page_manager.fork())]
    nxt, _, lg = model.step_mixed(None, [], tails, forks, **kw)
    outs.append((nxt.tolist(), lg.clone()))
    for cache in [c, cf, root, *d, *forks]:
        cache[0].page_manager.release()
    return outs


@pytest.mark.parametrize("name", list(MODELS))
def test_step_mixed_with_batched_chunks_ends_where_the_pass_without_it_does(golden_dir, knobs, name):
    cfg, dt, orc, model = load_tiny(golden_dir, name)
    pool = private_pool(model, 24)
    plain = mixed_passes(model, pool, cfg)
    for (toks, lg), (ptoks, plg) in zip(mixed_passes(model, pool, cfg, batched_chunks=True), plain):   # the rule takes one split at these sizes
        assert toks == ptoks and torch.equal(lg.view(torch.int16), plg.view(torch.int16)), name
    knobs("chunk_splits", 3)                                           # (clamped to the two pages of every chunk here: two splits and the merge)
    split = mixed_passes(model, pool, cfg, batched_chunks=True)
    for p, ((toks, lg), (ptoks, plg)) in enumerate(zip(split, plain)):
        assert toks == ptoks, (name, p)
        for r in range(len(toks)):                                     # assert_vec_close's defaults (c_max = c_rms = 4), test_gpu_spec_batch_mfma.py's for its flagged pass
            assert_vec_close(lg[r].float().cpu().numpy(), plg[r].float().cpu().numpy(), dt, what=f"{name} pass {p} row {r}")
    for r in (0, 1, 3):                                                # the decode rows and the fresh prompt's row: the merge must not touch them
        assert torch.equal(split[0][1][r].view(torch.int16), plain[0][1][r].view(torch.int16)), (name, r)
    assert pool.get_num_free_pages() == pool.size()
