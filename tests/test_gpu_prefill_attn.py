"""-m gpu: k_prefill_attn (csrc/prefill_attn.hpp) through its three op-level entries -- pie_sdpa_prefill, pie_sdpa_prefill_window and
pie_sdpa_segments -- against the float64 interval reference of tests/prefill_attn_reference.py, rounded once.

The data are that module's: edge needles (each row's softmax sits on the two keys inside and the two keys outside both ends of its own
interval; tests/test_prefill_attn_host.py shows that one key admitted or dropped at any edge of any row fails the bound used here) and
score staircases (the running maximum moves in every key block, or never after the first).  The bound is the one
test_sdpa_prefill_vs_oracle and test_sdpa_segments_vs_oracle apply to this kernel: assert_dot_close, at most 5 % of the elements differing
at all.

Instantiations that run here and in no other test:
- k_prefill_attn<T, D, R, 2, false, true>, the windowed form with two query tiles per workgroup (prefill_qt = 2, R in 1, 3, 4);
- k_prefill_attn<T, D, 1, 2, true>, the segmented form with two query tiles: segment_attn_launch_d reads no knob and picks it by
  ceil(N / 64) * H >= 512, so the cases have H = 64 and N = 449 (the smallest N that meets the rule at 64 heads) or 512.  A change of
  that threshold has to move these cases (prefill_attn_reference.SEGMENT_TWO_TILE_RULE; the host test pins that 448 rows do not reach it).
"""
import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests import prefill_attn_reference as ref
from tests._util import assert_dot_close, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from proxy_inference_engine_amd import _ffi, hip_ops
    _ffi.require_gpu()
    return hip_ops


def _dev(x, dt):
    return to_dev(po.to_bits(x, dt), dt)


def _run(ops, knobs, c):
    """The case through its entry -> the fraction of elements that differ from the rounded reference at all."""
    q, k, v, lo, hi, want = ref.case_data(c)
    scale = c.D ** -0.5
    if c.knob:
        knobs("prefill_qt", c.knob)
    if c.family == "segments":
        lo_d, hi_d = ops.segment_bounds(c.cu, "cuda")
        assert np.array_equal(lo_d.cpu().numpy(), lo) and np.array_equal(hi_d.cpu().numpy(), hi)
        got = ops.sdpa_segments(_dev(np.ascontiguousarray(q.transpose(1, 0, 2)), c.dt), _dev(k, c.dt), _dev(v, c.dt), lo_d, hi_d, scale).transpose(0, 1)
    elif c.family == "window":
        got = ops.sdpa_prefill_window(_dev(q, c.dt)[None], _dev(k, c.dt)[None], _dev(v, c.dt)[None], scale, c.off, c.W)[0]
    elif c.L == 1:      # hip_ops gives one query row to the decode attention: the prompt kernel's one-row launch goes through the C entry
        from proxy_inference_engine_amd import _ffi
        qd, kd, vd = _dev(np.ascontiguousarray(q.transpose(1, 0, 2)), c.dt), _dev(k, c.dt), _dev(v, c.dt)       # q [L, Hq, D]
        out = torch.empty_like(qd)
        _ffi.check(_ffi.load().pie_sdpa_prefill(_ffi.p(qd), _ffi.p(kd), _ffi.p(vd), c.Hkv * c.rep, c.Hkv, c.L, c.off, k.shape[1], c.D, float(scale),
                                                _ffi.dtype_code(qd.dtype), _ffi.p(out), _ffi.stream()))
        got = out.transpose(0, 1)
    else:
        got = ops.scaled_dot_product_attention(_dev(q, c.dt)[None], _dev(k, c.dt)[None], _dev(v, c.dt)[None], scale, mask="causal", T=c.off + c.L)[0]
    got = got.float().cpu().numpy()
    assert got.shape == want.shape
    frac = float((got != want).mean())
    print(f"differing fraction {frac:.4%}  {ref.case_id(c)}")
    assert_dot_close(got, want, c.dt, max_frac=0.05, what=ref.case_id(c))
    return frac


@pytest.mark.parametrize("c", ref.CAUSAL_CASES, ids=ref.case_id)
def test_causal_edges(ops, knobs, c):
    """pie_sdpa_prefill on edge-needle data: every ratio 1..8 at both head dims and dtypes with L >= 31 (one query tile per workgroup; two
    where the knob asks and rep <= 4), L on and next to the tile boundaries (65 / 96: the last workgroup's second tile is all padding;
    97: one live row), poisoned capacity past T.  The six L = 1 cases (one live row at an offset) call the C entry: through hip_ops one
    query row is decode attention, not this kernel.
    Elements differing from the rounded reference on MI355X (limit 5 %): at most 0.10 % (bf16) and 0.78 % (f16) of a case (the latter one
    element of a one-row case; 0.29 % among the others)."""
    _run(ops, knobs, c)


@pytest.mark.parametrize("c", ref.WINDOW_CASES, ids=ref.case_id)
def test_windowed_edges(ops, knobs, c):
    """pie_sdpa_prefill_window on edge-needle data: the lower edge offset + r - W (W + 1 keys in a full window) and the upper edge of every
    row, W below, at and above a key block, workgroups that start at a later key block (b_first > 0) and rows whose leading block is
    wholly masked, one and two query tiles per workgroup.
    Elements differing from the rounded reference on MI355X (limit 5 %): at most 0.09 % (bf16) and 0.23 % (f16) of a case."""
    _run(ops, knobs, c)


@pytest.mark.parametrize("c", ref.SEGMENT_CASES, ids=ref.case_id)
def test_segment_edges(ops, knobs, c):
    """pie_sdpa_segments on edge-needle data: ragged segments (1-row, 4-row, straddling tiles), and the two-tile form by the launcher's own
    rule ceil(N / 64) * H >= 512 (H = 64: N = 449 leaves the last workgroup one live row and a wholly padding second tile; N = 512).
    Elements differing from the rounded reference on MI355X (limit 5 %): at most 0.07 % (bf16) and 0.25 % (f16) of a case."""
    _run(ops, knobs, c)


@pytest.mark.parametrize("c", ref.STAIRCASE_CASES, ids=ref.case_id)
def test_online_softmax_staircase(ops, knobs, c):
    """Scores that rise by 0.25 per key (8 per 32-key block) force the rescale of l_run and of every oacc[dt] in every key block; the
    descending twin keeps the maximum in the first block while later terms fall to e^-58.  Causal and windowed, both tile counts.
    Elements differing from the rounded reference on MI355X (limit 5 %): at most 0.22 % (bf16) and 1.13 % (f16) of a case."""
    _run(ops, knobs, c)
