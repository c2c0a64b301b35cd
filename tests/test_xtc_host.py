"""No device: XTC's reference (tests/xtc_reference.py), its record (pie_xtc_pack), and the Python layers' defaults and routing."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import xtc_reference as ref

L = lambda p: np.float32(math.log(p))


# ------------------------------------------------------------------ the Philox restatement
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    M = 0xFFFFFFFF
    assert ref.philox4x32_10((0, 0, 0, 0), (0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert ref.philox4x32_10((M, M, M, M), (M, M)) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_coin_is_fp32_and_uses_the_block_no_id_reaches():
    seed, call = 0x0123456789ABCDEF, 2 ** 33 + 5
    r = ref.philox4x32_10((0xFFFFFFFF, 0, call & 0xFFFFFFFF, call >> 32), (seed & 0xFFFFFFFF, seed >> 32))[0]
    u = ref.coin_u(seed, call)
    assert u.dtype == np.float32 and u == np.float32((np.float32(r >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)) and 0.0 < u <= 1.0
    assert not ref.coin(seed, call, 0.0) and ref.coin(seed, call, 1.0) == bool(u < 1.0)
    assert not ref.coin(seed, call, float("nan"))
    assert 524288 // 4 < 0xFFFFFFFF                                      # the largest vocabulary's last block index
    hits = sum(ref.coin(7, c, 0.3) for c in range(2000))
    assert 500 < hits < 700                                              # about 0.3 of the calls


# ------------------------------------------------------------------ the record
def test_pack_ranges_and_sizes():
    from proxy_inference_engine_amd import _ffi, hip_ops
    lib = _ffi.load()
    assert lib.pie_xtc_bytes() == C.sizeof(_ffi.pie_xtc) == 80 and hip_ops.XTC_WORDS == 20
    assert lib.pie_row_tail_bytes() == 40                                # the sampler's record did not grow
    rec = hip_ops.xtc_pack(0.25, 0.1, (2, 128000, -1))
    assert rec.probability == 0.25 and rec.log_threshold == np.float32(math.log(0.1)) and rec.n_special == 3 and rec.reserved == 0
    assert list(rec.special) == [2, 128000, -1] + [0] * 13
    assert hip_ops.xtc_pack(0.0, 0.5).probability == 0.0 and hip_ops.xtc_pack(1.0, 0.5, range(16)).n_special == 16
    words = hip_ops.xtc_records([rec, hip_ops.xtc_pack()])
    assert words.shape == (2, 20) and words[0, 2].item() == 3 and words[0, hip_ops.XTC_PROBABILITY_WORD].item() == int(np.float32(0.25).view(np.int32))
    for bad in ((-0.1, 0.1, ()), (1.1, 0.1, ()), (float("nan"), 0.1, ()), (0.5, 0.0, ()), (0.5, 0.51, ()), (0.5, -0.1, ()), (0.5, float("nan"), ()),
                (0.5, 0.1, range(17)), (0.5, 0.1, (2 ** 31,))):
        with pytest.raises(ValueError):
            hip_ops.xtc_pack(*bad)
    out = _ffi.pie_xtc()
    assert lib.pie_xtc_pack(0.5, 0.1, None, 1, C.byref(out)) == -1 and lib.pie_xtc_pack(0.5, 0.1, None, 0, None) == -1
    assert lib.pie_xtc_pack(0.5, 0.1, None, 0, C.byref(out)) == 0


# ------------------------------------------------------------------ the reference's edge cases
def row(n=40):
    return np.full(n, L(0.001), np.float32)


def removed(lp, thr=0.1, special=()):
    return np.flatnonzero(ref.removed_set(lp, thr, special)).tolist()


def test_reference_edge_cases():
    lp = row()
    assert removed(lp) == []                                             # no candidate
    lp[7] = L(0.9)
    assert removed(lp) == []                                             # exactly one
    lp[3] = L(0.9)
    assert removed(lp) == []                                             # two, tied: nothing lies above the minimum
    lp = row(); lp[1] = L(0.5); lp[20] = lp[30] = L(0.2)
    assert removed(lp) == [1]                                            # three, two tied at the minimum: only the top one goes
    lp = row(); lp[0] = ref.log_threshold(0.1); lp[5] = L(0.5); lp[6] = L(0.3)
    assert removed(lp) == [5]                                            # lp == log_thr exactly is no candidate (it would be the minimum)
    lp[0] = np.nextafter(lp[0], np.float32(0))
    assert removed(lp) == [5, 6]                                         # one ulp above it is
    lp = row(); lp[2] = L(0.5); lp[3] = L(0.3); lp[4] = L(0.15)
    assert removed(lp, special=(2,)) == [3] and removed(lp, special=(2, 3, 4)) == [] and removed(lp, special=(4, 99, -3)) == [2, 3]
    lp[10:] = -np.inf
    assert removed(lp) == [2, 3]                                         # -inf entries are never candidates
    assert removed(np.array([L(0.9)], np.float32)) == [] and removed(np.array([L(0.6), L(0.4)], np.float32)) == [0]
    x = ref.edited(lp, ref.removed_set(lp, 0.1))
    assert np.isneginf(x[[2, 3]]).all() and x[4] == lp[4] and lp[2] == L(0.5)   # a copy


def test_min_p_case_removes_exactly_the_top_id():
    p = np.array([0.6, 0.2, 0.05] + [0.03] * 5)
    lp = np.log(p).astype(np.float32)
    assert removed(lp, 0.1) == [0]
    x = ref.edited(lp, ref.removed_set(lp, 0.1))
    keep = lambda v: np.flatnonzero(v >= v.max() + np.float32(math.log(0.1))).tolist()
    assert keep(lp) == [0, 1] and keep(x) == [1, 2, 3, 4, 5, 6, 7]       # the 0.03 ids pass min-p only against the survivors' maximum


# ------------------------------------------------------------------ the Python layers
def test_make_sampler_defaults_and_xtc():
    from proxy_inference_engine_amd import samplers
    for kw, spec in ((dict(temp=1.0), ("categorical", 1.0, 0.0, 0)), (dict(temp=0.8, top_k=5), ("top_k", 0.8, 0.0, 5)), (dict(temp=0.9, top_p=0.9), ("top_p", 0.9, 0.9, 0)),
                     (dict(temp=1.0, min_p=0.1, min_tokens_to_keep=2), ("min_p", 1.0, 0.1, 2))):
        plain = samplers.make_sampler(**kw)
        assert plain.hip_spec == spec and not hasattr(plain, "hip_xtc")
        off = samplers.make_sampler(**kw, xtc_probability=0.0, xtc_threshold=0.3, xtc_special_tokens=(1,))
        assert off.hip_spec == spec and not hasattr(off, "hip_xtc")
        on = samplers.make_sampler(**kw, xtc_probability=0.5, xtc_threshold=0.1, xtc_special_tokens=[2, 9])
        assert on.hip_spec == spec and on.hip_xtc == (0.5, 0.1, (2, 9))
    assert samplers.make_sampler(temp=0, xtc_probability=0.5, xtc_threshold=0.1) is samplers.greedy   # greedy ignores XTC
    for bad in (dict(xtc_probability=1.5, xtc_threshold=0.1), dict(xtc_probability=0.5), dict(xtc_probability=0.5, xtc_threshold=0.6),
                dict(xtc_probability=0.5, xtc_threshold=0.1, xtc_special_tokens=range(17)), dict(xtc_probability=float("nan"), xtc_threshold=0.1)):
        with pytest.raises(ValueError):
            samplers.make_sampler(temp=1.0, **bad)
    import torch
    with pytest.raises(ValueError):
        samplers.make_sampler(temp=1.0, xtc_probability=0.5, xtc_threshold=0.1)(torch.zeros(1, 8))   # host tensors are refused, as ever


def test_sampling_params_defaults_leave_the_record_unchanged():
    from proxy_inference_engine_amd.engine import SamplingParams
    sp = SamplingParams(temp=0.8, top_k=5, seed=3)
    assert sp.xtc() is None and sp.xtc({7}) is None
    assert bytes(sp.record(2)) == bytes(SamplingParams(temp=0.8, top_k=5, seed=3, xtc_probability=0.5, xtc_threshold=0.1).record(2))
    on = SamplingParams(temp=0.8, top_k=5, xtc_probability=0.5, xtc_threshold=0.1)
    assert on.xtc() == (0.5, 0.1, ()) and on.xtc({9, 2}) == (0.5, 0.1, (2, 9))
    assert SamplingParams(temp=0.8, xtc_probability=0.5, xtc_threshold=0.1, xtc_special_tokens=(4,)).xtc({9}) == (0.5, 0.1, (4,))
    assert SamplingParams(xtc_probability=0.5, xtc_threshold=0.1).xtc() is None and SamplingParams(xtc_probability=0.5, xtc_threshold=0.1).plain
    with pytest.raises(ValueError):
        SamplingParams(temp=1.0, xtc_probability=0.5, xtc_threshold=0.7).xtc()
    with pytest.raises(ValueError):
        SamplingParams(xtc_probability=2.0, xtc_threshold=0.1).xtc()   # checked for a greedy request too


def test_fused_tail_routing():
    from proxy_inference_engine_amd import samplers
    from proxy_inference_engine_amd.engine.inference_engine import InferenceEngine, fused_tail_plan, fused_tail_spec
    plain = samplers.make_sampler(temp=0.8, top_k=5)
    xtc = samplers.make_sampler(temp=0.8, top_k=5, xtc_probability=0.5, xtc_threshold=0.1, xtc_special_tokens=(2,))
    assert fused_tail_spec([], xtc) == fused_tail_spec([], plain) == (("top_k", 0.8, 0.0, 5), 1.0, 60)
    assert fused_tail_spec([], xtc, structuring_engine=object()) is None and fused_tail_spec([], xtc, tensor_parallel=True) is None
    assert "xtc" not in fused_tail_plan([], plain) and "xtc" not in fused_tail_plan([], samplers.greedy)
    plan = fused_tail_plan([], xtc)
    assert plan["xtc"] == (0.5, 0.1, (2,)) and {k: v for k, v in plan.items() if k != "xtc"} == fused_tail_plan([], plain)
    eng = InferenceEngine(model=object(), stop_tokens=[11, 7])
    assert eng.make_sampler(temp=1.0, xtc_probability=0.5, xtc_threshold=0.1).hip_xtc == (0.5, 0.1, (7, 11))     # the stop tokens by default
    assert eng.make_sampler(temp=1.0, xtc_probability=0.5, xtc_threshold=0.1, xtc_special_tokens=[3]).hip_xtc == (0.5, 0.1, (3,))
    assert not hasattr(eng.make_sampler(temp=1.0), "hip_xtc") and eng.make_sampler(temp=0, xtc_probability=0.5, xtc_threshold=0.1) is samplers.greedy
