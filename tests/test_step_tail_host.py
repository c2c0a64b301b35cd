"""CPU: the configurable step tail's host side -- the three C entry points are declared and bound, pie_logits_penalty
refuses bad arguments before any launch, make_sampler's closures and the repetition-penalty processor carry what the engine needs to
run them inside the decode step, and the engine's routing predicate picks the fused tail exactly where the design allows it."""
import ctypes
import math
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_header_declares_the_tail_entry_points():
    from proxy_inference_engine_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pie_hip.h").read_text(), flags=re.S)
    for proto in (r"int\s+pie_logits_penalty\s*\(\s*void\s*\*logits,\s*int V,\s*int dtype,\s*const int32_t\s*\*ids,\s*int n,\s*double penalty,\s*void\s*\*stream\)",
                  r"int\s+pie_decoder_set_logits_penalty\s*\(\s*pie_decoder\s*\*d,\s*double penalty,\s*int context_size,\s*int32_t\s*\*ids_by_pos,\s*int ids_cap\)",
                  r"int\s+pie_decoder_set_sampler\s*\(\s*pie_decoder\s*\*d,\s*int mode,\s*double temp,\s*double p,\s*int k,\s*unsigned long long seed,\s*"
                  r"unsigned long long\s*\*counter,\s*void\s*\*workspace,\s*size_t workspace_bytes\)"):
        assert re.search(proto, text), proto
    assert re.search(r"PIE_SAMPLE_GREEDY\s*=\s*-1", text) and _ffi.PIE_SAMPLE_GREEDY == -1
    lib = _ffi.load()
    for name in ("pie_logits_penalty", "pie_decoder_set_logits_penalty", "pie_decoder_set_sampler"):
        assert name in _ffi.EXPORTS and hasattr(lib, name)


def test_logits_penalty_refuses_bad_arguments_before_any_launch_without_gpu():
    from proxy_inference_engine_amd import _ffi
    lib = _ffi.load()
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)   # a host stand-in, never dereferenced: every call below is refused first
    ARG, SHAPE = -1, -2
    ok = [p, 512, _ffi.PIE_BF16, p, 60, 1.3, None]   # logits, V, dtype, ids, n, penalty, stream
    for i, v, code in ((5, -0.5, ARG), (5, math.inf, ARG), (5, math.nan, ARG), (5, -math.inf, ARG), (4, 0, ARG), (4, -3, ARG), (4, 1025, ARG),
                       (1, 0, SHAPE), (1, -7, SHAPE), (0, None, ARG), (3, None, ARG), (2, 7, ARG)):
        rc = lib.pie_logits_penalty(*(ok[:i] + [v] + ok[i + 1:]))
        err = lib.pie_last_error()
        assert rc == code and b"penalty" in err, (i, v, rc, err)
    # the setters refuse a missing decoder the same way (their other refusals need a decoder, hence a device: tests/test_gpu_step_tail.py)
    assert lib.pie_decoder_set_logits_penalty(None, 1.3, 60, p, 64) == ARG and b"pie_decoder_set_logits_penalty" in lib.pie_last_error()
    assert lib.pie_decoder_set_sampler(None, 0, 1.0, 0.0, 0, 1, p, p, 1 << 20) == ARG and b"pie_decoder_set_sampler" in lib.pie_last_error()


def test_make_sampler_closures_carry_their_hip_spec():
    from proxy_inference_engine_amd.samplers import greedy, make_sampler
    assert make_sampler(temp=0) is greedy and greedy.is_greedy and not hasattr(greedy, "hip_spec")
    assert make_sampler(temp=0, top_k=5, top_p=0.5) is greedy                      # temp == 0 wins over every filter
    cases = [
        (dict(temp=0.7, top_p=0.9), ("top_p", 0.7, 0.9, 0)),
        (dict(temp=0.7, top_p=0.9, min_p=0.1, top_k=5), ("top_p", 0.7, 0.9, 0)),   # top-p first
        (dict(temp=1.0, top_p=1.0, min_p=0.1, min_tokens_to_keep=2, top_k=5), ("min_p", 1.0, 0.1, 2)),   # top_p = 1.0 is no top-p
        (dict(temp=1.0, top_p=0.0, min_p=0.05), ("min_p", 1.0, 0.05, 1)),
        (dict(temp=0.8, top_k=5), ("top_k", 0.8, 0.0, 5)),
        (dict(temp=0.8, top_p=1.0, top_k=40), ("top_k", 0.8, 0.0, 40)),
        (dict(temp=1.3), ("categorical", 1.3, 0.0, 0)),
        (dict(temp=1.3, top_k=-1, top_p=0.0, min_p=0.0), ("categorical", 1.3, 0.0, 0)),
    ]
    for kw, spec in cases:
        s = make_sampler(**kw)
        assert callable(s) and not getattr(s, "is_greedy", False) and s.hip_spec == spec, (kw, s.hip_spec)


def test_penalty_processor_exposes_its_parameters():
    from proxy_inference_engine_amd.logits_processors import make_repetition_penalty, repetition_penalty_logits_processor
    proc = repetition_penalty_logits_processor(1.8, 20)
    assert callable(proc) and proc.penalty == 1.8 and proc.context_size == 20
    assert isinstance(proc.penalty, float) and isinstance(proc.context_size, int)
    d = make_repetition_penalty()
    assert (d.penalty, d.context_size) == (1.0, 60)
    with pytest.raises(ValueError):
        make_repetition_penalty(-1.0, 5)


def test_engine_routing_predicate():
    from proxy_inference_engine_amd.engine.inference_engine import fused_tail_spec
    from proxy_inference_engine_amd.logits_processors import make_repetition_penalty
    from proxy_inference_engine_amd.samplers import greedy, make_sampler
    topk, cat = make_sampler(temp=0.8, top_k=5), make_sampler(temp=1.0)
    foreign = lambda x: x                                  # noqa: E731  a sampler callable that is not make_sampler's
    other_proc = lambda tokens, logits: logits             # noqa: E731
    pen = make_repetition_penalty(1.1, 60)
    pse = object()
    table = [
        # processors, sampler, structuring engine, tensor parallel -> expected
        ([], greedy, None, False, (None, 1.0, 60)),
        (None, greedy, None, False, (None, 1.0, 60)),
        ([], topk, None, False, (("top_k", 0.8, 0.0, 5), 1.0, 60)),
        ([], cat, None, False, (("categorical", 1.0, 0.0, 0), 1.0, 60)),
        ([pen], greedy, None, False, (None, 1.1, 60)),
        ([pen], topk, None, False, (("top_k", 0.8, 0.0, 5), 1.1, 60)),
        ([make_repetition_penalty(2.0, 1)], greedy, None, False, (None, 2.0, 1)),
        ([make_repetition_penalty(2.0, 1024)], greedy, None, False, (None, 2.0, 1024)),
        ([make_repetition_penalty(0.0, 5)], greedy, None, False, (None, 0.0, 5)),
        ([make_repetition_penalty(2.0, 0)], greedy, None, False, None),       # context_size 0: tokens[-0:] is the WHOLE history upstream
        ([make_repetition_penalty(2.0, 1025)], greedy, None, False, None),
        ([pen, pen], greedy, None, False, None),
        ([other_proc], greedy, None, False, None),
        ([other_proc, pen], topk, None, False, None),
        ([], foreign, None, False, None),
        ([pen], foreign, None, False, None),
        ([], greedy, pse, False, None),
        ([pen], topk, pse, False, None),
        ([], greedy, None, True, None),
        ([pen], topk, None, True, None),
    ]
    for procs, sampler, se, tp, want in table:
        assert fused_tail_spec(procs, sampler, se, tp) == want, (procs, sampler, se, tp)
