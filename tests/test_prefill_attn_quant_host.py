"""pie_prefill_attn_quant and SpeculativeParams(quantized_kv=...) without a GPU: every refusal by code and name, the
split rule and the workspace's size, the flag's default and its refusals.  None of these calls reaches HIP."""
import ctypes as C

import pytest

from proxy_inference_engine_amd import _ffi
from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine
from proxy_inference_engine_amd.engine.inference_engine import SpeculativeParams, _check_generate_args

ARG, SHAPE, ALIGN = -1, -2, -3
GOOD = dict(q=1 << 20, kc=1 << 21, ks=1 << 22, kb=1 << 23, vc=1 << 24, vs=1 << 25, vb=1 << 26, Hq=8, Hkv=2, M=33, offset=31, cap=256, D=128, gs=64, bits=4,
            dtype=_ffi.PIE_BF16, splits=1, out=1 << 27, ws=None)


def call(lib, **kw):
    a = {**GOOD, **kw}
    return lib.pie_prefill_attn_quant(a["q"], a["kc"], a["ks"], a["kb"], a["vc"], a["vs"], a["vb"], a["Hq"], a["Hkv"], a["M"], a["offset"], a["cap"], a["D"],
                                      a["gs"], a["bits"], 0.125, a["dtype"], a["splits"], a["out"], a["ws"], None)


@pytest.mark.parametrize("bad,code,word", [
    *[({name: None}, ARG, b"null pointer") for name in ("q", "kc", "ks", "kb", "vc", "vs", "vb", "out")],
    (dict(dtype=7), ARG, b"dtype"), (dict(bits=6), ARG, b"bits"), (dict(gs=16), ARG, b"group_size"), (dict(D=96), SHAPE, b"head_dim"),
    (dict(D=64, gs=128), SHAPE, b"divide"),
    (dict(M=0), SHAPE, b"offset + M <= cap"), (dict(offset=-1), SHAPE, b"offset + M <= cap"), (dict(offset=224), SHAPE, b"offset + M <= cap"),
    (dict(Hq=6, Hkv=2), SHAPE, b"1, 2, 4 or 8"), (dict(Hq=7, Hkv=2), SHAPE, b"multiple"), (dict(splits=33), ARG, b"splits"),
    (dict(splits=2), ARG, b"workspace"), (dict(splits=0, M=8, offset=240), ARG, b"workspace"),
    (dict(q=(1 << 20) + 8), ALIGN, b"16-byte"), (dict(out=(1 << 27) + 2), ALIGN, b"16-byte"), (dict(kc=(1 << 21) + 4), ALIGN, b"8-byte"),
    (dict(vc=(1 << 24) + 4), ALIGN, b"8-byte")])
def test_every_refusal_has_its_code_and_name(bad, code, word):
    lib = _ffi.load()
    assert call(lib, **bad) == code, bad
    err = lib.pie_last_error()
    assert err.startswith(b"pie_prefill_attn_quant") and word in err, (bad, err)


@pytest.mark.parametrize("M,offset,Hq,Hkv,want", [
    (8, 32760, 32, 8, 32),      # a verify pass on the 8B geometry: 8 workgroups, 32 splits of 32 blocks
    (8, 504, 32, 8, 4),         # 16 blocks: a split keeps four
    (8, 0, 32, 8, 1),           # one block
    (256, 8192, 32, 8, 4),      # a chunk: 8 tiles x 8 kv-heads = 64 workgroups
    (4096, 0, 32, 8, 1),        # the grid fills the chip
    (65, 95, 8, 1, 1),          # 5 blocks: no split keeps four
    (0, 0, 8, 2, 1), (8, -1, 8, 2, 1), (8, 0, 7, 2, 1)])   # what the op refuses: one
def test_the_split_rule_and_the_workspace(M, offset, Hq, Hkv, want):
    lib = _ffi.load()
    got = lib.pie_prefill_attn_quant_splits(M, offset, Hq, Hkv)
    assert got == want
    assert lib.pie_prefill_attn_quant_workspace_bytes(max(M, 1), Hq, 128, got) == (0 if got == 1 else max(M, 1) * Hq * got * 130 * 4)
    assert lib.pie_prefill_attn_quant_workspace_bytes(8, 32, 64, 3) == 8 * 32 * 3 * 66 * 4 and lib.pie_prefill_attn_quant_workspace_bytes(8, 32, 64, 1) == 0


def test_the_flag_its_default_and_its_refusals():
    assert SpeculativeParams().quantized_kv is False and _ffi.PIE_OPT_KVQ_DIRECT == 5
    assert SpeculativeParams.__dataclass_fields__["quantized_kv"].kw_only
    with pytest.raises(ValueError, match="quantized_kv is a bool"):
        SpeculativeParams(quantized_kv=1)
    with pytest.raises(ValueError, match="quantized_kv is not available with grammar"):
        SpeculativeParams(quantized_kv=True, grammar=True)
    with pytest.raises(ValueError, match="quantized_kv is not available with a draft model"):
        SpeculativeParams(quantized_kv=True, draft_model="some/checkpoint")
    with pytest.raises(ValueError, match="not available with quantized_kv"):
        BatchedEngine(object(), num_pages=8, speculative=SpeculativeParams(quantized_kv=True))
    _check_generate_args(object(), None, None, 4, 64, None, None, None, SpeculativeParams(quantized_kv=True))   # admitted in the arguments
    null = C.c_void_p(None)
    lib = _ffi.load()
    assert lib.pie_decoder_configure(null, _ffi.PIE_OPT_KVQ_DIRECT, 1) == ARG and b"null decoder" in lib.pie_last_error()
