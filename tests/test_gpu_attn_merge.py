"""-m gpu: the split-KV merge inside the fused q|k|v + attention launch (w4_gemv.hpp FUSE, `merge`).

On the 32 / 8 / 128 head geometry the last split of a query head to arrive merges the head's partials into the decoder's attention vector,
and o_proj takes that vector as it is (PRO_NONE) instead of merging the partials again in each of its workgroups (PRO_ATTN).  Same merge,
same slots, same order, same rounding: three forms of the step must agree bit for bit --
    merged   knob attn_merge_in_launch at its default: merged in the fused launch,
    prologue knob attn_merge_in_launch = 0:            the fused launch, merged by o_proj's prologue,
    two      knob fuse_attn = 0:                       attention as a launch of its own, merged by o_proj's prologue.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests._util import TORCH_DT, codes_dev, to_bits, to_dev

pytestmark = pytest.mark.gpu

CFG = {"model_type": "llama", "hidden_size": 4096, "num_hidden_layers": 3, "intermediate_size": 14336,
       "num_attention_heads": 32, "num_key_value_heads": 8, "rms_norm_eps": 1e-5, "vocab_size": 8192,
       "rope_theta": 500000.0, "max_position_embeddings": 8192, "tie_word_embeddings": False,
       "quantization": {"group_size": 64, "bits": 4}}
HQ, D = 32, 128
MODES = {"merged": {}, "prologue": {"attn_merge_in_launch": 0}, "two": {"fuse_attn": 0}}


def build(w, dtype, **kw):
    from proxy_inference_engine_amd.models.llama import Model, ModelArgs
    dev = {k: codes_dev(v) if v.dtype == np.uint32 else to_dev(v, dtype) for k, v in w.items()}
    return Model(ModelArgs(**CFG), dev, **kw)


class _DevView:
    """A device buffer of the decoder (pie_debug_buffer) as something torch.as_tensor accepts."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def debug_tensor(model, which, n, typestr):
    from proxy_inference_engine_amd import _ffi
    fn = _ffi.load().pie_debug_buffer
    fn.restype, fn.argtypes = C.c_void_p, [C.c_void_p, C.c_int]
    torch.cuda.synchronize()
    return torch.as_tensor(_DevView(fn(model._dec, which), n, typestr), device="cuda").clone()


def rn_f32(x: Fraction) -> float:
    """x rounded to the nearest float32, ties to even (exact: no pass through float64)."""
    if x == 0:
        return 0.0
    ax = abs(x)
    e = ax.numerator.bit_length() - ax.denominator.bit_length()
    if Fraction(2) ** e > ax:
        e -= 1
    q = Fraction(2) ** (max(e, -126) - 23)
    return float(round(x / q) * q)                                      # round(Fraction): half to even; n * q is a float32


def host_merge(part_acc, part_ml, w, splits):
    """attn_merge_finish (attention.hpp) on the host, in its order: M = max m_j; Lsum = fma(w_j, l_j, Lsum), A = fma(w_j, acc_j, A) over
    the splits j = 0, 1, ..; out = A / Lsum -- every step one float32 rounding, computed exactly in rationals.  w_j = exp2(m_j - M) is the
    hardware's exponential (v_exp_f32), which no CPU reproduces bit for bit: it is evaluated on the device from the exposed m_j and handed in."""
    out = np.empty((HQ, D), np.float32)
    for h in range(HQ):
        lsum = 0.0
        for j in range(splits):
            lsum = rn_f32(Fraction(float(w[h, j])) * Fraction(float(part_ml[h, j, 1])) + Fraction(lsum))
        for d in range(D):
            a = 0.0
            for j in range(splits):
                a = rn_f32(Fraction(float(w[h, j])) * Fraction(float(part_acc[h, j, d])) + Fraction(a))
            out[h, d] = rn_f32(Fraction(a) / Fraction(lsum))
    return out


def check_attn_vector(model, dtype, splits, what):
    """d->attn after a step == the host merge of the partials the same step exposed, on the 16-bit words."""
    acc = debug_tensor(model, 3, HQ * splits * D, "<f4").view(HQ, splits, D)
    ml = debug_tensor(model, 4, HQ * splits * 2, "<f4").view(HQ, splits, 2)
    got = to_bits(debug_tensor(model, 1, HQ * D, "<i2").view(TORCH_DT[dtype]).view(HQ, D))
    m = ml[:, :, 0]
    w = torch.exp2(m - m.max(dim=1, keepdim=True).values)                # float32 on the device: IEEE subtraction, the hardware exponential
    assert float(w.max()) == 1.0 and float(ml[:, :, 1].min()) >= 0.0
    want = host_merge(acc.cpu().numpy(), ml.cpu().numpy(), w.cpu().numpy(), splits)
    want_bits = to_bits(torch.from_numpy(want).to(TORCH_DT[dtype]))      # pack2<T>: one rounding to nearest even
    bad = int((got != want_bits).sum())
    print(f"{what}: {bad} of {got.size} words of the merged attention vector differ from the host merge")
    assert bad == 0, what


def run(model, prompt, steps, graph):
    cache = model.make_cache()
    tok, _, logits = model.step(prompt, cache)
    rows, toks = [logits.clone()], [int(tok.item())]
    for _ in range(steps):
        tok, _, logits = model.step(tok, cache, graph=graph)
        rows.append(logits.clone()), toks.append(int(tok.item()))
    torch.cuda.synchronize()
    return torch.stack(rows), toks, [c.keys.clone() for c in cache], [c.values.clone() for c in cache], cache[0].capacity


@pytest.mark.parametrize("dtype,split_cases", [("bfloat16", (0, 1, 2)), ("float16", (0,))])
def test_merge_in_the_fused_launch_is_the_prologue_merge_bit_for_bit(dtype, split_cases, knobs):
    """Logits, tokens and K / V caches of the three forms are equal, eagerly and through the replayed graph:
      * 250-token prompt + 12 steps: the cache grows from 256 to 512 rows on the way;
      * 20-token prompt + 6 steps: attn_split leaves three of the four splits idle (T < 33), so their neutral partials go through the
        in-launch merge;
      * kv_splits pinned to 1 and 2 (bf16): one / two arrivals per head.
    In the merged form the attention vector the last layer left equals the host merge of the partials it exposed, and the graph holds
    what the fused form's holds (no new launch); no bounded wait gave up."""
    from proxy_inference_engine_amd import _ffi
    w = po.synth_checkpoint(CFG, seed=3, dtype=dtype, lm_head_gain=4.0)
    prompt = torch.from_numpy(np.random.default_rng(5).integers(0, CFG["vocab_size"], 250)).cuda()
    for kv_splits in split_cases:
        scenarios = [(250, 12), (20, 6)] if kv_splits == 0 else [(70, 6)]
        splits = kv_splits or 4
        results, launches = {}, {}
        for mode, sets in MODES.items():
            for name in ("fuse_attn", "attn_merge_in_launch"):
                knobs(name, sets.get(name))
            model = build(w, dtype, kv_splits=kv_splits)
            for n_prompt, steps in scenarios:
                for graph in (False, True):
                    results[(n_prompt, graph, mode)] = run(model, prompt[:n_prompt], steps, graph)
                    if mode == "merged":
                        check_attn_vector(model, dtype, splits, f"{dtype} kv_splits {kv_splits} prompt {n_prompt} graph {graph}")
            launches[mode] = model.graph_launches(True)
            err = C.c_uint(1)
            _ffi.check(_ffi.load().pie_decoder_status(model._dec, C.byref(err)))
            assert err.value == 0
            del model
        for (n_prompt, graph, mode), got in results.items():
            ref = results[(n_prompt, False, "two")]
            what = f"{dtype} kv_splits {kv_splits} prompt {n_prompt} graph {graph} {mode}"
            assert got[1] == ref[1], what
            assert torch.equal(got[0], ref[0]), what
            assert all(torch.equal(a, b) for a, b in zip(got[2], ref[2])) and all(torch.equal(a, b) for a, b in zip(got[3], ref[3])), what
            assert got[4] == (512 if n_prompt == 250 else 256), what
        assert launches["merged"] == launches["prologue"] == launches["two"] - CFG["num_hidden_layers"], launches


def test_o_proj_follows_the_decision_of_its_qkv_launch(knobs):
    """The form of a layer's attention is decided once, where its q|k|v launch is enqueued; the attention and o_proj launches follow that
    record, not the knobs.  Launched by name, a knob flipped between q|k|v and o_proj must not make o_proj read an input nobody wrote: the
    by-name sequence gives the step's logits whichever way the knobs move in between."""
    dtype = "bfloat16"
    w = po.synth_checkpoint(CFG, seed=3, dtype=dtype, lm_head_gain=4.0)
    prompt = torch.from_numpy(np.random.default_rng(5).integers(0, CFG["vocab_size"], 70)).cuda()
    model = build(w, dtype)
    cache = model.make_cache()
    model.step(prompt, cache)
    model.step(None, cache, graph=False)
    flips = [(None, None), (None, 0), (0, None)]       # (attn_merge_in_launch at q|k|v, after it), then the same for fuse_attn
    outs = []
    for knob in ("attn_merge_in_launch", "fuse_attn"):
        for at_qkv, after in flips:
            model.launch_kernel("embed")
            for li in range(CFG["num_hidden_layers"]):
                knobs(knob, at_qkv)
                model.launch_kernel("qkv", li)
                knobs(knob, after)
                for name in ("attn", "o_proj", "gate_up", "down"):
                    model.launch_kernel(name, li)
            model.launch_kernel("lm_head")
            torch.cuda.synchronize()
            outs.append(to_bits(model.logits).copy())
        knobs(knob, None)
    _, _, logits = model.step(None, cache, graph=False)
    want = to_bits(logits)
    assert all(np.array_equal(o, want) for o in outs)
