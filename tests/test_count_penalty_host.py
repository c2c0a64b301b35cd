"""Frequency and presence penalties without a device: the record's layout, the argument rules of the pack helper and of the
Python layers, SamplingParams' two fields, and where InferenceEngine routes a request that carries them."""
import ctypes as C

import numpy as np
import pytest
import torch

from proxy_inference_engine_amd import _ffi, hip_ops
from proxy_inference_engine_amd.engine import SamplingParams
from proxy_inference_engine_amd.engine.inference_engine import InferenceEngine, fused_tail_plan
from proxy_inference_engine_amd.logits_processors import count_penalty_logits_processor, make_logit_bias, make_repetition_penalty
from proxy_inference_engine_amd.samplers import make_sampler


def test_record_layout_matches_the_library():
    assert C.sizeof(_ffi.pie_count_penalty) == 16 == int(_ffi.load().pie_count_penalty_bytes()) and hip_ops.COUNT_PENALTY_WORDS == 4
    assert [(n, getattr(_ffi.pie_count_penalty, n).offset) for n, _ in _ffi.pie_count_penalty._fields_] == [("freq", 0), ("pres", 4), ("start", 8), ("counted_pos", 12)]
    rec = hip_ops.count_penalty_pack(0.5, -1.25, 24)
    assert (rec.freq, rec.pres, rec.start, rec.counted_pos) == (0.5, -1.25, 24, 23)                 # nothing counted yet
    assert hip_ops.count_penalty_pack(2.0, 2.0, 24, 30).counted_pos == 30
    words = np.frombuffer(bytes(rec), np.int32)
    assert words[:2].view(np.float32).tolist() == [0.5, -1.25] and words[2:].tolist() == [24, 23]
    table = hip_ops.count_penalty_records([rec, hip_ops.count_penalty_pack()])
    assert table.dtype == torch.int32 and table.shape == (2, 4) and table[0].tolist() == words.tolist() and table[1].tolist() == [0, 0, 0, -1]
    assert C.sizeof(_ffi.pie_row_tail) == 40                                                         # the sampler's record is untouched


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf"), 1e300])
def test_pack_refuses_what_is_not_finite(bad):
    rec = _ffi.pie_count_penalty()
    lib = _ffi.load()
    for f, p in ((bad, 0.0), (0.0, bad)):
        assert lib.pie_count_penalty_pack(f, p, 0, -1, C.byref(rec)) == -1 and b"pie_count_penalty_pack" in lib.pie_last_error()
        with pytest.raises(ValueError):
            hip_ops.count_penalty_pack(f, p, 0)
    assert lib.pie_count_penalty_pack(0.5, 0.5, -1, -1, C.byref(rec)) == -1 and lib.pie_count_penalty_pack(0.5, 0.5, 0, -2, C.byref(rec)) == -1
    assert lib.pie_count_penalty_pack(0.5, 0.5, 0, -1, None) == -1
    assert lib.pie_count_penalty_pack(-7.5, 100.0, 3, 2, C.byref(rec)) == 0 and (rec.freq, rec.pres) == (-7.5, 100.0)   # the ABI: any finite value


@pytest.mark.parametrize("f, p", [(2.5, 0.0), (0.0, -2.001), (float("nan"), 0.0), (0.0, float("inf"))])
def test_python_layers_accept_minus_two_to_two(f, p):
    with pytest.raises(ValueError):
        SamplingParams(frequency_penalty=f, presence_penalty=p).count_penalties()
    stub = CountStub([[1, 2, 3]], [SamplingParams(frequency_penalty=f, presence_penalty=p)])
    with pytest.raises(ValueError):
        BatchedEngine(stub, num_pages=8, max_batch=2).generate([[1, 2, 3]], 4, sampling=SamplingParams(frequency_penalty=f, presence_penalty=p))
    assert not stub.calls and stub.sets == 0                                                         # refused before anything ran or was armed
    eng = InferenceEngine(model=object())
    with pytest.raises(ValueError):
        eng.make_processors(frequency_penalty=f, presence_penalty=p)
    with pytest.raises(ValueError):
        count_penalty_logits_processor(f, p, 0)
    assert SamplingParams(frequency_penalty=-2.0, presence_penalty=2.0).count_penalties() == (-2.0, 2.0)


def test_sampling_params_account_for_the_penalties():
    sp = SamplingParams()
    assert sp.frequency_penalty == 0.0 and sp.presence_penalty == 0.0 and sp.tailless and sp.plain and not sp.counted
    for kw in (dict(frequency_penalty=0.5), dict(presence_penalty=-1.0), dict(frequency_penalty=2.0, presence_penalty=2.0)):
        sp = SamplingParams(**kw)
        assert sp.counted and not sp.tailless and not sp.plain and sp.recordless, kw
        assert sp.record().mode == -1 and sp.record().penalty == 1.0                                # pie_row_tail knows nothing of them
    assert not SamplingParams(temp=0.7, frequency_penalty=0.5).recordless


def test_make_processors_and_the_fused_plan():
    eng = InferenceEngine(model=object())
    assert eng.make_processors() == [] and eng.make_processors(frequency_penalty=0.0, presence_penalty=0.0) == []
    procs = eng.make_processors(frequency_penalty=0.5, presence_penalty=1.5)
    assert len(procs) == 1 and (procs[0].frequency_penalty, procs[0].presence_penalty, procs[0].prompt_len) == (0.5, 1.5, 0)
    greedy = make_sampler(temp=0.0)
    plan = fused_tail_plan(procs, greedy)
    assert plan is not None and plan["counts"] is procs[0] and plan["mask"] is None and plan["bias"] is None and plan["repetition_penalty"] == 1.0
    plan = fused_tail_plan(procs, make_sampler(temp=0.8, top_k=5))
    assert plan is not None and plan["sampler"] is not None and plan["counts"] is procs[0]
    # the order the kernels define: penalty, bias, frequency / presence
    full = eng.make_processors(repetition_penalty=1.3, logit_bias={3: 1.0}, presence_penalty=1.0)
    assert [hasattr(p, "penalty") for p in full] == [True, False, False] and hasattr(full[2], "presence_penalty")
    plan = fused_tail_plan(full, greedy)
    assert plan is not None and plan["counts"] is full[2] and plan["bias"] is full[1] and plan["repetition_penalty"] == 1.3
    assert fused_tail_plan([full[2], full[1]], greedy) is None and fused_tail_plan([procs[0], procs[0]], greedy) is None
    assert "counts" not in fused_tail_plan([make_repetition_penalty(1.3, 20), make_logit_bias({3: 1.0})], greedy)   # the plan it always got
    # a structuring engine, a tensor-parallel model, a foreign sampler: the processor branch
    assert fused_tail_plan(procs, greedy, structuring_engine=object()) is None
    assert fused_tail_plan(procs, greedy, tensor_parallel=True) is None
    assert fused_tail_plan(procs, lambda x: x) is None
    pse = type("Pse", (), {"process_logits": staticmethod(lambda toks, lg: lg), "sample": staticmethod(lambda x, s: s(x))})()
    eng = InferenceEngine(model=object(), structuring_engine=pse)
    procs = eng.make_processors(frequency_penalty=0.5)
    assert len(procs) == 2 and hasattr(procs[1], "frequency_penalty")
    assert fused_tail_plan(procs, eng.make_sampler(temp=0), eng.structuring_engine) is None


def test_reference_formula_and_counts():
    from tests.count_penalty_reference import count_penalty_reference, generated_counts
    from oracle import pie_oracle as po
    c = generated_counts([3, 3, 5, -1, 9, 3, 8], 8)
    assert c.tolist() == [0, 0, 0, 3, 0, 1, 0, 0] and c.dtype == np.int32
    x = po.to_bits(np.array([1.0, -2.0, 0.5, 4.0, -np.inf, -0.0, 3.0, 7.0], np.float32), "bfloat16")
    out = po.from_bits(count_penalty_reference(x, np.array([0, 1, 0, 3, 2, 1, 0, 70000]), 0.5, 0.25, "bfloat16"), "bfloat16")
    assert out.tolist()[:7] == [1.0, -2.75, 0.5, 2.25, -np.inf, -0.75, 3.0] and out[7] == np.float32(po.round_T(np.float32(7.0 - 35000.25), "bfloat16"))
    h = po.to_bits(np.array([-65504.0, 65504.0], np.float32), "float16")
    # f16 at 65504 (spacing 32): -65504 - 16 = -65520 is the tie that rounds to -inf, 65504 - 16 the tie that rounds to the even 65472
    assert count_penalty_reference(h, np.array([7, 7]), 2.0, 2.0, "float16").tolist() == [0xFC00, 0x7BFE]
    assert count_penalty_reference(h, np.array([7, 7]), -1.0, -0.25, "float16").tolist() == [0xFBFF, 0x7BFF]   # +7.25: both round back
    assert count_penalty_reference(h, np.array([70000, 0]), -1.0, -0.25, "float16").tolist() == [0x6C64, 0x7BFF]  # 4496.25 -> 4496; untouched


# ------------------------------------------------------------------ BatchedEngine's bookkeeping, on the stub model of tests/test_batch_engine_host.py
from collections import Counter  # noqa: E402

from proxy_inference_engine_amd.engine import BatchedEngine  # noqa: E402
from tests.test_batch_engine_host import StubModel, alone, requests  # noqa: E402


class CountStub(StubModel):
    """StubModel + the batch count penalty's surface.  It keeps every row's record and counts as the device would, counts every output
    row's input id by the kernel's rule, and then checks the row against the request that sits in it: a request with penalties finds its
    own (f, p, start = its prompt's length) and exactly the multiplicities of what it has generated so far; a request without, a prompt
    that is still filling and the shared prefix's own pass find a zero record."""

    def __init__(self, prompts, params):
        super().__init__()
        self.prompts, self.params = [list(p) for p in prompts], params
        self.rows, self.armed, self.sets, self.checked = {}, False, 0, 0

    def set_batch_count_penalty(self, rows_cap):
        self.armed, self.sets, self.rows_cap = True, self.sets + 1, rows_cap
        self.rows = {s: [0.0, 0.0, 0, -1, Counter()] for s in range(rows_cap)}

    def write_batch_count_penalty(self, rows, records, generated=None):
        assert self.armed and len(rows) == len(records) and (generated is None or len(generated) == len(rows))
        for i, (s, rec) in enumerate(zip(rows, records)):
            gen = list(generated[i]) if generated is not None and generated[i] is not None else []
            self.rows[s] = [0.0, 0.0, 0, -1, Counter()] if rec is None else [rec[0], rec[1], rec[2], rec[2] + len(gen) - 1, Counter(gen)]

    def clear_batch_count_penalty(self):
        self.armed = False

    def _tail(self, caches):
        if not self.armed:
            return
        assert len(caches) <= self.rows_cap
        for s, c in enumerate(caches):
            hist = self._hist(c[0].page_manager)
            f, p, start, counted, counts = row = self.rows[s]
            pos = len(hist) - 1
            if (f, p) != (0.0, 0.0) and pos >= start and pos > counted:      # the kernel's counting rule
                counts[hist[-1]] += 1
                row[3] = pos
            owner = [r for r, pr in enumerate(self.prompts) if hist[:len(pr)] == pr]
            if not owner or not self.params[owner[0]].counted:               # still filling, the shared prefix, or a request without penalties
                assert (f, p) == (0.0, 0.0), (s, owner)
                continue
            assert len(owner) == 1
            sp, n = self.params[owner[0]], len(self.prompts[owner[0]])
            assert (f, p, start) == (sp.frequency_penalty, sp.presence_penalty, n), (s, owner)
            assert +counts == Counter(hist[n:]) and row[3] == pos, (s, owner, counts, hist[n:])
            self.checked += 1

    def step_batch(self, tokens, caches):
        out = super().step_batch(tokens, caches)
        self._tail(caches)
        return out

    def prefill_batch(self, prompts, caches):
        out = super().prefill_batch(prompts, caches)
        self._tail(caches)
        return out

    def step_mixed(self, tokens, decode_caches, prompts, prompt_caches):
        out = super().step_mixed(tokens, decode_caches, prompts, prompt_caches)
        self._tail(list(decode_caches) + list(prompt_caches))
        return out


@pytest.mark.parametrize("kw", [dict(), dict(mixed=False), dict(prefill_chunk=16), dict(prefill_chunk=1), dict(share_prefix=True), dict(kv_dtype=torch.int8)])
@pytest.mark.parametrize("slots,pages", [(1, 8), (3, 12), (8, 48)])
def test_engine_keeps_every_rows_counts_with_its_occupant(kw, slots, pages):
    prefix = list(range(70)) if kw.get("share_prefix") else ()
    prompts = requests(11, 13, hi=120, prefix=prefix)
    kinds = [SamplingParams(frequency_penalty=0.5), SamplingParams(), SamplingParams(presence_penalty=-1.0, temp=0.7, seed=3),
             SamplingParams(frequency_penalty=2.0, presence_penalty=2.0, repetition_penalty=1.2)]
    params = [kinds[i % 4] for i in range(len(prompts))]
    stop, new = {3, 77}, 9
    model = CountStub(prompts, params)
    # (the stub's tokens ignore the penalties and the records: what is checked is whose state sits in which row, pass after pass)
    model.set_batch_tail = lambda rows_cap: None
    model.write_batch_tail = lambda rows, recs, fed=None: None
    model.clear_batch_tail = lambda: None
    eng = BatchedEngine(model, num_pages=pages, max_batch=slots, stop_tokens=stop, **kw)
    out = eng.generate(prompts, new, sampling=params)
    assert out == [alone(p, new, stop) for p in prompts]
    assert model.sets == 1 and not model.armed and model.checked > 0
    assert eng.generate(prompts, new, sampling=[SamplingParams(temp=0.7, seed=1)] * len(prompts)) == out and model.sets == 1   # nobody asks: not armed
