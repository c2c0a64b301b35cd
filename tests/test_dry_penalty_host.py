"""The DRY penalty without a device: the numpy reference on hand-computed windows, the record's layout, the argument rules of
the pack helper and of the Python layers, SamplingParams' fields, where InferenceEngine routes a request that carries it, and
BatchedEngine's bookkeeping of every row's record and ring on a stub model."""
import ctypes as C

import numpy as np
import pytest
import torch

from proxy_inference_engine_amd import _ffi, hip_ops
from proxy_inference_engine_amd.engine import BatchedEngine, SamplingParams
from proxy_inference_engine_amd.engine.inference_engine import InferenceEngine, check_speculative, fused_tail_plan
from proxy_inference_engine_amd.logits_processors import dry_logits_processor, make_logit_bias, make_repetition_penalty
from proxy_inference_engine_amd.samplers import make_sampler
from tests import dry_penalty_reference as ref
from tests.test_batch_engine_host import StubModel, alone, requests

M, B, A = 0.8, 1.75, 2


def test_reference_on_hand_computed_windows():
    win = np.tile(np.arange(5), 40)
    pen = ref.penalties(win, 100, M, B, A)
    assert list(pen) == [0] and pen[0][0] == 64 and pen[0][1] == np.float32(936373540000000.0)
    p = np.float32(M)
    for _ in range(62):
        p = np.float32(p * np.float32(B))
    assert pen[0][1] == p and pen[0][1].dtype == np.float32
    assert ref.penalties(win, 100, M, B, A, breakers=[3]) == {}
    for seed in range(3):
        rng = np.random.default_rng(seed)
        assert len(ref.penalties(rng.integers(0, 4, 1024), 100, M, B, A)) == 4
        assert ref.penalties(rng.integers(0, 4, 2), 100, M, B, A) == {} and ref.penalties(rng.integers(0, 4, 3), 100, M, B, A) == {}
        assert ref.penalties(rng.integers(0, 50000, 1024), 50000, M, B, A) == {}
    # small cases by hand: "a b a b a" -> the next b would extend a repeat of length 3 (a, b a, a b a is cut by the window's start at i = 2)
    assert {t: L for t, (L, _) in ref.penalties([7, 8, 7, 8, 7], 100, M, B, 1).items()} == {8: 3}
    assert ref.penalties([7, 8, 7, 8, 7], 100, M, B, 3)[8][1] == np.float32(M) and ref.penalties([7, 8, 7, 8, 7], 100, M, B, 4) == {}
    assert ref.penalties([7, 8, 7, 8, 7], 8, M, B, 1) == {}                    # t = 8 lies outside [0, V)
    assert ref.penalties([7, 8, 7, 8, 7], 100, 0.0, B, 1) == {}                # multiplier 0: off
    assert {t: L for t, (L, _) in ref.penalties([1, 2, 3, 9, 2, 3, 5, 1, 2, 3], 100, M, B, 1).items()} == {9: 3, 5: 2}
    x = np.array([0x3F80, 0x4000, 0xFF80], np.uint16)                          # bf16 1.0, 2.0, -inf
    assert ref.apply(x, "bfloat16", [1, 0, 1, 0, 1], M, B, 1).tolist() == [0xBFBA, 0x4000, 0xFF80]   # 1.0 - 0.8 * 1.75^2 = -1.45 -> bf16 -1.453125
    assert ref.apply(x, "bfloat16", [1, 2, 1, 2, 1], M, B, 1).tolist() == [0x3F80, 0x4000, 0xFF80]   # -inf stays -inf


def test_record_layout_matches_the_library():
    assert C.sizeof(_ffi.pie_dry_penalty) == 24 == int(_ffi.load().pie_dry_penalty_bytes()) and hip_ops.DRY_PENALTY_WORDS == 6
    assert [(n, getattr(_ffi.pie_dry_penalty, n).offset) for n, _ in _ffi.pie_dry_penalty._fields_] == \
        [("multiplier", 0), ("base", 4), ("allowed_length", 8), ("range", 12), ("n_breakers", 16), ("reserved", 20)]
    assert (hip_ops.DRY_MAX_MATCH, hip_ops.DRY_BREAKERS_MAX) == (64, 64)
    rec = hip_ops.dry_penalty_pack(0.5, 2.0, 3, 100, 7)
    assert (rec.multiplier, rec.base, rec.allowed_length, rec.range, rec.n_breakers, rec.reserved) == (0.5, 2.0, 3, 100, 7, 0)
    table = hip_ops.dry_penalty_records([rec, hip_ops.dry_penalty_pack()])
    assert table.dtype == torch.int32 and table.shape == (2, 6) and table[0, 2:].tolist() == [3, 100, 7, 0]
    assert table[1, :1].view(torch.float32).item() == 0.0                                              # the default is the zero record
    assert hip_ops.dry_breaker_table((5, 9)).tolist() == [5, 9] + [0] * 62


def test_pack_argument_rules():
    rec, lib = _ffi.pie_dry_penalty(), _ffi.load()
    ok = dict(m=0.8, b=1.75, a=2, r=1024, n=0)
    call = lambda **kw: lib.pie_dry_penalty_pack(*({**ok, **kw}[k] for k in "mbarn"), C.byref(rec))
    assert call() == 0 and call(m=0.0) == 0 and call(a=1) == 0 and call(a=64) == 0 and call(r=1) == 0 and call(n=64) == 0 and call(b=1e-30) == 0
    for bad in (dict(m=-0.1), dict(m=float("nan")), dict(m=float("inf")), dict(m=1e300), dict(b=0.0), dict(b=-1.75), dict(b=float("nan")),
                dict(b=float("inf")), dict(b=1e300), dict(b=1e-60), dict(a=0), dict(a=65), dict(r=0), dict(r=1025), dict(n=-1), dict(n=65)):
        assert call(**bad) == -1 and b"pie_dry_penalty_pack" in lib.pie_last_error(), bad
        full = {**ok, **bad}
        with pytest.raises(ValueError):
            hip_ops.dry_penalty_pack(full["m"], full["b"], full["a"], full["r"], full["n"])
    assert lib.pie_dry_penalty_pack(0.8, 1.75, 2, 1024, 0, None) == -1


@pytest.mark.parametrize("bad", [dict(dry_multiplier=-1.0), dict(dry_multiplier=float("nan")), dict(dry_multiplier=0.8, dry_base=0.0),
                                 dict(dry_multiplier=0.8, dry_base=float("inf")), dict(dry_multiplier=0.8, dry_allowed_length=0),
                                 dict(dry_multiplier=0.8, dry_allowed_length=65), dict(dry_multiplier=0.8, dry_allowed_length=2.5),
                                 dict(dry_multiplier=0.8, dry_range=0), dict(dry_multiplier=0.8, dry_range=1025),
                                 dict(dry_multiplier=0.8, dry_sequence_breakers=tuple(range(65))), dict(dry_multiplier=0.8, dry_sequence_breakers=(2 ** 31,))])
def test_python_layers_refuse_bad_arguments(bad):
    with pytest.raises(ValueError):
        SamplingParams(**bad).dry()
    stub = DryStub([[1, 2, 3]], [SamplingParams(**bad)])
    with pytest.raises(ValueError):
        BatchedEngine(stub, num_pages=8, max_batch=2).generate([[1, 2, 3]], 4, sampling=SamplingParams(**bad))
    assert not stub.calls and stub.sets == 0                                   # refused before anything ran or was armed
    with pytest.raises(ValueError):
        InferenceEngine(model=object()).make_processors(**bad)
    names = dict(dry_multiplier="multiplier", dry_base="base", dry_allowed_length="allowed_length", dry_range="range", dry_sequence_breakers="sequence_breakers")
    with pytest.raises(ValueError):
        dry_logits_processor(**{names[k]: v for k, v in bad.items()})


def test_sampling_params_account_for_dry():
    sp = SamplingParams()
    assert (sp.dry_multiplier, sp.dry_base, sp.dry_allowed_length, sp.dry_range, sp.dry_sequence_breakers) == (0.0, 1.75, 2, 1024, ())
    assert sp.tailless and sp.plain and not sp.dried and sp.dry() == (0.0, 1.75, 2, 1024, ())
    sp = SamplingParams(dry_multiplier=0.8, dry_sequence_breakers=[13, 198])
    assert sp.dried and not sp.tailless and not sp.plain and sp.recordless and not sp.counted
    assert sp.dry() == (0.8, 1.75, 2, 1024, (13, 198))
    assert sp.record().mode == -1 and sp.record().penalty == 1.0               # pie_row_tail knows nothing of it


def test_make_processors_and_the_fused_plan():
    eng = InferenceEngine(model=object())
    assert eng.make_processors() == [] and eng.make_processors(dry_multiplier=0.0) == [] and eng.make_processors(dry_multiplier=None) == []
    procs = eng.make_processors(dry_multiplier=0.8, dry_sequence_breakers=[13])
    assert len(procs) == 1
    p = procs[0]
    assert (p.dry_multiplier, p.dry_base, p.dry_allowed_length, p.dry_range, p.dry_sequence_breakers) == (0.8, 1.75, 2, 1024, (13,))
    greedy = make_sampler(temp=0.0)
    plan = fused_tail_plan(procs, greedy)
    assert plan is not None and plan["dry"] is p and plan["mask"] is None and plan["bias"] is None and "counts" not in plan and plan["repetition_penalty"] == 1.0
    plan = fused_tail_plan(procs, make_sampler(temp=0.8, top_k=5))
    assert plan is not None and plan["sampler"] is not None and plan["dry"] is p
    # the order the kernels define: penalty, bias, frequency / presence, DRY
    full = eng.make_processors(repetition_penalty=1.3, logit_bias={3: 1.0}, presence_penalty=1.0, dry_multiplier=0.5, dry_base=2.0, dry_allowed_length=3, dry_range=64)
    assert len(full) == 4 and hasattr(full[0], "penalty") and hasattr(full[2], "presence_penalty") and full[3].dry_range == 64
    plan = fused_tail_plan(full, greedy)
    assert plan is not None and plan["dry"] is full[3] and plan["counts"] is full[2] and plan["bias"] is full[1] and plan["repetition_penalty"] == 1.3
    assert fused_tail_plan([full[3], full[2]], greedy) is None and fused_tail_plan([p, p], greedy) is None and fused_tail_plan([full[3], full[0]], greedy) is None
    # a request without DRY gets the plan it always got
    for same in ([], [make_repetition_penalty(1.3, 20), make_logit_bias({3: 1.0})], eng.make_processors(frequency_penalty=0.5)):
        plan = fused_tail_plan(same, greedy)
        assert "dry" not in plan and set(plan) - {"counts"} == {"sampler", "repetition_penalty", "context_size", "mask", "bias"}
    # a structuring engine, a tensor-parallel model, a foreign sampler: the processor branch
    assert fused_tail_plan(procs, greedy, structuring_engine=object()) is None
    assert fused_tail_plan(procs, greedy, tensor_parallel=True) is None
    assert fused_tail_plan(procs, lambda x: x) is None


def test_a_dry_request_with_speculation_is_refused_as_logits_processors():
    procs = InferenceEngine(model=object()).make_processors(dry_multiplier=0.8)
    model = type("M", (), {"spec_step": None, "tp": None})()
    with pytest.raises(ValueError, match="logits processors"):
        check_speculative(model, make_sampler(temp=0.0), procs, None, None, None, None)
    check_speculative(model, make_sampler(temp=0.0), [], None, None, None, None)


# ------------------------------------------------------------------ BatchedEngine's bookkeeping, on the stub model of tests/test_batch_engine_host.py
class DryStub(StubModel):
    """StubModel + the batch DRY penalty's surface.  It keeps every row's record and ring as the device would -- every output row records
    its input id at ring[pos & 1023], zero record or not -- and then checks the row against the request that sits in it: a request with DRY
    finds its own record and, over its window, exactly the ids it has been fed; a request without, a prompt that is still filling and the
    shared prefix's own pass find a zero record."""

    def __init__(self, prompts, params):
        super().__init__()
        self.prompts, self.params = [list(p) for p in prompts], params
        self.rows, self.armed, self.sets, self.checked, self.rewritten = {}, False, 0, 0, 0

    def set_batch_dry_penalty(self, rows_cap):
        self.armed, self.sets, self.rows_cap = True, self.sets + 1, rows_cap
        self.rows = {s: [None, [-1] * 1024] for s in range(rows_cap)}

    def write_batch_dry_penalty(self, rows, records, fed=None):
        assert self.armed and len(rows) == len(records) and (fed is None or len(fed) == len(rows))
        for i, (s, rec) in enumerate(zip(rows, records)):
            ring = self.rows[s][1]
            if fed is not None and fed[i] is not None:
                ids = list(fed[i])
                ring = [0] * 1024
                for q in range(max(0, len(ids) - 1024), len(ids)):
                    ring[q & 1023] = ids[q]
                self.rewritten += rec is not None
            self.rows[s] = [rec, ring]

    def clear_batch_dry_penalty(self):
        self.armed = False

    def _tail(self, caches):
        if not self.armed:
            return
        assert len(caches) <= self.rows_cap
        for s, c in enumerate(caches):
            hist = self._hist(c[0].page_manager)
            rec, ring = self.rows[s]
            pos = len(hist) - 1
            ring[pos & 1023] = hist[-1]                                       # recorded on every live row
            owner = [r for r, pr in enumerate(self.prompts) if hist[:len(pr)] == pr]
            if not owner or not self.params[owner[0]].dried:                  # still filling, the shared prefix, or a request without DRY
                assert rec is None, (s, owner)
                continue
            assert len(owner) == 1
            sp = self.params[owner[0]]
            assert rec == sp.dry(), (s, owner, rec)
            n = min(pos + 1, rec[3])
            assert [ring[q & 1023] for q in range(pos + 1 - n, pos + 1)] == hist[-n:], (s, owner)
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


@pytest.mark.parametrize("kw", [dict(), dict(mixed=False), dict(prefill_chunk=16), dict(share_prefix=True), dict(kv_dtype=torch.int8)])
@pytest.mark.parametrize("slots,pages", [(1, 8), (3, 12), (8, 48)])
def test_engine_keeps_every_rows_ring_and_record_with_its_occupant(kw, slots, pages):
    prefix = list(range(70)) if kw.get("share_prefix") else ()
    prompts = requests(11, 13, hi=120, prefix=prefix)
    kinds = [SamplingParams(dry_multiplier=0.8), SamplingParams(), SamplingParams(dry_multiplier=0.5, dry_range=40, temp=0.7, seed=3),
             SamplingParams(dry_multiplier=2.0, dry_base=2.0, dry_allowed_length=3, dry_sequence_breakers=(3, 77), frequency_penalty=0.5)]
    params = [kinds[i % 4] for i in range(len(prompts))]
    stop, new = {3, 77}, 9
    model = DryStub(prompts, params)
    # (the stub's tokens ignore the penalties and the records: what is checked is whose state sits in which row, pass after pass)
    for name in ("set_batch_tail", "clear_batch_tail", "set_batch_count_penalty", "clear_batch_count_penalty"):
        setattr(model, name, lambda *a, **k: None)
    model.write_batch_tail = lambda rows, recs, fed=None: None
    model.write_batch_count_penalty = lambda rows, recs, generated=None: None
    eng = BatchedEngine(model, num_pages=pages, max_batch=slots, stop_tokens=stop, **kw)
    out = eng.generate(prompts, new, sampling=params)
    assert out == [alone(p, new, stop) for p in prompts]
    assert model.sets == 1 and not model.armed and model.checked > 0
    n_dry = sum(sp.dried for sp in params)
    assert model.rewritten >= n_dry                                           # every DRY request's ring and record were written when it took a row
    assert slots >= len(prompts) or model.rewritten > 0                       # rows were reseated: the later occupants found their own state (checked in _tail)
    assert eng.generate(prompts, new, sampling=[SamplingParams(temp=0.7, seed=1)] * len(prompts)) == out and model.sets == 1   # nobody asks: not armed
