"""Per-row tails without a device: the record packer of the C ABI (pie_row_tail_pack: a host function), its ctypes mirror,
SamplingParams' branch choice, and BatchedEngine's bookkeeping of which record sits in which row of a pass -- on the stub model of
tests/test_batch_engine_host.py, extended by a table that advances `calls` the way the draw kernel does."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from proxy_inference_engine_amd import _ffi, hip_ops
from proxy_inference_engine_amd.engine import BatchedEngine, SamplingParams
from tests.test_batch_engine_host import StubModel, V, requests

GREEDY = _ffi.PIE_SAMPLE_GREEDY


def pack(mode, temp=1.0, p=0.0, k=0, seed=0, calls=0, penalty=1.0, context=60):
    rec = _ffi.pie_row_tail()
    rc = _ffi.load().pie_row_tail_pack(mode, temp, p, k, seed, calls, penalty, context, C.byref(rec))
    return rc, rec


# ------------------------------------------------------------------ the packer
def test_ctypes_record_is_the_headers():
    assert C.sizeof(_ffi.pie_row_tail) == int(_ffi.load().pie_row_tail_bytes()) == 40
    assert hip_ops.ROW_TAIL_WORDS * 8 == C.sizeof(_ffi.pie_row_tail)
    offs = {name: getattr(_ffi.pie_row_tail, name).offset for name, _ in _ffi.pie_row_tail._fields_}
    assert offs == dict(mode=0, inv_temp=4, thr=8, k=12, seed=16, calls=24, penalty=32, context_size=36)


@pytest.mark.parametrize("args", [
    dict(mode=4), dict(mode=-2),                                          # unknown mode
    dict(mode=0, temp=0.0), dict(mode=1, temp=-1.0, k=3),                 # temperature must be positive
    dict(mode=1, k=0), dict(mode=1, k=-4),                                # top_k in (0, V)
    dict(mode=3, p=0.0, k=1), dict(mode=3, p=1.5, k=1), dict(mode=3, p=0.1, k=0),   # min_p in (0, 1], min_tokens_to_keep >= 1
    dict(mode=2, p=0.0), dict(mode=2, p=1.0),                             # top_p in (0, 1)
    dict(mode=GREEDY, penalty=-0.5), dict(mode=GREEDY, penalty=math.inf), dict(mode=0, penalty=math.nan),   # pie_logits_penalty's rule
    dict(mode=GREEDY, context=0), dict(mode=0, context=1025), dict(mode=GREEDY, context=-1),
])
def test_pack_refuses_what_the_single_row_ops_refuse(args):
    rc, _ = pack(**args)
    assert rc == -1, args                                                 # PIE_E_ARG, before anything reaches a device
    kw = dict(args)
    mode = kw.pop("mode")
    names = {v: k for k, v in hip_ops.SAMPLE_MODES.items()}
    if mode in names or mode == GREEDY:
        with pytest.raises(ValueError):
            hip_ops.row_tail_pack(names.get(mode), kw.get("temp", 1.0), kw.get("p", 0.0), kw.get("k", 0), penalty=kw.get("penalty", 1.0),
                                  context_size=kw.get("context", 60))


def test_pack_null_record_is_refused():
    assert _ffi.load().pie_row_tail_pack(0, 1.0, 0.0, 0, 0, 0, 1.0, 60, None) == -1


@pytest.mark.parametrize("temp", [0.05, 0.7, 0.8, 1.0, 3.0, 1e-3])
@pytest.mark.parametrize("p", [0.05, 0.1, 0.775, 0.9, 0.999])
def test_pack_derives_the_fp32_values_of_sample_launch(temp, p):
    rc, r = pack(2, temp, p)
    assert rc == 0 and r.mode == 2 and r.k == 0
    assert np.float32(r.inv_temp).view(np.uint32) == np.float32(1.0 / temp).view(np.uint32)
    assert np.float32(r.thr).view(np.uint32) == np.float32(1.0 - p).view(np.uint32)
    rc, r = pack(3, temp, p, k=4)
    assert rc == 0 and r.mode == 3 and r.k == 4
    assert np.float32(r.inv_temp).view(np.uint32) == np.float32(1.0 / temp).view(np.uint32)
    assert np.float32(r.thr).view(np.uint32) == np.float32(np.log(np.float64(p))).view(np.uint32)
    rc, r = pack(1, temp, p, k=7, seed=2 ** 64 - 3, calls=2 ** 40 + 5, penalty=1.3, context=1024)
    assert rc == 0 and (r.mode, r.k, r.thr, r.seed, r.calls, r.context_size) == (1, 7, 0.0, 2 ** 64 - 3, 2 ** 40 + 5, 1024)
    assert np.float32(r.penalty) == np.float32(1.3)
    rc, r = pack(0, temp, p, k=9)
    assert rc == 0 and (r.mode, r.k, r.thr) == (0, 0, 0.0)              # categorical takes neither p nor k


def test_greedy_record_ignores_the_sampler_arguments():
    rc, r = pack(GREEDY, temp=0.0, p=7.0, k=-3, seed=5, calls=9, penalty=1.1, context=8)
    assert rc == 0 and (r.mode, r.inv_temp, r.thr, r.k, r.seed, r.calls, r.context_size) == (GREEDY, 1.0, 0.0, 0, 5, 9, 8)
    assert np.float32(r.penalty) == np.float32(1.1)
    t = hip_ops.row_tail_table([r, hip_ops.row_tail_pack()])
    assert t.dtype == torch.int64 and tuple(t.shape) == (2, hip_ops.ROW_TAIL_WORDS)
    assert bytes(t[0].numpy().tobytes()) == bytes(r)


# ------------------------------------------------------------------ SamplingParams
def test_sampling_params_defaults_are_the_issues():
    sp = SamplingParams()
    assert (sp.temp, sp.top_p, sp.top_k, sp.min_p, sp.min_tokens_to_keep, sp.seed, sp.repetition_penalty, sp.repetition_context_size) == \
        (0.0, 1.0, -1, 0.0, 1, None, 1.0, 60)
    assert sp.hip_spec() is None and sp.plain and sp.record().mode == GREEDY


@pytest.mark.parametrize("kw,spec", [
    (dict(temp=0.0, top_p=0.5, top_k=5, min_p=0.2), None),                                                 # temp == 0 is greedy whatever else is set
    (dict(temp=0.8, top_p=0.9, min_p=0.1, top_k=5), ("top_p", 0.8, 0.9, 0)),                               # make_sampler's order: top_p first
    (dict(temp=0.8, top_p=1.0, min_p=0.1, min_tokens_to_keep=3, top_k=5), ("min_p", 0.8, 0.1, 3)),         # ... then min_p
    (dict(temp=0.8, top_p=0.0, top_k=5), ("top_k", 0.8, 0.0, 5)),                                          # ... then top_k
    (dict(temp=1.5), ("categorical", 1.5, 0.0, 0)),
    (dict(temp=1.5, top_p=1.0, top_k=-1, min_p=0.0), ("categorical", 1.5, 0.0, 0)),
])
def test_sampling_params_pick_make_samplers_branch(kw, spec):
    from proxy_inference_engine_amd.samplers import make_sampler
    sp = SamplingParams(seed=11, repetition_penalty=1.2, repetition_context_size=8, **kw)
    assert sp.hip_spec() == spec
    closure = make_sampler(temp=sp.temp, top_p=sp.top_p, min_p=sp.min_p, min_tokens_to_keep=sp.min_tokens_to_keep, top_k=sp.top_k)
    assert getattr(closure, "hip_spec", None) == spec                     # the very branch the closure factory takes
    r = sp.record(calls=4)
    assert (r.seed, r.calls, r.context_size) == (11, 4, 8) and np.float32(r.penalty) == np.float32(1.2)
    if spec is None:
        assert r.mode == GREEDY and not sp.plain
    else:
        want = hip_ops.row_tail_pack(*spec, seed=11, calls=4, penalty=1.2, context_size=8)
        assert bytes(r) == bytes(want) and r.mode == hip_ops.SAMPLE_MODES[spec[0]]


# ------------------------------------------------------------------ the engine's bookkeeping
class TailStub(StubModel):
    """StubModel + the batch tail's surface.  Every pass checks each output row's record and ring against the request that sits in the
    row, then advances `calls` of the rows that draw, as k_smp_draw's last workgroup does."""

    def __init__(self, prompts, params, seeds, mark):
        super().__init__()
        self.prompts, self.params, self.seeds, self.mark = prompts, params, seeds, mark
        self.table, self.rings, self.armed = None, None, False
        self.checked = self.writes = 0

    def set_batch_tail(self, rows_cap):
        self.table = [hip_ops.row_tail_pack(mode="categorical", seed=99, calls=99)] * rows_cap      # stale records of an earlier use
        self.rings = np.full((rows_cap, 1024), -7, np.int64)
        self.armed = True

    def clear_batch_tail(self):
        self.armed = False

    def write_batch_tail(self, rows, records, fed=None):
        assert self.armed and len(rows) == len(records) and (fed is None or len(fed) == len(rows))
        for i, (r, rec) in enumerate(zip(rows, records)):
            self.table[r] = _ffi.pie_row_tail.from_buffer_copy(bytes(rec))
            self.writes += 1
            if fed is not None and fed[i] is not None:
                ids = list(fed[i])
                for q in range(max(0, len(ids) - 1024), len(ids)):
                    self.rings[r, q & 1023] = ids[q]

    def _row(self, s, cache, ids):
        """Output row s is about to process `ids` (its last one is the row's input id) on `cache`."""
        if not self.armed:
            return
        seq = cache[0].page_manager
        hist = (list(self._hist(seq)) if seq.offset else []) + [int(t) for t in ids]
        rec = self.table[s]
        r = hist[self.mark] if len(hist) > self.mark else None            # the request: its index is the id behind the shared prefix
        if r is None or len(hist) < len(self.prompts[r]):                  # the shared prefix's own pass, a prompt still filling: greedy, no penalty
            assert rec.mode == GREEDY and rec.penalty == 1.0, s
            return
        sp, L = self.params[r], len(self.prompts[r])
        assert hist[:L] == self.prompts[r]
        want = sp.record(calls=len(hist) - L, seed=self.seeds[r])         # tokens drawn so far = ids fed beyond the prompt
        if want.mode == GREEDY:
            want.calls = rec.calls                                         # a greedy row never draws: its counter is neither read nor advanced
        assert bytes(rec) == bytes(want), (s, r, rec.calls, want.calls)
        pos = len(hist) - 1
        self.rings[s, pos & 1023] = hist[pos]                              # (the kernel records the row's input id)
        if sp.repetition_penalty != 1.0:
            for q in range(max(0, pos + 1 - sp.repetition_context_size), pos + 1):
                assert self.rings[s, q & 1023] == hist[q], (s, r, q)
        if rec.mode != GREEDY:
            rec.calls += 1
        self.checked += 1

    def step_batch(self, tokens, caches):
        for s, (c, t) in enumerate(zip(caches, tokens.tolist())):
            self._row(s, c, [t])
        return super().step_batch(tokens, caches)

    def prefill_batch(self, prompts, caches):
        for s, (c, p) in enumerate(zip(caches, prompts)):
            self._row(s, c, p)
        return super().prefill_batch(prompts, caches)

    def step_mixed(self, tokens, decode_caches, prompts, prompt_caches):
        for s, (c, t) in enumerate(zip(decode_caches, tokens.tolist() if decode_caches else [])):
            self._row(s, c, [t])
        for j, (c, p) in enumerate(zip(prompt_caches, prompts)):
            self._row(len(decode_caches) + j, c, p)
        return super().step_mixed(tokens, decode_caches, prompts, prompt_caches)


def mixed_params(n):
    kinds = [SamplingParams(temp=0.8, top_k=5), SamplingParams(), SamplingParams(temp=0.9, top_p=0.9, repetition_penalty=1.1),
             SamplingParams(repetition_penalty=1.3, repetition_context_size=8), SamplingParams(temp=1.0, min_p=0.1, min_tokens_to_keep=2)]
    return [SamplingParams(**{**kinds[i % len(kinds)].__dict__, "seed": 1000 + i}) for i in range(n)]


@pytest.mark.parametrize("kw", [dict(), dict(mixed=False), dict(batch_prefill=False), dict(prefill_chunk=16), dict(kv_dtype=torch.int8),
                                dict(share_prefix=True)])
@pytest.mark.parametrize("slots,pages", [(1, 8), (2, 12), (4, 30)])
def test_engine_seats_every_request_in_its_row(kw, slots, pages):
    prefix = list(range(100, 100 + 70)) if kw.get("share_prefix") else []
    prompts = [prefix + [i] + p for i, p in enumerate(requests(5, 9, lo=1, hi=90))]     # a distinct id behind the prefix: requests are told apart
    params = mixed_params(len(prompts))
    model = TailStub(prompts, params, [sp.seed for sp in params], len(prefix))
    eng = BatchedEngine(model, num_pages=pages + 2, max_batch=slots, stop_tokens={3, 77}, **kw)
    out = eng.generate(prompts, 7, sampling=params)
    assert model.checked >= sum(len(o) for o in out) - len([p for p in params if p.plain])   # every drawn token's row was checked
    assert not model.armed                                                                # the tail is cleared on the way out
    plain = BatchedEngine(StubModel(), num_pages=pages + 2, max_batch=slots, stop_tokens={3, 77}, **kw).generate(prompts, 7)
    assert out == plain                                                                    # (the stub's tokens do not depend on the records)


def test_generate_sampling_argument_checks():
    model = StubModel()
    eng = BatchedEngine(model, num_pages=8, max_batch=2, sampler=lambda lp: lp.argmax(-1))
    with pytest.raises(ValueError, match="exclude"):
        eng.generate([[1, 2, 3]], 4, sampling=SamplingParams(temp=0.7))
    eng = BatchedEngine(StubModel(), num_pages=8, max_batch=2)
    with pytest.raises(ValueError, match="one per prompt"):
        eng.generate([[1, 2, 3], [4, 5]], 4, sampling=[SamplingParams()])
    with pytest.raises(ValueError):                                                        # refused before any pass runs
        eng.generate([[1, 2, 3]], 4, sampling=SamplingParams(temp=0.7, repetition_penalty=-1.0))
    with pytest.raises(ValueError):
        eng.generate([[1, 2, 3]], 4, sampling=SamplingParams(temp=0.7, repetition_context_size=2000))
    # all-plain records: today's passes, the model's tail surface is not even needed (StubModel has none)
    assert eng.generate([[1, 2, 3]], 3, sampling=SamplingParams()) == eng.generate([[1, 2, 3]], 3)
