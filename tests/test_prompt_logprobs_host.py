"""CPU: log-probabilities of prompt tokens -- the exported symbols, every refusal of the op and of the decoder's setter
before any launch, the numpy reference, the maps the engines build from host records, and the targets and counts BatchedEngine writes
for every pass (checked by hand for a chunked prompt, and through the whole scheduler on a stub model)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import prompt_logprobs_reference as pref
from tests import top_logprobs_reference as tref
from tests.test_batch_engine_host import V, StubModel, alone, next_token, requests

ARG, SHAPE, ALIGN, STATE = -1, -2, -3, -5


def stand_ins():
    buf = ctypes.create_string_buffer(8192)
    base = (ctypes.addressof(buf) + 255) & ~255
    return buf, ctypes.c_void_p(base), ctypes.c_void_p(base + 1), ctypes.c_void_p(base + 2), ctypes.c_void_p(base + 4)   # never dereferenced


def test_symbols_and_sizes_without_gpu():
    from proxy_inference_engine_amd import _ffi, build
    build.build()
    lib = _ffi.load()
    for name in ("pie_prompt_logprobs_workspace_bytes", "pie_prompt_logprobs", "pie_decoder_prompt_logprobs_workspace_bytes", "pie_decoder_set_prompt_logprobs"):
        assert name in _ffi.EXPORTS and hasattr(lib, name)
    size = lib.pie_prompt_logprobs_workspace_bytes
    # per row: 256 partials of 16 bytes, one float (the rows' floats padded to 8 bytes), slices x n composites
    assert size(1, 128256, 20) == 4096 + 8 + 251 * 20 * 8 and size(3, 513, 5) == 3 * 4096 + 16 + 3 * 2 * 5 * 8 and size(2, 1, 1) == 2 * 4096 + 8 + 2 * 8
    assert size(65535, 524288, 20) == 65535 * 4096 + 65535 * 4 + 4 + 65535 * 1024 * 20 * 8
    for rows, Vv, n in ((0, 512, 5), (65536, 512, 5), (1, 0, 5), (1, 524289, 5), (1, 512, 0), (1, 512, 21), (-1, 512, 5)):
        assert size(rows, Vv, n) == 0, (rows, Vv, n)
    assert lib.pie_decoder_prompt_logprobs_workspace_bytes(None, 5, 256) == 0


def test_op_refuses_before_any_launch_without_gpu():
    """Every refusal pie_prompt_logprobs makes, its code, its order and the name pie_last_error() carries: none of these calls reaches HIP."""
    from proxy_inference_engine_amd import _ffi
    lib = _ffi.load()
    buf, p, odd1, odd2, odd4 = stand_ins()
    BF16 = _ffi.PIE_BF16
    ok = [p, 2, 512, BF16, 5, p, p, p, p, p, None]   # logits, rows, V, dtype, n, targets, count, out_ids, out_vals, workspace, stream
    cases = [(4, 0, ARG), (4, -1, ARG), (4, 21, ARG), (0, None, ARG), (7, None, ARG), (8, None, ARG), (9, None, ARG),
             (1, 0, SHAPE), (1, -2, SHAPE), (1, 65536, SHAPE), (2, 0, SHAPE), (2, -5, SHAPE), (2, 524289, SHAPE),
             (5, odd2, ALIGN), (6, odd2, ALIGN), (7, odd2, ALIGN), (8, odd2, ALIGN), (0, odd1, ALIGN), (9, odd2, ALIGN), (9, odd4, ALIGN),
             (3, 7, ARG), (3, -1, ARG)]
    for i, v, code in cases:
        args = ok[:i] + [v] + ok[i + 1:]
        rc = lib.pie_prompt_logprobs(*args)
        err = lib.pie_last_error()
        assert rc == code and err.split(b":")[0] == b"pie_prompt_logprobs", (i, v, rc, err)
    # n is judged first, then the shape, then the alignment, then the dtype
    assert lib.pie_prompt_logprobs(odd1, 0, 0, 7, 21, p, p, p, p, p, None) == ARG and b"n must be" in lib.pie_last_error()
    assert lib.pie_prompt_logprobs(odd1, 0, 512, 7, 5, p, p, p, p, p, None) == SHAPE
    assert lib.pie_prompt_logprobs(odd1, 2, 512, 7, 5, p, p, p, p, p, None) == ALIGN
    assert lib.pie_prompt_logprobs(p, 2, 512, 7, 5, p, p, p, p, p, None) == ARG and b"dtype" in lib.pie_last_error()


def check_setter_refusals(lib, dec, vocab):
    """Every refusal pie_decoder_set_prompt_logprobs makes on a live decoder `dec`, each before any launch, and the size helper's zeros.
    A decoder exists only where a device does, so tests/test_gpu_prompt_logprobs.py runs this; the pointers are stand-ins all the same."""
    buf, p, odd1, odd2, odd4 = stand_ins()
    size = lib.pie_decoder_prompt_logprobs_workspace_bytes
    need = size(dec, 5, 16)
    assert need == (16 * vocab * 2 + 15) // 16 * 16 + lib.pie_prompt_logprobs_workspace_bytes(16, vocab, 5)
    assert size(dec, 5, 7) == 0 and size(dec, 5, 1025) == 0 and size(dec, 0, 16) == 0 and size(dec, 21, 16) == 0
    ok = [dec, 5, 40, 16, p, p, p, p, p, need]    # d, n, rows_cap, block_rows, targets, count, out_ids, out_vals, workspace, workspace_bytes
    cases = [(1, 21, ARG), (1, -1, ARG), (3, 7, ARG), (3, 1025, ARG), (4, None, ARG), (5, None, ARG), (6, None, ARG), (7, None, ARG), (8, None, ARG),
             (2, 0, SHAPE), (2, 65536, SHAPE), (4, odd2, ALIGN), (5, odd2, ALIGN), (6, odd2, ALIGN), (7, odd2, ALIGN), (8, odd4, ALIGN),
             (8, ctypes.c_void_p(p.value + 8), ALIGN), (9, need - 1, SHAPE)]
    for i, v, code in cases:
        args = ok[:i] + [v] + ok[i + 1:]
        rc = lib.pie_decoder_set_prompt_logprobs(*args)
        err = lib.pie_last_error()
        assert rc == code and err.split(b":")[0] == b"pie_decoder_set_prompt_logprobs", (i, v, rc, err)
    assert lib.pie_decoder_set_prompt_logprobs(*ok) == 0
    assert lib.pie_decoder_set_prompt_logprobs(dec, 0, 0, 0, None, None, None, None, None, 0) == 0     # off: nothing else is looked at


def test_setter_refuses_a_null_decoder_without_gpu():
    """The setter's other rules need a decoder, and a decoder needs a device: check_setter_refusals runs with the GPU tests."""
    from proxy_inference_engine_amd import _ffi
    lib = _ffi.load()
    buf, p, odd1, odd2, odd4 = stand_ins()
    assert lib.pie_decoder_set_prompt_logprobs(None, 5, 40, 16, p, p, p, p, p, 1 << 30) == ARG
    assert lib.pie_last_error().split(b":")[0] == b"pie_decoder_set_prompt_logprobs"
    assert lib.pie_decoder_set_prompt_logprobs(None, 0, 0, 0, None, None, None, None, None, 0) == ARG


def test_reference_is_the_ranking_of_the_subtracted_row():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(700).astype(np.float32) * 3
    lse = pref.lse64(x)
    assert abs(lse - np.log(np.exp(x.astype(np.float64)).sum())) < 1e-12 and pref.lse64(np.full(4, -np.inf)) == -np.inf
    lp = pref.logprobs(x)
    assert lp.dtype == np.float32 and np.array_equal(lp, x - np.float32(lse))
    ids, bits = pref.reference(x, 5, target=9)
    want = tref.reference(lp, 5, token=9)
    assert np.array_equal(ids, want[0]) and np.array_equal(bits, want[1]) and ids[0] == 9
    assert pref.reference(x, 5, target=9, count=-1) is None
    # two distinct logits whose log-probabilities collide under a large lse: the lower id wins, though its logit is the smaller one
    y = np.full(64, -100.0, np.float32)
    y[7], y[40], y[41] = 30000.0, np.float32(1e-3), np.float32(2e-3)
    ids, bits = pref.reference(y, 3, target=41)
    assert ids[1:].tolist() == [7, 40, 41] and bits[2] == bits[3] == bits[0]


def test_maps_from_host_records():
    from proxy_inference_engine_amd.engine.inference_engine import prompt_maps, prompt_targets
    prompt = [5, 9, 9, 3]
    assert prompt_targets(prompt, 2) == ([9, 9, 3, 0], [2, 2, 2, -1])
    assert prompt_targets([8], 0) == ([0], [-1])
    n = 3
    ids = np.full((4, n + 1), -1, np.int32)
    vals = np.full((4, n + 1), -np.inf, np.float32)
    ids[0], vals[0] = [9, 4, 9, 1], [-1.0, -0.5, -1.0, -2.0]         # the token is among the best
    ids[1], vals[1] = [9, 2, 6, 7], [-4.0, -1.0, -1.0, -1.5]         # absent: appended; the tie 2 / 6 keeps the record's order (lowest id first)
    ids[2], vals[2] = [3, 1, -1, -1], [-0.25, -0.25, -np.inf, -np.inf]   # fewer ids than n: the fill is dropped
    ids[3], vals[3] = [-7, -7, -7, -7], [123.0] * 4                  # the last row's record is never read
    maps = prompt_maps(ids, vals, n)
    assert maps[0] is None and len(maps) == len(prompt)
    assert list(maps[1].items()) == [(4, -0.5), (9, -1.0), (1, -2.0)]
    assert list(maps[2].items()) == [(2, -1.0), (6, -1.0), (7, -1.5), (9, -4.0)]
    assert list(maps[3].items()) == [(1, -0.25), (3, -0.25)]
    assert [list(m.items()) for m in prompt_maps(ids, vals, 0)[1:]] == [[(9, -1.0)], [(9, -4.0)], [(3, -0.25)]]   # top_logprobs = 0: the token alone
    assert prompt_maps(ids[:1], vals[:1], 3) == [None]


def test_targets_and_counts_of_a_chunked_prompt():
    from proxy_inference_engine_amd.engine.batch_engine import pass_targets
    prompts = [[10, 11, 12, 13, 14, 15, 16], [20, 21, 22], [30, 31]]
    wants = [2, None, 0]
    # a pass behind two decode rows: rows 3..5 of prompt 0 (the chunk ends inside it), all of prompt 1 (not scored), all of prompt 2
    targets, counts = pass_targets(prompts, wants, [(0, 3, 3), (1, 0, 3), (2, 0, 2)])
    assert targets == [14, 15, 16, 0, 0, 0, 31, 0]          # the row at the chunk boundary (token 15) targets token 16 of the NEXT pass
    assert counts == [2, 2, 2, -1, -1, -1, 0, -1]           # prompt 2's last row, and every row of the unscored prompt: left alone
    targets, counts = pass_targets(prompts, wants, [(0, 6, 1)])
    assert (targets, counts) == ([0], [-1])                  # the prompt's last row, alone in its pass
    assert pass_targets(prompts, wants, [(0, 0, 7)]) == ([11, 12, 13, 14, 15, 16, 0], [2] * 6 + [-1])


def test_batched_engine_checks_prompt_logprobs_before_anything_runs():
    from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine
    model = StubModel()
    prompts = [[1, 2, 3], [4, 5]]
    with pytest.raises(ValueError, match="share_prefix"):
        BatchedEngine(model, num_pages=16, max_batch=2, share_prefix=True).generate(prompts, 4, prompt_logprobs=2)
    eng = BatchedEngine(model, num_pages=16, max_batch=2)
    for bad in ([3], [3, 0, 1], [3, 21], [-1, 2], 21, -1, [1.5, 2], [True, 2], True):
        with pytest.raises(ValueError, match="prompt_logprobs"):
            eng.generate(prompts, 4, prompt_logprobs=bad)
    with pytest.raises(ValueError, match="max_new_tokens"):
        eng.generate(prompts, 0, prompt_logprobs=2)
    assert not model.calls                                                   # no pass ran
    plain = eng.generate(prompts, 4)
    assert isinstance(plain, list) and isinstance(plain[0], list)            # None: the return shape of before
    assert eng.generate(prompts, 4, prompt_logprobs=[None, None]) == (plain, [None, None])     # nobody asked: nothing is armed (the stub has no setter)


class ScoringStub(StubModel):
    """StubModel with the prompt-scoring surface: every pass writes, for each of its prompt rows whose count is not negative, a record that is
    a function of the row's history alone -- slot 0 (target, -(history length)), then count pairs derived from next_token(history)."""

    def set_prompt_logprobs(self, rows_cap, n, block_rows=256):
        self.pl = {"targets": torch.zeros(rows_cap, dtype=torch.int32), "count": torch.full((rows_cap,), -1, dtype=torch.int32),
                   "ids": torch.full((rows_cap, n + 1), -7, dtype=torch.int32), "vals": torch.full((rows_cap, n + 1), 123.0)}
        self.pl_n = n
        return self.pl

    def clear_prompt_logprobs(self):
        self.pl = None

    @staticmethod
    def record(hist, target, c, n):
        best = [(next_token(hist) + 3 * k) % V for k in range(c)]
        return [target] + best + [-1] * (n - c), [-float(len(hist))] + [-0.5 - k for k in range(c)] + [float("-inf")] * (n - c)

    def _score(self, row0, prompts, caches):
        if getattr(self, "pl", None) is None:
            return
        r = row0
        for p, c in zip(prompts, caches):
            seq = c[0].page_manager
            hist = list(self._hist(seq)) if seq.offset else []
            for t in p:
                hist.append(int(t))
                cnt = int(self.pl["count"][r])
                if cnt >= 0:
                    ids, vals = self.record(hist, int(self.pl["targets"][r]), min(cnt, self.pl_n), self.pl_n)
                    self.pl["ids"][r], self.pl["vals"][r] = torch.tensor(ids, dtype=torch.int32), torch.tensor(vals)
                r += 1

    def step(self, ids, cache):
        self._score(0, [ids.reshape(-1).tolist()], [cache])
        return super().step(ids, cache)

    def prefill_batch(self, prompts, caches):
        self._score(0, prompts, caches)
        return super().prefill_batch(prompts, caches)

    def step_mixed(self, tokens, decode_caches, prompts, prompt_caches):
        self._score(len(decode_caches), prompts, prompt_caches)
        return super().step_mixed(tokens, decode_caches, prompts, prompt_caches)


@pytest.mark.parametrize("kw", [dict(), dict(mixed=False), dict(batch_prefill=False), dict(prefill_chunk=16), dict(prefill_chunk=1), dict(max_prefill_rows=64),
                                dict(kv_dtype=torch.int8)])
@pytest.mark.parametrize("slots,pages", [(1, 6), (3, 9), (8, 40)])
def test_every_prompt_token_gets_its_own_rows_record(kw, slots, pages):
    """However the scheduler cuts the prompts into passes, entry j of a request's list is the record of the row that holds token j - 1 of
    ITS prompt, with token j as the target -- and the outputs do not notice."""
    from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine
    prompts = requests(11, 9, hi=90)
    wants = [(None, 0, 2, 5, 20)[i % 5] for i in range(len(prompts))]
    stop, new = {3, 77}, 5
    model = ScoringStub()
    eng = BatchedEngine(model, num_pages=pages, max_batch=slots, stop_tokens=stop, **kw)
    out, maps = eng.generate(prompts, new, prompt_logprobs=wants)
    assert out == [alone(p, new, stop) for p in prompts] and model.pl is None
    from proxy_inference_engine_amd.engine.inference_engine import host_record_to_map
    for p, w, m in zip(prompts, wants, maps):
        if w is None:
            assert m is None
            continue
        assert len(m) == len(p) and m[0] is None
        for j in range(1, len(p)):
            ids, vals = ScoringStub.record(p[:j], p[j], w, max(max(x for x in wants if x is not None), 1))
            assert m[j] == host_record_to_map(np.asarray(ids, np.int32), np.asarray(vals, np.float32), w)[1], (j, w)
