"""CPU: the top-n log-probability contract -- the numpy reference against a brute-force sort, the op's refusals before any
launch, and BatchedEngine.generate's argument checks before anything runs."""
import ctypes

import numpy as np
import pytest

from tests import sampler_rows as sr
from tests import top_logprobs_reference as ref
from tests.test_batch_engine_host import StubModel

VOCABS = [7, 512, 1500, 4099]


@pytest.mark.parametrize("V", VOCABS)
def test_reference_equals_a_brute_force_sort(V):
    rows = ref.family_rows(V)
    assert [name for name, _ in rows][:len(sr.names(V))] == sr.names(V)
    for name, lp in rows:
        for n in (1, 5, 20):
            ids, bits = ref.reference(lp, n, token=V // 2)
            m = min(n, V)
            assert ids[1:1 + m].tolist() == ref.brute_force(lp, m), (name, V, n)
            assert np.array_equal(bits[1:1 + m], lp.view(np.uint32)[ids[1:1 + m]]), (name, V, n)
            assert ids[1 + m:].tolist() == [-1] * (n - m) and (bits[1 + m:] == 0xFF800000).all()
            assert ids[0] == V // 2 and bits[0] == lp.view(np.uint32)[V // 2]
        if name in ("uniform", "all_inf"):
            assert ref.reference(lp, 5)[0][1:].tolist() == list(range(min(5, V))) + [-1] * (5 - min(5, V))
        if name == "sparse3":
            allowed = sr.make("sparse3", V).notes["allowed"]
            ids = ref.reference(lp, 5)[0][1:]
            rest = [i for i in range(V) if i not in set(allowed.tolist())][:2]
            assert sorted(ids[:3].tolist()) == allowed.tolist() and ids[3:].tolist() == rest
        if name == "specials":
            top = lp.view(np.uint32)[ref.reference(lp, 4)[0][1:]].tolist()
            assert top == [0x7FC00000, 0x7F800000, 0x00000000, 0x80000000][:len(top)]
        if name == "boundary_tie":
            _, above, tie = ref.boundary_tie_row(V)
            ids = ref.reference(lp, 20)[0][1:]
            assert sorted(ids[:12].tolist()) == sorted(above.tolist()) and ids[12:].tolist() == np.sort(tie)[:8].tolist()
            assert len({int(i) // sr.SLICE for i in tie}) >= min(8, -(-V // sr.SLICE))


def test_reference_counts_and_slot_zero():
    lp = sr.quantized(1500, 3).lp
    full = ref.reference(lp, 20, token=7)
    assert ref.reference(lp, 20, token=7, count=-1) is None and ref.reference(lp, 20, token=7, count=-7) is None
    big = ref.reference(lp, 20, token=7, count=99)
    assert np.array_equal(big[0], full[0]) and np.array_equal(big[1], full[1])
    zero = ref.reference(lp, 20, token=7, count=0)
    assert zero[0].tolist() == [7] + [-1] * 20 and zero[1][0] == full[1][0]
    five = ref.reference(lp, 20, token=7, count=5)
    assert five[0][:6].tolist() == full[0][:6].tolist() and five[0][6:].tolist() == [-1] * 15
    for tok in (None, 1500, -3):
        ids, bits = ref.reference(lp, 5, token=tok)
        assert ids[0] == -1 and bits[0] == 0xFF800000
    items = ref.to_map(*ref.reference(lp, 3, token=int(full[0][2])), 3)
    assert [i for i, _ in items] == full[0][1:4].tolist()             # the token is among the best 3: not added again
    items = ref.to_map(*ref.reference(lp, 3, token=int(full[0][9])), 3)
    assert [i for i, _ in items] == full[0][1:4].tolist() + [int(full[0][9])]


def test_op_refuses_before_any_launch_without_gpu():
    """Every refusal pie_top_logprobs makes, its code and the name pie_last_error() carries: none of these calls reaches HIP."""
    from proxy_inference_engine_amd import _ffi, build
    build.build()
    lib = _ffi.load()
    buf = ctypes.create_string_buffer(8192)
    base = (ctypes.addressof(buf) + 255) & ~255
    p, odd2, odd4 = ctypes.c_void_p(base), ctypes.c_void_p(base + 2), ctypes.c_void_p(base + 4)   # stand-ins, never dereferenced
    ARG, SHAPE, ALIGN = -1, -2, -3
    ok = [p, 2, 512, 5, p, p, p, p, p, None]     # logprobs, rows, V, n, tokens, count, out_ids, out_vals, workspace, stream
    cases = [(3, 0, ARG), (3, -1, ARG), (3, 21, ARG), (0, None, ARG), (6, None, ARG), (7, None, ARG), (8, None, ARG),
             (2, 0, SHAPE), (2, 524289, SHAPE), (2, -5, SHAPE), (1, 0, SHAPE), (1, -2, SHAPE),
             (0, odd2, ALIGN), (4, odd2, ALIGN), (5, odd2, ALIGN), (6, odd2, ALIGN), (7, odd2, ALIGN), (8, odd2, ALIGN), (8, odd4, ALIGN)]
    for i, v, code in cases:
        args = ok[:i] + [v] + ok[i + 1:]
        rc = lib.pie_top_logprobs(*args)
        err = lib.pie_last_error()
        assert rc == code and err.split(b":")[0] == b"pie_top_logprobs", (i, v, rc, err)
    # n is judged first, then the shape, then the alignment
    assert lib.pie_top_logprobs(odd2, 0, 0, 21, p, p, p, p, p, None) == ARG
    assert lib.pie_top_logprobs(odd2, 0, 512, 5, p, p, p, p, p, None) == SHAPE
    # the workspace size: slices x n composites per row, 0 for what the op refuses
    size = lib.pie_top_logprobs_workspace_bytes
    assert size(1, 128256, 20) == 251 * 20 * 8 and size(32, 4099, 5) == 32 * 9 * 5 * 8 and size(1, 1, 1) == 8 and size(3, 524288, 20) == 3 * 1024 * 20 * 8
    assert size(0, 512, 5) == 0 and size(1, 0, 5) == 0 and size(1, 524289, 5) == 0 and size(1, 512, 0) == 0 and size(1, 512, 21) == 0
    assert _ffi.PIE_TOP_LOGPROBS_MAX == 20


def test_batched_engine_checks_logprobs_arguments_before_anything_runs():
    from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine
    model = StubModel()
    eng = BatchedEngine(model, num_pages=16, max_batch=2)
    prompts = [[1, 2, 3], [4, 5]]
    for bad in ([3], [3, 0, 1], [3, 21], [-1, 2], 21, -1, [1.5, 2], [True, 2]):
        with pytest.raises(ValueError, match="top_logprobs"):
            eng.generate(prompts, 4, logprobs=True, top_logprobs=bad)
    with_sampler = BatchedEngine(model, num_pages=16, max_batch=2, sampler=lambda lp: lp.argmax(-1))
    with pytest.raises(ValueError, match="sampler"):
        with_sampler.generate(prompts, 4, logprobs=True, top_logprobs=2)
    assert not model.calls                                                  # no pass ran
    # logprobs=False: top_logprobs is ignored, and the call returns what it always returned
    plain = eng.generate(prompts, 4)
    assert eng.generate(prompts, 4, logprobs=False, top_logprobs=[99]) == plain and isinstance(plain, list) and isinstance(plain[0], list)
    assert eng.generate(prompts, 0, logprobs=True, top_logprobs=[1, 2]) == ([[], []], [[], []])
