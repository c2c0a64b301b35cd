"""The int8-page switch of batched speculation on the CPU: SpeculativeParams(int8_pages=...) defaults to False and every
int8 refusal then keeps its words; with True BatchedEngine(kv_dtype=torch.int8, speculative=...) follows the simulated schedule on the
stub model; InferenceEngine refuses the flag by name; the new entry points are declared and exported."""
import ctypes

import pytest
import torch

from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine
from proxy_inference_engine_amd.engine.inference_engine import SpeculativeParams, _check_generate_args
from tests import spec_batch_reference as sb
from tests.test_spec_batch_host import SP, SpecStub, alone, cyclic, repeating

SP8 = SpeculativeParams(num_draft=7, ngram_max=3, ngram_min=1, min_draft=5, int8_pages=True)


class Int8Stub(SpecStub):
    """SpecStub whose passes take the keyword -- and must get it exactly when the pool holds int8 pages."""

    def spec_step_batch(self, *args, int8_pages=False, **kw):
        assert int8_pages == (self.pool.dtype == torch.int8)
        return super().spec_step_batch(*args, **kw)


def test_the_flag_defaults_to_false_and_the_refusals_keep_their_words():
    assert SP.int8_pages is False and SpeculativeParams().int8_pages is False
    with pytest.raises(TypeError):
        SpeculativeParams(7, 3, 1, 5, False, None, False, True)         # keyword-only, like batch_tail
    with pytest.raises(ValueError, match="int8_pages is a bool"):
        SpeculativeParams(int8_pages=1)
    with pytest.raises(ValueError, match=r"BatchedEngine\(speculative=...\): not available with kv_dtype=torch.int8 \(int8 KV pages\)"):
        BatchedEngine(SpecStub(), speculative=SP, kv_dtype=torch.int8)
    with pytest.raises(ValueError, match="configured_tail"):            # the other refusals stand beside the flag
        BatchedEngine(SpecStub(), speculative=SpeculativeParams(int8_pages=True, configured_tail=True), kv_dtype=torch.int8)
    with pytest.raises(ValueError, match="not available with int8_pages"):
        _check_generate_args(SpecStub(), None, None, None, None, None, None, None, SP8)


@pytest.mark.parametrize("kv_dtype", [torch.int8, None], ids=["int8_pool", "T_pool"])
def test_with_the_flag_the_engine_follows_the_simulated_schedule(kv_dtype):
    prompts, new = repeating(11, 6), 30
    want, schedule = sb.simulate_batch(prompts, cyclic, new, 2, (), SP8.num_draft, SP8.ngram_max, SP8.ngram_min, SP8.min_draft)
    model = Int8Stub()
    eng = BatchedEngine(model, num_pages=64, max_batch=2, speculative=SP8, kv_dtype=kv_dtype)   # on a T pool the flag does nothing
    assert eng.generate(prompts, new) == want == [alone(cyclic, p, new) for p in prompts]
    assert model.passes == [(e[2], e[3]) for e in schedule if e[0] == "pass"] and eng.spec_stats == sb.stats_of(schedule)
    assert eng.pool.get_num_free_pages() == eng.pool.size()


def test_the_new_entry_points_are_declared_and_exported():
    from proxy_inference_engine_amd import _ffi, build
    from tests.test_abi import declared_symbols
    lib, syms = ctypes.CDLL(str(build.build())), declared_symbols()
    for name in ("pie_paged_attn_verify_i8", "pie_paged_attn_verify_i8_splits", "pie_paged_attn_verify_i8_workspace_bytes"):
        assert name in syms and name in _ffi.EXPORTS and hasattr(lib, name)
    bound = _ffi.load()
    assert bound.pie_paged_attn_verify_i8_splits(2, 8, 128) == 16 and bound.pie_paged_attn_verify_i8_splits(32, 8, 8) == 1
    assert bound.pie_paged_attn_verify_i8_splits(1, 2, 8) == 8 and bound.pie_paged_attn_verify_i8_workspace_bytes(3, 4, 64, 33) == 0
