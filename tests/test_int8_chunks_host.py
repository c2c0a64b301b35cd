"""BatchedEngine(int8_chunks=True) on a stub model: the switches, and who is told int8_pages."""
import numpy as np
import torch

from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine
from tests.test_batch_engine_host import V, StubModel, alone, requests

SYSTEM = np.random.default_rng(3).integers(0, V, 150).tolist()   # two whole pages and a bit


class Int8ChunkStub(StubModel):   # step_mixed accepts and records int8_pages; a continuing prompt on the int8 pool passes only with it
    def step_mixed(self, tokens, decode_caches, prompts, prompt_caches, **kw):
        self.calls["int8_pages"] += bool(kw.get("int8_pages"))
        assert set(kw) <= {"int8_pages"}
        if not kw:
            return super().step_mixed(tokens, decode_caches, prompts, prompt_caches)
        dtype, self.pool.dtype = self.pool.dtype, torch.bfloat16        # (the stub's "needs T pages" assertion is dropped for this call only)
        try:
            return super().step_mixed(tokens, decode_caches, prompts, prompt_caches)
        finally:
            self.pool.dtype = dtype


def test_int8_chunks_keeps_chunked_prefill_and_shared_prefixes_on_an_int8_pool():
    prompts, n = requests(5, 6), 8
    model = Int8ChunkStub()
    eng = BatchedEngine(model, num_pages=64, max_batch=4, kv_dtype=torch.int8, prefill_chunk=16, int8_chunks=True)
    assert eng.prefill_chunk == 16 and eng.generate(prompts, n) == [alone(p, n, set()) for p in prompts]
    assert model.calls["continuing"] > 0 and model.calls["int8_pages"] == model.calls["step_mixed"] and model.max_rows <= max(16, 4)
    assert eng.pool.get_num_free_pages() == eng.pool.size()
    shared = requests(6, 4, lo=1, hi=40, prefix=SYSTEM)
    model = Int8ChunkStub()
    eng = BatchedEngine(model, num_pages=64, max_batch=4, kv_dtype=torch.int8, share_prefix=True, int8_chunks=True)
    assert eng.generate(shared, n) == [alone(p, n, set()) for p in shared] and eng.shared_pages == 2 and model.calls["continuing"] > 0
    assert eng.pool.get_num_free_pages() == eng.pool.size()


def test_without_int8_chunks_an_int8_pool_switches_both_off_and_never_passes_the_flag():
    shared, n = requests(6, 4, lo=1, hi=40, prefix=SYSTEM), 8
    model = Int8ChunkStub()
    eng = BatchedEngine(model, num_pages=64, max_batch=4, kv_dtype=torch.int8, prefill_chunk=16, share_prefix=True)
    assert eng.prefill_chunk is None and eng.generate(shared, n) == [alone(p, n, set()) for p in shared]
    assert eng.shared_pages == 0 and model.calls["int8_pages"] == 0 and model.calls["continuing"] == 0
    model = Int8ChunkStub()                                             # a 16-bit pool: the flag does nothing
    eng = BatchedEngine(model, num_pages=64, max_batch=4, prefill_chunk=16, int8_chunks=True)
    assert eng.generate(shared, n) == [alone(p, n, set()) for p in shared] and model.calls["int8_pages"] == 0 and model.calls["continuing"] > 0
