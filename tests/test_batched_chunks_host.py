"""BatchedEngine(batched_chunks=True) on a stub model: who is told batched_chunks, and the C ABI's new names."""
import re
from pathlib import Path

import pytest
import torch

from proxy_inference_engine_amd import _ffi
from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine
from tests.test_batch_engine_host import StubModel, alone, requests
from tests.test_int8_chunks_host import SYSTEM


class ChunkStub(StubModel):   # step_mixed records its keywords; the int8 pool's continuing prompts pass as in Int8ChunkStub
    def step_mixed(self, tokens, decode_caches, prompts, prompt_caches, **kw):
        assert all(v is True for v in kw.values())
        self.calls.update(kw)
        dtype, self.pool.dtype = self.pool.dtype, torch.bfloat16
        try:
            return super().step_mixed(tokens, decode_caches, prompts, prompt_caches)
        finally:
            self.pool.dtype = dtype


@pytest.mark.parametrize("kw,told", [(dict(batched_chunks=True), "batched_chunks"), (dict(), None), (dict(int8_chunks=True), None),
                                     (dict(kv_dtype=torch.int8, int8_chunks=True, batched_chunks=True), "int8_pages"),
                                     (dict(kv_dtype=torch.int8, batched_chunks=True), None)])
def test_step_mixed_is_told_batched_chunks_exactly_on_a_16_bit_pool_with_the_flag(kw, told):
    shared, n = requests(6, 4, lo=1, hi=40, prefix=SYSTEM), 8
    model = ChunkStub()
    eng = BatchedEngine(model, num_pages=64, max_batch=4, prefill_chunk=16, share_prefix=True, **kw)
    assert eng.generate(shared, n) == [alone(p, n, set()) for p in shared] and (model.calls["step_mixed"] > 0 or told is None)
    passes = model.calls["step_mixed"] - (eng.shared_pages > 0)        # (the shared prefix's own pass is a fresh prompt: no keyword)
    for flag in ("batched_chunks", "int8_pages"):                      # the one keyword on every pass of the loop, the other on none
        assert model.calls[flag] == (passes if flag == told else 0), (kw, flag)
    assert (model.calls["continuing"] > 0) == (kw.get("kv_dtype") is None or told == "int8_pages")


def test_the_new_names_are_exported_and_declared():
    header = (Path(__file__).resolve().parents[1] / "include" / "pie_hip.h").read_text()
    for name in ("pie_prefill_attn_paged_splits", "pie_prefill_attn_paged_workspace_bytes", "pie_prefill_attn_paged"):
        assert name in _ffi.EXPORTS and re.search(rf"\b{name}\(", header), name
    assert _ffi.PIE_OPT_CHUNK_BATCHED == 4 and "PIE_OPT_CHUNK_BATCHED = 4" in header
    assert _ffi.KNOBS["chunk_splits"] == 13 and "PIE_KNOB_CHUNK_SPLITS = 13" in header and "PIE_KNOB_COUNT = 14" in header
