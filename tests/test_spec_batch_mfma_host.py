"""The MFMA-verify switch of batched speculation on the CPU: SpeculativeParams(mfma_verify=...) defaults to False and is a
keyword-only bool; InferenceEngine refuses it by name; BatchedEngine hands mfma_verify=True to its passes exactly when it is set."""
import pytest

from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine
from proxy_inference_engine_amd.engine.inference_engine import SpeculativeParams, _check_generate_args
from tests.test_spec_batch_host import SP, SpecStub, alone, cyclic, repeating


class MfmaStub(SpecStub):
    """SpecStub whose passes record the keyword they were given (absent: None)."""

    def __init__(self):
        super().__init__()
        self.flags = set()

    def spec_step_batch(self, *args, **kw):
        self.flags.add(kw.pop("mfma_verify", None))
        return super().spec_step_batch(*args, **kw)


def test_the_flag_defaults_to_false_is_a_keyword_only_bool_and_inference_engine_refuses_it():
    assert SP.mfma_verify is False and SpeculativeParams().mfma_verify is False
    with pytest.raises(TypeError):
        SpeculativeParams(7, 3, 1, 5, False, None, False, True)
    with pytest.raises(ValueError, match="mfma_verify is a bool"):
        SpeculativeParams(mfma_verify=1)
    with pytest.raises(ValueError, match="not available with mfma_verify"):
        _check_generate_args(SpecStub(), None, None, None, None, None, None, None, SpeculativeParams(mfma_verify=True))


@pytest.mark.parametrize("flag", [True, False])
def test_the_engine_passes_the_keyword_only_when_set(flag):
    prompts, new = repeating(11, 6), 30
    model = MfmaStub()
    eng = BatchedEngine(model, num_pages=64, max_batch=2, speculative=SpeculativeParams(num_draft=7, ngram_max=3, ngram_min=1, min_draft=5, mfma_verify=flag))
    assert eng.generate(prompts, new) == [alone(cyclic, p, new) for p in prompts]
    assert model.passes and model.flags == ({True} if flag else {None})
