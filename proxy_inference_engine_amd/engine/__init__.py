from .batch_engine import BatchedEngine, SamplingParams
from .inference_engine import InferenceEngine, SpeculativeParams

__all__ = ["InferenceEngine", "BatchedEngine", "SamplingParams", "SpeculativeParams"]
