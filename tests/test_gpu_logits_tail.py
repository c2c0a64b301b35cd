"""-m gpu: the logits tail (csrc/tail.hpp: k_logits_stats + k_logits_finish, hip_ops.logprobs_argmax) against a float64 log_softmax of
the same 16-bit logits and the FIRST maximal index (mx.argmax), at the vocabulary sizes, ties and masks where a tiled reduction goes
wrong: V % 8 != 0 (the finish's scalar path), V < 256 (empty tiles), V = 1, ties across the 256 tiles and across the finish's 8-wide
vectors, -inf tiles, one finite id, an all -inf row, f16 at +-65504.  Then the engine's processor path, which feeds the tail masked rows.

Bound on a log-prob.  The kernel computes lse = M + logf(S) in fp32: S sums exp(x - m_tile) along a path of at most
n = ceil(tile_len / 256) sequential adds per thread + 6 (wave tree) + 2 (waves) per tile, then 16 + 6 + 2 adds merging the 256 tiles,
each term off by <= 2 ulp (expf) -- |S / S_true - 1| <= (n + 40) * 2^-24 + 2^-22 =: d, which moves log S by <= d (absolute).
log S, the sum M + log S and x - lse each round once more: |lp - lp_true| <= d + ulp(lse) + ulp(lp) (fp32 ulps of the values)."""
import json

import numpy as np
import pytest
import torch

from oracle import pie_oracle as po
from tests import sampler_rows as R
from tests._util import to_dev

pytestmark = pytest.mark.gpu
TILES = 256


def _ref(x):
    """float64 log_softmax and first argmax of the 16-bit values (as fp32 array x)."""
    xd = x.astype(np.float64)
    m = xd.max()
    lse = m + np.log(np.exp(xd - m).sum())
    return xd - lse, int(np.argmax(xd)), lse


def _bound(V, lse, lp_ref):
    tile_len = -(-V // TILES)
    d = (-(-tile_len // 256) + 40) * 2.0 ** -24 + 2.0 ** -22
    return d + np.spacing(np.float32(abs(lse))).astype(np.float64) + np.spacing(np.abs(lp_ref).astype(np.float32)).astype(np.float64)


def _run(x, dt):
    from proxy_inference_engine_amd import hip_ops
    bits = po.to_bits(x, dt)
    xq = po.from_bits(bits, dt).astype(np.float32)
    tok, lp = hip_ops.logprobs_argmax(to_dev(bits, dt))
    return xq, int(tok.item()), lp.cpu().numpy()


def _check(x, dt, what):
    xq, tok, lp = _run(x, dt)
    ref, arg, lse = _ref(xq)
    assert tok == arg, (what, tok, arg)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(lp), fin), what
    err = np.abs(lp[fin].astype(np.float64) - ref[fin])
    bound = _bound(len(x), lse, ref[fin])
    assert (err <= bound).all(), (what, float(err.max()), float(bound[np.argmax(err - bound)]))
    return xq, tok, lp


VS = sorted(set(R.VOCABS + [1, 3, 255, 257, 4099]))


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("V", VS)
def test_logprobs_and_first_argmax(V, dt):
    rng = np.random.default_rng(V)
    x = (rng.standard_normal(V) * 3.0).astype(np.float32)
    _check(x, dt, ("random", V))
    if V < 3:
        return
    # ties across a tile boundary: the last id of tile t and the first of tile t + 1 (and a later copy) -> the earlier one
    tl = -(-V // TILES)
    t = min(TILES - 2, (V - 1) // tl - 1) if V > tl else 0
    b = (t + 1) * tl
    if 0 < b < V:
        y = x.copy()
        y[[b - 1, b, V - 1]] = 20.0
        _check(y, dt, ("tile tie", V, b))
    # ties on both sides of an 8-wide vector boundary of the finish (m + 7 | m + 8) and an earlier copy: the earliest wins, all equal
    if V >= 24:
        y = x.copy()
        m = (V // 2) & ~7
        y[[m + 8, m + 7, m - 1]] = 20.0
        _, tok, lp = _check(y, dt, ("vector tie", V))
        assert tok == m - 1 and lp[m - 1] == lp[m + 7] == lp[m + 8]
    # bf16 log-probs repeat: a row of few distinct values, max repeated everywhere
    y = np.round(x).astype(np.float32)
    _check(y, dt, ("rounded", V))


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("V", [1, 2, 255, 513, 50257, 128256, R.V_MAX])
def test_masked_rows(V, dt):
    """-inf tiles, exactly one finite id (its log-prob exactly 0), and an all -inf row: the token is 0 there, as mx.argmax's."""
    rng = np.random.default_rng(V + 1)
    tl = -(-V // TILES)
    if V > 4 * tl:
        x = (rng.standard_normal(V) * 3.0).astype(np.float32)
        x[3 * tl:4 * tl] = -np.inf                                     # tile 3 entirely -inf
        x[:tl] = -np.inf                                               # and tile 0, where the first index lives
        _check(x, dt, ("-inf tiles", V))
    for i in sorted({0, V // 2, V - 1}):
        x = np.full(V, -np.inf, np.float32)
        x[i] = 1.5
        _, tok, lp = _check(x, dt, ("one finite", V, i))
        assert tok == i and lp[i] == 0.0 and np.isneginf(np.delete(lp, i)).all()
    _, tok, _ = _run(np.full(V, -np.inf, np.float32), dt)
    assert tok == 0, (V, tok)


@pytest.mark.parametrize("V", [7, 4099, 128256])
def test_f16_extremes(V):
    rng = np.random.default_rng(V + 2)
    x = (rng.standard_normal(V) * 1000.0).astype(np.float32)
    x[rng.choice(V, 3, replace=False)] = 65504.0
    x[rng.choice(V, 3, replace=False)] = -65504.0
    x[V // 3] = 65504.0
    _check(x, "float16", ("f16 extremes", V))


# ------------------------------------------------------------------ engine: a structuring engine's mask in front of the tail / sampler
class _MaskingEngine:
    """The part of a structuring engine _inference talks to: process_logits leaves only `allowed` finite."""
    has_reached_accept_state = False

    def __init__(self, allowed):
        self.allowed = torch.as_tensor(allowed, dtype=torch.long)

    def get_current_state(self):
        return None

    def process_logits(self, tokens, logits):
        idx = self.allowed.to(logits.device)
        out = torch.full_like(logits, float("-inf"))
        out[..., idx] = logits[..., idx]
        return out

    def sample(self, logprobs, sampler):
        return sampler(logprobs)


@pytest.fixture(scope="module")
def tiny(golden_dir):
    from tests.test_gpu_decode import build
    g = np.load(golden_dir / "tiny_llama_w4_bf16.npz")
    cfg = json.loads(str(g["config_json"]))
    return g, cfg, build(cfg, {k[2:]: g[k] for k in g.files if k.startswith("w:")})


@pytest.mark.parametrize("kw", [dict(temp=0), dict(temp=1.0), dict(temp=0.8, top_k=5), dict(temp=1.0, top_p=0.9), dict(temp=1.0, min_p=0.1),
                                dict(temp=1.0, top_k=3, repetition_penalty=1.3), dict(temp=0, repetition_penalty=1.3)])
def test_masking_processor_keeps_every_token_in_the_allowed_set(tiny, kw):
    from proxy_inference_engine_amd import InferenceEngine, samplers
    g, cfg, model = tiny
    V = cfg["vocab_size"]
    allowed = sorted({3, V // 3, V // 2 + 1, V - 2, 17})
    samplers.seed(12)
    for allow in (allowed, [V // 2 + 1]):
        eng = InferenceEngine(model=model, structuring_engine=_MaskingEngine(allow))
        eng.prepare_engine(g["prompt"], **kw)
        gen = eng.generate_step(torch.from_numpy(g["prompt"]))
        toks = []
        for _ in range(6):
            tok, lp = next(gen)
            toks.append(int(tok.reshape(-1)[0].item()))
            assert np.isfinite(lp.cpu().numpy()).sum() == len(allow)
        assert set(toks) <= set(allow), (kw, toks)
        if len(allow) == 1:
            assert toks == allow * 6
