"""-m gpu: the captured step graph across the parts of the single-sequence step's tail.  Every part's own suite sets it
alone; here one sequence walks through all of them -- nothing set, the repetition penalty, then also a logit bias, a token mask, frequency /
presence penalties, DRY, a top-k sampler, XTC and top-n, then new CONTENTS part by part, then one launch argument changed per part in turn,
then everything cleared -- once eagerly and once with graph=True, three steps per phase.  Each phase must give the eager twin's results
exactly; a set_step_tail that changes a launch argument must drop the graphs and one that only rewrites contents must not: a field of
StepTail that its part's comparison forgot would replay the previous phase's launch arguments instead."""
import numpy as np
import pytest

from tests.test_gpu_step_edits import half_mask, pack, vocab
from tests.test_gpu_step_tail import PROMPT, dev_ids, f32_bits, tiny  # noqa: F401  (tiny: the fixture)

pytestmark = pytest.mark.gpu
STEPS, SEED = 3, 12
SPEC = ("top_k", 0.8, 0.0, 5)
ARGS, CONTENTS = "a launch argument changes", "contents only"


def phases(V):
    """(name, ARGS | CONTENTS, what set_step_tail is given from here on, what it is given this once)"""
    return [
        ("nothing set", ARGS, {}, {}),
        ("repetition penalty", ARGS, dict(repetition_penalty=1.3, context_size=8), {}),
        ("+ logit bias", ARGS, dict(logit_bias=((301, 17), (-4.0, 1.5))), {}),
        ("+ token mask", ARGS, dict(token_mask=pack(half_mask(V, 1))), {}),
        ("+ frequency / presence", ARGS, dict(frequency_penalty=0.5, presence_penalty=0.25), dict(count_start=len(PROMPT))),
        ("+ DRY", ARGS, dict(dry=(0.8, 1.75, 2, 1024, ())), {}),
        ("+ top-k sampler", ARGS, dict(sampler=SPEC), {}),
        ("+ XTC", ARGS, dict(xtc=(0.5, 0.05, ())), {}),
        ("+ top-n", ARGS, dict(top_logprobs=4), {}),
        ("new mask words", CONTENTS, dict(token_mask=pack(half_mask(V, 2))), {}),
        ("new bias values of the same length", CONTENTS, dict(logit_bias=((450, 17), (2.0, -3.0))), {}),
        ("new DRY values", CONTENTS, dict(dry=(1.2, 1.5, 1, 512, (17,))), {}),
        ("new XTC values", CONTENTS, dict(xtc=(0.25, 0.2, (3,))), {}),
        ("another context size", ARGS, dict(context_size=5), {}),
        ("another number of bias entries", ARGS, dict(logit_bias=((450, 17, 301), (2.0, -3.0, 1.0))), {}),
        ("another top_logprobs n", ARGS, dict(top_logprobs=2), {}),
        ("another seed", ARGS, {}, {}),
        ("everything cleared", ARGS, None, {}),
    ]


def walk(model, V, graph):
    """One twin through the phases on a fresh cache -> per phase ([(token, logprob bits, top-n ids, top-n value bits) per step], graph_launches())."""
    from proxy_inference_engine_amd import samplers
    samplers.seed(SEED)
    model.set_step_tail()
    cache, kw, out = model.make_cache(), {}, []
    try:
        for i, (name, kind, update, once) in enumerate(phases(V)):
            kw = {} if update is None else {**kw, **update}
            if name == "another seed":
                samplers.seed(SEED + 1)
            before = model.graph_launches()
            model.set_step_tail(**kw, **once)
            if graph and kind == ARGS:
                assert model.graph_launches() == -1, name                          # dropped (phase 0: nothing was captured yet)
            if graph and kind == CONTENTS:
                assert before > 0 and model.graph_launches() == before, name       # the captured graph stays
            steps = []
            for s in range(STEPS):
                tok, lp, _ = model.step(dev_ids(PROMPT) if i == 0 and s == 0 else None, cache, graph=graph)
                top = [t.cpu().numpy().copy() for t in model.step_top_logprobs] if kw.get("top_logprobs") is not None else None
                steps.append((int(tok.item()), f32_bits(lp), None if top is None else top[0], None if top is None else top[1].view(np.uint32)))
            out.append((steps, model.graph_launches()))
    finally:
        model.set_step_tail()
    return out


def test_every_part_of_the_step_tail_keys_the_graph(tiny):
    g, cfg, model = tiny
    V = vocab(cfg)
    names = [p[0] for p in phases(V)]
    eager, graph = walk(model, V, False), walk(model, V, True)
    for name, (want, l_eager), (got, l_graph) in zip(names, eager, graph):
        assert l_eager == -1 and l_graph > 0, name                                 # the eager twin captured nothing, the other one every phase
        for st, (w, h) in enumerate(zip(want, got)):
            assert h[0] == w[0], (name, st, "tokens")
            assert np.array_equal(h[1], w[1]), (name, st, "logprobs")
            assert (w[2] is None) == (h[2] is None) == (names.index(name) < 8 or name == names[-1]), (name, st)
            if w[2] is not None:
                assert np.array_equal(h[2], w[2]) and np.array_equal(h[3], w[3]), (name, st, "top-n records")
    assert graph[-1][1] == graph[0][1]                                             # cleared: the unconfigured step's launches again
    assert graph[8][1] > graph[0][1]
