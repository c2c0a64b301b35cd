"""-m gpu: the captured batch graph's key across the kinds of per-row tail state.  Every kind's own suite arms it alone;
here one sequence of step_batch calls walks through all of them -- nothing armed, the batch tail, then also the edits, then also the count
penalty, then also top-n, then the tail re-armed with another rows_cap, then everything cleared -- once eagerly and once with
graph=True.  Each phase must run eager, capture, replay, and give the eager twin's results exactly: a field of RowsTail that key() forgot
would replay the previous phase's launches instead."""
import numpy as np
import pytest
import torch

from tests.test_gpu_batch_edits import make_model
from tests.test_gpu_batch_tail import dev_ids, f32_bits, prefilled

pytestmark = pytest.mark.gpu
PHASES = ("nothing armed", "batch tail", "+ edits", "+ count penalty", "+ top-n", "tail at another rows_cap", "all cleared")
STEPS = 3


def walk(model, prompts, graph):
    """One twin through PHASES on fresh caches -> per phase ([(tokens, logprob bits, top-n ids, top-n value bits) per step], replays)."""
    from proxy_inference_engine_amd.engine.batch_engine import SamplingParams
    V, rows = model.args.vocab_size, [0, 1, 2]
    params = [SamplingParams(temp=0.8, top_k=5, repetition_penalty=1.3, repetition_context_size=8), SamplingParams(temp=1.1), SamplingParams(repetition_penalty=0.7)]
    mask = torch.arange(V) % 3 != 1
    caches, first = prefilled(model, prompts)
    fed, feed, top, out = [list(p) for p in prompts], dev_ids(first), None, []

    def tail(rows_cap):
        model.set_batch_tail(rows_cap)
        model.write_batch_tail(rows, [sp.record(len(f) - len(p), 40 + i) for i, (sp, f, p) in enumerate(zip(params, fed, prompts))], fed)

    try:
        for phase in range(len(PHASES)):
            if phase in (1, 5):
                tail(3 if phase == 1 else 5)
            elif phase == 2:
                model.set_batch_edits(3, masks=True, bias_cap=4)
                model.write_batch_edits(rows, masks=[mask, None, mask.roll(1)], biases=[None, ([5, 9], [3.0, -2.0]), ([int(first[2])], [-4.0])])
            elif phase == 3:
                model.set_batch_count_penalty(3)
                model.write_batch_count_penalty(rows, [(0.5, 0.0, len(fed[0])), None, (0.0, 1.5, len(fed[2]))], [[], None, []])
            elif phase == 4:
                top = model.set_batch_top_logprobs(3, 4)
                top["count"].copy_(dev_ids([4, 0, 2]))
            elif phase == 6:
                model.clear_batch_tail(), model.clear_batch_edits(), model.clear_batch_count_penalty(), model.clear_batch_top_logprobs()
                top = None
            replays, steps = model.batch_graph_replays(), []
            for _ in range(STEPS):
                for f, t in zip(fed, feed.tolist()):
                    f.append(t)
                nxt, lp, _ = model.step_batch(feed, caches, graph=graph)
                steps.append((nxt.tolist(), f32_bits(lp), None if top is None else top["ids"].cpu().numpy().copy(), None if top is None else f32_bits(top["vals"])))
                feed = nxt.clone()
            out.append((steps, model.batch_graph_replays() - replays))
    finally:
        model.clear_batch_tail(), model.clear_batch_edits(), model.clear_batch_count_penalty(), model.clear_batch_top_logprobs()
    return out


def test_every_kind_of_row_state_is_in_the_graph_key(golden_dir):
    g, cfg, model = make_model(golden_dir)          # a model of its own: its decoder has captured nothing yet
    model.enable_paged_kv(num_pages=16)
    prompts = [g["prompt"][:3].tolist(), g["prompt"][3:7].tolist(), g["prompt"][7:12].tolist()]
    eager, graph = walk(model, prompts, False), walk(model, prompts, True)
    for name, (want, r_eager), (got, r_graph) in zip(PHASES, eager, graph):
        assert r_eager == 0 and r_graph == STEPS - 2, name                      # eager, capture, then replays only
        for st, (w, h) in enumerate(zip(want, got)):
            assert h[0] == w[0], (name, st, "tokens")
            assert np.array_equal(h[1], w[1]), (name, st, "logprobs")
            assert (w[2] is None) == (h[2] is None) == (name in PHASES[:4] or name == PHASES[6]), (name, st)
            if w[2] is not None:
                assert np.array_equal(h[2], w[2]) and np.array_equal(h[3], w[3]), (name, st, "top-n records")
