"""What BatchedEngine asks of the model, pass by pass (engine/batch_engine.py), on the CPU: the stub model of tests/test_batch_engine_host.py
logging every call in order -- which entry ran, which request sat in which row, which rows of which prompt it carried -- interleaved with
every _RowSeats.seat, every _PromptScores.arm / collect and every call of the host sampler.  tests/test_batch_engine_host.py pins the tokens;
a pass that forgot to seat its rows, or armed the wrong span, would still produce them on a stub.  The small scenarios are written out
whole; the grids are compared with digests recorded in tests/golden/batch_engine_passes.json (regenerate: run this module as a script).

Log entries:
    ("seat", rows)                        _RowSeats.seat's `rows`: a request index, or None for a prompt that is still filling
    ("arm", n_decode, parts)              _PromptScores.arm: parts = [(request, first row's index in its prompt, rows)]
    ("collect",)                          _PromptScores.collect
    (entry, decode, parts)                a model call: the decode rows' requests in row order, and every prompt part as (request, its cache's
                                          offset before the call = the first row's index in its prompt, rows); "root": the shared prefix's own sequence
    ("sampler", rows, ids)                the host sampler: how many rows it was given and their argmax ids"""
import hashlib
import json
from collections import Counter
from pathlib import Path
from unittest import mock

import pytest
import torch

from proxy_inference_engine_amd.engine import batch_engine
from proxy_inference_engine_amd.engine.batch_engine import BatchedEngine, SamplingParams
from tests.test_batch_engine_host import V, alone, next_token, requests
from tests.test_prompt_logprobs_host import ScoringStub

GOLDEN = Path(__file__).parent / "golden" / "batch_engine_passes.json"


class LogStub(ScoringStub):
    """The stub model + the per-row setters as no-ops + the log.  A sequence is told apart by the order in which the model first sees it:
    the engine admits requests in order, so the k-th new sequence is request k -- checked against the prompt on every call.  The sequence
    others were forked from is the shared prefix's root."""

    def __init__(self, prompts, log):
        super().__init__()
        self.prompts, self.log = [list(p) for p in prompts], log
        self.args = type("Args", (), {"vocab_size": V})
        self.who, self.seqs = {}, []       # id(sequence) -> request; the sequences themselves, kept alive so that no id comes back

    def __getattr__(self, name):
        if not name.startswith(("set_batch_", "write_batch_", "clear_batch_")):
            raise AttributeError(name)

        def call(*a, **kw):
            if name == "set_batch_top_logprobs":
                return {"ids": torch.zeros((a[0], a[1] + 1), dtype=torch.int32), "vals": torch.zeros((a[0], a[1] + 1)), "count": torch.zeros(a[0], dtype=torch.int32)}
        return call

    def _who(self, cache, ids):
        seq = cache[0].page_manager
        if id(seq) not in self.who:
            if seq.offset > 0 and not hasattr(seq, "_hist") and "root" not in self.who.values():
                # the first fork: the one sequence seen so far was no request's but the prefix's
                assert len(self.who) == 1
                self.who[next(iter(self.who))] = "root"
            self.who[id(seq)] = sum(r != "root" for r in self.who.values())
            self.seqs.append(seq)
        r = self.who[id(seq)]
        if r != "root":
            fed = (list(self._hist(seq)) if seq.offset else []) + [int(t) for t in ids]
            assert fed[:len(self.prompts[r])] == self.prompts[r][:len(fed)], "request %d is fed another request's rows" % r
        return seq

    def _entry(self, name, tokens, decode_caches, prompts, prompt_caches):
        decode = [self._who(c, [t]) for c, t in zip(decode_caches, tokens.tolist() if decode_caches else [])]
        parts = [(self._who(c, p), c[0].offset, len(p)) for c, p in zip(prompt_caches, prompts)]
        self.log.append([name, decode, parts])

    def step(self, ids, cache):
        self._entry("step", None, [], [ids.reshape(-1).tolist()], [cache])
        return super().step(ids, cache)

    def step_batch(self, tokens, caches):
        self._entry("step_batch", tokens, caches, [], [])
        return super().step_batch(tokens, caches)

    def prefill_batch(self, prompts, caches):
        self._entry("prefill_batch", None, [], prompts, caches)
        return super().prefill_batch(prompts, caches)

    def step_mixed(self, tokens, decode_caches, prompts, prompt_caches):
        self._entry("step_mixed", tokens, decode_caches, prompts, prompt_caches)
        return super().step_mixed(tokens, decode_caches, prompts, prompt_caches)

    def named(self):
        """The log with every sequence replaced by its request (the root is known only once it has been forked)."""
        who = self.who
        return [(e[0], [who[id(s)] for s in e[1]], [(who[id(s)], at, n) for s, at, n in e[2]]) if isinstance(e, list) else e for e in self.log]


def run(prompts, new, stop=(), sampler=None, gen=None, **kw):
    """One generate() under the log: (log, engine, what generate returned)."""
    log = []

    class Seats(batch_engine._RowSeats):
        def seat(self, rows, active):
            log.append(("seat", list(rows)))
            return super().seat(rows, active)

    class Scores(batch_engine._PromptScores):
        def arm(self, n_decode, parts):
            log.append(("arm", n_decode, [tuple(p) for p in parts]))
            return super().arm(n_decode, parts)

        def collect(self):
            log.append(("collect",))
            return super().collect()

    def logged(logprobs):
        assert logprobs.dim() == 2 and logprobs.shape[1] == V
        log.append(("sampler", logprobs.shape[0], logprobs.argmax(dim=-1).tolist()))
        return sampler(logprobs)

    model = LogStub(prompts, log)
    eng = BatchedEngine(model, stop_tokens=stop, sampler=logged if sampler else None, **kw)
    with mock.patch.object(batch_engine, "_RowSeats", Seats), mock.patch.object(batch_engine, "_PromptScores", Scores):
        res = eng.generate(prompts, new, **(gen or {}))
    assert eng.pool.get_num_free_pages() == eng.pool.size()                          # every page came back
    return model.named(), eng, res


def toks(p, k):
    """The k-th token request `p` generates alone (0: its first)."""
    return alone(p, k + 1, ())[k]


def plus_one(logprobs):
    return (logprobs.argmax(dim=-1) + 1) % V


def alone_plus_one(p, n):
    hist, out = list(p), []
    for _ in range(n):
        out.append((next_token(hist) + 1) % V)
        hist.append(out[-1])
    return out


# ------------------------------------------------------------------ (a) whole logs, derived by hand from the scheduling rules
A, B, C = [5, 6], [10, 11, 12, 13, 14, 15, 16, 17], [20, 21, 22]


def test_chunked_a_prompt_spans_three_passes_while_another_decodes():
    """Budget 4 rows a pass, decode rows included.  Pass 1: all of A (2 rows, its last: seated) + B's rows 0-1 (still filling: None).
    Passes 2, 3: A's decode row + 3 rows of B; the third finishes B, whose row is seated from then on.  Then decode steps: one for both,
    which gives A its fourth token, and two more for B, whose first token came out of pass 3."""
    log, eng, out = run([A, B], 4, num_pages=8, max_batch=2, prefill_chunk=4)
    assert out == [alone(A, 4, ()), alone(B, 4, ())]
    assert log == [("seat", [0, None]), ("step_mixed", [], [(0, 0, 2), (1, 0, 2)]),
                   ("seat", [0, None]), ("step_mixed", [0], [(1, 2, 3)]),
                   ("seat", [0, 1]), ("step_mixed", [0], [(1, 5, 3)]),
                   ("seat", [0, 1]), ("step_batch", [0, 1], []),                     # A's fourth token
                   ("seat", [1]), ("step_batch", [1], []),
                   ("seat", [1]), ("step_batch", [1], [])]
    assert (eng.steps, eng.mixed_passes, eng.shared_pages) == (6, 2, 0)


def test_chunked_host_sampler_is_not_shown_a_filling_prompts_row():
    """The passes of the test above under a host sampler: it sees the rows that produce a request's token -- never the row of B's unfinished chunks."""
    log, eng, out = run([A, B], 3, sampler=plus_one, num_pages=8, max_batch=2, prefill_chunk=4)
    a, b = alone_plus_one(A, 3), alone_plus_one(B, 3)
    assert out == [a, b]
    assert log == [("seat", [0, None]), ("step_mixed", [], [(0, 0, 2), (1, 0, 2)]), ("sampler", 1, [next_token(A)]),
                   ("seat", [0, None]), ("step_mixed", [0], [(1, 2, 3)]), ("sampler", 1, [next_token(A + a[:1])]),
                   ("seat", [0, 1]), ("step_mixed", [0], [(1, 5, 3)]), ("sampler", 2, [next_token(A + a[:2]), next_token(B)]),
                   ("seat", [1]), ("step_batch", [1], []), ("sampler", 1, [next_token(B + b[:1])]),
                   ("seat", [1]), ("step_batch", [1], []), ("sampler", 1, [next_token(B + b[:2])])]
    assert (eng.steps, eng.mixed_passes) == (5, 2)


def test_mixed_pass_and_the_lone_step_before_it():
    """max_prefill_rows=4 admits A (2 rows) and C (3 rows would make 5) apart: A alone through Model.step -- no seat --, then C rides A's
    decode step.  With prompt scoring: every pass that carries prompt rows is armed before and collected after."""
    log, eng, (out, maps) = run([A, C], 3, gen=dict(prompt_logprobs=1), num_pages=8, max_batch=2, max_prefill_rows=4)
    assert out == [alone(A, 3, ()), alone(C, 3, ())] and [len(m) for m in maps] == [2, 3]
    assert log == [("arm", 0, [(0, 0, 2)]), ("step", [], [(0, 0, 2)]), ("collect",),
                   ("seat", [0, 1]), ("arm", 1, [(1, 0, 3)]), ("step_mixed", [0], [(1, 0, 3)]), ("collect",),
                   ("seat", [0, 1]), ("step_batch", [0, 1], []),
                   ("seat", [1]), ("step_batch", [1], [])]
    assert (eng.steps, eng.mixed_passes) == (3, 1)


def test_joint_prompt_pass_then_the_decode_step_without_mixing():
    """mixed=False: B alone first (max_prefill_rows=8 holds its 8 rows only), then A and C in one prompt pass of their own, seated as rows 0
    and 1 of THAT pass, and B's decode step after it in the same iteration."""
    log, eng, out = run([B, A, C], 3, num_pages=8, max_batch=3, max_prefill_rows=8, mixed=False)
    assert out == [alone(p, 3, ()) for p in (B, A, C)]
    assert log == [("step", [], [(0, 0, 8)]),
                   ("seat", [1, 2]), ("prefill_batch", [], [(1, 0, 2), (2, 0, 3)]), ("seat", [0]), ("step_batch", [0], []),
                   ("seat", [0, 1, 2]), ("step_batch", [0, 1, 2], []),
                   ("seat", [1, 2]), ("step_batch", [1, 2], [])]
    assert (eng.steps, eng.mixed_passes) == (3, 0)


def test_host_sampler_sees_every_row_of_the_other_passes_once():
    """The same schedule under a host sampler: one call per pass over all its rows, the lone step's as a block of one."""
    log, eng, out = run([B, A, C], 2, sampler=plus_one, num_pages=8, max_batch=3, max_prefill_rows=8, mixed=False)
    b, a, c = (alone_plus_one(p, 2) for p in (B, A, C))
    assert out == [b, a, c]
    assert log == [("step", [], [(0, 0, 8)]), ("sampler", 1, [next_token(B)]),
                   ("seat", [1, 2]), ("prefill_batch", [], [(1, 0, 2), (2, 0, 3)]), ("sampler", 2, [next_token(A), next_token(C)]),
                   ("seat", [0]), ("step_batch", [0], []), ("sampler", 1, [next_token(B + b[:1])]),
                   ("seat", [1, 2]), ("step_batch", [1, 2], []), ("sampler", 2, [next_token(A + a[:1]), next_token(C + c[:1])])]
    log, eng, out = run([A, C], 2, sampler=plus_one, num_pages=8, max_batch=2, max_prefill_rows=4)
    a, c = alone_plus_one(A, 2), alone_plus_one(C, 2)
    assert out == [a, c]
    assert log == [("step", [], [(0, 0, 2)]), ("sampler", 1, [next_token(A)]),
                   ("seat", [0, 1]), ("step_mixed", [0], [(1, 0, 3)]), ("sampler", 2, [next_token(A + a[:1]), next_token(C)]),
                   ("seat", [1]), ("step_batch", [1], []), ("sampler", 1, [next_token(C + c[:1])])]


def test_lone_prompt_takes_the_single_sequence_step():
    log, eng, out = run([C], 2, num_pages=4, max_batch=2)
    assert out == [alone(C, 2, ())]
    assert log == [("step", [], [(0, 0, 3)]), ("seat", [0]), ("step_batch", [0], [])]
    assert (eng.steps, eng.mixed_passes) == (1, 0)


def test_lone_prompt_with_a_sampler_record_is_a_batch_of_one():
    log, eng, out = run([C], 2, gen=dict(sampling=SamplingParams(temp=0.8, seed=1)), num_pages=4, max_batch=2)
    assert log == [("seat", [0]), ("prefill_batch", [], [(0, 0, 3)]), ("seat", [0]), ("step_batch", [0], [])]
    assert (eng.steps, eng.mixed_passes) == (1, 0)


def test_lone_prompt_on_int8_pages_is_a_batch_of_one():
    log, eng, out = run([C], 2, num_pages=4, max_batch=2, kv_dtype=torch.int8)
    assert out == [alone(C, 2, ())]
    assert log == [("seat", [0]), ("prefill_batch", [], [(0, 0, 3)]), ("seat", [0]), ("step_batch", [0], [])]


def test_suffixes_behind_a_shared_prefix_and_the_root_pass():
    """One whole page in common: the root pass computes it unseated, for no request; both suffixes then continue it from row 64 in one
    pass without decode rows."""
    system = list(range(100, 164))
    p, q = system + [1, 2], system + [3]
    log, eng, out = run([p, q], 2, num_pages=8, max_batch=2, share_prefix=True)
    assert out == [alone(p, 2, ()), alone(q, 2, ())]
    assert log == [("step_mixed", [], [("root", 0, 64)]),
                   ("seat", [0, 1]), ("step_mixed", [], [(0, 64, 2), (1, 64, 1)]),
                   ("seat", [0, 1]), ("step_batch", [0, 1], [])]
    assert (eng.steps, eng.mixed_passes, eng.shared_pages) == (1, 0, 1)


def test_a_request_that_retires_leaves_its_row_to_the_next():
    """Two slots, three requests; A's first token is a stop token.  It retires at the first read-back; B moves up to row 0 and C, admitted
    into the free slot, rides B's decode step in row 1."""
    stop = {next_token(A)}
    assert not stop & set(alone(B, 3, ()) + alone(C, 3, ()))
    log, eng, out = run([A, B, C], 3, stop=stop, num_pages=8, max_batch=2)
    assert out == [[next_token(A)], alone(B, 3, ()), alone(C, 3, ())]
    assert log == [("seat", [0, 1]), ("prefill_batch", [], [(0, 0, 2), (1, 0, 8)]),
                   ("seat", [1, 2]), ("step_mixed", [1], [(2, 0, 3)]),
                   ("seat", [1, 2]), ("step_batch", [1, 2], []),
                   ("seat", [2]), ("step_batch", [2], [])]
    assert (eng.steps, eng.mixed_passes) == (3, 1)


# ------------------------------------------------------------------ (b), (c) the grids, against the record of the parent commit
ENGINES = [dict(), dict(mixed=False), dict(batch_prefill=False), dict(prefill_chunk=16), dict(prefill_chunk=1), dict(prefill_chunk=300),
           dict(mixed=False, prefill_chunk=40), dict(max_prefill_rows=64), dict(kv_dtype=torch.int8), dict(kv_dtype=torch.int8, prefill_chunk=16)]
POOLS = [(1, 6), (3, 9), (8, 40)]
SHARED = [dict(), dict(prefill_chunk=24), dict(mixed=False)]
KINDS = [SamplingParams(), SamplingParams(temp=0.8, top_k=5, seed=11), SamplingParams(repetition_penalty=1.3, repetition_context_size=8),
         SamplingParams(frequency_penalty=0.5, presence_penalty=-1.0), SamplingParams(temp=0.9, top_p=0.9, seed=12, dry_multiplier=0.8)]


def name_of(form, kw, slots=None, pages=None):
    cfg = ",".join("%s=%s" % (k, str(v).replace("torch.", "")) for k, v in kw.items()) or "default"
    return "%s[%s]" % (form, cfg) + ("" if slots is None else "[%d,%d]" % (slots, pages))


def grid_case(form, kw, slots, pages):
    """One case of the grid of test_every_request_gets_the_tokens_it_gets_alone: (log, engine, outputs, expected outputs)."""
    prompts, stop, new = requests(7, 17), {3, 77}, 9
    gen = {"plain": None, "sampling": dict(sampling=[KINDS[i % len(KINDS)] for i in range(len(prompts))], logprobs=True, top_logprobs=2),
           "prompt_logprobs": dict(prompt_logprobs=1)}[form]
    log, eng, res = run(prompts, new, stop=stop, gen=gen, num_pages=pages, max_batch=slots, **kw)
    return log, eng, res if gen is None else res[0], [alone(p, new, stop) for p in prompts]


def shared_case(kw):
    import numpy as np
    system = np.random.default_rng(3).integers(0, V, 150).tolist()
    prompts = requests(11, 12, lo=1, hi=60, prefix=system)
    prompts[5] = system[:140] + [V - 1, V - 2]
    log, eng, res = run(prompts, 7, stop={5}, num_pages=12, max_batch=4, share_prefix=True, **kw)
    return log, eng, res, [alone(p, 7, {5}) for p in prompts]


def summary(log, eng):
    return {"digest": hashlib.sha256(repr(log).encode()).hexdigest()[:24], "entries": dict(sorted(Counter(e[0] for e in log).items())),
            "steps": eng.steps, "mixed_passes": eng.mixed_passes, "shared_pages": eng.shared_pages}


def cases():
    for form in ("plain", "sampling", "prompt_logprobs"):
        for slots, pages in POOLS:
            for kw in ENGINES:
                yield name_of(form, kw, slots, pages), (lambda form=form, kw=kw, slots=slots, pages=pages: grid_case(form, kw, slots, pages))
    for kw in SHARED:
        yield name_of("shared", kw), (lambda kw=kw: shared_case(kw))


def regenerate():
    GOLDEN.write_text(json.dumps({name: summary(*case()[:2]) for name, case in cases()}, indent=1) + "\n")


@pytest.fixture(scope="module")
def recorded():
    return json.loads(GOLDEN.read_text())


@pytest.mark.parametrize("name,case", list(cases()), ids=[name for name, _ in cases()])
def test_the_call_log_is_the_recorded_one(name, case, recorded):
    log, eng, out, want = case()
    assert out == want
    got = summary(log, eng)
    if got != recorded[name]:
        print("\n".join(repr(e) for e in log))
    assert got == recorded[name]


def test_the_record_holds_these_cases_only(recorded):
    assert sorted(recorded) == sorted(name for name, _ in cases())


if __name__ == "__main__":
    regenerate()
