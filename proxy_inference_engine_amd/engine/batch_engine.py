"""Continuous batching on top of the multi-sequence decode step (SURVEY.md 8 row f2's "unlocks multi-sequence batching").

The reference declares this shape -- a `Scheduler` that forms `BatchDetails` from prefill- and decode-state sequences over the
paged pool (src/pie_core/include/engine/batch_details.hpp:10-88, scheduler.hpp) -- without a body (`Scheduler::step` is
empty, the Python engine serves one sequence).  This is the smallest complete loop over the pieces that exist here: requests
wait in a queue, join the batch when a slot and enough pages are free -- their prompt rows ride the decode step of the sequences
in flight (`Model.step_mixed`: both kinds of sequence in one pass over the weights, as BatchDetails holds both), or run as a
prompt pass of their own when nothing is decoding -- every step decodes all active sequences with one pass over the weights
(`Model.step_batch`), finished sequences leave and return their pages.  Every such pass is formed and run by `BatchedEngine._pass`.  Greedy by default; `generate(sampling=...)` gives every request
its own `SamplingParams`, run per row inside the passes -- its token mask and logit_bias included, and its
frequency and presence penalties over the counts of what it has generated;
`sampler` maps a [B, V] log-probability block to B token ids;
`generate(logprobs=True, top_logprobs=...)` also returns every token's top-n log-probabilities, selected per row inside the passes;
`generate(prompt_logprobs=...)` also returns the log-probabilities of the prompts' own tokens, scored inside the prompt passes."""
from __future__ import annotations

from collections import deque
from contextlib import contextmanager
from dataclasses import dataclass, field
from typing import Callable, Iterable

import numpy as np
import torch

from ..cache.kv_cache.paged import TOKEN_CAPACITY_PER_PAGE
from .inference_engine import host_record_to_map


@dataclass
class SamplingParams:
    """One request's sampler and repetition penalty: the reference's per-Sequence SamplingParams (temperature, top_p, top_k, min_p, rng_seed;
    include/sequence/sampling_params.hpp) and LogitsParams (repetition_penalty, repetition_context_size; logits_params.hpp).  The branch
    is make_sampler's: temp == 0 greedy, else top_p inside (0, 1), else min_p != 0, else top_k > 0, else plain categorical.
    seed None: a fresh random seed per request.
    token_mask: what make_token_mask takes -- packed int32 words, a bool [V] mask, or a callable that receives every id the request has
    been fed so far (the prompt, then the prompt plus every generated token) and returns packed words, a bool mask or the allowed ids: the
    hook a grammar engine binds to.  logit_bias: {id: bias} under make_logit_bias's rules (1..1024 entries, finite values).  Both run per
    row inside the passes, in the single-sequence tail's order: mask, repetition penalty, bias.
    frequency_penalty / presence_penalty (each -2.0 .. 2.0; the two remaining fields of LogitsParams): logits[v] -= frequency_penalty *
    c[v] + presence_penalty wherever c[v] > 0, c = how often the request has GENERATED id v so far (its prompt does not count), per row
    inside the passes, after the bias: mask, repetition penalty, bias, frequency / presence.
    dry_multiplier != 0: the DRY penalty over the last dry_range ids the request has been fed, per row inside the passes,
    after the frequency / presence penalties: the token that would extend a repeat of the sequence's tail of at least dry_allowed_length
    ids loses dry_multiplier * dry_base ** (length - dry_allowed_length).  dry_sequence_breakers: up to 64 token ids a repeat does not cross.
    xtc_probability > 0 with xtc_threshold in (0, 0.5]: the request's draw runs under XTC, per row inside the passes' sampler;
    xtc_special_tokens: up to 16 ids XTC never removes, None: the engine's stop tokens.  A greedy request (temp == 0) ignores XTC.
    token_automaton: a logits_processors.TokenAutomaton -- a grammar compiled ahead of time, where token_mask stands and
    exclusive with it: the request's row derives its mask from the automaton's state inside the passes and advances the state by the token
    it drew (Model.set_batch_automata), so no callable runs for it on the host.
    Under BatchedEngine(speculative=...) a request's parameters must be plain, unless the engine was built with
    SpeculativeParams(batch_tail=True): then temp, top_p, top_k, min_p, min_tokens_to_keep, seed, XTC, repetition_penalty
    and logit_bias also run inside the speculative passes, per seat; token_mask, token_automaton, frequency_penalty / presence_penalty
    and DRY stay refused there."""
    temp: float = 0.0
    top_p: float = 1.0
    top_k: int = -1
    min_p: float = 0.0
    min_tokens_to_keep: int = 1
    seed: int | None = None
    repetition_penalty: float = 1.0
    repetition_context_size: int = 60
    token_mask: object = None
    logit_bias: dict | None = None
    frequency_penalty: float = 0.0
    presence_penalty: float = 0.0
    dry_multiplier: float = 0.0
    dry_base: float = 1.75
    dry_allowed_length: int = 2
    dry_range: int = 1024
    dry_sequence_breakers: tuple = ()
    xtc_probability: float = 0.0
    xtc_threshold: float = 0.0
    xtc_special_tokens: tuple | None = None
    token_automaton: object = None

    def xtc(self, stop_tokens=()) -> tuple | None:
        """(probability, threshold, special ids) under samplers.check_xtc's rules (ValueError otherwise), None when the request draws
        without XTC: probability 0, or a greedy request."""
        from ..samplers import check_xtc
        special = sorted(int(t) for t in stop_tokens) if self.xtc_special_tokens is None else self.xtc_special_tokens
        checked = check_xtc(self.xtc_probability, self.xtc_threshold, special, "SamplingParams")
        return None if self.temp == 0 else checked

    def hip_spec(self) -> tuple | None:
        """None (greedy) or (mode, temp, p, k) as hip_ops.sample / row_tail_pack take them."""
        from ..samplers import sampler_spec
        spec = sampler_spec(self.temp, self.top_p, self.min_p, self.min_tokens_to_keep, self.top_k)
        return None if spec is None else (spec[0], float(spec[1]), float(spec[2]), int(spec[3]))

    @property
    def recordless(self) -> bool:
        """Greedy without a repetition penalty: the request needs no record in the batch tail's table."""
        return self.temp == 0 and self.repetition_penalty == 1.0

    @property
    def counted(self) -> bool:
        """A frequency or a presence penalty: the request needs a row of the batch count penalty's state."""
        return self.frequency_penalty != 0.0 or self.presence_penalty != 0.0

    @property
    def tailless(self) -> bool:
        """Greedy without a penalty of any kind: the request's row needs no per-row state in a pass's tail."""
        return self.recordless and not self.counted and not self.dried

    @property
    def dried(self) -> bool:
        """A DRY penalty: the request needs a row of the batch DRY penalty's state."""
        return self.dry_multiplier != 0.0

    def dry(self) -> tuple:
        """(multiplier, base, allowed_length, range, breaker ids) under hip_ops.check_dry's rules: ValueError otherwise."""
        from .. import hip_ops
        return hip_ops.check_dry(self.dry_multiplier, self.dry_base, self.dry_allowed_length, self.dry_range, self.dry_sequence_breakers, "SamplingParams")

    @property
    def plain(self) -> bool:
        """Greedy without a penalty, a mask or a bias: today's tail."""
        return self.tailless and self.token_mask is None and self.logit_bias is None and self.token_automaton is None

    def automaton(self, vocab_size: int):
        """The request's TokenAutomaton or None, checked against the vocabulary: ValueError for another type, another vocabulary, and
        together with a token_mask."""
        from ..logits_processors import TokenAutomaton
        a = self.token_automaton
        if a is None:
            return None
        if self.token_mask is not None:
            raise ValueError("SamplingParams: token_mask and token_automaton are exclusive")
        if not isinstance(a, TokenAutomaton):
            raise ValueError("SamplingParams: token_automaton is a logits_processors.TokenAutomaton")
        a.check_vocab(vocab_size)
        return a

    def count_penalties(self) -> tuple[float, float]:
        """(frequency_penalty, presence_penalty), each within -2.0 .. 2.0: ValueError otherwise."""
        from .. import hip_ops
        return hip_ops.check_count_penalties(self.frequency_penalty, self.presence_penalty, "SamplingParams")

    def edits(self, vocab_size: int) -> tuple:
        """(the token mask's processor or None, (ids, values) of the bias table or None), checked as make_token_mask / make_logit_bias
        check them and against the vocabulary: ValueError for a bool mask of another length, too few packed words, a mask that allows
        nothing, a bad bias table."""
        from ..logits_processors import check_vocab, make_logit_bias, make_token_mask, packed_token_mask
        proc = bias = None
        if self.token_mask is not None:
            proc = make_token_mask(self.token_mask)
            check_vocab(proc, vocab_size)
            if proc.mask is not None:
                packed_token_mask(proc.mask, vocab_size)
        if self.logit_bias is not None:
            b = make_logit_bias(self.logit_bias)
            bias = (b.ids, b.values)
        return proc, bias

    def record(self, calls: int = 0, seed: int | None = None):
        """The request's device record (hip_ops.row_tail_pack) after `calls` drawn tokens; ValueError for arguments the samplers refuse."""
        from .. import hip_ops
        spec = self.hip_spec() or (None, 1.0, 0.0, 0)
        return hip_ops.row_tail_pack(*spec, seed=(self.seed or 0) if seed is None else seed, calls=calls, penalty=self.repetition_penalty,
                                     context_size=self.repetition_context_size)


@dataclass
class _Active:
    request: int
    cache: list
    token: torch.Tensor           # [1] int32 on the device: the input of the next step
    generated: list = field(default_factory=list)
    rec: torch.Tensor | None = None   # int32 [2 (n + 1)] on the device: the top-n record of `token` (ids, then the values' bits); None: not asked for
    fresh: list | None = None     # batched speculation: the tokens the last pass chose, already on the host (the last of them is `token`); None: read `token` back


SPEC_SEG_DRAFTS, SPEC_PASS_ROWS = 7, 256   # drafts of one sequence in a batched speculative pass; rows of the pass (hip_ops.SPEC_SEG_ROWS - 1, SPEC_BATCH_ROWS)


def spec_plan(counts: list, room: list, min_draft: int) -> list:
    """The drafts m_s every decode row presents in one batched speculative pass.  counts[s]: the ids the drafter found for
    row s (0: none, or none that is still valid); room[s]: the tokens the request may still generate.  m_s = count_s where count_s >=
    min_draft, else 0; then the three clamps: m_s <= 7; m_s <= room_s (the pass writes positions up to the fed token's + m_s, and the
    request's pages are reserved only as far as len(prompt) + max_new_tokens); sum(1 + m_s) <= 256, the largest drafts shortened first
    (the lowest row among equals)."""
    m = [min(c if c >= min_draft else 0, SPEC_SEG_DRAFTS, max(r, 0)) for c, r in zip(counts, room)]
    while len(m) + sum(m) > SPEC_PASS_ROWS and any(m):
        m[m.index(max(m))] -= 1
    return m


def cut_run(generated: list, tokens: list, stop_tokens, max_new_tokens: int) -> bool:
    """Appends the tokens one pass chose for a request to `generated`, in order, up to and including the first stop token or the
    max_new_tokens-th token: what lies behind that cut is dropped.  True: the request retires."""
    for t in tokens:
        generated.append(int(t))
        if int(t) in stop_tokens or len(generated) >= max_new_tokens:
            return True
    return False


class _SpecSeats:
    """Batched speculation's per-seat state of one generate() call.  Seat s is row s of the decode passes.  ids [max_batch,
    cap] / len [max_batch] on the device hold the ids of the request in the seat -- its prompt and what it has generated, the last id being
    the input of its next pass; a row is uploaded when its occupant changes (a request takes the seat, or moves to it when another retires)
    and is moved on by the passes themselves otherwise: the speculative pass's accept launch appends what it chose, a plain step's tokens
    are appended by one scatter.  Behind every decode pass ONE drafter launch over the seats is queued (Model.draft_rows); its counts come
    to the host with the pass's own read-back, and a draft counts only for the (request, tokens generated) it was made for."""

    def __init__(self, model, params, max_batch: int, prompts: list, max_new_tokens: int):
        self.model, self.p, self.prompts, self.max_new = model, params, prompts, max_new_tokens
        dev = model.device
        self.cap = max(len(p) for p in prompts) + max_new_tokens + SPEC_SEG_DRAFTS + 1   # a run may pass max_new_tokens before the host cuts it
        self.ids = torch.zeros((max_batch, self.cap), dtype=torch.int32, device=dev)
        self.len = torch.zeros(max_batch, dtype=torch.int32, device=dev)
        self.drafts = torch.full((max_batch, int(params.num_draft)), -1, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(max_batch, dtype=torch.int32, device=dev)
        self.held: list = [None] * max_batch      # (request, tokens generated) whose ids seat s holds
        self.drafted: list = [None] * max_batch   # (request, tokens generated) the draft in seat s was made for
        self.host_counts: list = [0] * max_batch  # that draft's count, once read
        self.pending = 0                          # seats whose counts are still on the device (a plain step's drafter launch)

    def sync(self, active: list) -> None:
        """Before a pass of decode rows only: every seat holds its occupant's ids."""
        for s, a in enumerate(active):
            want = (a.request, len(a.generated))
            if self.held[s] != want:
                seq = torch.tensor(list(self.prompts[a.request]) + a.generated, dtype=torch.int32)
                self.ids[s, :seq.numel()].copy_(seq)
                self.len[s:s + 1].fill_(seq.numel())
                self.held[s] = want
        for s in range(len(active), len(self.held)):
            self.held[s] = self.drafted[s] = None

    def plan(self, active: list) -> list:
        counts = [self.host_counts[s] if self.drafted[s] == (a.request, len(a.generated)) else 0 for s, a in enumerate(active)]
        return spec_plan(counts, [self.max_new - len(a.generated) for a in active], self.p.min_draft)

    def moved(self, active: list, n: list) -> None:
        """After a decode pass that chose n[s] tokens for seat s and queued the drafter behind them."""
        for s, a in enumerate(active):
            self.held[s] = self.drafted[s] = (a.request, len(a.generated) + n[s])

    def stale(self) -> None:
        """After a pass that moved the requests without moving the seats (it carried prompt rows): every seat is uploaded again."""
        self.held = [None] * len(self.held)
        self.drafted = [None] * len(self.held)
        self.pending = 0

    def after_step(self, active: list, nxt: torch.Tensor) -> None:
        """Behind a plain step of the seats: its tokens go behind the seats' ids on the device, and the drafter is queued."""
        B = len(active)
        self.ids[:B].scatter_(1, self.len[:B].long().clamp_(max=self.cap - 1)[:, None], nxt[:B, None])
        self.len[:B] += 1
        self.model.draft_rows(self.ids[:B], self.len[:B], self.p.ngram_max, self.p.ngram_min, self.p.num_draft, out=(self.drafts[:B], self.counts[:B]))
        self.moved(active, [1] * B)
        self.pending = B


@dataclass
class _Admitted:
    """A prompt that holds its slot and its pages and is not yet fully in them: fed whole in one pass, or prefill_chunk rows at a time."""
    request: int
    rows: list                    # what is fed: the prompt behind the shared prefix
    cache: list
    done: int = 0                 # rows fed so far


def per_prompt_counts(value, n_prompts: int, name: str, optional: bool = False) -> list:
    """generate's `top_logprobs` / `prompt_logprobs`: one value for every prompt or one per prompt, each an int in 0..20 -- or None where
    `optional`.  ValueError otherwise."""
    wants = list(value) if isinstance(value, Iterable) else [value] * n_prompts
    if len(wants) != n_prompts:
        raise ValueError(f"generate: `{name}` is " + ("None, one int, or one int or None per prompt" if optional else "one int or one per prompt"))
    if not all((optional and w is None) or (isinstance(w, int) and not isinstance(w, bool) and 0 <= w <= 20) for w in wants):
        raise ValueError(f"generate: every `{name}` is " + ("None or an int in 0..20" if optional else "an int in 0..20"))
    return wants


def request_kinds(model, n_prompts: int, sampling, top_logprobs, stop_tokens, host_sampler: bool, always_tails: bool = False) -> dict:
    """What one generate() call asks of the passes' per-row state, as _RowSeats' keyword arguments: every request's arguments are checked
    here, before anything runs (ValueError), and a kind is None -- neither armed nor written -- unless some request asks for it.
    sampling: generate's; top_logprobs: generate's, None without logprobs=True.  always_tails (batched speculation under batch_tail): a
    given `sampling` arms the batch tail whatever it holds -- the speculative pass applies a bias or draws under XTC through the tail."""
    kinds = dict.fromkeys(("tails", "edits", "cnts", "tops", "drys", "xtcs", "autos"))
    if top_logprobs is not None:
        if host_sampler:
            raise ValueError("generate: `logprobs` and the constructor's `sampler` callable exclude each other (a host sampler picks the token after the pass)")
        kinds["tops"] = per_prompt_counts(top_logprobs, n_prompts, "top_logprobs")
    if sampling is None:
        return kinds
    if host_sampler:
        raise ValueError("generate: `sampling` and the constructor's `sampler` callable exclude each other")
    params = [sampling] * n_prompts if isinstance(sampling, SamplingParams) else list(sampling)
    if len(params) != n_prompts or not all(isinstance(sp, SamplingParams) for sp in params):
        raise ValueError("generate: `sampling` is one SamplingParams or one per prompt")
    import os
    seeds = [int.from_bytes(os.urandom(8), "little") if sp.seed is None else int(sp.seed) for sp in params]
    for sp, sd in zip(params, seeds):
        sp.record(0, sd)
        sp.count_penalties()          # (the record knows nothing of these two: their own range check)
    asked = lambda each: each if any(e is not None for e in each) else None
    if any(sp.token_automaton is not None for sp in params):            # (these two need the model's vocabulary)
        kinds["autos"] = [sp.automaton(model.args.vocab_size) for sp in params]
    if any(sp.token_mask is not None or sp.logit_bias is not None for sp in params):
        kinds["edits"] = [sp.edits(model.args.vocab_size) for sp in params]
    kinds["cnts"] = asked([sp.count_penalties() if sp.counted else None for sp in params])
    drys = [sp.dry() for sp in params]                    # (checked for every request, armed or not: as XTC is below)
    kinds["drys"] = asked([d if sp.dried else None for sp, d in zip(params, drys)])
    kinds["xtcs"] = asked([sp.xtc(stop_tokens) for sp in params])
    if always_tails or not all(sp.recordless for sp in params):   # a request with only a mask, a bias or count penalties arms no batch tail
        kinds["tails"] = (params, seeds)
    return kinds


def pass_targets(prompts: list, wants: list, parts: list) -> tuple[list[int], list[int]]:
    """What the host writes for the prompt rows of one pass (Model.set_prompt_logprobs), in row order.  parts: (request, start, rows) --
    the pass holds rows prompts[request][start : start + rows].  The row of token j has target = token j + 1 of its prompt -- in this
    chunk or in a later pass's -- and count = the request's wants; a prompt's last row, which nothing follows, and every row of a request
    that is not scored (wants None) have count -1: their records are left alone."""
    targets, counts = [], []
    for req, start, rows in parts:
        p, w = prompts[req], wants[req]
        for j in range(start, start + rows):
            scored = w is not None and j + 1 < len(p)
            targets.append(int(p[j + 1]) if scored else 0)
            counts.append(int(w) if scored else -1)
    return targets, counts


class _PromptScores:
    """The prompts' own log-probabilities of one generate() call: arms the rows of every pass that carries prompt rows, keeps the pass's
    records on the device until the loop's next read-back of the tokens, and builds the maps from them there."""

    def __init__(self, model, prompts: list, wants: list, rows_cap: int):
        self.model, self.prompts, self.wants = model, prompts, wants
        self.bufs = model.set_prompt_logprobs(rows_cap, max(max(w for w in wants if w is not None), 1))
        self.maps: list = [None if w is None else [None] * len(p) for p, w in zip(prompts, wants)]
        self.pending: list = []      # (request, first row's token index, rows, int32 [rows, 2 (n + 1)] on the device: ids, then the values' bits)
        self.span = None

    def arm(self, n_decode: int, parts: list) -> None:
        """Before a pass whose rows n_decode.. are `parts` (pass_targets)."""
        targets, counts = pass_targets(self.prompts, self.wants, parts)
        dev = self.bufs["targets"].device
        self.bufs["targets"][n_decode:n_decode + len(targets)].copy_(torch.tensor(targets, dtype=torch.int32, device=dev))
        self.bufs["count"][n_decode:n_decode + len(counts)].copy_(torch.tensor(counts, dtype=torch.int32, device=dev))
        self.span = (n_decode, parts)

    def collect(self) -> None:
        """After that pass: its scored rows' records as fresh device tensors (the next pass overwrites the buffers)."""
        r, parts = self.span
        for req, start, rows in parts:
            if self.wants[req] is not None:
                self.pending.append((req, start, rows, torch.cat([self.bufs["ids"][r:r + rows], self.bufs["vals"][r:r + rows].view(torch.int32)], dim=1)))
            r += rows
        self.span = None

    def tensors(self) -> list:
        return [t.reshape(-1) for _, _, _, t in self.pending]

    def absorb(self, words) -> None:
        """words: the pending records as read back (numpy int32, flat, in `tensors` order)."""
        at = 0
        for req, start, rows, t in self.pending:
            rec = words[at:at + t.numel()].reshape(rows, 2, -1)
            at += t.numel()
            for k in range(rows):
                if start + k + 1 < len(self.prompts[req]):   # row of token j scores token j + 1
                    self.maps[req][start + k + 1] = host_record_to_map(rec[k, 0], rec[k, 1].view(np.float32), self.wants[req])[1]
        self.pending = []

    def flush(self) -> None:
        if self.pending:
            self.absorb(torch.cat(self.tensors()).cpu().numpy())


@contextmanager
def scored(scores: _PromptScores | None, n_decode: int, parts: list):
    """Around a pass whose rows n_decode.. are `parts` (pass_targets): armed before it, collected after it.  Nothing without `scores` or
    without prompt rows, and nothing is collected from a pass that raised."""
    on = scores is not None and bool(parts)
    if on:
        scores.arm(n_decode, parts)
    yield
    if on:
        scores.collect()


def same_occupant(have, want) -> bool:
    """What a row holds and what the coming pass wants there, each (request, tokens it has generated) or None: the same request one token
    further on is the row's own progress (the pass advances the device's state by that token itself), not a new occupant."""
    return want == have or (want is not None and have is not None and want[0] == have[0] and want[1] == have[1] + 1)


class _RowSeats:
    """The per-row tail state of one generate() call: which request's sampler record, top-n count, mask, bias table and counts every output
    row of the device buffers holds, rewritten where a row's occupant changes.  tails: (params, seeds) or None; edits: every request's
    SamplingParams.edits or None; cnts: every request's (frequency, presence) or None, or None; drys: every request's SamplingParams.dry or
    None, or None; tops: every request's top_logprobs or None
    (then `maps` collects their records' maps).  A kind that is None is neither armed nor written.  As a context manager: arms the kinds
    asked for with every row neutral, and clears them on the way out, whatever happened."""

    def __init__(self, model, max_batch: int, prompts: list, tails=None, edits=None, cnts=None, tops=None, drys=None, xtcs=None, autos=None):
        self.model, self.max_batch, self.prompts = model, max_batch, prompts
        self.autos = autos            # every request's TokenAutomaton or None, or None
        self.aseats: list = []        # token automata: what row s of the records holds, (request, tokens generated) or None = unarmed
        self.tails, self.edits, self.cnts, self.tops, self.drys = tails, edits, cnts, tops, drys
        self.xtcs = xtcs if tails is not None else None   # every request's SamplingParams.xtc or None, or None: XTC rides the batch tail's sampler
        self.maps = None if tops is None else [[] for _ in prompts]
        self.bufs = None              # the armed top-n buffers
        self.slots: list = []         # per-request tails: what the device table's row s holds, (request, tokens drawn) or None = greedy
        self.counts: list = []        # top-n records: the count the device holds for row s (-1: the row reports nothing)
        self.seats: list = []         # per-request edits: the request whose mask and bias table row s holds, None = unarmed
        self.words: list = []         # ... and the mask words row s holds when that request's mask is a callable
        self.cseats: list = []        # frequency / presence penalties: what row s of the counting state holds, (request, tokens generated) or None = a zero record
        self.dseats: list = []        # DRY penalty: what row s of the DRY state holds, (request, tokens generated) or None = a zero record

    def __enter__(self):
        m, every = self.model, list(range(self.max_batch))
        try:
            if self.tails is not None:
                m.set_batch_tail(self.max_batch)
                m.write_batch_tail(every, [SamplingParams().record()] * self.max_batch)   # (a cached table may hold an earlier call's records)
            if self.xtcs is not None:
                m.set_batch_xtc(self.max_batch)
                m.write_batch_xtc(every, [None] * self.max_batch)   # (cached buffers may hold an earlier call's rows)
            if self.edits is not None:
                any_mask, cap = any(k is not None for k, _ in self.edits), max(len(b[0]) if b else 0 for _, b in self.edits)
                m.set_batch_edits(self.max_batch, masks=any_mask, bias_cap=cap)
                m.write_batch_edits(every, [None] * self.max_batch if any_mask else None, [None] * self.max_batch if cap else None)   # (cached buffers may hold an earlier call's rows)
            if self.autos is not None:   # behind the edits: the automata write the edits' masks, and arm a mask part where none is set
                distinct = {id(a): a for a in self.autos if a is not None}
                m.set_batch_automata(self.max_batch, sum(a.words().size for a in distinct.values()))
            if self.cnts is not None:
                m.set_batch_count_penalty(self.max_batch)
                m.write_batch_count_penalty(every, [None] * self.max_batch)   # (cached buffers may hold an earlier call's rows)
            if self.drys is not None:
                m.set_batch_dry_penalty(self.max_batch)
                m.write_batch_dry_penalty(every, [None] * self.max_batch)   # (cached buffers may hold an earlier call's rows)
            if self.tops is not None:
                self.bufs = m.set_batch_top_logprobs(self.max_batch, max(max(self.tops, default=1), 1))
                self.bufs["count"].fill_(-1)       # (cached buffers may hold an earlier call's counts)
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc) -> None:
        for asked, clear in ((self.autos, "clear_batch_automata"), (self.tails, "clear_batch_tail"), (self.edits, "clear_batch_edits"), (self.cnts, "clear_batch_count_penalty"),
                             (self.drys, "clear_batch_dry_penalty"), (self.xtcs, "clear_batch_xtc"),
                             (self.tops, "clear_batch_top_logprobs")):
            if asked is not None:
                getattr(self.model, clear)()

    @staticmethod
    def _changed(held: list, want: list, same=same_occupant, empty=None) -> list[int]:
        """The rows of `want` that do not hold the `same` as `held` records (rows it has not seen: `empty`); `held` is brought up to date."""
        held.extend([empty] * (len(want) - len(held)))
        rows = [s for s, w in enumerate(want) if not same(held[s], w)]
        held[:len(want)] = want
        return rows

    def seat(self, rows: list, active: list) -> None:
        """The coming pass's output rows, in order: a request index (its own record; its ring rows from the ids it has been fed) or
        None (a prompt still filling: greedy, its token is discarded).  Rewrites the rows whose occupant changed -- the moment at which
        step_batch rewrites the block table; a row a request keeps is left alone (its `calls` advances on the device).  The rows' top-n
        counts follow the same rule: a request's own top_logprobs, -1 for a prompt still filling.  active: the sequences in flight."""
        prompts, edits, cnts = self.prompts, self.edits, self.cnts
        gen_by = {a.request: a.generated for a in active}
        if self.tops is not None:
            want_c = [-1 if r is None else self.tops[r] for r in rows]
            changed, count = self._changed(self.counts, want_c, int.__eq__, -1), self.bufs["count"]
            if changed:
                count.index_copy_(0, torch.tensor(changed, dtype=torch.long, device=count.device),
                                  torch.tensor([want_c[s_] for s_ in changed], dtype=torch.int32, device=count.device))
        if self.autos is not None:
            # a row's automaton record and state are rewritten where its sampler record is: when its occupant changes, the state being the
            # automaton's walk over the ids the request has generated so far (the last of them is the row's input).  A row a request keeps
            # is left alone: the pass advanced its state on the device.  A prompt that is still filling, and a request without an
            # automaton, hold a zero record.  In front of the edits: a row that loses its automaton loses the mask it wrote.
            autos = self.autos
            want = [None if r is None or autos[r] is None else (r, len(gen_by.get(r, []))) for r in rows]
            a_rows = self._changed(self.aseats, want)
            moved = [want[s_] for s_ in a_rows]
            self.model.write_batch_automata(a_rows, [None if w is None else autos[w[0]] for w in moved],
                                            [None if w is None else autos[w[0]].walk(gen_by.get(w[0], [])) for w in moved])
        if edits is not None:
            # a row's mask and bias table are rewritten where its record is: when its occupant changes.  A callable mask is evaluated for
            # every live row, every pass, on what the request has been fed -- the loop's read-back already brought the tokens -- and the
            # rows whose words changed go up in one copy.
            from ..logits_processors import packed_token_mask
            V, seats, words = self.model.args.vocab_size, self.seats, self.words
            want_e = [r if r is not None and edits[r] != (None, None) else None for r in rows]
            seats.extend([None] * (len(want_e) - len(seats)))
            words.extend([None] * (len(want_e) - len(words)))
            m_rows, m_new, b_rows, b_new = [], [], [], []
            for s_, r in enumerate(want_e):
                proc, bias = edits[r] if r is not None else (None, None)
                moved = seats[s_] != r
                if moved:
                    if any(b is not None for _, b in edits):
                        b_rows.append(s_), b_new.append(bias)
                    words[s_] = None
                if proc is not None and proc.mask_fn is not None:
                    w = packed_token_mask(proc.mask_fn(list(prompts[r]) + list(gen_by.get(r, []))), V)
                    if words[s_] is None or not torch.equal(words[s_], w):
                        m_rows.append(s_), m_new.append(w)
                        words[s_] = w
                elif moved and any(m is not None for m, _ in edits):
                    m_rows.append(s_), m_new.append(None if proc is None else proc.mask)
                seats[s_] = r
            if m_rows:
                self.model.write_batch_edits(m_rows, masks=m_new)
            if b_rows:
                self.model.write_batch_edits(b_rows, biases=b_new)
        if cnts is not None:
            # a row's record and counts are rebuilt where its sampler record is: when its occupant changes, from the ids the request has
            # generated so far (the host holds them; the last of them is the row's input, counted here and not again by the pass).  A
            # prompt that is still filling, and a request without penalties, hold a zero record.
            want = [None if r is None or cnts[r] is None else (r, len(gen_by.get(r, []))) for r in rows]
            c_rows = self._changed(self.cseats, want)
            moved = [want[s_] for s_ in c_rows]
            self.model.write_batch_count_penalty(c_rows, [None if w is None else (*cnts[w[0]], len(prompts[w[0]])) for w in moved],
                                                 [None if w is None else list(gen_by.get(w[0], [])) for w in moved])
        if self.drys is not None:
            # a row's record, breaker table and ring are rebuilt where its sampler record is: when its occupant changes, from the ids the
            # request has been fed so far (the pass records the row's own input id).  A prompt that is still filling, and a request
            # without DRY, hold a zero record.
            drys = self.drys
            want = [None if r is None or drys[r] is None else (r, len(gen_by.get(r, []))) for r in rows]
            d_rows = self._changed(self.dseats, want)
            moved = [want[s_] for s_ in d_rows]
            self.model.write_batch_dry_penalty(d_rows, [None if w is None else drys[w[0]] for w in moved],
                                               [None if w is None else list(prompts[w[0]]) + list(gen_by.get(w[0], [])[:-1]) for w in moved])
        if self.tails is None:
            return
        params, seeds = self.tails
        want = [None if r is None else (r, len(gen_by.get(r, []))) for r in rows]
        idx = self._changed(self.slots, want)
        recs, fed = [], []
        for w in (want[s_] for s_ in idx):
            if w is None:
                recs.append(SamplingParams().record())
                fed.append(None)
            else:
                sp = params[w[0]]
                recs.append(sp.record(w[1], seeds[w[0]]))
                fed.append(None if sp.repetition_penalty == 1.0 else list(prompts[w[0]]) + list(gen_by.get(w[0], [])[:-1]))
        self.model.write_batch_tail(idx, recs, fed)
        if self.xtcs is not None:  # a row's XTC record moves with its sampler record
            self.model.write_batch_xtc(idx, [None if want[s_] is None else self.xtcs[want[s_][0]] for s_ in idx])

    def moved(self, n: list) -> None:
        """Behind a speculative pass under the seats' tails that chose n[s] tokens for seat s: the device moved the seat's
        `calls` and ring by n[s] itself, so what the table's row holds moves with it -- the same request n[s] tokens further on, which the
        next `seat` finds in place and does not rewrite.  A seat whose occupant then changes is rewritten from the host's state, as ever."""
        for s, k in enumerate(n):
            if self.slots[s] is not None:
                self.slots[s] = (self.slots[s][0], self.slots[s][1] + k)

    def lone_step(self, idx) -> bool:
        """A lone prompt takes the single-sequence prompt pass (greedy tail) unless its request has a record, a mask or a bias of its
        own, or wants log-probabilities: then it is a batch of one.  Frequency / presence penalties alone do not make it one: a request's
        first token is chosen against empty counts, which is the unpenalised row, so the greedy prompt pass gives the token the
        penalised one would; the request's row of the counting state is written when it first sits in a pass (`seat`).  A DRY penalty
        does make it one: the first token is chosen against the prompt's own window.  So does a token automaton: the first token is chosen
        under the start state's mask."""
        return self.tops is None and (self.autos is None or self.autos[idx] is None) and (self.drys is None or self.drys[idx] is None) and (self.tails is None or self.tails[0][idx].tailless) and (self.edits is None or self.edits[idx] == (None, None))

    def records(self, n_rows: int):
        """The last pass's top-n records of output rows [0, n_rows) as one fresh int32 [n_rows, 2 (n + 1)] tensor (ids, then the values'
        bits): row views of it outlive the next pass.  None when log-probabilities are not asked for."""
        if self.tops is None:
            return [None] * n_rows
        return torch.cat([self.bufs["ids"][:n_rows], self.bufs["vals"][:n_rows].view(torch.int32)], dim=1)


class BatchedEngine:
    def __init__(self, model, num_pages: int = 1024, max_batch: int = 32, stop_tokens: Iterable[int] = (),
                 sampler: Callable[[torch.Tensor], torch.Tensor] | None = None, batch_prefill: bool = True, max_prefill_rows: int = 4096,
                 kv_dtype: torch.dtype | None = None, kv_scales=None, mixed: bool = True, prefill_chunk: int | None = None, share_prefix: bool = False,
                 speculative=None):
        """kv_dtype=torch.int8 (+ kv_scales = (k, v) float16 [n_layers, n_kv_heads]): the pool holds the reference KVPage's int8 pages with
        per-head scales (page.hpp:25-32) -- half the cache bytes per token, so twice the sequences / context per pool.
        speculative=SpeculativeParams(num_draft=, ngram_max=, ngram_min=, min_draft=): greedy prompt-lookup speculation for
        every request at once.  Behind every decode pass one drafter launch looks every sequence's last ids up in the sequence itself; an
        iteration of decode rows only then gives sequence s 1 + m_s rows of ONE pass over the weights (Model.spec_step_batch) -- m_s = its
        draft where that has at least min_draft ids, at most 7, else 0 -- and accepts each draft while it equals the greedy token of the
        row before it; an iteration in which no sequence has a draft is the replayed step as ever, and an iteration that carries prompt
        rows runs without drafts.  The tokens are greedy decoding's; `spec_stats` counts the passes.  None: today's engine exactly.
        ValueError, by name: a `sampler`, kv_dtype=torch.int8, a tensor-parallel model, num_draft > 7, draft_model, grammar and
        configured_tail; generate() then refuses any request whose SamplingParams is not plain, logprobs, top_logprobs and prompt_logprobs.
        SpeculativeParams(batch_tail=True): generate() also admits requests whose SamplingParams set temp, top_p, top_k,
        min_p, min_tokens_to_keep, seed, XTC, repetition_penalty and logit_bias -- with `sampling` given the pass is
        Model.spec_step_batch_tail, which applies every seat's own record, ring, bias table and XTC record to the rows of its segment and
        accepts a draft while it equals the row's draw: the tokens are those the plain passes draw.  Still refused by name: a token mask,
        a token automaton, frequency / presence penalties, DRY, logprobs, top_logprobs and prompt_logprobs."""
        if speculative is not None:
            who = "BatchedEngine(speculative=...): "
            for bad, name in ((sampler is not None, "a `sampler` callable"), (kv_dtype == torch.int8, "kv_dtype=torch.int8 (int8 KV pages)"),
                              (getattr(model, "tp", None) is not None, "a tensor-parallel model"), (int(speculative.num_draft) > SPEC_SEG_DRAFTS, "num_draft > 7"),
                              (speculative.draft_model is not None, "draft_model"), (bool(speculative.grammar), "grammar"),
                              (bool(speculative.configured_tail), "configured_tail")):
                if bad:
                    raise ValueError(who + "not available with " + name)
        self.speculative = speculative
        self.spec_stats = {"passes": 0, "steps": 0, "drafted": 0, "accepted": 0}   # of the last generate(): speculative passes, plain decode passes, ids drafted / accepted
        self.model = model
        self.pool = model.enable_paged_kv(num_pages=num_pages, kv_dtype=kv_dtype, kv_scales=kv_scales)
        self._i8 = self.pool.dtype == torch.int8   # int8 pages are written by the batch paths only: lone prompts go through prefill_batch too
        self.max_batch = max_batch
        self.stop_tokens = set(int(t) for t in stop_tokens)
        self.sampler = sampler
        self.batch_prefill = batch_prefill          # admit several waiting prompts with one pass over the weights
        self.max_prefill_rows = max_prefill_rows    # prompt tokens per such pass
        self.mixed = mixed            # prompts admitted while sequences are decoding join THAT pass (Model.step_mixed) instead of a pass of their own
        # chunked prefill: an admitted prompt is fed at most this many rows per pass (all filling prompts together), every pass also decoding the
        # sequences in flight -- a long prompt no longer stalls them for its whole length.  T pages only (a continuing prompt reads T pages).
        self.prefill_chunk = None if (prefill_chunk is None or self._i8) else max(1, int(prefill_chunk))
        # shared prompt prefix (a system prompt): the whole pages of the requests' longest common prefix are computed ONCE and shared by
        # reference count (KVPage::add_ref, page.hpp:55-68 -- PagedSequence.fork); every request then feeds only its own suffix, as a prompt
        # continuing a cached prefix.  T pages only.
        self.share_prefix = bool(share_prefix) and not self._i8
        self.shared_pages = 0         # pages of the last generate()'s shared prefix
        self.steps = 0                # batched decode steps taken (for throughput accounting)
        self.mixed_passes = 0         # ... of which carried prompt rows as well

    def _pages_for(self, n_tokens: int) -> int:
        return (n_tokens + TOKEN_CAPACITY_PER_PAGE - 1) // TOKEN_CAPACITY_PER_PAGE

    def generate(self, prompts: list, max_new_tokens: int, sampling: SamplingParams | list | None = None, logprobs: bool = False,
                 top_logprobs: int | list = 0, prompt_logprobs: int | list | None = None):
        """Token ids generated for every prompt (in order), at most max_new_tokens each, ending early at a stop token.
        sampling: None (greedy, or the constructor's `sampler`), one SamplingParams for every request, or one per prompt: each request's
        own sampler, seed and repetition penalty, applied to its row inside every pass (Model.set_batch_tail) -- a request's tokens depend
        on its seed and on what it was fed, not on the row it occupies or on its neighbours' parameters.  A request's frequency_penalty and
        presence_penalty run on per-row counts of its own generated tokens (Model.set_batch_count_penalty), rebuilt from the ids the
        host holds whenever the request takes another row; so does its DRY penalty (dry_multiplier != 0), on a ring of the ids it has
        been fed (Model.set_batch_dry_penalty).  A request's token_mask and
        logit_bias ride the same passes (Model.set_batch_edits); a callable mask is evaluated on the host after the per-pass read-back of
        the tokens and only the rows whose words changed are uploaded.  With logprobs=True the maps report the processed log-probabilities.
        logprobs=True: returns (outputs, maps) -- maps[i][j] is the {token id: log-probability} dict of outputs[i][j], as
        InferenceEngine.generate yields it: the best top_logprobs pairs by decreasing log-probability (ties: lowest id first), then the
        token itself when absent.  top_logprobs: one int for every request or one per prompt, each 0..20; ignored with logprobs=False.  The
        records are selected per row inside the passes (Model.set_batch_top_logprobs) and fetched in the per-pass read-back of the tokens.
        prompt_logprobs: None (nothing changes, the return shape included), one int for every request, or one int or None per prompt, each
        0..20: the prompt maps are appended as the last element of the returned tuple -- prompt_maps[i] is None for a request that asked
        for none, else a list as long as prompt i: entry 0 None, entry j the {id: log-probability} map of prompt token j given the tokens
        before it, under the raw model distribution: the best prompt_logprobs pairs, then the token itself when absent
        (InferenceEngine.score's list).  Scored inside the prompt passes (Model.set_prompt_logprobs), across prefill_chunk
        boundaries, and fetched in the per-pass read-back of the tokens.
        With speculative= set on the engine: `sampling` must be plain and logprobs, top_logprobs and prompt_logprobs are refused; under
        SpeculativeParams(batch_tail=True) `sampling` may set a sampler, XTC, a repetition penalty and a logit_bias -- the
        tokens are then the ones the plain passes draw, token j of a request being draw j of its seed from its own row -- and a token
        mask, a token automaton, frequency / presence penalties and DRY are refused by name.  ValueError with share_prefix=True (the shared pages' rows are
        computed once, for no request in particular, and cannot be scored) and with max_new_tokens < 1 (InferenceEngine.score runs a prompt only)."""
        if self.speculative is not None:
            who = "generate: batched speculation is greedy and raw -- not available with "
            params = [] if sampling is None else [sampling] if isinstance(sampling, SamplingParams) else list(sampling)
            if self.speculative.batch_tail:
                who = "generate: batched speculation under batch_tail -- not available with "
                for sp in (sp for sp in params if isinstance(sp, SamplingParams)):
                    for bad, name in ((sp.token_mask is not None, "a token mask"), (sp.token_automaton is not None, "a token automaton"),
                                      (sp.counted, "frequency / presence penalties"), (sp.dried, "a DRY penalty")):
                        if bad:
                            raise ValueError(who + name)
            elif any(not (isinstance(sp, SamplingParams) and sp.plain) for sp in params):
                raise ValueError(who + "a request whose `sampling` is not plain (a sampler, penalty, mask, bias or automaton)")
            if logprobs:
                raise ValueError(who + "`logprobs`")
            if not (isinstance(top_logprobs, int) and top_logprobs == 0):
                raise ValueError(who + "`top_logprobs`")
            if prompt_logprobs is not None:
                raise ValueError(who + "`prompt_logprobs`")
        if prompt_logprobs is None:
            return self._run(prompts, max_new_tokens, sampling, logprobs, top_logprobs, None)
        wants = per_prompt_counts(prompt_logprobs, len(prompts), "prompt_logprobs", optional=True)
        if self.share_prefix:
            raise ValueError("generate: `prompt_logprobs` and share_prefix=True exclude each other (the shared pages' rows are never computed for a request)")
        if max_new_tokens < 1:
            raise ValueError("generate: `prompt_logprobs` needs max_new_tokens >= 1 (InferenceEngine.score runs a prompt only)")
        scores = None
        try:
            if any(w is not None for w in wants):
                rows_cap = min(65535, self.max_batch + max([self.max_prefill_rows, self.prefill_chunk or 0] + [len(p) for p in prompts]))
                scores = _PromptScores(self.model, prompts, wants, rows_cap)
            res = self._run(prompts, max_new_tokens, sampling, logprobs, top_logprobs, scores)
        finally:
            if scores is not None:
                self.model.clear_prompt_logprobs()
        maps = scores.maps if scores is not None else [None] * len(prompts)
        return (*res, maps) if logprobs else (res, maps)

    def _run(self, prompts, max_new_tokens, sampling, logprobs, top_logprobs, scores):
        """generate's body; scores: the call's _PromptScores or None."""
        kinds = request_kinds(self.model, len(prompts), sampling, top_logprobs if logprobs else None, self.stop_tokens, self.sampler is not None,
                              always_tails=self.speculative is not None and self.speculative.batch_tail)
        if max_new_tokens < 1:
            return ([[] for _ in prompts], [[] for _ in prompts]) if logprobs else [[] for _ in prompts]
        with _RowSeats(self.model, self.max_batch, prompts, **kinds) as seats:
            out = self._generate(prompts, max_new_tokens, seats, scores)
        return out if seats.tops is None else (out, seats.maps)

    def _pass(self, seats: _RowSeats, scores, P: int, active: list, parts: list) -> list:
        """One pass over the weights: a decode step of `active` (_Active, in row order) and, behind them, parts = (_Admitted, rows) -- the next
        `rows` rows of each admitted prompt.  Seats the output rows, arms and collects the prompt scores, picks the Model entry, counts the
        pass, lets the host sampler redraw, and hands every row its token and top-n record: the decode rows in place; the prompts that this
        pass finished are returned as new _Active.  P: the shared prefix in force (such prompts continue cached pages).
        A token is a row view of the pass's result: the varlen passes return fresh tensors, and step_batch's buffer, which the model owns per
        batch size, is next written by the next iteration's decode step -- after that iteration's read-back."""
        nb = len(active)
        ends = [p.done + n == len(p.rows) for p, n in parts]                # a part that does not finish its prompt produces no token: seated None
        seats.seat([a.request for a in active] + [p.request if end else None for (p, _), end in zip(parts, ends)], active)
        tokens, caches = torch.cat([a.token for a in active]) if active else None, [a.cache for a in active]
        rows, into = [p.rows[p.done:p.done + n] for p, n in parts], [p.cache for p, _ in parts]
        with scored(scores, nb, [(p.request, p.done, n) for p, n in parts]):
            if not parts:
                nxt, logprobs, _ = self.model.step_batch(tokens, caches)
            elif not active and not self.prefill_chunk and P == 0:          # fresh whole prompts alone (int8 pages take prompts through this entry only)
                nxt, logprobs, _ = self.model.prefill_batch(rows, into)
            else:
                nxt, logprobs, _ = self.model.step_mixed(tokens, caches, rows, into)
        self.steps += bool(active or self.prefill_chunk)                     # a decode step, or the chunked pass (which stands for one)
        self.mixed_passes += bool(active and parts)
        if self.sampler is not None:
            # the sampler sees generation steps only: the decode rows and the rows of prompts whose LAST chunk is in this pass; the row
            # of a prompt that is still filling is discarded (its greedy id stands in), so a seeded sampler's stream and a stateful
            # sampler's history do not depend on the chunk size
            live = list(range(nb)) + [nb + i for i, end in enumerate(ends) if end]
            if live:
                some = len(live) < nb + len(parts)
                idx = torch.tensor(live, dtype=torch.long, device=logprobs.device) if some else slice(None)   # (every row: the block itself)
                drawn = self.sampler(logprobs[idx]).reshape(-1).to(torch.int32)
                if some:
                    nxt[idx] = drawn                                         # (only a pass with prompt rows has such rows: its result is a fresh tensor)
                else:
                    nxt = drawn
        recs = seats.records(nb + len(parts))
        for i, a in enumerate(active):
            a.token, a.rec = nxt[i:i + 1], recs[i]
        joined = []
        for i, ((p, n), end) in enumerate(zip(parts, ends), nb):
            p.done += n
            if end:                                                          # the row's token is the request's first
                joined.append(_Active(p.request, p.cache, nxt[i:i + 1], rec=recs[i]))
        return joined

    def _spec_decode(self, spec: _SpecSeats, seats: _RowSeats, scores, P: int, active: list) -> None:
        """An iteration of decode rows only under batched speculation: the seats' ids are brought up to date, every row
        gets its drafts (spec_plan), and the iteration is ONE speculative pass -- or, where no row has a draft, the replayed step untouched,
        its tokens appended to the seats' ids on the device.  Either way the next drafter launch is queued behind it.  The pass is the
        greedy and raw one, or -- where the seats hold a batch tail -- the one under the seats' tails, behind which the
        seats' bookkeeping moves by what the device moved."""
        spec.sync(active)
        m = spec.plan(active)
        if not any(m):
            self._pass(seats, scores, P, active, [])
            spec.after_step(active, torch.cat([a.token for a in active]))
            self.spec_stats["steps"] += 1
            return
        seats.seat([a.request for a in active], active)
        sp = self.speculative
        entry = self.model.spec_step_batch if seats.tails is None else self.model.spec_step_batch_tail   # (a tail: `sampling` was given under batch_tail)
        n, toks, nxt = entry(torch.cat([a.token for a in active]), [a.cache for a in active], spec.drafts, m, spec.ids, spec.len,
                             then_draft=(sp.ngram_max, sp.ngram_min, sp.num_draft, spec.drafts))
        if seats.tails is not None:
            seats.moved(n)
        spec.moved(active, n)
        spec.host_counts[:len(active)] = nxt
        last = torch.tensor([t[-1] for t in toks], dtype=torch.int32, device=self.model.device)   # (the record is on the host already: one small upload)
        for s, (a, t) in enumerate(zip(active, toks)):
            a.fresh, a.token = t, last[s:s + 1]
        self.steps += 1
        self.spec_stats["passes"] += 1
        self.spec_stats["drafted"] += sum(m)
        self.spec_stats["accepted"] += sum(n) - len(n)

    def _lone_prompt(self, scores, p: _Admitted) -> _Active:
        """The one prompt pass that is not a batch pass: a lone prompt whose request needs no per-row state (_RowSeats.lone_step) through the
        single-sequence Model.step -- nothing to seat, no top-n record."""
        with scored(scores, 0, [(p.request, 0, len(p.rows))]):              # (record i belongs to row i of the prompt)
            tok, logprobs, _ = self.model.step(torch.as_tensor(p.rows, dtype=torch.int32).reshape(-1).to(self.model.device), p.cache)
        if self.sampler is not None:
            tok = self.sampler(logprobs[None]).reshape(1).to(torch.int32)
        return _Active(p.request, p.cache, tok.reshape(1).clone())

    def _generate(self, prompts: list, max_new_tokens: int, seats: _RowSeats, scores=None) -> list[list[int]]:
        for p in prompts:
            if self._pages_for(len(p) + max_new_tokens) > self.pool.size():
                raise ValueError("a prompt does not fit the page pool")
        pending = deque(enumerate(prompts))
        active: list[_Active] = []
        out: list[list[int]] = [[] for _ in prompts]
        reserved = 0                  # pages promised to the active sequences for their full length
        need = {}
        root, P = None, 0             # the sequence holding the shared prefix, its length (whole pages)
        self.shared_pages = 0
        if self.share_prefix and len(prompts) > 1:
            lcp = min(len(p) for p in prompts) - 1                         # every request keeps at least one token of its own
            first = prompts[0]
            for p in prompts[1:]:
                n = 0
                while n < lcp and p[n] == first[n]:
                    n += 1
                lcp = n
            P = lcp // TOKEN_CAPACITY_PER_PAGE * TOKEN_CAPACITY_PER_PAGE
            if P and self._pages_for(P) + self._pages_for(max(len(p) for p in prompts) - P + max_new_tokens) <= self.pool.size():
                root = self.model.make_cache()
                self.model.step_mixed(None, [], [list(first[:P])], [root])    # one pass over the prefix; its pages are shared from here on (no top-n record: every count is still -1)
                reserved = self.shared_pages = P // TOKEN_CAPACITY_PER_PAGE
            else:
                P = 0

        def new_cache():
            if root is None:
                return self.model.make_cache()
            seq = root[0].page_manager.fork()                               # whole pages: add_ref only, nothing is copied
            return [type(root[0])(seq, i) for i in range(len(root))]
        filling: list[_Admitted] = []   # chunked prefill: the admitted prompts not yet fully in their pages, oldest first
        tops = seats.tops
        spec = _SpecSeats(self.model, self.speculative, self.max_batch, prompts, max_new_tokens) if self.speculative is not None and prompts else None
        self.spec_stats = dict.fromkeys(self.spec_stats, 0)
        run = lambda rows, parts: self._pass(seats, scores, P, rows, parts)
        whole = lambda admitted: [(p, len(p.rows)) for p in admitted]

        while pending or active or filling:
            # 1. every active sequence holds one token not yet recorded (from its prompt or from the last pass): record, retire
            if active and spec is not None and all(a.fresh is not None for a in active):
                chosen = [a.fresh for a in active]   # a speculative pass read its own record back: nothing is left on the device
            elif active:
                # one read-back per pass for the stop / length checks -- and, in the same copy, the tokens' top-n records
                n_top = sum(a.rec.numel() for a in active) if tops is not None else 0
                counts = [spec.counts[:spec.pending]] if spec is not None and spec.pending else []   # (the counts of the draft queued behind a plain step)
                host = torch.cat([a.token for a in active] + ([a.rec for a in active] if tops is not None else []) + (scores.tensors() if scores else []) + counts).cpu().numpy()
                if counts:
                    spec.host_counts[:spec.pending], host, spec.pending = host[-spec.pending:].tolist(), host[:-spec.pending], 0
                if scores:
                    scores.absorb(host[len(active) + n_top:])
                if tops is not None:
                    recs = host[len(active):len(active) + n_top].reshape(len(active), 2, -1)
                    for a, r in zip(active, recs):
                        seats.maps[a.request].append(host_record_to_map(r[0], r[1].view(np.float32), tops[a.request])[1])
                chosen = [[t] if a.fresh is None else a.fresh for a, t in zip(active, host[:len(active)].tolist())]   # (fresh: a speculative pass's run beside newly joined prompts)
            if active:
                keep = []
                for a, run_tokens in zip(active, chosen):
                    a.fresh = None
                    if cut_run(a.generated, run_tokens, self.stop_tokens, max_new_tokens):   # (a plain pass's one token; a speculative pass's run, cut)
                        out[a.request] = a.generated
                        a.cache[0].page_manager.release()
                        reserved -= need.pop(a.request)
                    else:
                        keep.append(a)
                active = keep
            # 2. admit while there is a slot and the pool can hold the request to its end; the admitted prompts run as ONE pass
            batch: list[_Admitted] = []
            rows = 0
            while pending and len(active) + len(batch) + len(filling) < self.max_batch:
                idx, prompt = pending[0]
                n_pages = self._pages_for(len(prompt) + max_new_tokens) - P // TOKEN_CAPACITY_PER_PAGE
                if reserved + n_pages > self.pool.size() or (rows > 0 and rows + len(prompt) - P > self.max_prefill_rows):
                    break
                pending.popleft()
                need[idx] = n_pages
                reserved += n_pages
                rows += len(prompt) - P
                batch.append(_Admitted(idx, prompt[P:] if P else prompt, new_cache()))
            if self.prefill_chunk:
                filling, batch = filling + batch, []
            if not active and not batch and not filling:
                if pending:
                    raise RuntimeError("no request fits the page pool")  # unreachable after the check above
                break
            # 3. the passes of this iteration.  Admitted prompts ride the decode step of the sequences in flight (one pass over the weights for both)
            # while the decode rows do not push the prompt rows into another 256-row GEMM tile: 8 sequences + a prompt of
            # 8 / 64 / 192 / 256 / 384 rows on the 8B model take 0.61 / 0.76 / 0.75 / 0.97 / 0.84 of a prompt pass + a step, but
            # 508 / 2048 rows take 1.08 / 1.06 (516 rows are three 256-row tiles' worth of work for the GEMMs, 508 are two).
            n_mix = len(active) + rows
            carried = False               # this iteration's decode rows rode a pass that carried prompt rows
            mix = active and batch and self.mixed and (n_mix <= 512 or (n_mix + 255) // 256 == (rows + 255) // 256)
            if filling:
                # one pass: every decoding sequence's step + the next rows of the filling prompts, oldest first, prefill_chunk rows in all (decode rows included)
                take, budget = [], max(1, self.prefill_chunk - len(active))   # the pass's rows INCLUDING the decode rows: a chunk of 256 + 8 decode rows would cost the GEMMs a second 256-row tile
                for p in filling:
                    n = min(len(p.rows) - p.done, budget)
                    if n > 0:
                        take.append((p, n))
                        budget -= n
                joined = run(active, take)
                filling = [p for p in filling if p.done < len(p.rows)]
                carried = bool(active)
            elif mix:
                joined = run(active, whole(batch))
                carried = True
            else:
                # the prompts in passes of their own -- one each for a single prompt and without batch_prefill, unless they continue the
                # shared prefix; else jointly --, then the decode step
                if batch and not P and (len(batch) == 1 or not self.batch_prefill):
                    joined = []
                    for p in batch:                                       # (int8 pages are written by the batch passes only)
                        joined += [self._lone_prompt(scores, p)] if not self._i8 and seats.lone_step(p.request) else run([], whole([p]))
                else:
                    joined = run([], whole(batch)) if batch else []
                if active and spec is not None:
                    self._spec_decode(spec, seats, scores, P, active)
                elif active:
                    run(active, [])
            if spec is not None and carried:                            # decode rows rode a pass with prompt rows: plain rows, and they moved on without their seats
                spec.stale()
                self.spec_stats["steps"] += 1
            # 4. the prompts that finished decode from the next pass on
            active += joined
        if root is not None:
            root[0].page_manager.release()
        if scores is not None:
            scores.flush()   # (the loop's last read-back leaves nothing pending: every pass with prompt rows is followed by one)
        return out
