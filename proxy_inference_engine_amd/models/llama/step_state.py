"""The tail state of the single-sequence step (step / step_embeds), as `Model` owns it: the sampler and the repetition penalty, the token
mask and the bias table, the top-n record, frequency / presence counts, the DRY record, the XTC record and the token automaton.  Every part
lives in device buffers at stable addresses, made when first used: the library (csrc/decoder.hpp: StepTail) is asked only when a part is
switched on or off or one of its launch arguments changes, and new contents are a copy in stream order -- a replay, not a re-capture."""
from __future__ import annotations

import torch

from ... import _ffi, hip_ops

# The step-tail surface: what a wrapper around a text tower forwards to it (models/intern/ensemble.py) -- all of these, and nothing else.
STEP_TAIL_SURFACE = ("set_step_tail", "reset_step_counts", "step_tail", "step_tail_edits", "step_tail_counts", "step_tail_dry",
                     "step_top_logprobs", "step_xtc_record", "reset_step_automaton", "step_tail_automaton")


class StepTailState:
    """Mixin of `Model`: needs self._dec, self.device, self.logprobs and self.fed_ids."""

    def _init_step_state(self) -> None:
        self._tail = (None, None, None)  # (sampler spec, (penalty, context_size), seed)
        # the token mask and the logit bias: (mask on, bias entries) as the library knows them, and the objects last uploaded
        self._mask_words, self._bias_table, self._edits, self._edit_src = None, None, (False, 0), (None, None)
        self._top_n, self._top_rec = None, None   # the top-n log-probability record: n while on, (ids, vals, workspace)
        # what set_step_tail was given while the part is on, then the part's buffers: frequency / presence (freq, pres, start), the record and the
        # [V] counts; DRY's five values, the record and the 64-entry breaker table; XTC (probability, threshold, special ids) and the record
        self._cnt, self._cnt_rec, self._cnt_counts = None, None, None
        self._dry, self._dry_rec, self._dry_brk = None, None, None
        self._xtc, self._xtc_rec = None, None
        # the token automaton while the part is on, then its buffers: the arena (cls, then trans), the record, the state, the mask words it writes
        self._dfa, self._dfa_arena, self._dfa_rec, self._dfa_state, self._dfa_mask = None, None, None, None, None
        # the automaton's forced table (TokenAutomaton.forced()), next to the arena: int32 [capacity, 2], and the states it holds
        self._dfa_forced, self._dfa_forced_states = None, 0

    @property
    def _step_tail_plain(self) -> bool:
        """Nothing but XTC is set: the step ends in the greedy tail over raw logits (XTC alone configures nothing, as in the library)."""
        return self._tail[:2] == (None, None) and self._edits == (False, 0) and self._top_n is None and self._cnt is None and self._dry is None and self._dfa is None

    def set_step_tail(self, sampler: tuple | None = None, repetition_penalty: float = 1.0, context_size: int = 60,
                      token_mask=None, logit_bias=None, top_logprobs: int | None = None, frequency_penalty: float = 0.0,
                      presence_penalty: float = 0.0, count_start: int | None = None, dry: tuple | None = None,
                      xtc: tuple | None = None, rng: tuple | None = None, token_automaton=None) -> None:
        """What `step` / `step_embeds` end in (pie_decoder_set_logits_penalty / _set_sampler / _set_logits_mask / _set_logit_bias;
        DESIGN.md 10, 12), inside the replayed graph:
        sampler None = the greedy argmax, or (mode, temp, p, k) as hip_ops.sample takes them (make_sampler's `hip_spec`), drawn from
        samplers' random stream (samplers.seed) -- the returned token is then the drawn one; repetition_penalty != 1.0 with context_size
        1..1024: the penalty over the last context_size fed ids (`fed_ids`), applied to the returned logits before the log-softmax.
        token_mask: packed int32 words (hip_ops.pack_token_mask; host or device) -- a disallowed id is -inf in the returned logits,
        whatever else is configured; logit_bias: (ids, values), 1..1024 entries added after the penalty.  The model owns one mask buffer
        and one bias table at stable addresses and copies the contents in, in stream order: new words every token are a copy and a
        replay, not a re-capture (a new number of bias entries is one).  A mask tensor, or a pair of bias sequences, already uploaded is not copied
        again: pass new objects for new contents.
        top_logprobs: None (off) or 0..20 -- the step also leaves the (n + 1)-pair record of hip_ops.top_logprobs over the returned
        logprobs, slot 0 being the returned token, in `step_top_logprobs`; 0 means slot 0 only.  The model owns the record
        and the workspace at stable addresses.
        frequency_penalty / presence_penalty (each -2.0 .. 2.0): logits[v] -= frequency_penalty * c[v] + presence_penalty
        wherever c[v] > 0, c = how often id v was GENERATED so far (prompt tokens do not count, nor the token about to be chosen), after
        the mask's, the repetition penalty's and the bias' turn: mask (physically last), repetition penalty, logit_bias, frequency /
        presence.  The model owns one record and one [V] count buffer at stable addresses; the step counts every token it is fed from
        position count_start on, inside the replayed graph.  count_start given: the counts start afresh from that position
        (reset_step_counts); None: the counting state stays and only the two values are rewritten -- a copy and a replay.
        dry: None (off) or (multiplier, base, allowed_length, range, breaker_ids) -- the DRY penalty (hip_ops.check_dry's rules; DESIGN.md
        18) over the last `range` fed ids (`fed_ids`), behind the frequency / presence penalties.  The model owns one record and one
        64-entry breaker table at stable addresses: new values are a copy and a replay, not a re-capture.  A multiplier of 0 is off.
        xtc: None (off) or (probability, threshold, special_ids) -- XTC (hip_ops.xtc_pack's rules): the sampler's draw hides
        the top choices with the given probability; the returned logits, logprobs and top-n record stay those before XTC.  Ignored without
        a sampler (a greedy tail), and a probability of 0 is off.  The model owns one record at a stable address (`step_xtc_record`): new
        values are a copy and a replay, not a re-capture.
        token_automaton: None (off) or a logits_processors.TokenAutomaton -- the step derives its token mask from the
        automaton's state on the device and advances the state by the token it feeds back, inside the replayed graph: no mask is uploaded
        and no token is read back.  Exclusive with token_mask.  The model owns the arena, the record, the state and the mask words at
        stable addresses: a new automaton that fits the arena is a copy and a state reset -- a replay, not a re-capture; the same object
        again changes nothing, the state included (reset_step_automaton rewrites it).
        rng: None = samplers' random stream, or (seed, counter int64 [2] device) -- a stream of the caller's own: a draft model draws
        under samplers._rng.draft_state, never under the target's seed.
        The defaults restore the documented greedy contract.  A no-op when nothing changed (a new seed is a change).  `__call__` keeps
        returning raw logits."""
        if token_mask is not None and token_automaton is not None:
            raise ValueError("set_step_tail: token_mask and token_automaton are exclusive -- the automaton writes the step's mask")
        if token_automaton is None:  # off before a mask goes on, on after a mask went off: the library refuses the two together
            self._set_tail_automaton(None)
        self._set_tail_edits(token_mask, logit_bias)
        self._set_tail_automaton(token_automaton)
        self._set_tail_top_logprobs(top_logprobs)
        self._set_tail_counts(frequency_penalty, presence_penalty, count_start)
        self._set_tail_dry(dry)
        self._set_tail_xtc(xtc if sampler is not None else None)
        pen = (float(repetition_penalty), int(context_size)) if repetition_penalty != 1.0 and context_size != 0 else None
        seed = counter = None
        if sampler is not None:
            from ...samplers import _rng
            seed, counter = _rng.hip_state(self.device) if rng is None else (int(rng[0]), rng[1])
            sampler = (str(sampler[0]), float(sampler[1]), float(sampler[2]), int(sampler[3]))
        tail = (sampler, pen, seed)
        if tail == self._tail:
            return
        lib = _ffi.load()
        if pen != self._tail[1]:
            _ffi.check(lib.pie_decoder_set_logits_penalty(self._dec, pen[0] if pen else 1.0, pen[1] if pen else 0, _ffi.p(self.fed_ids), self.fed_ids.numel()))
            self._tail = (self._tail[0], pen, self._tail[2])
        if sampler is None:
            _ffi.check(lib.pie_decoder_set_sampler(self._dec, _ffi.PIE_SAMPLE_GREEDY, 1.0, 0.0, 0, 0, None, None, 0))
        else:
            self._tail_ws = ws = hip_ops.sample_workspace(self.device, 1, self.logprobs.numel())  # (kept alive while the decoder points at it)
            _ffi.check(lib.pie_decoder_set_sampler(self._dec, hip_ops.SAMPLE_MODES[sampler[0]], sampler[1], sampler[2], sampler[3], seed, _ffi.p(counter),
                                                   _ffi.p(ws), ws.numel() * 8))
        self._tail = tail

    def _set_tail_top_logprobs(self, n: int | None) -> None:
        """The step's top-n record: asked of the library only when n changes.  n == 0 runs the op with one candidate and reports slot 0."""
        if n is not None and not 0 <= int(n) <= hip_ops.TOP_LOGPROBS_MAX:
            raise ValueError(f"set_step_tail: top_logprobs is None or 0..{hip_ops.TOP_LOGPROBS_MAX}")
        n = None if n is None else int(n)
        if n == self._top_n:
            return
        lib = _ffi.load()
        if n is None:
            _ffi.check(lib.pie_decoder_set_top_logprobs(self._dec, 0, None, None, None, 0))
        else:
            if self._top_rec is None:  # sized for the largest n once: the addresses never change
                m = hip_ops.TOP_LOGPROBS_MAX
                self._top_rec = (torch.full((m + 1,), -1, dtype=torch.int32, device=self.device),
                                 torch.full((m + 1,), float("-inf"), dtype=torch.float32, device=self.device),
                                 hip_ops.top_logprobs_workspace(self.device, 1, self.logprobs.numel(), m))
            ids, vals, ws = self._top_rec
            _ffi.check(lib.pie_decoder_set_top_logprobs(self._dec, max(n, 1), _ffi.p(ids), _ffi.p(vals), _ffi.p(ws), ws.numel() * 8))
        self._top_n = n

    def _set_tail_edits(self, token_mask, logit_bias) -> None:
        """The mask words and the bias table into the model's own buffers; the library is asked only when an edit is switched on or
        off or the number of bias entries changes (the addresses never do)."""
        lib = _ffi.load()
        V = self.logprobs.numel()
        if token_mask is not None and token_mask is not self._edit_src[0]:
            words = token_mask.reshape(-1)
            if words.dtype != torch.int32 or words.numel() < (V + 31) // 32:
                raise ValueError(f"set_step_tail: token_mask is {(V + 31) // 32} packed int32 words (hip_ops.pack_token_mask)")
            if not words.is_cuda:  # seen on the host: a mask that allows no token below V is refused here, not decoded as token 0
                from ...logits_processors import packed_token_mask
                words = packed_token_mask(words, V)
            if self._mask_words is None:
                self._mask_words = torch.zeros((V + 31) // 32, dtype=torch.int32, device=self.device)
            self._mask_words.copy_(words[:self._mask_words.numel()])
        n = 0
        if logit_bias is not None:
            ids, values = logit_bias
            n = len(ids)
            if not 1 <= n <= 1024 or len(values) != n:
                raise ValueError("set_step_tail: logit_bias is (ids, values) with 1..1024 entries each")
            prev = self._edit_src[1]
            if prev is None or ids is not prev[0] or values is not prev[1]:  # (the same two objects: uploaded already)
                if self._bias_table is None:
                    self._bias_table = (torch.zeros(1024, dtype=torch.int32, device=self.device), torch.zeros(1024, dtype=torch.float32, device=self.device))
                self._bias_table[0][:n].copy_(torch.as_tensor(ids, dtype=torch.int32))
                self._bias_table[1][:n].copy_(torch.as_tensor(values, dtype=torch.float32))
        self._edit_src = (token_mask, logit_bias)
        if (token_mask is not None) != self._edits[0]:
            _ffi.check(lib.pie_decoder_set_logits_mask(self._dec, _ffi.p(self._mask_words) if token_mask is not None else None,
                                                       self._mask_words.numel() if token_mask is not None else 0))
            self._edits = (token_mask is not None, self._edits[1])
        if n != self._edits[1]:
            _ffi.check(lib.pie_decoder_set_logit_bias(self._dec, _ffi.p(self._bias_table[0]) if n else None, _ffi.p(self._bias_table[1]) if n else None, n))
            self._edits = (self._edits[0], n)

    # The counts, DRY and XTC parts share one shape -- a record at a stable address, made on first use; new values a copy; the library asked
    # only when the feature is switched on or off -- as three plain methods: what they validate, pack and own differs in every other line.
    def _set_tail_counts(self, frequency_penalty, presence_penalty, count_start) -> None:
        f, p = hip_ops.check_count_penalties(frequency_penalty, presence_penalty, "set_step_tail")
        if count_start is not None and int(count_start) < 0:
            raise ValueError("set_step_tail: count_start >= 0")
        lib = _ffi.load()
        if f == 0.0 and p == 0.0:
            if self._cnt is not None:
                _ffi.check(lib.pie_decoder_set_count_penalty(self._dec, None, None))
                self._cnt = None
            return
        if self._cnt_rec is None:
            self._cnt_rec = hip_ops.count_penalty_records([hip_ops.count_penalty_pack()], self.device)
            self._cnt_counts = torch.zeros(self.logprobs.numel(), dtype=torch.int32, device=self.device)
        was = self._cnt
        if was is None:
            _ffi.check(lib.pie_decoder_set_count_penalty(self._dec, _ffi.p(self._cnt_rec), _ffi.p(self._cnt_counts)))
        if count_start is not None or was is None:
            self._cnt = (f, p, int(count_start or 0))
            self.reset_step_counts(self._cnt[2])
        elif (f, p) != was[:2]:
            self._cnt = (f, p, was[2])
            self._cnt_rec[0, :2].copy_(hip_ops.count_penalty_records([hip_ops.count_penalty_pack(f, p)])[0, :2])  # (counted_pos lives on the device: left alone)

    def _set_tail_dry(self, dry) -> None:
        if dry is not None:
            if len(dry) != 5:
                raise ValueError("set_step_tail: dry is (multiplier, base, allowed_length, range, breaker_ids)")
            dry = hip_ops.check_dry(*dry, who="set_step_tail")
            if dry[0] == 0.0:
                dry = None
        if dry == self._dry:
            return
        if dry is not None:
            if self._dry_rec is None:
                self._dry_rec = hip_ops.dry_penalty_records([hip_ops.dry_penalty_pack()], self.device)
                self._dry_brk = torch.zeros(hip_ops.DRY_BREAKERS_MAX, dtype=torch.int32, device=self.device)
            self._dry_rec.copy_(hip_ops.dry_penalty_records([hip_ops.dry_penalty_pack(*dry[:4], len(dry[4]))]))
            self._dry_brk.copy_(hip_ops.dry_breaker_table(dry[4]))
        if (dry is None) != (self._dry is None):  # switched on or off
            on = (_ffi.p(self._dry_rec), _ffi.p(self._dry_brk), _ffi.p(self.fed_ids), self.fed_ids.numel()) if dry is not None else (None, None, None, 0)
            _ffi.check(_ffi.load().pie_decoder_set_dry_penalty(self._dec, *on))
        self._dry = dry

    def _set_tail_xtc(self, xtc) -> None:
        if xtc is not None:
            if len(xtc) != 3:
                raise ValueError("set_step_tail: xtc is (probability, threshold, special_ids)")
            xtc = (float(xtc[0]), float(xtc[1]), tuple(int(i) for i in xtc[2]))
            rec = hip_ops.xtc_pack(*xtc)  # (the ABI's range checks, before anything changes)
            if xtc[0] == 0.0:
                xtc = None
        if xtc == self._xtc:
            return
        if xtc is not None:
            if self._xtc_rec is None:
                self._xtc_rec = torch.zeros((1, hip_ops.XTC_WORDS), dtype=torch.int32, device=self.device)
            self._xtc_rec.copy_(hip_ops.xtc_records([rec]))
        if (xtc is None) != (self._xtc is None):  # switched on or off
            _ffi.check(_ffi.load().pie_decoder_set_xtc(self._dec, _ffi.p(self._xtc_rec) if xtc is not None else None))
        self._xtc = xtc

    def _set_tail_automaton(self, automaton) -> None:
        """The automaton's words into the model's arena; the library is asked only when the part is switched on or off or the arena has to
        grow (the record's, the state's and the mask words' addresses never change)."""
        if automaton is self._dfa:
            return
        lib = _ffi.load()
        if automaton is None:
            _ffi.check(lib.pie_decoder_set_token_dfa(self._dec, None, None, None, 0, None, 0))
            self._dfa = None
            return
        from ...logits_processors.token_automaton import TokenAutomaton
        if not isinstance(automaton, TokenAutomaton):
            raise ValueError("set_step_tail: token_automaton is a logits_processors.TokenAutomaton")
        V = self.logprobs.numel()
        automaton.check_vocab(V)
        words = torch.from_numpy(automaton.words())
        if self._dfa_rec is None:
            self._dfa_rec = torch.zeros((1, hip_ops.DFA_WORDS), dtype=torch.int32, device=self.device)
            self._dfa_state = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._dfa_mask = torch.zeros((V + 31) // 32, dtype=torch.int32, device=self.device)
        grown = self._dfa_arena is None or words.numel() > self._dfa_arena.numel()
        if grown:
            self._dfa_arena = torch.zeros(words.numel(), dtype=torch.int32, device=self.device)
        self._dfa_arena[:words.numel()].copy_(words)
        self._dfa_rec.copy_(hip_ops.token_dfa_records([(0, V, automaton.n_states, automaton.n_classes)]))
        forced = hip_ops.token_dfa_forced(automaton)  # the grammar-aware drafter's hint: a launch argument of no graph, grown like the arena
        if self._dfa_forced is None or forced.shape[0] > self._dfa_forced.shape[0]:
            self._dfa_forced = torch.full((forced.shape[0], 2), -1, dtype=torch.int32, device=self.device)
        self._dfa_forced[:forced.shape[0]].copy_(forced)
        self._dfa_forced_states = forced.shape[0]
        if grown or self._dfa is None:
            _ffi.check(lib.pie_decoder_set_token_dfa(self._dec, _ffi.p(self._dfa_rec), _ffi.p(self._dfa_state), _ffi.p(self._dfa_arena), self._dfa_arena.numel(),
                                                     _ffi.p(self._dfa_mask), self._dfa_mask.numel()))
        self._dfa = automaton
        self.reset_step_automaton()

    def reset_step_automaton(self, state: int | None = None) -> None:
        """The automaton's state is rewritten in stream order: `state`, or the start state -- at a request's start, and after a cache was
        trimmed (state = automaton.walk(the ids generated so far))."""
        if self._dfa is None:
            raise RuntimeError("reset_step_automaton: set_step_tail(token_automaton=...) first")
        self._dfa_state.fill_(self._dfa.start if state is None else int(state))

    @property
    def step_tail_automaton(self) -> tuple:
        """(the automaton or None, the state): the state is a device view (int32 [1]) of what the next step will mask with (None before the
        feature was first used)."""
        return self._dfa, self._dfa_state

    @property
    def _step_automaton_forced(self) -> torch.Tensor | None:
        """The set automaton's forced table on the device (int32 [S, 2]; hip_ops.token_dfa_draft's hint), None while no automaton is set."""
        return None if self._dfa is None else self._dfa_forced[:self._dfa_forced_states]

    def reset_step_counts(self, start: int, generated_ids=()) -> None:
        """The step's frequency / presence counting starts afresh, in stream order: the counts become the multiplicities of
        `generated_ids` (the tokens generated so far, the first of which sits at position `start`), all of them counted already; positions
        below `start` hold the prompt and never count.  At a request's start (start = the prompt's length, nothing generated), and after
        a cache was trimmed."""
        if self._cnt is None:
            raise RuntimeError("reset_step_counts: set_step_tail(frequency_penalty=..., presence_penalty=...) first")
        ids = torch.as_tensor(generated_ids, dtype=torch.int64).reshape(-1)
        V = self._cnt_counts.numel()
        self._cnt = (self._cnt[0], self._cnt[1], int(start))
        self._cnt_counts.zero_()
        kept = ids[(ids >= 0) & (ids < V)]
        if kept.numel():
            kept = kept.to(self.device)
            self._cnt_counts.index_add_(0, kept, torch.ones(kept.numel(), dtype=torch.int32, device=self.device))
        rec = hip_ops.count_penalty_pack(self._cnt[0], self._cnt[1], int(start), int(start) + ids.numel() - 1)
        self._cnt_rec.copy_(hip_ops.count_penalty_records([rec]))

    @property
    def step_tail(self) -> tuple:
        """(sampler or None, (penalty, context_size) or None)."""
        return self._tail[:2]

    @property
    def step_tail_edits(self) -> tuple:
        """(token mask or None, logit bias or None): the model's device buffers -- the packed int32 words, and (ids int32 [n], values
        float32 [n])."""
        on, n = self._edits
        return (self._mask_words if on else None, (self._bias_table[0][:n], self._bias_table[1][:n]) if n else None)

    @property
    def step_tail_counts(self) -> tuple:
        """((frequency_penalty, presence_penalty, start) or None, counts): counts is a device view of the int32 [V] counts of the tokens
        generated so far (None before the feature was first used)."""
        return self._cnt, self._cnt_counts

    @property
    def step_tail_dry(self) -> tuple | None:
        """(multiplier, base, allowed_length, range, breaker ids) of the DRY penalty, None while it is off."""
        return self._dry

    @property
    def step_top_logprobs(self):
        """(ids int32 [n + 1], vals fp32 [n + 1]) of the last step under set_step_tail(top_logprobs=n): slot 0 the returned token and its
        log-probability, then the n best by (value descending, id ascending).  Device views, valid until the next call."""
        if self._top_n is None:
            raise RuntimeError("step_top_logprobs: set_step_tail(top_logprobs=n) first")
        return self._top_rec[0][:self._top_n + 1], self._top_rec[1][:self._top_n + 1]

    @property
    def step_xtc_record(self) -> torch.Tensor | None:
        """The step's XTC record on the device (int32 [1, hip_ops.XTC_WORDS]) while set_step_tail(xtc=) is on, else None: rewriting its
        contents in stream order changes the next replay's draw without a new capture."""
        return self._xtc_rec if self._xtc is not None else None
