"""The per-row tail state of the multi-sequence passes (step_batch / prefill_batch / step_mixed), as `Model` owns it: sampler records and
rings, top-n records, token masks and bias tables, frequency / presence counts, DRY records, token automata, and the prompt passes' log-probability records.  Every
kind is a set_* / write_* / clear_* family over device buffers kept per rows_cap by one `RowsCapCache`."""
from __future__ import annotations

import numpy as np
import torch

from ... import _ffi, hip_ops


class RowsCapCache:
    """Buffers owned per rows_cap: get(rows_cap) returns the cached object -- so one rows_cap keeps its device addresses across
    set / clear / set, which the captured batch graph's key relies on -- or make(rows_cap); the 4 most recently used are kept, most
    recent last (a serving loop revisits few batch sizes)."""
    KEEP = 4

    def __init__(self, make):
        self._make, self._own = make, {}

    def get(self, rows_cap: int):
        own = self._own.pop(rows_cap, None)
        if own is None:
            while len(self._own) >= self.KEEP:
                self._own.pop(next(iter(self._own)))
            own = self._make(rows_cap)
        self._own[rows_cap] = own  # most recently used last
        return own


def _records(own: dict, rows_cap: int, n: int) -> dict:
    """`own` with "ids" / "vals" as the [rows_cap, n + 1] views of its allocations sized for n = 20."""
    return {**own, "ids": own["ids"][:rows_cap * (n + 1)].view(rows_cap, n + 1), "vals": own["vals"][:rows_cap * (n + 1)].view(rows_cap, n + 1)}


class RowsTailState:
    """Mixin of `Model`: needs self._dec, self.device, self.args.vocab_size and self.tp."""

    def _init_rows_state(self) -> None:
        dev, V, m = self.device, self.args.vocab_size, hip_ops.TOP_LOGPROBS_MAX
        i32 = lambda shape, fill=0: torch.full(shape if isinstance(shape, tuple) else (shape,), fill, dtype=torch.int32, device=dev)
        f32 = lambda n, fill: torch.full((n,), fill, dtype=torch.float32, device=dev)
        self._batch_tails = RowsCapCache(lambda r: {
            "table": hip_ops.row_tail_table([hip_ops.row_tail_pack()] * r, dev), "recent": i32((r, hip_ops.RECENT_IDS)),
            "ws": torch.zeros(int(_ffi.load().pie_sample_workspace_bytes(r, V)) // 8, dtype=torch.int64, device=dev)})
        self._batch_tops = RowsCapCache(lambda r: {
            "ids": i32(r * (m + 1), -1), "vals": f32(r * (m + 1), float("-inf")), "count": i32(r, -1), "ws": hip_ops.top_logprobs_workspace(dev, r, V, m)})
        self._prompt_lps = RowsCapCache(lambda r: {"targets": i32(r), "count": i32(r, -1), "ids": i32(r * (m + 1), -1), "vals": f32(r * (m + 1), float("-inf"))})
        self._batch_edit_bufs = RowsCapCache(lambda r: {   # (the bias tables: one allocation sized for 1024 entries)
            "masks": i32((r, (V + 31) // 32)), "mask_on": i32(r), "bias_ids": i32(r * 1024), "bias_vals": f32(r * 1024, 0.0), "bias_n": i32(r)})
        self._batch_count_bufs = RowsCapCache(lambda r: {
            "records": hip_ops.count_penalty_records([hip_ops.count_penalty_pack()] * r, dev), "counts": i32((r, V))})
        self._batch_dry_bufs = RowsCapCache(lambda r: {
            "records": hip_ops.dry_penalty_records([hip_ops.dry_penalty_pack()] * r, dev), "breakers": i32((r, hip_ops.DRY_BREAKERS_MAX)),
            "recent": i32((r, hip_ops.RECENT_IDS))})
        self._batch_xtc_bufs = RowsCapCache(lambda r: {"records": torch.zeros((r, hip_ops.XTC_WORDS), dtype=torch.int32, device=dev)})
        self._batch_dfa_bufs = RowsCapCache(lambda r: {"records": i32((r, hip_ops.DFA_WORDS)), "states": i32(r), "tables": i32(1)})
        self._batch_tail = self._batch_edits = self._batch_counts = self._batch_dry = self._batch_xtc = self._batch_dfa = None   # the armed buffers
        self._prompt_lp_ws = None      # (block_rows, its logits block + the op's workspace)

    # ------------------------------------------------------------------ the multi-sequence passes' tail
    def set_batch_tail(self, rows_cap: int) -> dict:
        """From now on step_batch / prefill_batch / step_mixed end every output row in its own repetition penalty and sampler
        (pie_decoder_set_batch_tail): row s follows record s of a device table this model owns -- {"table": int64 [rows_cap, ROW_TAIL_WORDS],
        "recent": int32 [rows_cap, 1024] rings of fed ids, "ws": the sampler's workspace}, returned, and kept per rows_cap (the 4 most
        recent, like the step's buffers).  A new table holds greedy records without a penalty: the passes' results are the untailed ones
        until write_batch_tail changes a row.  The returned tokens are then the drawn ones, logits the processed ones."""
        rows_cap = int(rows_cap)
        if rows_cap < 1:
            raise ValueError("set_batch_tail: rows_cap >= 1")
        bt = self._batch_tails.get(rows_cap)
        _ffi.check(_ffi.load().pie_decoder_set_batch_tail(self._dec, _ffi.p(bt["table"]), rows_cap, _ffi.p(bt["recent"]), _ffi.p(bt["ws"])))
        self._batch_tail = bt
        return bt

    def write_batch_tail(self, rows: list[int], records: list, fed: list | None = None) -> None:
        """Rewrites the records of `rows` of the armed table (hip_ops.row_tail_pack), in stream order, one copy for all of them -- when a
        row's occupant changes; `calls` of a record = the tokens that request has drawn so far.  fed[i] (None: leave the ring): the ids the
        occupant of rows[i] has been fed so far, by position, of which the ring keeps the last 1024."""
        bt = self._batch_tail
        if bt is None:
            raise RuntimeError("write_batch_tail: no batch tail is set (set_batch_tail)")
        if not rows:
            return
        idx = torch.tensor(rows, dtype=torch.long, device=self.device)
        bt["table"].index_copy_(0, idx, hip_ops.row_tail_table(records, self.device))
        ring_rows, rings = [], []
        for r, ids in zip(rows, fed or []):
            if ids is None:
                continue
            ids = np.asarray(ids, dtype=np.int32).reshape(-1)
            q = np.arange(max(0, ids.size - hip_ops.RECENT_IDS), ids.size)
            ring = np.zeros(hip_ops.RECENT_IDS, np.int32)
            ring[q & (hip_ops.RECENT_IDS - 1)] = ids[q]
            ring_rows.append(r), rings.append(ring)
        if rings:
            bt["recent"].index_copy_(0, torch.tensor(ring_rows, dtype=torch.long, device=self.device), torch.from_numpy(np.stack(rings)).to(self.device))

    def clear_batch_tail(self) -> None:
        """Back to the greedy tail of the multi-sequence passes; the buffers stay cached for the next set_batch_tail."""
        _ffi.check(_ffi.load().pie_decoder_set_batch_tail(self._dec, None, 0, None, None))
        self._batch_tail = None

    # ------------------------------------------------------------------ the multi-sequence passes' top-n log-probabilities
    def set_batch_top_logprobs(self, rows_cap: int, n: int) -> dict:
        """From now on step_batch / prefill_batch / step_mixed also leave every output row's record of hip_ops.top_logprobs over its returned
        logprobs and token (pie_decoder_set_batch_top_logprobs), with or without a batch tail: {"ids": int32 [rows_cap, n + 1], "vals": fp32
        [rows_cap, n + 1], "count": int32 [rows_cap]}, returned, owned by the model and kept per rows_cap (the 4 most recent, like
        set_batch_tail's buffers: one allocation sized for n = 20, of which "ids" / "vals" are the [rows_cap, n + 1] views).  Row s reports
        count[s] pairs (more than n acts as n, 0: slot 0 only, negative: the row's record is left alone); a new count is all -1.  The
        caller writes count in stream order; a captured step keeps replaying."""
        rows_cap, n = int(rows_cap), int(n)
        if rows_cap < 1 or not 1 <= n <= hip_ops.TOP_LOGPROBS_MAX:
            raise ValueError(f"set_batch_top_logprobs: rows_cap >= 1 and 1 <= n <= {hip_ops.TOP_LOGPROBS_MAX}")
        bt = _records(self._batch_tops.get(rows_cap), rows_cap, n)
        _ffi.check(_ffi.load().pie_decoder_set_batch_top_logprobs(self._dec, n, rows_cap, _ffi.p(bt["ids"]), _ffi.p(bt["vals"]), _ffi.p(bt["count"]), _ffi.p(bt["ws"])))
        return bt

    def clear_batch_top_logprobs(self) -> None:
        """The multi-sequence passes launch what they launched before set_batch_top_logprobs; the buffers stay cached."""
        _ffi.check(_ffi.load().pie_decoder_set_batch_top_logprobs(self._dec, 0, 0, None, None, None, None))

    # ------------------------------------------------------------------ log-probabilities of prompt tokens
    def set_prompt_logprobs(self, rows_cap: int, n: int, block_rows: int = 256) -> dict:
        """From now on every prompt pass -- step / step_embeds / __call__ with more than one row, prefill_batch, step_mixed -- also leaves
        the record of hip_ops.prompt_logprobs for each of its prompt rows (pie_decoder_set_prompt_logprobs): record i belongs to row i of
        the call (step_mixed: the decode rows come first and are not scored).  Returns {"targets": int32 [rows_cap], "count": int32
        [rows_cap], "ids": int32 [rows_cap, n + 1], "vals": fp32 [rows_cap, n + 1]}, owned by the model and kept per rows_cap (the 4 most
        recent; one allocation sized for n = 20).  The caller writes, in stream order, targets[i] = the id that follows row i in its prompt
        and count[i] = how many pairs row i reports (0: the target's own only, -1: none -- a prompt's last row); a new count is all -1.  The rows
        are scored block_rows (8..1024) at a time through a T [block_rows, V] logits block; the log-probabilities are of the raw model
        distribution, whatever tail is configured."""
        rows_cap, n, block_rows = int(rows_cap), int(n), int(block_rows)
        if not 1 <= rows_cap <= 65535 or not 1 <= n <= hip_ops.TOP_LOGPROBS_MAX or not 8 <= block_rows <= 1024:
            raise ValueError(f"set_prompt_logprobs: 1 <= rows_cap <= 65535, 1 <= n <= {hip_ops.TOP_LOGPROBS_MAX} and 8 <= block_rows <= 1024")
        if self.tp is not None:
            raise ValueError("set_prompt_logprobs: not available on a tensor-parallel model")
        m = hip_ops.TOP_LOGPROBS_MAX
        pl = _records(self._prompt_lps.get(rows_cap), rows_cap, n)
        lib = _ffi.load()
        if self._prompt_lp_ws is None or self._prompt_lp_ws[0] != block_rows:  # the logits block + the op's workspace, sized for n = 20
            self._prompt_lp_ws = None
            nbytes = int(lib.pie_decoder_prompt_logprobs_workspace_bytes(self._dec, m, block_rows))
            self._prompt_lp_ws = (block_rows, torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=self.device))
        ws = self._prompt_lp_ws[1]
        _ffi.check(lib.pie_decoder_set_prompt_logprobs(self._dec, n, rows_cap, block_rows, _ffi.p(pl["targets"]), _ffi.p(pl["count"]), _ffi.p(pl["ids"]),
                                                       _ffi.p(pl["vals"]), _ffi.p(ws), ws.numel() * 8))
        return pl

    def clear_prompt_logprobs(self) -> None:
        """The prompt passes launch what they launched before set_prompt_logprobs; the buffers stay cached."""
        _ffi.check(_ffi.load().pie_decoder_set_prompt_logprobs(self._dec, 0, 0, 0, None, None, None, None, None, 0))

    # ------------------------------------------------------------------ the multi-sequence passes' per-row masks and biases
    def set_batch_edits(self, rows_cap: int, masks: bool = True, bias_cap: int = 0) -> dict:
        """From now on step_batch / prefill_batch / step_mixed apply every output row's own token mask and logit bias
        (pie_decoder_set_batch_logits_edits), with or without a batch tail: {"masks": int32 [rows_cap, ceil(V / 32)] packed words
        (hip_ops.pack_token_mask's layout), "mask_on": int32 [rows_cap], "bias_ids": int32 [rows_cap, bias_cap], "bias_vals": fp32 [rows_cap,
        bias_cap], "bias_n": int32 [rows_cap]}, returned (a part that is not asked for is None), owned by the model and kept per rows_cap
        at stable addresses (the 4 most recent, like set_batch_tail's buffers; the bias tables are views of one allocation sized for 1024
        entries).  Fresh buffers start with mask_on and bias_n all zero: the passes' results are the unedited ones until
        write_batch_edits (or the caller, in stream order) arms a row."""
        rows_cap, bias_cap = int(rows_cap), int(bias_cap)
        if rows_cap < 1 or not 0 <= bias_cap <= 1024 or not (masks or bias_cap):
            raise ValueError("set_batch_edits: rows_cap >= 1, 0 <= bias_cap <= 1024, and a mask part or a bias part")
        own = self._batch_edit_bufs.get(rows_cap)
        be = dict.fromkeys(own)   # a part that is not asked for is None
        if masks:
            be["masks"], be["mask_on"] = own["masks"], own["mask_on"]
        if bias_cap:
            be["bias_ids"], be["bias_vals"] = (own[k][:rows_cap * bias_cap].view(rows_cap, bias_cap) for k in ("bias_ids", "bias_vals"))
            be["bias_n"] = own["bias_n"]
        _ffi.check(_ffi.load().pie_decoder_set_batch_logits_edits(self._dec, rows_cap, _ffi.p(be["masks"]), be["masks"].shape[1] if masks else 0,
                                                                  _ffi.p(be["mask_on"]), _ffi.p(be["bias_ids"]), _ffi.p(be["bias_vals"]), _ffi.p(be["bias_n"]),
                                                                  bias_cap))
        self._batch_edits = be
        return be

    def write_batch_edits(self, rows: list[int], masks: list | None = None, biases: list | None = None) -> None:
        """Rewrites the masks and / or the bias tables of `rows` of the armed buffers, in stream order, one copy per array for all of them.
        masks[i]: the mask of rows[i] in any form packed_token_mask takes (packed int32 words, a bool [V] tensor, allowed ids), or None:
        the row is unmasked; an all-zero mask is refused here (ValueError), not decoded.  biases[i]: (ids, values) of 1..bias_cap entries, or
        None: no bias.  masks / biases None as a whole: that part of the rows is left as it is."""
        be = self._batch_edits
        if be is None:
            raise RuntimeError("write_batch_edits: no batch edits are set (set_batch_edits)")
        if not rows:
            return
        if (masks is not None and len(masks) != len(rows)) or (biases is not None and len(biases) != len(rows)):
            raise ValueError("write_batch_edits: one mask and one bias table per row")
        idx = torch.tensor(rows, dtype=torch.long, device=self.device)
        if masks is not None:
            if be["masks"] is None:
                raise RuntimeError("write_batch_edits: the batch edits were set without a mask part")
            from ...logits_processors import packed_token_mask
            V, W = self.args.vocab_size, be["masks"].shape[1]
            words = [None if m is None else packed_token_mask(m, V)[:W] for m in masks]     # every mask is checked before any row is written
            armed = [i for i, w in enumerate(words) if w is not None]
            if armed:
                be["masks"].index_copy_(0, idx[armed], torch.stack([words[i] for i in armed]).to(self.device))
            be["mask_on"].index_copy_(0, idx, torch.tensor([int(w is not None) for w in words], dtype=torch.int32, device=self.device))
        if biases is not None:
            if be["bias_ids"] is None:
                raise RuntimeError("write_batch_edits: the batch edits were set without a bias part")
            cap = be["bias_ids"].shape[1]
            ids, vals = np.zeros((len(rows), cap), np.int32), np.zeros((len(rows), cap), np.float32)
            n = np.zeros(len(rows), np.int32)
            for i, b in enumerate(biases):
                if b is None:
                    continue
                if not 1 <= len(b[0]) <= cap or len(b[1]) != len(b[0]):
                    raise ValueError(f"write_batch_edits: a bias table is (ids, values) with 1..{cap} entries each")
                n[i] = len(b[0])
                ids[i, :n[i]], vals[i, :n[i]] = np.asarray(b[0], dtype=np.int32), np.asarray(b[1], dtype=np.float32)
            for k, a in (("bias_ids", ids), ("bias_vals", vals), ("bias_n", n)):
                be[k].index_copy_(0, idx, torch.from_numpy(a).to(self.device))

    def clear_batch_edits(self) -> None:
        """The multi-sequence passes launch what they launched before set_batch_edits; the buffers stay cached."""
        _ffi.check(_ffi.load().pie_decoder_set_batch_logits_edits(self._dec, 0, None, 0, None, None, None, None, 0))
        self._batch_edits = None

    # ------------------------------------------------------------------ the multi-sequence passes' frequency / presence penalties
    def set_batch_count_penalty(self, rows_cap: int) -> dict:
        """From now on step_batch / prefill_batch / step_mixed apply every output row's own frequency and presence penalties
        (pie_decoder_set_batch_count_penalty), with or without a batch tail or batch edits: {"records": int32 [rows_cap,
        COUNT_PENALTY_WORDS], "counts": int32 [rows_cap, V]}, returned, owned by the model and kept per rows_cap at stable addresses (the
        4 most recent, like set_batch_tail's buffers).  Fresh buffers hold zero records and zero counts: the passes' results are the
        unpenalised ones until write_batch_count_penalty arms a row."""
        rows_cap = int(rows_cap)
        if rows_cap < 1:
            raise ValueError("set_batch_count_penalty: rows_cap >= 1")
        bc = self._batch_count_bufs.get(rows_cap)
        _ffi.check(_ffi.load().pie_decoder_set_batch_count_penalty(self._dec, _ffi.p(bc["records"]), _ffi.p(bc["counts"]), rows_cap))
        self._batch_counts = bc
        return bc

    def write_batch_count_penalty(self, rows: list[int], records: list, generated: list | None = None) -> None:
        """Rewrites the records and the counts of `rows` of the armed buffers, in stream order -- when a row's occupant changes.
        records[i]: (frequency_penalty, presence_penalty, start) of the occupant of rows[i] (start = its prompt's length), or None: a zero
        record (a row without penalties, a prompt that is still filling; so is a pair of zeros: such a row's counts stay zero).  generated[i]: the ids that request has generated so far, the
        first of which sits at position start: the row's counts become their multiplicities, all of them counted already."""
        bc = self._batch_counts
        if bc is None:
            raise RuntimeError("write_batch_count_penalty: no batch count penalty is set (set_batch_count_penalty)")
        if not rows:
            return
        if len(records) != len(rows) or (generated is not None and len(generated) != len(rows)):
            raise ValueError("write_batch_count_penalty: one record and one list of generated ids per row")
        V = bc["counts"].shape[1]
        packed, flat = [], []
        for i, (r, rec) in enumerate(zip(rows, records)):
            gen = [int(t) for t in (generated[i] if generated is not None and generated[i] is not None else ())]
            f, p = (0.0, 0.0) if rec is None else hip_ops.check_count_penalties(rec[0], rec[1], "write_batch_count_penalty")
            if f == 0.0 and p == 0.0:  # a zero record reads no counts and counts nothing: its row stays zero
                packed.append(hip_ops.count_penalty_pack())
                continue
            packed.append(hip_ops.count_penalty_pack(f, p, int(rec[2]), int(rec[2]) + len(gen) - 1))
            flat.extend(int(r) * V + t for t in gen if 0 <= t < V)
        idx = torch.tensor(rows, dtype=torch.long, device=self.device)
        bc["records"].index_copy_(0, idx, hip_ops.count_penalty_records(packed, self.device))
        bc["counts"].index_fill_(0, idx, 0)
        if flat:
            at = torch.tensor(flat, dtype=torch.long, device=self.device)
            bc["counts"].view(-1).index_add_(0, at, torch.ones(at.numel(), dtype=torch.int32, device=self.device))

    def clear_batch_count_penalty(self) -> None:
        """The multi-sequence passes launch what they launched before set_batch_count_penalty; the buffers stay cached."""
        _ffi.check(_ffi.load().pie_decoder_set_batch_count_penalty(self._dec, None, None, 0))
        self._batch_counts = None

    # ------------------------------------------------------------------ the multi-sequence passes' DRY penalty
    def set_batch_dry_penalty(self, rows_cap: int) -> dict:
        """From now on step_batch / prefill_batch / step_mixed apply every output row's own DRY penalty (pie_decoder_set_batch_dry_penalty),
        with or without a batch tail, batch edits or batch counts: {"records": int32 [rows_cap, DRY_PENALTY_WORDS], "breakers": int32
        [rows_cap, 64], "recent": int32 [rows_cap, 1024] rings of fed ids (its own, not the batch tail's)}, returned, owned by the model
        and kept per rows_cap at stable addresses (the 4 most recent, like set_batch_tail's buffers).  Fresh buffers hold zero records:
        the passes' results are the unpenalised ones until write_batch_dry_penalty arms a row."""
        rows_cap = int(rows_cap)
        if rows_cap < 1:
            raise ValueError("set_batch_dry_penalty: rows_cap >= 1")
        bd = self._batch_dry_bufs.get(rows_cap)
        _ffi.check(_ffi.load().pie_decoder_set_batch_dry_penalty(self._dec, _ffi.p(bd["records"]), _ffi.p(bd["breakers"]), _ffi.p(bd["recent"]), rows_cap))
        self._batch_dry = bd
        return bd

    def write_batch_dry_penalty(self, rows: list[int], records: list, fed: list | None = None) -> None:
        """Rewrites the records and breaker tables of `rows` of the armed buffers, in stream order, one copy per array for all of them --
        when a row's occupant changes.  records[i]: (multiplier, base, allowed_length, range, breaker_ids) of the occupant of rows[i]
        (hip_ops.check_dry's rules), or None: a zero record (a row without DRY, a prompt that is still filling).  fed[i] (None: leave the
        ring): the ids the occupant of rows[i] has been fed so far, by position, of which the ring keeps the last 1024."""
        bd = self._batch_dry
        if bd is None:
            raise RuntimeError("write_batch_dry_penalty: no batch DRY penalty is set (set_batch_dry_penalty)")
        if not rows:
            return
        if len(records) != len(rows) or (fed is not None and len(fed) != len(rows)):
            raise ValueError("write_batch_dry_penalty: one record and one list of fed ids per row")
        packed, tables = [], []
        for rec in records:
            m, b, a, r, brk = hip_ops.check_dry(0.0, who="write_batch_dry_penalty") if rec is None else hip_ops.check_dry(*rec, who="write_batch_dry_penalty")
            packed.append(hip_ops.dry_penalty_pack(m, b, a, r, len(brk)))
            tables.append(hip_ops.dry_breaker_table(brk))
        idx = torch.tensor(rows, dtype=torch.long, device=self.device)
        bd["records"].index_copy_(0, idx, hip_ops.dry_penalty_records(packed, self.device))
        bd["breakers"].index_copy_(0, idx, torch.stack(tables).to(self.device))
        ring_rows, rings = [], []
        for r, ids in zip(rows, fed or []):
            if ids is None:
                continue
            ids = np.asarray(ids, dtype=np.int32).reshape(-1)
            q = np.arange(max(0, ids.size - hip_ops.RECENT_IDS), ids.size)
            ring = np.zeros(hip_ops.RECENT_IDS, np.int32)
            ring[q & (hip_ops.RECENT_IDS - 1)] = ids[q]
            ring_rows.append(r), rings.append(ring)
        if rings:
            bd["recent"].index_copy_(0, torch.tensor(ring_rows, dtype=torch.long, device=self.device), torch.from_numpy(np.stack(rings)).to(self.device))

    def clear_batch_dry_penalty(self) -> None:
        """The multi-sequence passes launch what they launched before set_batch_dry_penalty; the buffers stay cached."""
        _ffi.check(_ffi.load().pie_decoder_set_batch_dry_penalty(self._dec, None, None, None, 0))
        self._batch_dry = None

    # ------------------------------------------------------------------ the multi-sequence passes' XTC
    def set_batch_xtc(self, rows_cap: int) -> dict:
        """From now on the batch tail's sampler draws every output row under the row's own XTC record (pie_decoder_set_batch_xtc):
        {"records": int32 [rows_cap, XTC_WORDS]}, returned, owned by the model and kept per rows_cap at a stable address (the 4 most
        recent, like set_batch_tail's buffers).  Fresh records are zero -- probability 0, off -- until write_batch_xtc arms a row.  Without
        a batch tail (set_batch_tail) the passes stay greedy and ignore the records."""
        rows_cap = int(rows_cap)
        if rows_cap < 1:
            raise ValueError("set_batch_xtc: rows_cap >= 1")
        bx = self._batch_xtc_bufs.get(rows_cap)
        _ffi.check(_ffi.load().pie_decoder_set_batch_xtc(self._dec, _ffi.p(bx["records"]), rows_cap))
        self._batch_xtc = bx
        return bx

    def write_batch_xtc(self, rows: list[int], records: list) -> None:
        """Rewrites the records of `rows` of the armed buffer, in stream order, one copy for all of them -- when a row's occupant changes.
        records[i]: (probability, threshold, special_ids) of the occupant of rows[i] (hip_ops.xtc_pack's rules), or None: a zero record."""
        bx = self._batch_xtc
        if bx is None:
            raise RuntimeError("write_batch_xtc: no batch XTC is set (set_batch_xtc)")
        if not rows:
            return
        if len(records) != len(rows):
            raise ValueError("write_batch_xtc: one record per row")
        packed = [_ffi.pie_xtc() if rec is None else hip_ops.xtc_pack(*rec) for rec in records]
        idx = torch.tensor(rows, dtype=torch.long, device=self.device)
        bx["records"].index_copy_(0, idx, hip_ops.xtc_records(packed, self.device))

    def clear_batch_xtc(self) -> None:
        """The multi-sequence passes launch what they launched before set_batch_xtc; the buffers stay cached."""
        _ffi.check(_ffi.load().pie_decoder_set_batch_xtc(self._dec, None, 0))
        self._batch_xtc = None

    # ------------------------------------------------------------------ the multi-sequence passes' token automata
    def set_batch_automata(self, rows_cap: int, tables_words: int) -> dict:
        """From now on step_batch / prefill_batch / step_mixed derive the token mask of every armed output row from its automaton's state
        and advance the state by the token the row drew (pie_decoder_set_batch_token_dfa): {"records": int32 [rows_cap, DFA_WORDS],
        "states": int32 [rows_cap], "tables": the arena, int32 [>= tables_words]}, returned, owned by the model and kept per rows_cap (the
        4 most recent; the arena grows to the largest size asked for and starts empty at every call).  The masks are the batch edits':
        without a mask part set (set_batch_edits) this call sets one, and clear_batch_automata then clears it again.  Fresh records are
        zero -- unarmed: such a row keeps the mask write_batch_edits gave it, or none -- until write_batch_automata arms a row."""
        rows_cap, tables_words = int(rows_cap), int(tables_words)
        if rows_cap < 1 or tables_words < 1:
            raise ValueError("set_batch_automata: rows_cap >= 1 and tables_words >= 1")
        own = self._batch_dfa_bufs.get(rows_cap)
        if own["tables"].numel() < tables_words:
            own["tables"] = torch.zeros(tables_words, dtype=torch.int32, device=self.device)
        own["records"].zero_()
        own["states"].zero_()
        own.update(used=0, uploaded={}, armed=set(), own_edits=False)
        be = self._batch_edits
        if be is None or be["masks"] is None:
            self.set_batch_edits(rows_cap if be is None else be["bias_n"].numel(), True, 0 if be is None else be["bias_ids"].shape[1])
            own["own_edits"] = be is None
            self._batch_edits["mask_on"].zero_()   # (cached buffers may hold an earlier call's rows)
        _ffi.check(_ffi.load().pie_decoder_set_batch_token_dfa(self._dec, rows_cap, _ffi.p(own["records"]), _ffi.p(own["states"]), _ffi.p(own["tables"]),
                                                               own["tables"].numel()))
        self._batch_dfa = own
        return own

    def upload_automaton(self, automaton) -> tuple[int, int]:
        """(cls_off, trans_off) of `automaton` (a logits_processors.TokenAutomaton) inside the armed arena, in words; every distinct
        object is uploaded once, in stream order.  ValueError for another vocabulary and for an arena that cannot hold it."""
        bd = self._batch_dfa
        if bd is None:
            raise RuntimeError("upload_automaton: no batch automata are set (set_batch_automata)")
        hit = bd["uploaded"].get(id(automaton))
        if hit is not None:
            return hit[1], hit[2]
        automaton.check_vocab(self.args.vocab_size)
        words = torch.from_numpy(automaton.words())
        at, n = bd["used"], words.numel()
        if at + n > bd["tables"].numel():
            raise ValueError(f"upload_automaton: the arena holds {bd['tables'].numel()} words, {at} of them used, and the automaton needs {n} (set_batch_automata's tables_words)")
        bd["tables"][at:at + n].copy_(words)
        bd["used"] = at + n
        bd["uploaded"][id(automaton)] = (automaton, at, at + automaton.vocab_size)  # (the object is kept: its id stays its own)
        return at, at + automaton.vocab_size

    def write_batch_automata(self, rows: list[int], automata: list, states: list | None = None) -> None:
        """Rewrites the records and the states of `rows` of the armed buffers, in stream order, one copy per array for all of them -- when
        a row's occupant changes.  automata[i]: the TokenAutomaton of the occupant of rows[i] (uploaded when the arena does not hold it
        yet), or None: a zero record -- a row without one, a prompt that is still filling.  states[i]: the state the row's next pass
        masks with (automaton.walk(the ids the request has generated so far)); None: the start state.  A row that held an automaton and
        loses it also gets mask_on = 0 -- the words its last pass wrote are stale: write_batch_edits for such a row comes after this call."""
        bd = self._batch_dfa
        if bd is None:
            raise RuntimeError("write_batch_automata: no batch automata are set (set_batch_automata)")
        if not rows:
            return
        if len(automata) != len(rows) or (states is not None and len(states) != len(rows)):
            raise ValueError("write_batch_automata: one automaton and one state per row")
        recs, sts = [], []
        for i, a in enumerate(automata):
            if a is None:
                recs.append(None), sts.append(0)
                continue
            cls_off, trans_off = self.upload_automaton(a)
            recs.append((cls_off, trans_off, a.n_states, a.n_classes))
            sts.append(a.start if states is None or states[i] is None else int(states[i]))
        idx = torch.tensor(rows, dtype=torch.long, device=self.device)
        bd["records"].index_copy_(0, idx, hip_ops.token_dfa_records(recs, self.device))
        bd["states"].index_copy_(0, idx, torch.tensor(sts, dtype=torch.int32, device=self.device))
        lost = [r for r, a in zip(rows, automata) if a is None and r in bd["armed"]]
        if lost and self._batch_edits is not None and self._batch_edits["mask_on"] is not None:
            self._batch_edits["mask_on"].index_fill_(0, torch.tensor(lost, dtype=torch.long, device=self.device), 0)
        bd["armed"].difference_update(lost)
        bd["armed"].update(r for r, a in zip(rows, automata) if a is not None)

    def clear_batch_automata(self) -> None:
        """The multi-sequence passes launch what they launched before set_batch_automata; the buffers stay cached, the arena empty."""
        bd = self._batch_dfa
        _ffi.check(_ffi.load().pie_decoder_set_batch_token_dfa(self._dec, 0, None, None, None, 0))
        self._batch_dfa = None
        if bd is not None:
            if bd["armed"] and self._batch_edits is not None and self._batch_edits["mask_on"] is not None:
                self._batch_edits["mask_on"].index_fill_(0, torch.tensor(sorted(bd["armed"]), dtype=torch.long, device=self.device), 0)
            bd.update(used=0, uploaded={}, armed=set())
            if bd["own_edits"]:
                self.clear_batch_edits()
