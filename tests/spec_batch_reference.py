"""Plain restatements of batched speculation's host rules (engine/batch_engine.py, Model.spec_step_batch), written from the
rules' text: how a pass's rows are formed, the three clamps on a row's drafts, the acceptance per segment, how an accepted run is cut -- and
the host simulation of BatchedEngine's whole schedule from a model of next-token choices, built on speculative_reference's drafter.

simulate_batch models the engine at its defaults (mixed=True, no prefill_chunk) with a pool that never refuses an admission:
  * every iteration first records what the last pass chose for every active request, cut at a stop token and at max_new_tokens, and
    retires the requests that ended; then admits waiting requests while seats are free;
  * admitted prompts and active requests: ONE pass carries both, the decode rows plain (a "step"); admitted prompts alone: a prompt pass;
  * active requests alone: row s presents m_s drafts -- the draft made behind the last decode pass for exactly this request in exactly
    this seat at exactly this length, where it has at least min_draft ids, clamped -- in one speculative pass, or, where every m_s is 0,
    in one plain step.  Behind either the drafter runs over every seat.  A pass that carried prompt rows leaves no draft behind, and a
    request that changes seats (another one before it retired) loses the one it had."""
from tests import speculative_reference as ref

MAX_DRAFTS, MAX_ROWS = 7, 256


def form_rows(offsets, counts):
    """(seg_first [B + 1], row_seq [N], row_context_lens [N]) of a pass in which sequence s, with offsets[s] positions cached, presents
    1 + counts[s] rows: consecutive rows, the r-th of them at position offsets[s] + r, attending that position and everything before it."""
    seg_first, row_seq, row_ctx = [0], [], []
    for s, (o, m) in enumerate(zip(offsets, counts)):
        for r in range(1 + m):
            row_seq.append(s)
            row_ctx.append(o + r + 1)
        seg_first.append(len(row_seq))
    return seg_first, row_seq, row_ctx


def clamp_drafts(counts, room, min_draft):
    """m_s for every row: count_s where count_s >= min_draft, else 0; at most 7; at most room_s = the tokens the request may still generate;
    and while the pass would hold more than 256 rows, the largest draft (the lowest row among equals) loses one id."""
    m = []
    for c, r in zip(counts, room):
        c = c if c >= min_draft else 0
        m.append(max(0, min(c, MAX_DRAFTS, r)))
    while len(m) + sum(m) > MAX_ROWS and max(m) > 0:
        m[m.index(max(m))] -= 1
    return m


def accept_segments(greedy_rows, seg_first, drafts):
    """Per segment (n, tokens): speculative_reference.accept on the segment's own rows and its first rows - 1 drafts; an idle slot: (0, [])."""
    out = []
    for s in range(len(seg_first) - 1):
        rows = greedy_rows[seg_first[s]:seg_first[s + 1]]
        if not len(rows):
            out.append((0, []))
            continue
        n_acc, toks = ref.accept(rows, list(drafts[s])[:len(rows) - 1])
        out.append((n_acc + 1, toks[:n_acc + 1]))
    return out


def cut_run(generated, tokens, stop_tokens, max_new_tokens):
    """(generated + the run up to and including its first stop token or the max_new_tokens-th token, whether the request ends there)."""
    out = list(generated)
    for t in tokens:
        out.append(int(t))
        if int(t) in stop_tokens or len(out) >= max_new_tokens:
            return out, True
    return out, False


def simulate_batch(prompts, next_token, max_new_tokens, max_batch, stop_tokens=(), num_draft=7, ngram_max=3, ngram_min=1, min_draft=5):
    """(outputs, schedule) for a model whose greedy choice after the ids `seq` is next_token(seq).  One schedule entry per pass that
    carried decode rows: ("step", requests) -- plain rows, alone or beside prompt rows -- or ("pass", requests, m, n) with every row's
    drafts m_s and chosen tokens n_s."""
    stop = set(int(t) for t in stop_tokens)
    prompts = [[int(t) for t in p] for p in prompts]
    out = [None] * len(prompts)
    pending = list(range(len(prompts)))
    active = []            # [request, generated, the tokens the last pass chose and the loop has not recorded yet]
    drafted = {}           # seat -> (request, tokens generated, draft)
    schedule = []
    while pending or active:
        keep = []
        for req, gen, run in active:
            gen, ended = cut_run(gen, run, stop, max_new_tokens)
            if ended:
                out[req] = gen
            else:
                keep.append([req, gen, []])
        active = keep
        batch = []
        while pending and len(active) + len(batch) < max_batch:
            batch.append(pending.pop(0))
        if not active and not batch:
            break
        joined = [[r, [], [next_token(prompts[r])]] for r in batch]
        if active and batch:          # one pass for both kinds: the decode rows are plain, and no draft is left behind
            for a in active:
                a[2] = [next_token(prompts[a[0]] + a[1])]
            schedule.append(("step", [a[0] for a in active]))
            drafted = {}
        elif active:
            counts, seqs = [], [prompts[a[0]] + a[1] for a in active]
            for s, a in enumerate(active):
                d = drafted.get(s)
                counts.append(len(d[2]) if d is not None and d[:2] == (a[0], len(a[1])) else 0)
            m = clamp_drafts(counts, [max_new_tokens - len(a[1]) for a in active], min_draft)
            if any(m):
                n = []
                for s, a in enumerate(active):
                    draft, seq, greedy = drafted[s][2][:m[s]] if m[s] else [], list(seqs[s]), []
                    for i in range(m[s] + 1):       # row i's greedy token, while the fed drafts agree with greedy decoding
                        greedy.append(next_token(seq))
                        if i == m[s] or draft[i] != greedy[-1]:
                            break
                        seq.append(draft[i])
                    a[2] = greedy
                    n.append(len(greedy))
                schedule.append(("pass", [a[0] for a in active], m, n))
            else:
                for s, a in enumerate(active):
                    a[2] = [next_token(seqs[s])]
                schedule.append(("step", [a[0] for a in active]))
            # the drafter behind the pass, over every seat: the ids the request will hold once the loop has recorded the run
            drafted = {s: (a[0], len(a[1]) + len(a[2]), ref.ngram_draft(seqs[s] + a[2], ngram_max, ngram_min, num_draft)) for s, a in enumerate(active)}
        active += joined
    return out, schedule


def stats_of(schedule):
    """BatchedEngine.spec_stats for a schedule."""
    passes = [e for e in schedule if e[0] == "pass"]
    return {"passes": len(passes), "steps": len(schedule) - len(passes), "drafted": sum(sum(e[2]) for e in passes),
            "accepted": sum(sum(e[3]) - len(e[3]) for e in passes)}
