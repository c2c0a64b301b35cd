"""Host restatement of speculative decoding under a sampler (include/pie_hip.h: pie_spec_verify_sampled,
pie_decoder_spec_step_tail), written from the rule's text and not from the kernels: which stream position a row draws at, which drafts are
accepted, where the stream stands afterwards, and which ids a row's repetition penalty sees.  The draws themselves are the sampler's
(tests/sampler_reference.py, hip_ops.sample): this file only says WHICH draw a row takes."""


def stream_positions(c: int, rows: int) -> list[int]:
    """Row r draws as the one-row call number c + r of the seed: the position the plain loop's r-th draw from here would have."""
    return [int(c) + r for r in range(rows)]


def accept(row_tokens, draft, V: int) -> tuple[int, list[int]]:
    """(n_acc, out_tokens) for the rows' drawn tokens t_0 .. t_{rows - 1} and the rows - 1 drafted ids: n_acc is the largest j with
    draft[i] == t_i for all i < j; an id outside [0, V) is never accepted.  out_tokens = t_0 .. t_{n_acc}, then -1 up to rows."""
    t = [int(x) for x in row_tokens]
    if len(draft) != len(t) - 1:
        raise ValueError("rows - 1 drafted ids")
    n_acc = 0
    for i, d in enumerate(draft):
        if not 0 <= int(d) < V or int(d) != t[i]:
            break
        n_acc = i + 1
    return n_acc, t[:n_acc + 1] + [-1] * (len(t) - n_acc - 1)


def counter_after(c: int, n_acc: int) -> tuple[int, int]:
    """The stream afterwards: out_n = n_acc + 1 positions are consumed, the draws of the rows behind the accepted run are not."""
    return int(c) + n_acc + 1, 0


def row_window(ids_before, fed_token: int, draft, o: int, r: int, context: int) -> list[int]:
    """The ids row r's repetition penalty sees: positions max(0, o + r + 1 - context) .. o + r of the sequence ids_before[0 .. o) ++
    [the fed token] ++ draft -- what a plain step at position o + r would see had the drafts before it been fed one by one."""
    seq = [int(t) for t in ids_before[:o]] + [int(fed_token)] + [int(t) for t in draft[:r]]
    if len(seq) != o + r + 1:
        raise ValueError("ids_before holds the o ids below the offset")
    return seq[max(0, o + r + 1 - context):]


def recorded_ids(ids_before, fed_token: int, out_tokens, o: int) -> list[int]:
    """The ids by position after a pass, whole up to the token about to be fed: the fed token at o, token i at o + 1 + i."""
    return [int(t) for t in ids_before[:o]] + [int(fed_token)] + [int(t) for t in out_tokens if int(t) >= 0]
