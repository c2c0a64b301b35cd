"""numpy restatements of greedy speculative decoding's two rules (include/pie_hip.h: pie_ngram_draft, pie_spec_verify), written
from the rules' text and not from the kernels: the drafter searches by START position and by n, as the rule is worded; the kernel searches by
end position.  Plus the host simulation of the engine's whole schedule from a model of next-token choices."""
import numpy as np


def ngram_draft(ids, ngram_max: int, ngram_min: int, k: int) -> list[int]:
    """The draft for the sequence `ids` (the last id is the token about to be fed): [] without a match."""
    ids = [int(t) for t in ids]
    L = len(ids)
    if L <= ngram_min:
        return []
    for n in range(ngram_max, ngram_min - 1, -1):
        if n > L:
            continue
        suffix = ids[L - n:]
        starts = [p for p in range(0, L - 1 - n + 1) if ids[p:p + n] == suffix]   # p + n <= L - 1
        if starts:
            p = max(starts)
            h = list(ids)
            for i in range(k):                      # the overlapped copy: h grows while it is read
                h.append(h[p + n + i])
            return h[L:]
    return []


def accept(greedy_tokens, draft) -> tuple[int, list[int]]:
    """(n_acc, out_tokens) for the rows' greedy tokens a_0 .. a_{rows - 1} and the rows - 1 drafted ids."""
    a = [int(t) for t in greedy_tokens]
    n_acc = 0
    while n_acc < len(draft) and int(draft[n_acc]) == a[n_acc]:
        n_acc += 1
    return n_acc, a[:n_acc + 1] + [-1] * (len(a) - n_acc - 1)


def log_softmax_f32(row) -> np.ndarray:
    x = np.asarray(row, np.float32)
    m = x.max()
    return x - (m + np.log(np.exp(x - m).sum(dtype=np.float32)))


def simulate(prompt, next_token, n_tokens: int, num_draft=7, ngram_max=3, ngram_min=1, min_draft=5, min_rows=6):
    """The engine's schedule for a model whose greedy choice after the ids `seq` is next_token(seq): (tokens, schedule) with one schedule
    entry per iteration -- ("step",) or ("pass", n_draft, n_acc) -- until at least n_tokens tokens were produced."""
    seq = [int(t) for t in prompt]
    tokens, schedule = [next_token(seq)], []
    floor = max(min_draft, min_rows - 1)
    while len(tokens) < n_tokens:
        draft = ngram_draft(seq + [tokens[-1]], ngram_max, ngram_min, num_draft)
        if len(draft) >= floor:
            greedy, s = [], seq + [tokens[-1]]
            for i in range(len(draft) + 1):         # row i's greedy token, while the fed drafts agree with greedy decoding
                greedy.append(next_token(s))
                if i < len(draft) and draft[i] != greedy[-1]:
                    break
                if i < len(draft):
                    s = s + [draft[i]]
            n_acc = len(greedy) - 1
            schedule.append(("pass", len(draft), n_acc))
            seq = seq + [tokens[-1]] + greedy[:-1]
            tokens.extend(greedy)
        else:
            schedule.append(("step",))
            seq = seq + [tokens[-1]]
            tokens.append(next_token(seq))
    return tokens, schedule
