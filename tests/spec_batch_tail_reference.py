"""Plain restatements of the segmented sampled verify's rules (pie_spec_verify_rows_sampled), written from the rules' text:
which ids the repetition penalty of row (s, j) sees, the acceptance per segment over given row tokens, and what the one commit launch
leaves in a seat's ring and stream counter.  numpy and lists only; nothing here draws or penalises -- the GPU tests do that with the
existing one-row ops over what these functions return."""
import numpy as np

RING = 1024          # slots of a seat's ring: position q lives in slot q & 1023
SEG_ROWS = 8         # rows of one segment: the fed token and up to 7 drafts


def window(ring, fed_seg, pos0: int, j: int, context: int) -> list:
    """The ids at positions max(0, p + 1 - context) .. p, p = pos0 + j, of row j of a segment whose first row sits at position pos0:
    a position below pos0 comes from the seat's ring, position pos0 + i (0 <= i <= j) is the pass's own input fed_seg[i] -- never the
    ring, whose slot may still hold position pos0 + i - 1024.  context is clamped to 1..1024 as the kernels clamp it."""
    context = max(1, min(int(context), RING))
    p = pos0 + j
    out = []
    for q in range(max(0, p + 1 - context), p + 1):
        out.append(int(ring[q & (RING - 1)]) if q < pos0 else int(fed_seg[q - pos0]))
    return out


def accept_rows(row_tokens, seg_first, drafts, V: int) -> list:
    """Per segment (n, tokens [n]): n - 1 = the longest run drafts[s][i] == row_tokens[first + i], i < rows - 1; a draft outside [0, V)
    ends it.  An idle slot: (0, [])."""
    out = []
    for s in range(len(seg_first) - 1):
        r0, rows = int(seg_first[s]), min(int(seg_first[s + 1]) - int(seg_first[s]), SEG_ROWS)
        if rows <= 0:
            out.append((0, []))
            continue
        n_acc = 0
        while n_acc < rows - 1 and n_acc < len(drafts[s]):
            d = int(drafts[s][n_acc])
            if d < 0 or d >= V or d != int(row_tokens[r0 + n_acc]):
                break
            n_acc += 1
        out.append((n_acc + 1, [int(t) for t in row_tokens[r0:r0 + n_acc + 1]]))
    return out


def commit(rings, calls, draws, fed, seg_first, pos0, n):
    """(rings, calls) after the commit launch: seat s's calls moves by n[s] where the seat draws (draws[s]), and its ring takes the n[s]
    ids the pass fed for good -- ring[(pos0[s] + i) & 1023] = fed[first_s + i], i < n[s] -- and nothing else.  An idle slot: untouched."""
    rings = np.array(rings, dtype=np.int64, copy=True)
    calls = [int(c) for c in calls]
    for s in range(len(seg_first) - 1):
        if n[s] <= 0:
            continue
        if draws[s]:
            calls[s] += int(n[s])
        for i in range(int(n[s])):
            rings[s, (int(pos0[s]) + i) & (RING - 1)] = int(fed[int(seg_first[s]) + i])
    return rings, calls
