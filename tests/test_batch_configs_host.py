"""CPU only: the oracle alone on every case and seed of tests/test_gpu_batch_configs.py.  That module checks a greedy token only where the oracle's
top-1 / top-2 gap exceeds twice the logits bound ("margin permitting"), and a logits bound relative to max|logit| says little about a vector
that is nearly zero: here the seeds are held to references on which those checks bite."""
import numpy as np
import pytest

from tests import test_gpu_batch_configs as bc


@pytest.mark.parametrize("name", bc.ALL)
def test_batch_config_references_have_margins_and_are_not_degenerate(name):
    """At least three quarters of the (row, step) pairs test 1 compares with the oracle (per row count: rows 0 .. min(B, 4) - 1, four steps, the
    regime of B rows) have a gap above the token bound, so the token check runs on them; no logits vector compared with the oracle in tests 1, 4
    and 5 is degenerate (max |logit| > 0.5)."""
    pairs = []
    for B in bc.STEP_B:
        rows = bc.oracle_step_rows(name, 6 if B < 6 else 1)[:min(B, bc.ORC_ROWS)]
        pairs += [row[st + 1] for row in rows for st in range(bc.STEPS)]
    others = [v for pair in bc.oracle_prefill(name) for v in pair] if name in bc.PREFILL_CASES else []
    if name in bc.MIXED_CASES:
        firsts, rows = bc.oracle_mixed(name)
        others += firsts + rows
    for v in pairs + others:
        assert np.abs(v).max() > 0.5, f"{name}: a reference logits vector is degenerate (max |logit| {np.abs(v).max():.3f})"
    decided = sum(1 for v in pairs if np.diff(np.sort(v)[-2:])[0] > bc.token_bound(name, v))
    assert decided >= 0.75 * len(pairs), f"{name}: only {decided} of {len(pairs)} compared (row, step) pairs have a decided greedy token"
