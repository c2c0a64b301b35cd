"""The long-context tests' data must make single rows matter (no GPU): at every op-level shape of tests/test_gpu_long_context.py the
float64 reference restated without the marker at row T - 1, or with the first poison row past T attended, misses the bound the kernel
must meet.
A case whose data cannot tell these apart would let an off-by-one in the kernel pass."""
import numpy as np
import pytest

from oracle import pie_oracle as po
from tests._util import LONG_OP_CASES, assert_bits_close, long_op_case, ordinary_row, sdpa_f64


@pytest.mark.parametrize("T,rep,D,dt", LONG_OP_CASES)
def test_op_level_data_tells_off_by_one_rows_apart(T, rep, D, dt):
    q, k, v = long_op_case(T, rep, D, dt)
    ulp = 2 if dt == "bfloat16" else 4                                        # test_sdpa_decode_random_sweep's bound
    want = po.to_bits(sdpa_f64(q, k, v, D ** -0.5, T), dt)
    k2, v2 = ordinary_row(k, v, T)
    for what, got in (("without the row T - 1 marker", sdpa_f64(q, k2, v2, D ** -0.5, T)),
                      ("with the first poison row", sdpa_f64(q, k, v, D ** -0.5, T + 1))):
        with pytest.raises(AssertionError):
            assert_bits_close(po.to_bits(got, dt), want, max_ulp=ulp, max_frac=0.05, what=what)


@pytest.mark.parametrize("T,rep,D,dt", [c for c in LONG_OP_CASES if c[0] <= 8193])
def test_float64_reference_is_the_oracle_where_fp32_summation_suffices(T, rep, D, dt):
    """sdpa_f64 restates the oracle's fused contract: at T <= 8193 (a serial fp32 sum that still keeps the ordinary rows' terms) the two
    agree under the kernel's bound, so the float64 reference changes the precision of the comparison, not what is computed."""
    q, k, v = long_op_case(T, rep, D, dt)
    assert_bits_close(po.to_bits(po.sdpa(q, k, v, D ** -0.5, None, dt, True, T=T), dt), po.to_bits(sdpa_f64(q, k, v, D ** -0.5, T), dt),
                      max_ulp=2 if dt == "bfloat16" else 4, max_frac=0.05, what="oracle vs float64")
