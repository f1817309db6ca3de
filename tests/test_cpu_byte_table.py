"""CPU: the oracle's 1-byte ops equal the plain numpy table over all 65,536
(a, b) byte pairs (small_launch.byte_table), so the GPU byte-table test's
reference and the oracle every other test uses are tied together."""
import numpy as np
import pytest

import small_launch as SL


@pytest.mark.parametrize("op,dtype", [(op, dt) for dt, ops in SL.BYTE_OPS.items() for op in ops])
def test_oracle_equals_numpy_byte_table(oracle, op, dtype):
    a, b = SL.byte_pairs()
    want = SL.byte_table(op, dtype)
    for x, y in ((a, b), (b, a)):           # inout = in op inout: either role
        inout = y.copy()
        assert oracle.op(op, dtype, x.copy(), inout, a.size) == 0
        bad = np.flatnonzero(inout != want)
        assert bad.size == 0, [(int(a[i]), int(b[i]), int(inout[i]), int(want[i])) for i in bad[:4]]


def test_byte_table_spot_values():
    """The numpy table itself, at values worked by hand."""
    at = lambda op, dt, a, b: int(SL.byte_table(op, dt)[a * 256 + b])   # noqa: E731
    assert at(102, 2, 200, 100) == 44 and at(102, 1, 0x7f, 1) == 0x80       # SUM wraps
    assert at(103, 2, 16, 16) == 0 and at(103, 1, 0xff, 0xff) == 1          # PROD wraps; -1 * -1
    assert at(100, 1, 0x80, 0x7f) == 0x7f and at(100, 2, 0x80, 0x7f) == 0x80   # signed / unsigned MAX
    assert at(101, 1, 0x80, 0x7f) == 0x80 and at(101, 2, 0x80, 0x7f) == 0x7f
    assert at(104, 1, 0x80, 1) == 1 and at(104, 2, 0, 7) == 0
    assert at(106, 1, 0, 0) == 0 and at(108, 2, 3, 0x80) == 0 and at(108, 2, 0, 0x80) == 1
    assert at(105, 3, 0xf0, 0x3c) == 0x30 and at(107, 3, 0xf0, 0x3c) == 0xfc and at(109, 3, 0xf0, 0x3c) == 0xcc
