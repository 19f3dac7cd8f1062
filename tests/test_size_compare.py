"""The comparison of tests/test_gpu_size_contract.py bites: size_cases.find_bad_period on numpy arrays with
a toy mark of 2^16 in place of 2^32.  A kernel whose offset wraps at the mark reads, for byte k behind it,
byte k mod 2^16 of the same buffer; a kernel that skips a period leaves the pre-fill."""
import numpy as np

from tests import size_cases as S

MARK = 1 << 16
PERIOD, COUNT = 1155, 70            # 3 * 5 * 7 * 11 bytes: no power-of-two wrap maps a period onto itself
MARKS = (("2^15 B", MARK >> 1), ("2^16 B", MARK))


def _clean():
    one = np.random.default_rng(5).integers(0, 256, PERIOD).astype(np.uint8)
    return np.tile(one, COUNT)


def test_a_clean_buffer_passes():
    assert PERIOD & (PERIOD - 1) and PERIOD * COUNT > MARK + 2 * PERIOD
    for slice_bytes in (S.SLICE_BYTES, 4 * PERIOD, 1):
        assert S.find_bad_period(_clean(), PERIOD, COUNT, MARKS, slice_bytes) is None


def test_a_period_read_at_the_wrapped_offset_is_named():
    buf = _clean()
    k = MARK // PERIOD + 2                          # wholly behind the mark
    at = np.arange(k * PERIOD, (k + 1) * PERIOD)
    buf[at] = buf[at % MARK]
    for slice_bytes in (S.SLICE_BYTES, 4 * PERIOD, 1):
        msg = S.find_bad_period(buf, PERIOD, COUNT, MARKS, slice_bytes)
        assert msg is not None and msg.startswith("period %d " % k), msg
        assert "2^15 B: behind, 2^16 B: behind" in msg


def test_an_unwritten_period_is_named_and_placed():
    buf = _clean()
    k = MARK // PERIOD                              # the period that lies across the mark
    buf[k * PERIOD:(k + 1) * PERIOD] = 255 - buf[:PERIOD]
    msg = S.find_bad_period(buf, PERIOD, COUNT, MARKS)
    assert msg is not None and msg.startswith("period %d " % k) and "differs from period 0 in %d bytes" % PERIOD in msg
    assert "2^15 B: behind, 2^16 B: across" in msg
    buf = _clean()
    buf[3 * PERIOD + 7] ^= 1                        # one byte in front of both marks
    msg = S.find_bad_period(buf, PERIOD, COUNT, MARKS)
    assert msg.startswith("period 3 ") and "in 1 bytes" in msg and "2^15 B: in front, 2^16 B: in front" in msg


def test_the_aligned_wrap_is_left_to_the_tail():
    """A period of a power of two maps onto itself under the wrap: the comparison cannot see it, which is
    why size_cases.run refuses such periods and compares the tail B as well."""
    one = np.random.default_rng(6).integers(0, 256, 1024).astype(np.uint8)
    buf = np.tile(one, 80)
    at = np.arange(70 * 1024, 71 * 1024)
    buf[at] = buf[at % MARK]
    assert S.find_bad_period(buf, 1024, 80, MARKS) is None
