"""The guarded arena of the buffer-contract tests on a CPU tensor: residues, gaps and what
assert_only_changed reports."""
import pytest

from tests import arena as A

torch = pytest.importorskip("torch")


def _arena(fill=0xA5, sizes=(26331, 105, 1, 4096, 8777)):
    return A.Arena(torch, "cpu", A.arena_bytes(sizes), fill), sizes


@pytest.mark.parametrize("fill", [0x00, 0xA5, 0xFF])
def test_place_gives_the_requested_residues_and_gaps(fill):
    ar, sizes = _arena(fill)
    asked = [(1, 1), (255, 1), (0, 1), (16, 16), (12, 4)]
    regions = [ar.place(s, res, elem, name="b%d" % i) for i, (s, (res, elem)) in enumerate(zip(sizes, asked))]
    assert bool((ar.buf == fill).all())
    prev_end = 0
    for r, s, (res, elem) in zip(regions, sizes, asked):
        assert r.nbytes == s and ar.ptr(r) % A.ALIGN == res and ar.ptr(r) == ar.base + r.offset
        assert r.offset - prev_end >= A.GUARD
        prev_end = r.end
    assert ar.buf.numel() - prev_end >= A.GUARD + A.TAIL
    # typed views start at the region's first byte
    v = ar.view(regions[4], (3, 5), torch.float32)
    assert v.data_ptr() == ar.ptr(regions[4]) and v.dtype == torch.float32 and tuple(v.shape) == (3, 5)
    assert ar.view(regions[0], (67, 131, 3), torch.uint8).data_ptr() == ar.ptr(regions[0])


def test_place_refuses_bad_residues_and_a_full_arena():
    ar, _ = _arena()
    for res, elem in ((256, 1), (-1, 1), (6, 4), (4, 8)):
        with pytest.raises(ValueError):
            ar.place(16, res, elem)
    small = A.Arena(torch, "cpu", A.TAIL + 2 * A.GUARD + 1000, 0)
    small.place(400, 3)
    with pytest.raises(ValueError, match="too small"):
        small.place(400, 5, name="second")


def _placed():
    ar, _ = _arena(sizes=(26331, 26331, 4096))
    src = ar.place(26331, 1, name="src")
    dst = ar.place(26331, 3, name="dst")
    ws = ar.place(4096, 16, 16, name="workspace")
    ar.write(src, torch.arange(26331, dtype=torch.int32).numpy().astype("uint8"))
    ar.snapshot()
    return ar, src, dst, ws


def test_a_write_inside_an_output_is_not_reported():
    ar, src, dst, ws = _placed()
    ar.bytes(dst)[:] = 7
    ar.bytes(ws)[-1] = 9
    ar.assert_only_changed([dst, ws])
    # the same bytes, with the workspace not listed
    with pytest.raises(AssertionError, match=r"1 byte\(s\) changed inside workspace .*offset 4095 relative to its start"):
        ar.assert_only_changed([dst])


@pytest.mark.parametrize("where,pattern", [
    ("before", r"1 byte\(s\) changed before dst .*first at offset -1 relative to its start"),
    ("after", r"1 byte\(s\) changed after dst .*first at offset 0 relative to its end"),
    ("far_after", r"2 byte\(s\) changed after dst .*first at offset 11 relative to its end"),
    ("input", r"1 byte\(s\) changed inside src .*first at offset 26330 relative to its start"),
    ("tail", r"1 byte\(s\) changed after workspace "),
    ("head", r"1 byte\(s\) changed before src .*first at offset -4096 relative"),
])
def test_one_byte_outside_is_reported_by_name(where, pattern):
    ar, src, dst, ws = _placed()
    ar.bytes(dst)[5] = 1                            # an output changes as well
    if where == "before":
        ar.buf[dst.offset - 1] ^= 0xFF
    elif where == "after":
        ar.buf[dst.end] ^= 0xFF
    elif where == "far_after":
        ar.buf[dst.end + 11] ^= 1
        ar.buf[dst.end + 12] ^= 1
    elif where == "input":
        ar.buf[src.end - 1] ^= 1
    elif where == "tail":
        ar.buf[ar.buf.numel() - 1] ^= 1
    else:
        ar.buf[src.offset - 4096] ^= 1
    with pytest.raises(AssertionError, match=pattern):
        ar.assert_only_changed([dst, ws])


def test_a_store_that_writes_the_old_value_is_no_change_and_a_snapshot_is_required():
    ar, src, dst, ws = _placed()
    ar.buf[dst.end] = 0xA5
    ar.assert_only_changed([dst])
    fresh, _ = _arena()
    with pytest.raises(AssertionError, match="snapshot"):
        fresh.assert_only_changed([])
