"""One guarded allocation for the buffer-contract tests (tests/test_gpu_buffer_contract.py).

An Arena is a single uint8 tensor filled with one byte value.  Every buffer of a call - inputs,
outputs, workspace - is a region placed inside it at a chosen device address modulo 256, with at
least GUARD untouched bytes before and after it and TAIL bytes of slack behind the last one.  A
snapshot taken before the call and assert_only_changed() after it turn a store outside an output or
a declared workspace byte into a changed guard byte that is reported by name: never into a fault,
since nothing is ever placed at the end of an allocation.

Works on a CPU tensor as well (tests/test_arena.py), so the arithmetic needs no device.
"""
import numpy as np

GUARD = 4096          # untouched bytes before and after every region, at least
TAIL = 1 << 20        # slack kept free behind the last region
ALIGN = 256           # residues are taken modulo this


class Region(object):
    """nbytes bytes of an arena at byte `offset`."""

    def __init__(self, name, offset, nbytes):
        self.name, self.offset, self.nbytes = name, int(offset), int(nbytes)

    @property
    def end(self):
        return self.offset + self.nbytes

    def __repr__(self):
        return "Region(%r, offset %d, %d bytes)" % (self.name, self.offset, self.nbytes)


def arena_bytes(sizes):
    """Bytes an Arena needs to place regions of these sizes, whatever residues are asked for."""
    return sum(int(s) + GUARD + ALIGN for s in sizes) + GUARD + TAIL


class Arena(object):
    def __init__(self, torch, device, nbytes, fill):
        self.torch = torch
        self.fill = int(fill)
        self.buf = torch.full((int(nbytes),), self.fill, dtype=torch.uint8, device=device)
        self.base = self.buf.data_ptr()
        self.regions = []
        self._cursor = 0
        self._snap = None

    def place(self, nbytes, residue, elem=1, name=None):
        """A region of nbytes whose address is = residue (mod 256); residue is a multiple of elem."""
        nbytes, residue, elem = int(nbytes), int(residue), int(elem)
        if nbytes < 0 or not 0 <= residue < ALIGN or elem < 1 or residue % elem:
            raise ValueError("place(%d, residue %d, elem %d)" % (nbytes, residue, elem))
        at = self._cursor + GUARD
        at += (residue - (self.base + at)) % ALIGN
        if at + nbytes + GUARD + TAIL > self.buf.numel():
            raise ValueError("arena of %d bytes is too small for %r (%d bytes at %d)"
                             % (self.buf.numel(), name, nbytes, at))
        region = Region(name if name is not None else "region%d" % len(self.regions), at, nbytes)
        self.regions.append(region)
        self._cursor = region.end
        return region

    def ptr(self, region):
        return self.base + region.offset

    def bytes(self, region):
        return self.buf[region.offset:region.end]

    def view(self, region, shape, dtype):
        """A typed view of the region's first prod(shape) elements."""
        count = int(np.prod(shape, dtype=np.int64))
        size = self.torch.empty((), dtype=dtype).element_size()
        if count * size > region.nbytes:
            raise ValueError("%d elements of %d bytes do not fit %r" % (count, size, region))
        flat = self.buf[region.offset:region.offset + count * size]
        if dtype != self.torch.uint8:
            flat = flat.view(dtype)
        return flat.view(*shape)

    def write(self, region, array):
        """Copy a host array's bytes to the start of the region."""
        raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        if raw.size > region.nbytes:
            raise ValueError("%d bytes do not fit %r" % (raw.size, region))
        self.buf[region.offset:region.offset + raw.size] = self.torch.from_numpy(raw.copy()).to(self.buf.device)

    def snapshot(self):
        self._snap = self.buf.clone()

    def assert_only_changed(self, regions):
        """Every byte outside `regions` must equal the snapshot."""
        assert self._snap is not None, "snapshot() was not taken"
        diff = self.buf != self._snap
        for r in regions:
            diff[r.offset:r.end] = False
        if not bool(diff.any()):
            return
        changed = np.flatnonzero(diff.cpu().numpy())
        allowed = set(id(r) for r in regions)
        first = int(changed[0])
        # the zones of the arena in address order: before / inside / after each placed region; a gap
        # between two regions is split in the middle
        zones, prev_end = [], 0
        order = sorted(self.regions, key=lambda r: r.offset)
        for i, r in enumerate(order):
            nxt = order[i + 1].offset if i + 1 < len(order) else self.buf.numel()
            mid = r.end + (nxt - r.end) // 2 if i + 1 < len(order) else nxt
            zones.append((prev_end, r.offset, r, "before"))
            if id(r) not in allowed:
                zones.append((r.offset, r.end, r, "inside"))
            zones.append((r.end, mid, r, "after"))
            prev_end = mid
        for lo, hi, r, side in zones:
            if lo <= first < hi:
                count = int(np.count_nonzero((changed >= lo) & (changed < hi)))
                where = first - r.offset if side != "after" else first - r.end
                raise AssertionError(
                    "%d byte(s) changed %s %s (%d bytes at arena offset %d): first at offset %d "
                    "relative to its %s (arena offset %d); %d changed byte(s) outside the outputs in all"
                    % (count, side, r.name, r.nbytes, r.offset, where,
                       "end" if side == "after" else "start", first, changed.size))
        raise AssertionError("%d byte(s) changed outside every region, first at arena offset %d"
                             % (changed.size, first))
