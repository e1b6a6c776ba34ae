"""Where a caller's arrays lie: a helper that puts an array at a chosen offset inside a larger allocation.

place(array, lead, guard, fill) -> a flat uint8 tensor VIEW of exactly array.nbytes bytes that holds the array's bytes.
Its first byte lies `lead` bytes past a 256-byte boundary, so the view's address modulo 256 is `lead` (lead < 256).
At least `guard` bytes lie before and behind the view inside the same allocation, all of them filled with `fill` (an
int 0..255, or a sequence of ints that is repeated from the start of the allocation: (1, 2) gives 01 02 01 02 ...).
The view carries its Placement as `view.placement`; `view.placement.address` is the address to hand to a C entry.

For an OUTPUT the same call gives a view of exactly the capacity the entry is told, between two canary bands:
pass the capacity as an array of that many bytes (place_out does it).  check_canaries(view, ...) asserts afterwards
that every byte of both bands still holds its fill.

Guards and canaries are ordinary memory of the allocation: a stray read returns the fill, a stray write lands in a
band -- nothing here can fault a device.  Works on CPU tensors as well (tests/test_dev_place_model.py).

LEADS: the offsets the device entries are tested at: a byte array anywhere (1 and 3), every other array
at the natural alignment of its element and no more -- u32 and records of u32 fields at 4, u64 at 8, u16 at 2.
"""
import numpy as np

ALIGN = 256
LEADS = {"u8": (1, 3), "u16": (2,), "u32": (4,), "u64": (8,), "rec32": (4,)}


class Placement:
    """the allocation behind a placed view: `store` (flat uint8, 256-byte aligned base), the view's offset and size in it,
    and the fill every other byte holds"""

    def __init__(self, store, offset, nbytes, pattern, lead, guard):
        self.store, self.offset, self.nbytes, self.pattern, self.lead, self.guard = store, offset, nbytes, pattern, lead, guard
        self.address = store.data_ptr() + offset  # (of the view's first byte: an empty view has no data_ptr of its own)

    def bands(self):
        """the bytes in front of and behind the view, as host numpy arrays, and what they have to hold"""
        img = self.store.cpu().numpy()
        want = fill_image(img.size, self.pattern)
        end = self.offset + self.nbytes
        return (img[:self.offset], want[:self.offset]), (img[end:], want[end:])


def fill_image(nbytes, pattern):
    reps = -(-nbytes // len(pattern))
    return np.tile(np.asarray(pattern, np.uint8), reps)[:nbytes]


def _pattern_of(fill):
    if isinstance(fill, (int, np.integer)):
        fill = (int(fill),)
    pattern = tuple(int(x) for x in fill)
    assert pattern and all(0 <= x <= 255 for x in pattern), "fill: bytes"
    return pattern


def place(array, lead, guard, fill, device="cpu"):
    import torch
    raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
    pattern = _pattern_of(fill)
    assert 0 <= lead < ALIGN and guard >= 0
    front = -(-guard // ALIGN) * ALIGN + lead      # a multiple of 256, plus the lead: >= guard bytes of fill in front
    total = front + raw.size + guard
    total = -(-total // ALIGN) * ALIGN
    # a base on a 256-byte boundary whatever the allocator hands out (torch's CPU allocator promises 64)
    slab = torch.empty(total + ALIGN, dtype=torch.uint8, device=device)
    skip = (-slab.data_ptr()) % ALIGN
    store = slab[skip:skip + total]
    assert store.data_ptr() % ALIGN == 0, "the base of the allocation is not 256-byte aligned"
    img = fill_image(total, pattern).copy()
    img[front:front + raw.size] = raw
    store.copy_(torch.from_numpy(img))
    view = store[front:front + raw.size]
    view.placement = Placement(store, front, raw.size, pattern, lead, guard)
    assert view.placement.address % ALIGN == lead and view.numel() == raw.size
    assert raw.size == 0 or view.data_ptr() == view.placement.address
    return view


def place_out(nbytes, lead, guard, fill, device="cpu", init=0xEE):
    """an output of exactly `nbytes` bytes between two canary bands; the view itself starts out as `init` bytes"""
    return place(np.full(int(nbytes), init, np.uint8), lead, guard, fill, device=device)


def read_back(view, dtype=np.uint8):
    """the bytes of a placed view as a host array of `dtype`"""
    return view.cpu().numpy().copy().view(dtype)


def check_canaries(*views):
    """both bands of every view untouched; the message names the first byte that is not"""
    for view in views:
        p = view.placement
        for side, (got, want) in zip(("in front of", "behind"), p.bands()):
            bad = np.flatnonzero(got != want)
            if bad.size:
                at = int(bad[0]) - (got.size if side == "in front of" else 0)
                raise AssertionError("canary %s the view written: byte %+d of %d holds 0x%02x, not 0x%02x (%d bytes changed)"
                                     % (side, at, p.nbytes, int(got[bad[0]]), int(want[bad[0]]), bad.size))
