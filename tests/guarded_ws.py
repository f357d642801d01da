"""A guarded, exact-size workspace allocator for the tests of the workspace contract (include/msae.h).

An instance stands in for ``ops._workspace(dev, nbytes)`` (``monkeypatch.setattr(ops, "_workspace", gws)``) and serves
direct C-ABI calls through ``block(nbytes)``.  Every request gets ONE device allocation

    [ front guard | nbytes, start 256-B aligned | rear guard ]

and the caller sees exactly ``nbytes`` of it, so the library receives ``ws_bytes == nbytes`` -- not the 1 MiB minimum and
the grow-only slack of the product's allocator.  Both guards are GUARD_BYTES (1 MiB) of the 32-bit word 5; ``check()``
synchronises and asserts that every guard word of every block handed out since the last check is unchanged.  A kernel that
walks up to 1 MiB past its last region (or in front of its first) therefore lands in this block's own guard, never in
somebody else's tensor.

The interior is filled according to ``fill``:

    "zero"      all zero: what a fresh block of the caching allocator usually holds.
    "word3"     every 32-bit word is 3: the integer 3, a float near zero (4.2e-45), a u64 key 0x0000000300000003, a non-zero
                byte flag.  Any dependence on zeroed scratch changes the result, while a count or an index misread from it
                stays tiny: no wild address, no long loop.
    "recycled"  the block of the previous request is handed out again as that call left it (same or smaller size: the rear
                guard moves up to the new end); a larger request gets a new block whose head is the old block's contents and
                whose rest is word 3.  The first block of an instance is born word 3.
"""
from __future__ import annotations

import sys

import torch

GUARD_BYTES = 1 << 20
GUARD_WORD = 5
FILL_WORD = 3
FILLS = ("zero", "recycled", "word3")


class Block:
    """One guarded allocation: `raw` (uint8, the whole block), the workspace = raw[GUARD_BYTES : GUARD_BYTES + nbytes]."""

    def __init__(self, dev, capacity: int):
        total = GUARD_BYTES + (capacity + 3) // 4 * 4 + GUARD_BYTES
        self.words = torch.full((total // 4 + 64,), GUARD_WORD, dtype=torch.int32, device=dev)
        skip = -self.words.data_ptr() % 256                   # (the caching allocator's blocks are 512-B aligned: 0 there)
        self.raw = self.words.view(torch.uint8)[skip:skip + total]
        assert self.raw.data_ptr() % 256 == 0 and skip % 4 == 0
        self.capacity = capacity
        self.nbytes = 0
        self.what = ""

    @property
    def ptr(self) -> int:
        return self.raw.data_ptr() + GUARD_BYTES

    @property
    def view(self) -> torch.Tensor:
        return self.raw[GUARD_BYTES:GUARD_BYTES + self.nbytes]

    def _pattern(self, lo: int, hi: int, word: int) -> None:
        """bytes [lo, hi) of raw <- the bytes a block filled with `word` from a 4-byte boundary holds there"""
        a, b = (lo + 3) // 4 * 4, hi // 4 * 4
        if a <= b:
            if b > a:
                self.raw[a:b].view(torch.int32).fill_(word)
            edges = list(range(lo, min(a, hi))) + list(range(max(b, lo), hi))
        else:
            edges = list(range(lo, hi))
        for o in edges:
            self.raw[o] = word if o % 4 == 0 else 0

    def set_size(self, nbytes: int) -> None:
        """the workspace is the first `nbytes` of the interior; everything behind it is guard"""
        assert 0 <= nbytes <= self.capacity
        self.nbytes = nbytes
        self._pattern(GUARD_BYTES + nbytes, self.raw.numel(), GUARD_WORD)

    def fill(self, word: int) -> None:
        self._pattern(GUARD_BYTES, GUARD_BYTES + self.nbytes, word)

    def first_damage(self):
        """None, or (byte offset of the first changed guard word relative to the END of the workspace, its value).  Offsets of
        the front guard are negative beyond -nbytes."""
        end = GUARD_BYTES + self.nbytes
        a = (end + 3) // 4 * 4
        front, rear = self.raw[:GUARD_BYTES].view(torch.int32), self.raw[a:].view(torch.int32)
        head = self.raw[end:a].tolist()
        want = [GUARD_WORD if o % 4 == 0 else 0 for o in range(end, a)]
        if head != want:
            return 0, head
        bad_r, bad_f = rear != GUARD_WORD, front != GUARD_WORD
        if bool(bad_r.any()):
            i = int(bad_r.nonzero()[0])
            return a - end + 4 * i, int(rear[i])
        if bool(bad_f.any()):
            i = int(bad_f.nonzero()[0])
            return 4 * i - end, int(front[i])
        return None


class GuardedWorkspace:
    """Callable like ops._workspace(dev, nbytes).  `what`: the entry and shape under test, for the failure message."""

    def __init__(self, fill: str = "zero", dev=None):
        assert fill in FILLS, fill
        self.fill, self.dev = fill, dev
        self.what = ""
        self.live: list = []          # blocks handed out since the last check()
        self.requests: list = []      # (caller, nbytes) of every request: what the test asserts the sizes from
        self._last = None             # "recycled": the block of the previous request

    def _new(self, dev, nbytes: int) -> Block:
        blk = Block(dev, nbytes)
        blk.set_size(nbytes)
        return blk

    def _get(self, dev, nbytes: int, fill: str, caller: str) -> Block:
        if fill == "recycled":
            old = self._last
            if old is not None and old.raw.device == torch.device(dev) and nbytes <= old.capacity:
                blk = old
                blk.set_size(nbytes)
            else:
                blk = self._new(dev, nbytes)
                blk.fill(FILL_WORD)
                if old is not None and old.raw.device == torch.device(dev):
                    n = min(old.nbytes, nbytes)
                    blk.raw[GUARD_BYTES:GUARD_BYTES + n].copy_(old.raw[GUARD_BYTES:GUARD_BYTES + n])
            self._last = blk
        else:
            blk = self._new(dev, nbytes)
            blk.fill(FILL_WORD if fill == "word3" else 0)
        blk.what = f"{self.what or caller} (requested by {caller})"
        if blk not in self.live:
            self.live.append(blk)
        self.requests.append((caller, nbytes))
        return blk

    def __call__(self, dev, nbytes: int) -> torch.Tensor:
        """ops._workspace's signature: the uint8 view of exactly nbytes (an empty view of a guarded block for 0)."""
        return self._get(dev, int(nbytes), self.fill, sys._getframe(1).f_code.co_name).view

    def block(self, nbytes: int, fill: str | None = None, dev=None):
        """For a direct C-ABI call: (device pointer, nbytes, handle); handle.view is the workspace, check() covers it."""
        blk = self._get(dev or self.dev, int(nbytes), fill or self.fill, sys._getframe(1).f_code.co_name)
        return blk.ptr, blk.nbytes, blk

    def check(self) -> None:
        """Synchronise; every guard word of every block handed out since the last check must be unchanged."""
        live, self.live = self.live, []
        if any(blk.raw.is_cuda for blk in live):
            torch.cuda.synchronize()
        for blk in live:
            hit = blk.first_damage()
            assert hit is None, (
                f"{blk.what}: workspace of {blk.nbytes} bytes (fill {self.fill!r}): guard word changed at byte offset "
                f"{hit[0]:+d} relative to the end of the workspace (value {hit[1]!r}, guard {GUARD_WORD})")
