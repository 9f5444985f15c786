"""A workspace for tests of the workspace contract (include/disyolo.h, "Workspaces"): exact size, guard bands, poison.

``lib.Workspace.get`` hands every wrapper its whole buffer (1 MiB at the least) and the wrappers pass ``buf.numel()`` as
``workspace_bytes``, so with it neither an under-reporting size query nor a carve that runs past the reported size can
fail.  ``GuardedWorkspace.get(n)`` returns a view of exactly ``n`` bytes: the wrappers then make the exact-size call, what
an entry point writes past ``n`` (or in front of the view) lands in a guard band that ``check()`` reads back, and what it
reads without having written it is the poison byte instead of the zeros of a fresh allocation.
"""
import torch

from disyolo_amd import lib as L

GUARD_BYTE = 0xA5
ALIGN = 256


class GuardedWorkspace(L.Workspace):
    """``get(n)``: a uint8 view of exactly ``n`` bytes at a fixed 256-byte-aligned address inside one private allocation
    made at construction (a recorded command list can hold the address; a request above ``capacity`` raises).  ``guard``
    bytes of 0xA5 lie in front of the view and ``guard`` bytes behind the largest ``n`` requested so far (``high_water``);
    everything else is ``poison``.  The views share their start, so the rear guard sits behind the LARGEST request: a
    smaller request that over-runs into the room of a larger one is not seen."""

    def __init__(self, device, poison: int, guard: int = 65536, capacity: int = 8 << 20):
        if not 0 <= int(poison) <= 255 or int(poison) == GUARD_BYTE:
            raise ValueError("poison must be a byte other than 0x%02X" % GUARD_BYTE)
        if guard <= 0 or capacity <= 0:
            raise ValueError("guard and capacity must be positive")
        self.device = torch.device(device)
        self.poison, self.guard, self.capacity = int(poison), int(guard), int(capacity)
        self.frozen = False
        self.high_water = 0
        self._all = torch.empty(self.guard + self.capacity + self.guard + ALIGN, dtype=torch.uint8, device=self.device)
        self._start = self.guard + (-(self._all.data_ptr() + self.guard)) % ALIGN      # offset of the views in _all
        self._all.fill_(self.poison)
        self._all[self._start - self.guard:self._start].fill_(GUARD_BYTE)
        self._all[self._start:self._start + self.guard].fill_(GUARD_BYTE)
        self._sync()

    # what lib.Workspace exposes as its buffer: the largest view handed out so far
    @property
    def buf(self) -> torch.Tensor:
        return self._all[self._start:self._start + self.high_water]

    def _sync(self) -> None:
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def get(self, nbytes: int) -> torch.Tensor:
        n = int(nbytes)
        if n < 0 or n > self.capacity:
            raise L.DisyoloError("guarded workspace of %d bytes cannot hold %d (it never moves)" % (self.capacity, n))
        if n > self.high_water:
            # the rear guard moves behind the new largest request: look at it where it stood first (what over-ran it would be
            # lost), and let nothing be in flight while its bytes change
            self.check()
            s = self._start
            self._all[s + self.high_water:s + n].fill_(self.poison)
            self._all[s + n:s + n + self.guard].fill_(GUARD_BYTE)
            self.high_water = n
            self._sync()
        return self._all[self._start:self._start + n]

    def repoison(self) -> None:
        """fill everything but the two guards with the poison byte again"""
        self._sync()
        s, e = self._start, self._start + self.high_water
        self._all[s:e].fill_(self.poison)
        self._all[e + self.guard:].fill_(self.poison)
        self._sync()

    def _bad(self, lo: int, hi: int):
        """offsets, relative to the end of the largest view, of the first and last byte of _all[lo:hi] that is not 0xA5"""
        bad = (self._all[lo:hi] != GUARD_BYTE).nonzero()
        if bad.numel() == 0:
            return None
        end = self._start + self.high_water
        return lo + int(bad[0]) - end, lo + int(bad[-1]) - end, int(bad.numel())

    def check(self) -> None:
        """both guards still hold 0xA5 everywhere"""
        self._sync()
        s, e = self._start, self._start + self.high_water
        for name, lo, hi in (("behind", e, e + self.guard), ("in front of", s - self.guard, s)):
            bad = self._bad(lo, hi)
            assert bad is None, ("%d bytes of the guard %s a workspace of %d bytes were overwritten: offsets %+d .. %+d "
                                 "from the end of the view" % (bad[2], name, self.high_water, bad[0], bad[1]))

    def interior_untouched(self) -> bool:
        """whether every byte of the largest view still holds the poison (the call wrote nothing into its workspace)"""
        self._sync()
        return bool((self.buf == self.poison).all())
