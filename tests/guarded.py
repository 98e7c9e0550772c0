"""Guarded device buffers for tests of the C ABI's buffer contract (tests/test_buffer_contracts_gpu.py).

An Arena is ONE uint8 device tensor.  Every buffer gets a slot of its own: a guard zone of GUARD bytes, the buffer at a
chosen byte offset from the slot's 256-byte boundary, and at least GUARD bytes of guard behind it.  The guards hold a fixed
pattern; a buffer holds its data (an input) or a named fill ("00", "ff", "random").  After the calls under test, check()
compares on the device that every guard byte is unchanged and that every const input is byte-identical, and names the
buffer, the side and the first differing offset.  Pointers are raw addresses (arena base + slot offset) for gs.lib.*;
results are read back from the arena's bytes.  A stray store stays inside the arena, so a broken sort trips a guard
instead of faulting."""
import numpy as np
import torch

GUARD = 128 * 1024          # more than one 8192-element tile of 8-byte keys, plus padding
FILLS = ("00", "ff", "random")


def _align256(x):
    return (x + 255) & ~255


_PATTERN = {}


def _pattern(size, device):
    """The guard pattern: fixed pseudo-random bytes, so that no run of zeros, ones or a repeated word passes for it."""
    p = _PATTERN.get(device)
    if p is None or p.numel() < size:
        g = torch.Generator().manual_seed(0x6A4D)
        p = torch.randint(0, 256, (max(size, 1 << 24),), dtype=torch.uint8, generator=g).to(device)
        _PATTERN[device] = p
    return p[:size]


class Arena:
    def __init__(self, device, seed=0, all_const=False):
        self.device = device
        self.all_const = all_const   # every buffer must come out unchanged (a refused call)
        self.seed = seed
        self.slots = {}          # name -> (start, nbytes, slot_lo, slot_hi): the slot [slot_lo, slot_hi) tiles the arena
        self._specs = []         # (name, nbytes, offset, fill, data, const)
        self.mem = None

    def add(self, name, nbytes, offset=0, fill="ff", data=None, const=None):
        """Reserve a buffer of nbytes at `offset` bytes past a 256-byte boundary.  data (a numpy array of exactly nbytes
        bytes) is its content; otherwise it gets `fill`.  const: check() requires the bytes to be unchanged (None: only in
        an all_const arena)."""
        assert name not in [s[0] for s in self._specs] and 0 <= offset < 256 and self.mem is None
        if data is not None:
            data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            assert data.size == nbytes, (name, data.size, nbytes)
        else:
            assert fill in FILLS, fill
        self._specs.append((name, int(nbytes), int(offset), fill, data, const))
        return self

    def build(self):
        at = 0
        for name, nbytes, offset, _, _, _ in self._specs:
            start = at + GUARD + offset
            end = _align256(start + nbytes + GUARD)
            self.slots[name] = (start, nbytes, at, end)
            at = end
        self.size = at
        self.pattern = _pattern(self.size, self.device)
        self.mem = self.pattern.clone()
        assert self.mem.data_ptr() % 256 == 0
        self.guard_mask = torch.ones(self.size, dtype=torch.bool, device=self.device)
        self._const = {}
        self.init = {}           # name -> the bytes the buffer held before the calls (host copy)
        rng = np.random.default_rng(self.seed)
        for name, nbytes, offset, fill, data, const in self._specs:
            start = self.slots[name][0]
            self.guard_mask[start:start + nbytes] = False
            if data is None:
                if fill == "random":
                    data = rng.integers(0, 256, nbytes, dtype=np.uint8)
                else:
                    data = np.full(nbytes, 0 if fill == "00" else 0xFF, dtype=np.uint8)
            self.init[name] = data
            if nbytes == 0:
                continue
            self.mem[start:start + nbytes] = torch.from_numpy(data.copy()).to(self.device)
            if const or (const is None and self.all_const):
                self._const[name] = self.mem[start:start + nbytes].clone()
        torch.cuda.synchronize()
        return self

    def ptr(self, name):
        return self.mem.data_ptr() + self.slots[name][0]

    def nbytes(self, name):
        return self.slots[name][1]

    def read(self, name, dtype, count=None):
        start, nbytes = self.slots[name][:2]
        a = self.mem[start:start + nbytes].cpu().numpy().view(dtype)
        return a if count is None else a[:count]

    def _region(self, i):
        """(buffer name, side, distance from the buffer's edge) of arena byte i, which lies in a guard."""
        for name, (start, nbytes, lo, hi) in self.slots.items():
            if lo <= i < start:
                return name, "before", start - i
            if start + nbytes <= i < hi:
                return name, "after", i - (start + nbytes)
        raise AssertionError("arena byte %d is in no slot" % i)

    def check(self):
        """Raise AssertionError naming the first guard byte that changed, else every const input that changed."""
        torch.cuda.synchronize()
        bad = (self.mem != self.pattern) & self.guard_mask
        idx = torch.nonzero(bad)
        if idx.numel():
            i = int(idx[0])
            name, side, off = self._region(i)
            where = "%d byte(s) before its start" % off if side == "before" else "%d byte(s) past its end" % off
            raise AssertionError("guard hit %s buffer %r: %d guard byte(s) changed, the first %s" % (side, name, int(bad.sum()), where))
        for name, orig in self._const.items():
            start, nbytes = self.slots[name][:2]
            diff = torch.nonzero(self.mem[start:start + nbytes] != orig)
            if diff.numel():
                raise AssertionError("const input %r changed: %d byte(s), the first at byte %d" % (name, diff.numel(), int(diff[0])))
