"""8- and 16-bit keys above 2^32 elements (gs_lsb_sort_narrow_large), checked on the device in chunks
(tests/test_narrow_large_gpu.py::test_above_2p32).

    python tools/narrow_large_check.py CASE...
    CASE: u8_heavy       u8 keys, 2^32 + 2^21 + 7 of them, more than 2^32 of which hold ONE value (every 4096th key is random): the
                         only shape at which a 32-bit count wraps.  The output's per-value counts equal the input's, and it ascends;
          u8_rowid       uniform u8 keys with their u64 row ids at the same size, bits [0, 8), ascending: the keys are in order,
                         row ids strictly ascend inside a key, every id is < n and keys_in[id] == key_out (together: THE stable sort);
          u8_rowid_desc  the same, descending;
          u16_keys       uniform u16 keys, 2^32 + 4099 of them: two passes through the workspace intermediate; counts and order.
Inputs are built and results checked chunk by chunk (whole-tensor torch operations at these sizes have returned wrong entries).
Every case also checks that the input keys are unchanged.  Prints "<case> -> OK" per case; exits 1 at the first failure.  The
row-id cases hold about 75 GiB."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sort_amd as gs  # noqa: E402
from gpu_sort_amd._lib import check  # noqa: E402

CHUNK = 1 << 28
N_ODD = (1 << 32) + (1 << 21) + 7
N_U16 = (1 << 32) + 4099
HEAVY = 0x5A


def _chunks(n):
    return [(lo, min(lo + CHUNK, n)) for lo in range(0, n, CHUNK)]


def _fill_random(t, card, seed):
    g = torch.Generator(device=t.device)
    g.manual_seed(seed)
    for lo, hi in _chunks(t.numel()):
        t[lo:hi] = torch.randint(0, card, (hi - lo,), device=t.device, generator=g, dtype=torch.int32).to(t.dtype)   # (wraps: every bit pattern)


def _counts(t, card, offset):
    c = torch.zeros(card, dtype=torch.int64, device=t.device)
    for lo, hi in _chunks(t.numel()):
        c += torch.bincount(t[lo:hi].to(torch.int64) + offset, minlength=card)
    return c


def _in_order(t, desc=False, u16=False):
    for lo, hi in _chunks(t.numel()):
        s = t[max(lo - 1, 0):hi]
        if u16:                               # u16 keys held in an int16 tensor: compare the bit patterns
            s = s.to(torch.int32) & 0xFFFF
        if not bool((s[1:] <= s[:-1]).all() if desc else (s[1:] >= s[:-1]).all()):
            return False
    return True


def _checksum(t):
    return sum(int(t[lo:hi].to(torch.int64).sum().item()) * (i + 1) for i, (lo, hi) in enumerate(_chunks(t.numel())))


def _sort(kin, vin, n, kt, bits, desc):
    vb = vin.element_size() if vin is not None else 0
    nb = gs.lib.gs_lsb_narrow_large_temp_bytes(n, kt, vb)
    ws = torch.empty(nb, dtype=torch.uint8, device=kin.device)
    kout = torch.empty_like(kin)
    vout = torch.empty_like(vin) if vb else None
    torch.cuda.synchronize()
    t0 = time.time()
    check(gs.lib.gs_lsb_sort_narrow_large(ws.data_ptr(), nb, kin.data_ptr(), kout.data_ptr(), vin.data_ptr() if vb else None,
                                          vout.data_ptr() if vb else None, n, kt, vb, 0, bits, int(desc), None), "gs_lsb_sort_narrow_large")
    torch.cuda.synchronize()
    return kout, vout, time.time() - t0


def run(case, dev):
    if case in ("u8_heavy", "u16_keys"):
        if case == "u8_heavy":
            n, kt, bits, card, off = N_ODD, gs.GS_KEY_U8, 8, 256, 0
            kin = torch.empty(n, dtype=torch.uint8, device=dev)
            g = torch.Generator(device=dev)
            g.manual_seed(5)
            for lo, hi in _chunks(n):             # (every chunk starts on a multiple of 4096)
                kin[lo:hi] = HEAVY
                m = (hi - lo + 4095) // 4096
                kin[lo:hi:4096] = torch.randint(0, 256, (m,), device=dev, generator=g, dtype=torch.int32).to(torch.uint8)
        else:
            n, kt, bits, card, off = N_U16, gs.GS_KEY_U16, 16, 65536, 32768      # (held in an int16 tensor)
            kin = torch.empty(n, dtype=torch.int16, device=dev)
            _fill_random(kin, 65536, 6)
        before, csum = _counts(kin, card, off), _checksum(kin)
        kout, _, dt = _sort(kin, None, n, kt, bits, False)
        after = _counts(kout, card, off)
        same, ordered, untouched = bool(torch.equal(before, after)), _in_order(kout, u16=bits == 16), _checksum(kin) == csum
        top = int(before.max().item())
        ok = same and ordered and untouched and (case != "u8_heavy" or top > 1 << 32)
        print("%s n=%d: %.3f s (host wall), largest count %d, counts %s, in order %s, input unchanged %s -> %s"
              % (case, n, dt, top, "equal" if same else "DIFFERENT", ordered, untouched, "OK" if ok else "FAIL"), flush=True)
        return ok

    if case in ("u8_rowid", "u8_rowid_desc"):
        n, desc = N_ODD, case.endswith("desc")
        kin = torch.empty(n, dtype=torch.uint8, device=dev)
        _fill_random(kin, 256, 7)
        vin = torch.empty(n, dtype=torch.int64, device=dev)
        for lo, hi in _chunks(n):
            torch.arange(lo, hi, dtype=torch.int64, out=vin[lo:hi])
        csum = _checksum(kin)
        kout, vout, dt = _sort(kin, vin, n, gs.GS_KEY_U8, 8, desc)
        del vin
        torch.cuda.empty_cache()
        ordered = _in_order(kout, desc)
        bad_range = bad_key = bad_tie = 0
        for lo, hi in _chunks(n):
            k, v = kout[lo:hi], vout[lo:hi]
            inside = (v >= 0) & (v < n)
            bad_range += int((~inside).sum().item())
            bad_key += int((kin[torch.where(inside, v, torch.zeros_like(v))] != k).sum().item())
            p = max(lo - 1, 0)
            ks, vs = kout[p:hi], vout[p:hi]
            bad_tie += int(((ks[1:] == ks[:-1]) & (vs[1:] <= vs[:-1])).sum().item())
        untouched = _checksum(kin) == csum
        ok = ordered and bad_range == 0 and bad_key == 0 and bad_tie == 0 and untouched
        print("%s n=%d: %.3f s (host wall), in order %s, ids out of range %d, ids naming another key %d, ties out of id order %d, "
              "input unchanged %s -> %s" % (case, n, dt, ordered, bad_range, bad_key, bad_tie, untouched, "OK" if ok else "FAIL"), flush=True)
        return ok
    raise SystemExit("unknown case %s" % case)


def main():
    dev = torch.device("cuda:0")
    for case in sys.argv[1:]:
        ok = run(case, dev)
        torch.cuda.empty_cache()
        if not ok:
            sys.exit(1)


if __name__ == "__main__":
    main()
