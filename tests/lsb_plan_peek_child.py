"""Child process of tests/test_lsb_plan_peek_gpu.py: runs the cases of the host's look at the keys-only plan's decision
(gs_lsb_plan.hip) in THIS process's mode -- GS_LSB_PLAN_PEEK, GS_LSB_KEYS_PLAN, GS_LSB_PLAN_SCATTER2 and
GS_LSB_PLAN_MIN_ITEMS are read once per process -- and writes one JSON record per sort:

    python tests/lsb_plan_peek_child.py OUT.json [CASE]

With CASE only that single case runs (no reuse, thread or capture sequences).  Each record holds: ok_numpy (the result
equals numpy's sort of the order-mapped keys, byte for byte), sha (of the result bytes), sel (the selector on return),
status (gs_lsb_plan_status' eight words), cursor (gs_lsb_plan_cursor_status' four words), peek (gs_lsb_plan_peek_status'
four words, read on the thread that sorted, right after the call), rule (the plan rule restated in numpy), guards (guard
bands around both key buffers and the workspace intact) and n.  The parent compares the records of the modes."""
import ctypes as C
import hashlib
import json
import sys
import threading

import numpy as np

from lsb_plan_child import CAP, F32, I32, U32, f32_specials, grouped, ordmap, plan_rule

TILE = 8192
MIX_PREFIXES = [0x0003, 0x7fff, 0x8000, 0xfffe] + [0x1000 + 257 * i for i in range(20)]
MIX_SIZES = [CAP[3], CAP[2], CAP[1], CAP[0]] + [2000] * 20       # one group that fills each class exactly, twenty of class 0


def heavy(keys, kt, top16, count):
    """keys with the first `count` of them moved into one group: for these key types a constant top half of the key is a
    constant top half of the mapped key"""
    k = keys.copy()
    k[:count] = (k[:count] & np.uint32(0xffff)) | (np.uint32(top16) << np.uint32(16))
    return k


def make_cases():
    """name -> (keys, key type, descending)"""
    rng = np.random.default_rng(20262)
    uni = lambda n: rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    c = {}
    c["ragged_planned"] = (uni(200003), U32, 0)
    c["class_mix"] = (grouped(rng, MIX_PREFIXES, MIX_SIZES), U32, 0)
    sizes = list(MIX_SIZES)
    sizes[0] = CAP[3] + 1
    c["class_mix_classic"] = (grouped(rng, MIX_PREFIXES, sizes), U32, 0)
    # the first look workgroup counts 131072 keys of one group: its 16-bit counter wraps, and the decision is CLASSIC on that
    c["wrapped_classic"] = (heavy(uni(200003), U32, 0x0042, 140000), U32, 0)
    c["tiles_24"] = (uni(24 * TILE), U32, 0)
    c["tiles_24_plus_1"] = (uni(24 * TILE + 1), U32, 0)
    n = (1 << 17) + 77
    c["f32_desc_planned"] = (f32_specials(rng, n), F32, 1)
    c["f32_desc_classic"] = (heavy(f32_specials(rng, n), F32, 0x3f80, 20000), F32, 1)
    c["i32_asc_planned"] = (uni(n), I32, 0)
    c["i32_asc_classic"] = (heavy(uni(n), I32, 0x8001, 20000), I32, 0)
    return c


def route_inputs(seed, n):
    """a PLANNED and a CLASSIC input of n keys"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    return p, heavy(rng.integers(0, 1 << 32, size=n, dtype=np.uint32), U32, 0x00a5, 30000)


def main(out_path, only=None):
    import torch
    import gpu_sort_amd as gs
    from guarded import Arena

    dev = torch.device("cuda:0")
    lib = gs.lib

    def run(arena, n, kt, desc, ws_bytes, stream=None):
        """one sort and the three diagnostics; the status calls synchronise the stream"""
        kp = (C.c_void_p * 2)(arena.ptr("k0"), arena.ptr("k1"))
        sel = C.c_int(0)
        rc = lib.gs_lsb_sort_u32(arena.ptr("ws"), ws_bytes, kp, None, C.byref(sel), n, 0, 32, desc, kt, stream)
        assert rc == 0, rc
        pk, st, cu = (C.c_uint32 * 4)(), (C.c_uint32 * 8)(), (C.c_uint32 * 4)()
        assert lib.gs_lsb_plan_peek_status(pk) == 0
        assert lib.gs_lsb_plan_status(arena.ptr("ws"), n, st, stream) == 0
        assert lib.gs_lsb_plan_cursor_status(arena.ptr("ws"), n, cu, stream) == 0
        return sel.value, list(st), list(cu), list(pk)

    def record(keys, kt, desc, got, sel, st, cu, pk, guards):
        exp = keys[np.argsort(ordmap(keys, kt, desc), kind="stable")]
        return {"ok_numpy": bool(np.array_equal(got, exp)), "sha": hashlib.sha256(got.tobytes()).hexdigest(), "sel": sel,
                "status": st, "cursor": cu, "peek": pk, "rule": plan_rule(keys, kt, desc), "guards": guards, "n": int(keys.size)}

    def guards_ok(arena):
        try:
            arena.check()
            return True
        except AssertionError as e:
            print("guard:", e)
            return False

    res = {}
    for name, (keys, kt, desc) in make_cases().items():
        if only and name != only:
            continue
        n = keys.size
        ws_bytes = lib.gs_lsb_temp_bytes(n, 0)
        arena = Arena(dev, seed=5)
        arena.add("k0", 4 * n, data=keys).add("k1", 4 * n, fill="random").add("ws", ws_bytes, fill="random").build()
        sel, st, cu, pk = run(arena, n, kt, desc, ws_bytes)
        torch.cuda.synchronize()
        res[name] = record(keys, kt, desc, arena.read("k%d" % sel, np.uint32), sel, st, cu, pk, guards_ok(arena))

    def sequence(seq, stream, seed, start=None):
        """the inputs of `seq`, one after the other, on one workspace and one stream, from the calling thread (which waits at
        `start` once its buffers exist)"""
        n = seq[0].size
        ws_bytes = lib.gs_lsb_temp_bytes(n, 0)
        arena = Arena(dev, seed=seed)
        arena.add("k0", 4 * n, fill="00").add("k1", 4 * n, fill="random").add("ws", ws_bytes, fill="ff").build()
        k0 = arena.slots["k0"][0]
        ts = torch.cuda.current_stream() if stream is None else stream
        got = []
        if start:
            start.wait()
        for keys in seq:
            with torch.cuda.stream(ts):
                arena.mem[k0:k0 + 4 * n] = torch.from_numpy(keys.view(np.uint8).copy()).to(dev)
            ts.synchronize()
            sel, st, cu, pk = run(arena, n, U32, 0, ws_bytes, None if stream is None else stream.cuda_stream)
            ts.synchronize()
            with torch.cuda.stream(ts):
                out = arena.read("k%d" % sel, np.uint32)
            got.append((keys, out, sel, st, cu, pk))
        return arena, got

    if not only:
        n = 17 * TILE + 4099
        p0, c0 = route_inputs(31, n)
        p1, c1 = route_inputs(32, n)

        # one workspace, one thread: PLANNED, CLASSIC, CLASSIC, PLANNED
        arena, got = sequence([p0, c0, c1, p1], None, 6)
        ok = guards_ok(arena)
        for i, (keys, out, sel, st, cu, pk) in enumerate(got):
            res["reuse_%d" % i] = record(keys, U32, 0, out, sel, st, cu, pk, ok)

        # two host threads, each with its own stream, workspace and route sequence, sorting at the same time
        seqs = {"a": [p0, c0, p1, c1], "b": [c1, p1, p0, c0]}
        streams = {t: torch.cuda.Stream() for t in seqs}
        done, errors = {}, []
        start = threading.Barrier(len(seqs))

        def worker(t):
            try:
                torch.cuda.set_device(dev)
                done[t] = sequence(seqs[t], streams[t], 7, start)
            except BaseException as e:   # noqa: B902  (reported by the parent thread)
                errors.append("%s: %r" % (t, e))
                start.abort()

        threads = [threading.Thread(target=worker, args=(t,)) for t in seqs]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        torch.cuda.synchronize()
        for t, (arena, got) in done.items():
            ok = guards_ok(arena)
            for i, (keys, out, sel, st, cu, pk) in enumerate(got):
                res["thread_%s_%d" % (t, i)] = record(keys, U32, 0, out, sel, st, cu, pk, ok)

        # stream capture: one captured sort replayed on a PLANNED and on a CLASSIC input, then an eager sort
        src = torch.empty(n, dtype=torch.int32, device=dev)
        a, b = torch.empty_like(src), torch.empty_like(src)
        dk = gs.DoubleBuffer(a, b)
        nb = gs.DeviceRadixSort.SortKeys(None, 0, dk, n)
        temp = torch.empty(nb, dtype=torch.uint8, device=dev)
        side = torch.cuda.Stream()
        src.copy_(torch.from_numpy(p0.view(np.int32).copy()).to(dev))
        with torch.cuda.stream(side):
            a.copy_(src)
            gs.DeviceRadixSort.SortKeys(temp, nb, dk, n, key_type=gs.GS_KEY_U32)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        dk.selector = 0
        with torch.cuda.graph(g, stream=side):
            a.copy_(src)
            gs.DeviceRadixSort.SortKeys(temp, nb, dk, n, key_type=gs.GS_KEY_U32)
            pk = (C.c_uint32 * 4)()
            assert lib.gs_lsb_plan_peek_status(pk) == 0
        sel = dk.selector
        out = dk.Current()
        for i, keys in enumerate([p0, c0]):
            src.copy_(torch.from_numpy(keys.view(np.int32).copy()).to(dev))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            st, cu = (C.c_uint32 * 8)(), (C.c_uint32 * 4)()
            assert lib.gs_lsb_plan_status(temp.data_ptr(), n, st, None) == 0
            assert lib.gs_lsb_plan_cursor_status(temp.data_ptr(), n, cu, None) == 0
            res["graph_%d" % i] = record(keys, U32, 0, out.cpu().numpy().view(np.uint32), sel, list(st), list(cu), list(pk), True)
        arena, got = sequence([c1], None, 8)
        keys, out, sel, st, cu, pk = got[0]
        res["eager_after_graph"] = record(keys, U32, 0, out, sel, st, cu, pk, guards_ok(arena))

    with open(out_path, "w") as f:
        json.dump(res, f)
    print("peek child ok", len(res))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else None)
