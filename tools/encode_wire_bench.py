"""Field lines encoded in one launch (qhuff_encode_wire) against what a caller
launches without it, on 1M items in a field-line mix.

The mix, per group of four items over the synthetic batch's U[8,64] token
strings:

  a literal line with a static name reference   one item: a 4-bit-prefix
                                                index + a 7-bit-prefix value
  a literal line with a literal name            two items: a 3-bit-prefix
                                                name, a 7-bit-prefix value
  an indexed line                               one item: a 6-bit-prefix
                                                index (an empty string)

Timed, after checking that (a), (c) and (d) give the same bytes:

  (a) qhuff_encode_wire over the items                   kernel time
  (b) one qhuff_encode_batch per prefix width of the mix
      (LITERAL3 over the names, LITERAL7 over the
      values; the default, full kernel; b_lean: the
      lean one), the sum: the integers and instruction
      bits are then still to be spliced in on the host   kernel time
  (l7) one LITERAL7 launch over all the strings          kernel time
  (c) qhuff_encode_wire_host                             host clock
  (d) one qhuff_encode_batch_host per prefix width over
      strings gathered beforehand, then the integers
      coded and everything spliced with numpy            host clock

(a), (b) and (l7) by qhuff_timing_* over blocks of warmed launches
alternated in one process, (c) and (d) by a host clock around the
synchronous calls, also alternated.  One JSON line, printed and written to
profiles/encode_wire/encode_wire_bench.json."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ls-qpack_amd"))

import numpy as np
import torch
import qhuff


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def spread(starts, lens):
    """indices starts[i] .. starts[i] + lens[i], concatenated"""
    base = np.cumsum(lens) - lens
    return np.repeat(starts - base, lens) + np.arange(int(lens.sum()),
                                                      dtype=np.int64)


def int_code(ival, ib, ifirst):
    """lsqpack_enc_int over arrays -> (bytes [n, 6], lengths [n])"""
    v, mask = ival.astype(np.int64), (1 << ib.astype(np.int64)) - 1
    has, small = ib > 0, ival.astype(np.int64) < (1 << ib.astype(np.int64)) - 1
    B = np.zeros((len(v), 6), dtype=np.uint8)
    B[:, 0] = np.where(has, ifirst | np.where(small, v, mask), 0)
    L = has.astype(np.int64)
    r, cont = v - mask, has & ~small
    for j in range(1, 6):
        more = cont & (r >= 128)
        B[:, j] = np.where(cont, np.where(more, 0x80 | (r & 0x7F), r), 0)
        L += cont
        r = np.where(more, r >> 7, r)
        cont = more
    return B, L


def mix(n, seed=1):
    """-> (data, off [n + 1], items uint8 [8n], fields)"""
    assert n % 4 == 0
    g = n // 4
    sdata, soff = qhuff.synth_batch(3 * g)
    lens = np.zeros(n, dtype=np.int64)
    slen = np.diff(soff.astype(np.int64))
    lit = np.ones(n, dtype=bool)
    lit[3::4] = False                          # the indexed lines
    lens[lit] = slen
    off = np.zeros(n + 1, dtype=np.uint32)
    np.cumsum(lens, out=off[1:])
    rng = np.random.default_rng(seed)
    k = np.arange(n) % 4
    ib = np.choose(k, [4, 0, 0, 6]).astype(np.uint8)
    ifirst = np.choose(k, [0x50, 0, 0, 0xC0]).astype(np.uint8)
    sb = np.choose(k, [7, 3, 7, 0]).astype(np.uint8)
    sfirst = np.choose(k, [0, 0x20, 0, 0]).astype(np.uint8)
    # static-table indices; one indexed line in eight refers to a dynamic
    # entry with a larger index
    ival = np.where(ib > 0, rng.integers(0, 99, n), 0)
    ival = np.where((k == 3) & (rng.integers(0, 8, n) == 0),
                    rng.integers(0, 4000, n), ival).astype(np.uint32)
    items = np.zeros((n, 8), dtype=np.uint8)
    items[:, :4] = ival.view(np.uint8).reshape(-1, 4)
    items[:, 4], items[:, 5], items[:, 6], items[:, 7] = ib, ifirst, sb, sfirst
    return sdata, off, items.reshape(-1), (ival, ib, ifirst, sb, sfirst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "encode_wire", "encode_wire_bench.json"))
    args = ap.parse_args()
    n = args.n
    dev = torch.device("cuda", 0)
    data, off, items, (ival, ib, ifirst, sb, sfirst) = mix(n)
    assert qhuff.items_check(items) == (qhuff.OK, None)
    in_bytes = int(off[-1])
    codec = qhuff.Codec(0)
    L = qhuff.lib()
    st = torch.cuda.current_stream()
    bound = qhuff.encode_wire_bound(in_bytes, n)
    off64 = off.astype(np.int64)

    # the classes a caller encodes today: the strings of each prefix width,
    # gathered (not timed)
    classes = {}
    for pw in (3, 7):
        idx = np.flatnonzero(sb == pw)
        lens = off64[idx + 1] - off64[idx]
        coff = np.zeros(len(idx) + 1, dtype=np.uint32)
        np.cumsum(lens, out=coff[1:])
        cdata = np.concatenate([data[spread(off64[idx], lens)],
                                np.zeros(16, dtype=np.uint8)])
        cb = qhuff.encode_bound(int(coff[-1]), len(idx), pw)
        classes[pw] = dict(
            idx=idx, data=cdata, off=coff, n=len(idx),
            out=np.zeros(cb, dtype=np.uint8),
            oo=np.zeros(len(idx) + 1, dtype=np.uint32),
            d=torch.from_numpy(cdata).to(dev),
            o=torch.from_numpy(coff.view(np.int32)).to(dev),
            dout=torch.empty(cb, dtype=torch.uint8, device=dev),
            doo=torch.empty(len(idx) + 1, dtype=torch.int32, device=dev))

    # (d): the batches per width, then the splice
    out_d = np.zeros(bound, dtype=np.uint8)
    oo_d = np.zeros(n + 1, dtype=np.uint32)

    def call_d():
        for pw, c in classes.items():
            rc = L.qhuff_encode_batch_host(codec._ctx, p(c["data"]),
                                           p(c["off"]), c["n"], pw,
                                           p(c["out"]), p(c["oo"]))
            assert rc == qhuff.OK, rc
        B, IL = int_code(ival, ib, ifirst)
        size = IL.copy()
        for c in classes.values():
            size[c["idx"]] += np.diff(c["oo"].astype(np.int64))
        oo = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(size, out=oo[1:])
        for j in range(6):
            m = IL > j
            if m.any():
                out_d[oo[:-1][m] + j] = B[m, j]
        for c in classes.values():
            eoff = c["oo"].astype(np.int64)
            at = oo[c["idx"]] + IL[c["idx"]]
            out_d[spread(at, np.diff(eoff))] = c["out"][:eoff[-1]]
            out_d[at] |= sfirst[c["idx"]]
        oo_d[:] = oo
    call_d()
    total = int(oo_d[-1])

    # (c)
    src = np.concatenate([data, np.zeros(16, dtype=np.uint8)])
    out_c = np.zeros(bound, dtype=np.uint8)
    oo_c = np.zeros(n + 1, dtype=np.uint32)

    def call_c():
        rc = L.qhuff_encode_wire_host(codec._ctx, p(src), p(off), p(items), n,
                                      p(out_c), p(oo_c))
        assert rc == qhuff.OK, rc
    call_c()
    assert np.array_equal(oo_c, oo_d)
    assert np.array_equal(out_c[:total], out_d[:total])

    # (a)
    d = torch.from_numpy(src).to(dev)
    o = torch.from_numpy(off.view(np.int32)).to(dev)
    it = torch.from_numpy(items).to(dev)
    out_a = torch.empty(bound, dtype=torch.uint8, device=dev)
    oo_a = torch.empty(n + 1, dtype=torch.int32, device=dev)

    def call_a():
        codec.encode_wire_into(d, o, it, n, out_a, oo_a, st)
    call_a()
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    assert np.array_equal(oo_a.cpu().numpy().view(np.uint32), oo_d)
    assert np.array_equal(out_a[:total].cpu().numpy(), out_d[:total])

    # (b), (l7)
    out_7 = torch.empty(qhuff.encode_bound(in_bytes, n, 7), dtype=torch.uint8,
                        device=dev)
    oo_7 = torch.empty(n + 1, dtype=torch.int32, device=dev)

    def call_b(lean=False):
        for pw, c in classes.items():
            if lean:
                codec.batch_hint(qhuff.KIND_ENCODE, 0)
            codec.encode_into(c["d"], c["o"], c["n"], pw, c["dout"], c["doo"],
                              st)

    def call_l7():
        codec.encode_into(d, o, n, 7, out_7, oo_7, st)

    def block(fn, k, per):
        """k timed calls of fn, `per` launches each -> the calls' kernel
        times (us), summed over their launches"""
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        codec.timing(True)
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        t = codec.timing_read()
        codec.timing(False)
        assert len(t) == k * per
        assert all(kd == qhuff.KIND_ENCODE for kd, _ in t)
        us = [u for _, u in t]
        return [sum(us[i * per:(i + 1) * per]) for i in range(k)]

    per_b = len(classes)
    k_b = min(args.launches, qhuff.TIMING_SLOTS // per_b)
    ta, tb, tbl, t7 = [], [], [], []
    for r in range(args.rounds):
        for which in ((0, 1, 2, 3), (3, 2, 1, 0))[r % 2]:
            if which == 0:
                ta += block(call_a, args.launches, 1)
            elif which == 1:
                tb += block(call_b, k_b, per_b)
            elif which == 2:
                tbl += block(lambda: call_b(True), k_b, per_b)
            else:
                t7 += block(call_l7, args.launches, 1)
    assert codec.device_error() == 0

    tc, td = [], []
    for r in range(args.host_reps):
        for fn, acc in ((call_c, tc), (call_d, td))[::1 if r % 2 else -1]:
            t0 = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t0) * 1e6)
    med = lambda v: float(np.median(v))
    res = {
        "tool": "encode_wire_bench", "n": n, "in_bytes": in_bytes,
        "wire_bytes": total, "prefix_widths": sorted(classes),
        "launches_each": len(ta), "host_calls_each": len(tc),
        "a_encode_wire_us": round(med(ta), 2),
        "b_encode_batch_per_width_us": round(med(tb), 2),
        "b_lean_encode_batch_per_width_us": round(med(tbl), 2),
        "l7_one_literal7_launch_us": round(med(t7), 2),
        "a_over_b": round(med(ta) / med(tb), 3),
        "a_over_b_lean": round(med(ta) / med(tbl), 3),
        "a_over_l7": round(med(ta) / med(t7), 3),
        "a_min_us": round(min(ta), 2), "b_min_us": round(min(tb), 2),
        "l7_min_us": round(min(t7), 2),
        "c_encode_wire_host_us": round(med(tc), 1),
        "d_batch_host_per_width_and_splice_us": round(med(td), 1),
        "c_over_d": round(med(tc) / med(td), 3),
        "c_min_us": round(min(tc), 1), "d_min_us": round(min(td), 1),
    }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    codec.close()


if __name__ == "__main__":
    main()
