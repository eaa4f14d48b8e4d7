"""Field sections scanned on the device (qhuff_scan_sections) and the whole
decode path in one call (qhuff_decode_sections_host) against the path a
caller takes without them, on about 1M literals.

The data: the field-line mix of tools/encode_wire_bench.py framed by
qhuff_encode_wire_host, cut into field sections of 16 lines, a two-byte
section prefix each.  Timed, after checking at this size that (b), (c), (d)
and the device form give the same descriptors and (b) and (c) the same
decoded bytes:

  (a) the three launches of qhuff_scan_sections, summed
      (QHUFF_KIND_SCAN), and beside it qhuff_decode_wire
      on the descriptors the scan left                      kernel time
  (b) what a caller does without the scan: one
      qhuff_scan_field_section per section (through ctypes;
      the call overhead measured on zero-length chunks and
      reported raw and subtracted), then
      qhuff_decode_wire_host                                host clock
  (c) qhuff_decode_sections_host on the same bytes          host clock
  (d) qhuff_scan_sections_cpu, one call: the host walker's
      own rate                                              host clock

(a) by qhuff_timing_* over blocks of warmed calls alternated in one process,
(b), (c), (d) by a host clock around the synchronous calls, alternated; the
spread of (b) is its max - min over the repeats, and (c) counts as faster
only when the medians differ by more than that.  One JSON line, printed and
written to profiles/scan/scan_bench.json, and a README.txt beside it."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ls-qpack_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch
import qhuff
from encode_wire_bench import mix, p

LINES = 16


def sections(codec, n):
    """-> (wire uint8 (+16 slack), sec_off uint32 [m + 1], literals)"""
    data, off, items, (ival, ib, ifirst, sb, sfirst) = mix(n)
    src = np.concatenate([data, np.zeros(16, dtype=np.uint8)])
    out, oo = codec.encode_wire_host(src, off, items)
    # an item starts a line unless it is the value of a literal-name line
    starts = np.flatnonzero(np.arange(n) % 4 != 2)
    cuts = np.append(oo[starts[::LINES]].astype(np.int64), int(oo[-1]))
    m = len(cuts) - 1
    wire = np.insert(out, np.repeat(cuts[:-1], 2), 0)
    sec_off = (cuts + 2 * np.arange(m + 1)).astype(np.uint32)
    assert len(wire) == sec_off[-1]
    return (np.concatenate([wire, np.zeros(16, dtype=np.uint8)]), sec_off,
            int((sb > 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1398016,
                    help="items of the mix (3 literals per 4 items)")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan",
                                                  "scan_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    codec = qhuff.Codec(0)
    L = qhuff.lib()
    wire, sec_off, n_lits = sections(codec, args.n)
    m = len(sec_off) - 1
    wire_bytes = int(sec_off[-1])
    max_len = qhuff.MAX_STRLEN
    bound = qhuff.decode_bound(wire_bytes, 0)

    # (b): a second handle on the library, its scanner taking addresses
    L2 = C.CDLL(qhuff.LIB_PATH)
    scan1 = L2.qhuff_scan_field_section
    scan1.restype = C.c_int
    scan1.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p,
                      C.c_uint32, C.c_void_p]
    lits_b = np.zeros(16 * n_lits, dtype=np.uint8)
    cnt = C.c_uint32()
    cnt_ref = C.byref(cnt)
    base, lbase = wire.ctypes.data, lits_b.ctypes.data
    so = [int(x) for x in sec_off]
    out_b = np.zeros(bound, dtype=np.uint8)
    oo_b = np.zeros(n_lits + 1, dtype=np.uint32)
    st_b = np.ones(n_lits, dtype=np.uint8)
    lo_b = np.zeros(m + 1, dtype=np.uint32)
    t_b = {}

    def call_b(zero=False):
        t0 = time.perf_counter()
        k = 0
        for i in range(m):
            rc = scan1(base + so[i], 0 if zero else so[i + 1] - so[i], so[i],
                       lbase + 16 * k, n_lits - k, cnt_ref)
            if not zero:
                assert rc == qhuff.OK
                k += cnt.value
                lo_b[i + 1] = k
        t1 = time.perf_counter()
        if zero:
            return (t1 - t0) * 1e6
        assert k == n_lits
        rc = L.qhuff_decode_wire_host(codec._ctx, p(wire), p(lits_b), k,
                                      max_len, p(out_b), p(oo_b), p(st_b))
        assert rc == qhuff.OK, rc
        t2 = time.perf_counter()
        t_b["scan"], t_b["decode"] = (t1 - t0) * 1e6, (t2 - t1) * 1e6
        return (t2 - t0) * 1e6
    call_b()
    assert not st_b.any()

    # (c)
    lits_c = np.zeros(16 * n_lits, dtype=np.uint8)
    lo_c = np.zeros(m + 1, dtype=np.uint32)
    rc_c = np.ones(m, dtype=np.int32)
    used_c = np.zeros(m, dtype=np.uint32)
    out_c = np.zeros(bound, dtype=np.uint8)
    oo_c = np.zeros(n_lits + 1, dtype=np.uint32)
    st_c = np.ones(n_lits, dtype=np.uint8)

    def call_c():
        t0 = time.perf_counter()
        rc = L.qhuff_decode_sections_host(
            codec._ctx, p(wire), p(sec_off), m, qhuff.SCAN_FIELD_SECTION,
            max_len, p(lits_c), n_lits, p(lo_c), p(rc_c), p(used_c), p(out_c),
            p(oo_c), p(st_c))
        assert rc == qhuff.OK, rc
        return (time.perf_counter() - t0) * 1e6
    call_c()
    total = int(oo_b[-1])
    assert not rc_c.any() and np.array_equal(used_c, np.diff(sec_off))
    assert np.array_equal(lo_c, lo_b) and np.array_equal(lits_c, lits_b)
    assert np.array_equal(oo_c, oo_b) and np.array_equal(st_c, st_b)
    assert np.array_equal(out_c[:total], out_b[:total])

    # (d)
    lits_d = np.zeros(16 * n_lits, dtype=np.uint8)
    lo_d = np.zeros(m + 1, dtype=np.uint32)
    rc_d = np.ones(m, dtype=np.int32)

    def call_d():
        t0 = time.perf_counter()
        rc = L.qhuff_scan_sections_cpu(p(wire), p(sec_off), m,
                                       qhuff.SCAN_FIELD_SECTION, p(lits_d),
                                       n_lits, p(lo_d), p(rc_d), None)
        assert rc == qhuff.OK, rc
        return (time.perf_counter() - t0) * 1e6
    call_d()
    assert np.array_equal(lo_d, lo_b) and np.array_equal(lits_d, lits_b)

    # (a)
    st = torch.cuda.current_stream()
    wire_dev = torch.from_numpy(wire).to(dev)
    so_dev = torch.from_numpy(sec_off.view(np.int32)).to(dev)
    lits_a = torch.empty(16 * n_lits, dtype=torch.uint8, device=dev)
    lo_a = torch.empty(m + 1, dtype=torch.int32, device=dev)
    rc_a = torch.empty(m, dtype=torch.int32, device=dev)
    used_a = torch.empty(m, dtype=torch.int32, device=dev)
    out_a = torch.empty(bound, dtype=torch.uint8, device=dev)
    oo_a = torch.empty(n_lits + 1, dtype=torch.int32, device=dev)
    st_a = torch.empty(n_lits, dtype=torch.uint8, device=dev)

    def call_scan():
        codec.scan_sections_into(wire_dev, so_dev, m, qhuff.SCAN_FIELD_SECTION,
                                 lits_a, n_lits, lo_a, rc_a, used_a, st)

    def call_dec():
        codec.decode_wire_into(wire_dev, lits_a, n_lits, max_len, out_a, oo_a,
                               st_a, st)
    call_scan()
    call_dec()
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    assert np.array_equal(lits_a.cpu().numpy(), lits_b)
    assert np.array_equal(lo_a.cpu().numpy().view(np.uint32), lo_b)
    assert np.array_equal(out_a[:total].cpu().numpy(), out_b[:total])

    def block(fn, k, per, kind):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        codec.timing(True)
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        t = codec.timing_read()
        codec.timing(False)
        assert len(t) == k * per and all(kd == kind for kd, _ in t)
        return np.array([us for _, us in t]).reshape(k, per)

    ts, tw = [], []
    for r in range(args.rounds):
        for which in ((0, 1), (1, 0))[r % 2]:
            if which == 0:
                ts.append(block(call_scan, args.launches, 3, qhuff.KIND_SCAN))
            else:
                tw.append(block(call_dec, args.launches, 1, qhuff.KIND_DECODE))
    ts, tw = np.concatenate(ts), np.concatenate(tw)[:, 0]
    assert codec.device_error() == 0

    tb, tc, td, tz, tbs, tbd = [], [], [], [], [], []
    for r in range(args.host_reps):
        order = ("b", "c", "d", "z") if r % 2 else ("z", "d", "c", "b")
        for w in order:
            if w == "b":
                tb.append(call_b())
                tbs.append(t_b["scan"])
                tbd.append(t_b["decode"])
            elif w == "c":
                tc.append(call_c())
            elif w == "d":
                td.append(call_d())
            else:
                tz.append(call_b(zero=True))
    med = lambda v: float(np.median(v))
    scan_us = ts.sum(axis=1)
    b_spread = max(tb) - min(tb)
    res = {
        "tool": "scan_bench", "items": args.n, "sections": m,
        "lines_per_section": LINES, "literals": n_lits,
        "wire_bytes": wire_bytes, "descriptor_bytes": 16 * n_lits,
        "decoded_bytes": total,
        "launches_each": len(scan_us), "host_calls_each": len(tb),
        "a_scan_three_launches_us": round(med(scan_us), 2),
        "a_scan_min_us": round(float(scan_us.min()), 2),
        "a_scan_count_us": round(med(ts[:, 0]), 2),
        "a_scan_top_us": round(med(ts[:, 1]), 2),
        "a_scan_write_us": round(med(ts[:, 2]), 2),
        "a_decode_wire_us": round(med(tw), 2),
        "a_decode_wire_min_us": round(float(tw.min()), 2),
        "a_scan_over_decode_wire": round(med(scan_us) / med(tw), 3),
        "b_per_section_scan_plus_decode_wire_host_us": round(med(tb), 1),
        "b_min_us": round(min(tb), 1), "b_max_us": round(max(tb), 1),
        "b_spread_us": round(b_spread, 1),
        "b_scan_loop_us": round(med(tbs), 1),
        "b_decode_wire_host_us": round(med(tbd), 1),
        "b_ctypes_overhead_us": round(med(tz), 1),
        "b_less_ctypes_overhead_us": round(med(tb) - med(tz), 1),
        "c_decode_sections_host_us": round(med(tc), 1),
        "c_min_us": round(min(tc), 1), "c_max_us": round(max(tc), 1),
        "c_over_b": round(med(tc) / med(tb), 3),
        "c_over_b_less_ctypes_overhead": round(
            med(tc) / (med(tb) - med(tz)), 3),
        "c_faster_than_b_beyond_spread":
            bool(med(tb) - med(tz) - med(tc) > b_spread),
        "d_scan_sections_cpu_us": round(med(td), 1),
        "d_min_us": round(min(td), 1),
        "d_wire_mb_per_s": round(wire_bytes / med(td), 1),
    }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    with open(os.path.join(os.path.dirname(args.out), "README.txt"), "w") as f:
        f.write(
            "qhuff_scan_sections records (MI355X; tools/scan_bench.py: %d field\n"
            "sections of %d lines, %d literals, %d wire bytes; the descriptors\n"
            "are %d bytes).\n\n"
            "scan_bench.json  the tree's run: kernel times by dispatch-stamped\n"
            "    events (medians of %d warmed calls each, alternated blocks), host\n"
            "    calls by a host clock (medians of %d alternated calls).\n\n"
            "  (a) scan, three launches   %10.2f us  (count %.2f, top %.2f, write %.2f)\n"
            "      qhuff_decode_wire      %10.2f us  on the same descriptors\n"
            "  (b) per-section host scan + qhuff_decode_wire_host\n"
            "                             %10.1f us  (min %.1f, max %.1f: spread %.1f)\n"
            "      its scan loop          %10.1f us, of which ctypes calls %.1f us\n"
            "      less that overhead     %10.1f us\n"
            "  (c) qhuff_decode_sections_host\n"
            "                             %10.1f us  (min %.1f, max %.1f)\n"
            "  (d) qhuff_scan_sections_cpu %9.1f us  (%.1f MB/s of wire bytes)\n\n"
            "(c) faster than (b) less the ctypes overhead by more than (b)'s\n"
            "spread: %s.\n" % (
                m, LINES, n_lits, wire_bytes, 16 * n_lits, len(scan_us),
                len(tb), med(scan_us), med(ts[:, 0]), med(ts[:, 1]),
                med(ts[:, 2]), med(tw), med(tb), min(tb), max(tb), b_spread,
                med(tbs), med(tz), med(tb) - med(tz), med(tc), min(tc),
                max(tc), med(td), wire_bytes / med(td),
                "yes" if res["c_faster_than_b_beyond_spread"] else "no"))
    codec.close()


if __name__ == "__main__":
    main()
