"""The header calls over a set of dynamic tables measured (recorded, nothing
asserted about a time), on the batch of tools/encode_headers_dyn_bench.py --
the QIF corpus' header lists repeated to about 1M headers in sections of 16 --
and its table: the corpus' 128 most frequent (name, value) pairs,
max_entries 128.

  (a) T = 1, sec_tab all 0: every new launch beside the _dyn launch it
      copies, on the same arrays, alternated in one process -- the index
      build, the lookup (encode form and lookup form) and the prefix launch
      of qhuff_encode_headers_tabs / qhuff_dyn_lookup_tabs beside
      qhuff_encode_headers_dyn / qhuff_dyn_lookup's, the scan's count and
      write launches beside qhuff_scan_headers_dyn's, and the two host calls
      (encode, decode) beside theirs: the price of the indirection;
  (b) T = 32 and 1024 tables that each hold the same 128 entries, sections
      dealt round-robin: the lookup launch's time beside T = 1's (the design
      claim: it does not grow with T), and the index build at D = 128, 4,096
      and 131,072.

Kernel times by qhuff_timing_* (the dispatches' own time stamps) over blocks
of warmed launches, medians; the host calls by a host clock.  Every timed
call's result is first checked: the T = 1 output against the _dyn call's
bytes, T = 32 and 1024 against T = 1's (the tables are equal, so the sections
are), the scan's arrays against the _dyn scan's.  One JSON line, printed and
written to profiles/headers_tabs/headers_tabs_bench.json."""
import argparse
import collections
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ls-qpack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch
import qhuff
from headers_bench import corpus, p

TABLE = 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--section", type=int, default=16)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--tables", type=int, nargs="*", default=[32, 1024])
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "headers_tabs", "headers_tabs_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    data, off, sec_hdr = corpus(args.n, args.section)
    n, m = (len(off) - 1) // 2, len(sec_hdr) - 1
    total = int(off[-1])
    data = np.concatenate([data, np.zeros(16, np.uint8)])
    codec = qhuff.Codec(0)
    L = qhuff.lib()
    st = torch.cuda.current_stream()

    db = data.tobytes()
    hdr = [(db[off[2 * i]:off[2 * i + 1]], db[off[2 * i + 1]:off[2 * i + 2]])
           for i in range(n)]
    top = [h for h, _ in collections.Counter(hdr).most_common(TABLE)]
    d1 = len(top)
    one = b"".join(a + b for a, b in top)
    lens = np.array([len(x) for h in top for x in h], dtype=np.int64)
    toff = np.zeros(2 * d1 + 1, np.uint32)
    np.cumsum(lens, out=toff[1:])
    table = (np.frombuffer(one + bytes(16), np.uint8), toff, 0, TABLE)

    def tables(T):
        """T tables of the same entries -> the set's host arrays"""
        o = np.zeros(2 * d1 * T + 1, np.uint32)
        np.cumsum(np.tile(lens, T), out=o[1:])
        return (np.frombuffer(one * T + bytes(16), np.uint8), o,
                (np.arange(T + 1) * d1).astype(np.uint32),
                np.zeros(T, np.uint32), np.full(T, TABLE, np.uint32))

    def sec_tab(T):
        return (np.arange(m) % T).astype(np.uint32)

    # the results, checked once
    want = codec.encode_headers_dyn_host(data, off, sec_hdr, table)
    assert want[0] == qhuff.OK
    wire, so_w = want[1], want[2]
    for T in [1] + args.tables:
        got = codec.encode_headers_tabs_host(data, off, sec_hdr, tables(T),
                                             sec_tab(T))
        assert got[0] == qhuff.OK
        for a, b in zip(got[1:], want[1:]):
            assert np.array_equal(a, b)
    wire16 = np.concatenate([wire, np.zeros(16, np.uint8)])
    res_d = codec.decode_headers_dyn_host(wire16, so_w, table, max_hdrs=n)
    res_t = codec.decode_headers_tabs_host(wire16, so_w, tables(1), sec_tab(1),
                                           max_hdrs=n)
    assert res_d[0] == res_t[0] == qhuff.OK
    for a, b in zip(res_d[1:], res_t[1:]):
        assert np.array_equal(a, b)
    assert np.array_equal(res_t[7], data[:total])

    def d8(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def d32(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    D, O, SH = d8(data), d32(off), d32(sec_hdr)
    W, SO = d8(wire16), d32(so_w)
    bound = qhuff.encode_headers_dyn_bound(total, n, m)
    out = torch.empty(bound, dtype=torch.uint8, device=dev)
    so = torch.empty(m + 1, dtype=torch.int32, device=dev)
    kind, sid, hf = (torch.empty(n, dtype=torch.uint8, device=dev)
                     for _ in range(3))
    did, h1, h2, rc = (torch.empty(n, dtype=torch.int32, device=dev)
                       for _ in range(4))
    strs = torch.empty(32 * n, dtype=torch.uint8, device=dev)
    ho = torch.empty(m + 1, dtype=torch.int32, device=dev)
    TD, TO = d8(table[0]), d32(toff)
    tab_dyn = qhuff.DynTable(TD.data_ptr(), TO.data_ptr(), d1, 0, TABLE)
    sets = {}
    for T in [1] + args.tables:
        keep = [d8(x) if i == 0 else d32(x) for i, x in enumerate(tables(T))]
        sets[T] = (codec.dyn_tables_dev(*keep), d32(sec_tab(T)), keep)

    def enc_dyn():
        codec.encode_headers_dyn_into(D, O, n, None, SH, m, tab_dyn, None,
                                      None, out, so, kind, sid, did, st)

    def enc_tabs(T):
        def f():
            codec.encode_headers_tabs_into(D, O, n, None, SH, m, sets[T][0],
                                           sets[T][1], None, None, out, so,
                                           kind, sid, did, st)
        return f

    def look_dyn():
        assert L.qhuff_dyn_lookup(
            codec._ctx, D.data_ptr(), O.data_ptr(), n, C.byref(tab_dyn), 0,
            d1, h1.data_ptr(), h2.data_ptr(), kind.data_ptr(), sid.data_ptr(),
            did.data_ptr(), None) == qhuff.OK

    def look_tabs():
        codec.dyn_lookup_tabs_into(D, O, n, SH, m, sets[1][0], sets[1][1],
                                   None, h1, h2, kind, sid, did, st)

    def scan_dyn():
        codec.scan_headers_dyn_into(W, SO, m, TO, d1, 0, TABLE, None, strs, n,
                                    ho, rc, kind, sid, hf, did, st)

    def scan_tabs():
        codec.scan_headers_tabs_into(W, SO, m, sets[1][0], sets[1][1], None,
                                     strs, n, ho, rc, kind, sid, hf, did, st)

    def snap(fn, arrs):
        for a in arrs:
            a.zero_()
        fn()
        torch.cuda.synchronize()
        assert codec.device_error() == 0
        return [a.cpu().numpy().copy() for a in arrs]
    ref = snap(enc_dyn, (so, kind, sid, did))
    for T in sets:
        for a, b in zip(ref, snap(enc_tabs(T), (so, kind, sid, did))):
            assert np.array_equal(a, b)
    assert np.array_equal(ref[0].view(np.uint32), so_w)
    ref = snap(look_dyn, (h1, h2, kind, sid, did))
    for a, b in zip(ref, snap(look_tabs, (h1, h2, kind, sid, did))):
        assert np.array_equal(a, b)
    ref = snap(scan_dyn, (strs, ho, rc, kind, sid, hf, did))
    for a, b in zip(ref, snap(scan_tabs, (strs, ho, rc, kind, sid, hf, did))):
        assert np.array_equal(a, b)

    def block(fn, k, kinds):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        codec.timing(True)
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        t = codec.timing_read()
        codec.timing(False)
        per = len(kinds)
        assert [kd for kd, _ in t] == list(kinds) * k, [kd for kd, _ in t][:8]
        return [[u for _, u in t[j::per]] for j in range(per)]

    H, E, S = qhuff.KIND_HASH, qhuff.KIND_ENCODE, qhuff.KIND_SCAN
    calls = [("enc_dyn", enc_dyn, (H, H, H, E)),
             ("look_dyn", look_dyn, (H, H)), ("look_tabs", look_tabs, (H, H)),
             ("scan_dyn", scan_dyn, (S, S, S)),
             ("scan_tabs", scan_tabs, (S, S, S))]
    calls += [("enc_tabs_%d" % T, enc_tabs(T), (H, H, H, E)) for T in sets]
    t = {key: [[] for _ in kinds] for key, _, kinds in calls}
    for r in range(args.rounds):
        for key, fn, kinds in calls[::1 if r % 2 else -1]:
            for acc, got in zip(t[key], block(fn, args.launches, kinds)):
                acc += got
    assert codec.device_error() == 0

    # the host calls, alternated
    tt, keep1 = qhuff.dyn_table_host(*table)
    ts, keep2 = qhuff.dyn_tables_host(*tables(1))
    stab = sec_tab(1)
    hb = {"out": np.zeros(bound, np.uint8), "so": np.zeros(m + 1, np.uint32)}
    dbound = qhuff.decode_headers_dyn_bound(len(wire), n, int(
        (toff[2::2] - toff[:-2:2]).max()))
    hd = {"ho": np.zeros(m + 1, np.uint32), "rc": np.zeros(m, np.int32),
          "out": np.zeros(dbound, np.uint8),
          "off": np.zeros(2 * n + 1, np.uint32),
          "status": np.zeros(2 * n, np.uint8)}

    def henc_dyn():
        assert L.qhuff_encode_headers_dyn_host(
            codec._ctx, p(data), p(off), n, None, p(sec_hdr), m, C.byref(tt),
            None, None, p(hb["out"]), p(hb["so"]), None, None,
            None) == qhuff.OK

    def henc_tabs():
        assert L.qhuff_encode_headers_tabs_host(
            codec._ctx, p(data), p(off), n, None, p(sec_hdr), m, C.byref(ts),
            p(stab), None, None, p(hb["out"]), p(hb["so"]), None, None,
            None) == qhuff.OK

    def hdec_dyn():
        assert L.qhuff_decode_headers_dyn_host(
            codec._ctx, p(wire16), p(so_w), m, C.byref(tt), None, 0, n,
            p(hd["ho"]), p(hd["rc"]), None, None, None, None, p(hd["out"]),
            p(hd["off"]), p(hd["status"]), None, None) == qhuff.OK

    def hdec_tabs():
        assert L.qhuff_decode_headers_tabs_host(
            codec._ctx, p(wire16), p(so_w), m, C.byref(ts), p(stab), None, 0,
            n, p(hd["ho"]), p(hd["rc"]), None, None, None, None,
            p(hd["out"]), p(hd["off"]), p(hd["status"]), None,
            None) == qhuff.OK
    hosts = (("henc_dyn", henc_dyn), ("henc_tabs", henc_tabs),
             ("hdec_dyn", hdec_dyn), ("hdec_tabs", hdec_tabs))
    th = {k: [] for k, _ in hosts}
    for _, fn in hosts:
        fn()
    assert np.array_equal(hb["so"], so_w) and np.array_equal(hd["off"], off)
    for _ in range(args.host_reps):
        for key, fn in hosts:
            t0 = time.perf_counter()
            fn()
            th[key].append((time.perf_counter() - t0) * 1e6)
    del keep1, keep2
    med = lambda v: float(np.median(v))  # noqa: E731
    r2 = lambda v: round(med(v), 2)  # noqa: E731
    ratio = lambda a, b: round(med(a) / med(b), 3)  # noqa: E731
    e1, ed = t["enc_tabs_1"], t["enc_dyn"]
    res = {
        "tool": "headers_tabs_bench", "n": n, "sections": m,
        "header_bytes": total, "wire_bytes": int(so_w[-1]),
        "table_entries": d1, "launches_each": len(ed[0]),
        "a_dyn_index_us": r2(ed[0]), "a_tabs_index_us": r2(e1[0]),
        "a_dyn_lookup_enc_us": r2(ed[1]), "a_tabs_lookup_enc_us": r2(e1[1]),
        "a_lookup_enc_tabs_over_dyn": ratio(e1[1], ed[1]),
        "a_dyn_prefix_us": r2(ed[2]), "a_tabs_prefix_us": r2(e1[2]),
        "a_dyn_encode_us": r2(ed[3]), "a_tabs_encode_us": r2(e1[3]),
        "a_dyn_lookup_alone_us": r2(t["look_dyn"][1]),
        "a_tabs_lookup_alone_us": r2(t["look_tabs"][1]),
        "a_lookup_alone_tabs_over_dyn": ratio(t["look_tabs"][1],
                                              t["look_dyn"][1]),
        "a_dyn_scan_count_us": r2(t["scan_dyn"][0]),
        "a_tabs_scan_count_us": r2(t["scan_tabs"][0]),
        "a_dyn_scan_write_us": r2(t["scan_dyn"][2]),
        "a_tabs_scan_write_us": r2(t["scan_tabs"][2]),
        "a_scan_tabs_over_dyn": round(
            (med(t["scan_tabs"][0]) + med(t["scan_tabs"][2]))
            / (med(t["scan_dyn"][0]) + med(t["scan_dyn"][2])), 3),
        "a_encode_headers_dyn_host_us": round(med(th["henc_dyn"]), 1),
        "a_encode_headers_tabs_host_us": round(med(th["henc_tabs"]), 1),
        "a_decode_headers_dyn_host_us": round(med(th["hdec_dyn"]), 1),
        "a_decode_headers_tabs_host_us": round(med(th["hdec_tabs"]), 1),
        "a_host_calls": len(th["henc_dyn"]),
        "b_tables": [1] + args.tables,
        "b_entries": [T * d1 for T in sets],
        "b_index_slots": [qhuff.dyn_tables_index_slots(T * d1) for T in sets],
        "b_index_us": [r2(t["enc_tabs_%d" % T][0]) for T in sets],
        "b_lookup_us": [r2(t["enc_tabs_%d" % T][1]) for T in sets],
        "b_prefix_us": [r2(t["enc_tabs_%d" % T][2]) for T in sets],
        "b_lookup_over_one_table": [ratio(t["enc_tabs_%d" % T][1], e1[1])
                                    for T in sets],
    }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    codec.close()


if __name__ == "__main__":
    main()
