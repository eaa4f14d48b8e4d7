"""qhuff_decode_headers_dyn measured (recorded, not asserted), on the batch of
tools/decode_headers_bench.py: the QIF corpus' header lists repeated to about
1M headers, in sections of 16.

  (a) the static-only batch, the new launch against the old one:
      qhuff_decode_headers_dyn (no table) and qhuff_decode_headers on the same
      descriptors, alternated in one process -- the cost of the third source
      when it is unused;
  (b) the same header lists with a table: the corpus' 128 most frequent
      (name, value) pairs are the table's entries; a header found there is
      re-encoded as an indexed dynamic line, one whose name alone is there (and
      not in the static table) as a dynamic name reference with its value
      literal kept.  The scan's and the decode's launch times, the host call,
      and the share of tiles on each path: dynamic entries raise a tile's
      output, so the out-of-line share rises; no speed is promised for it.

Kernel times by qhuff_timing_* over blocks of warmed launches, the host call
by a host clock.  Every timed call's result is first checked against the
header lists that were encoded.  One JSON line, printed and written to
profiles/decode_headers_dyn/decode_headers_dyn_bench.json."""
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
from decode_headers_bench import HSTR
from headers_bench import corpus, p

TABLE = 128


def enc_int(first, value, bits):
    mask = (1 << bits) - 1
    if value < mask:
        return bytes([first | value])
    out, value = bytearray([first | mask]), value - mask
    while value >= 128:
        out.append(0x80 | (value & 0x7f))
        value >>= 7
    out.append(value)
    return bytes(out)


def with_table(wire, sec_off, strs, hdr_off, kind, data, off):
    """the static-only sections re-encoded against the table -> (wire,
    sec_off, entries, counts)"""
    s = strs.view(HSTR)
    n = len(kind)
    db = data.tobytes()
    hdr = [(db[off[2 * i]:off[2 * i + 1]], db[off[2 * i + 1]:off[2 * i + 2]])
           for i in range(n)]
    top = [h for h, _ in collections.Counter(hdr).most_common(TABLE)]
    pair = {h: k for k, h in enumerate(top)}
    name = {}
    for k, (a, _) in enumerate(top):
        name.setdefault(a, k)
    wb = wire.tobytes()
    out, new_off, cnt = [], [0], collections.Counter()
    for sec in range(len(hdr_off) - 1):
        lo, hi = int(hdr_off[sec]), int(hdr_off[sec + 1])
        end = int(sec_off[sec + 1])
        lines, refs = [], []
        for i in range(lo, hi):
            at = int(s["instr"][2 * i])
            nxt = int(s["instr"][2 * i + 2]) if i + 1 < hi else end
            k = pair.get(hdr[i])
            if k is not None:
                lines.append(("i", k))
                refs.append(k)
            elif kind[i] == 2 and hdr[i][0] in name:
                v0 = int(s["pos"][2 * i]) + int(s["len"][2 * i])
                lines.append(("n", name[hdr[i][0]], wb[v0:nxt],
                              wb[at] >> 4 & 1))
                refs.append(name[hdr[i][0]])
            else:
                lines.append(("s", wb[at:nxt]))
        ric = max(refs) + 1 if refs else 0
        b = bytearray(enc_int(0, ric % (2 * TABLE) + 1 if ric else 0, 8) + b"\0")
        for l in lines:
            if l[0] == "i":
                b += enc_int(0x80, ric - 1 - l[1], 6)
            elif l[0] == "n":
                b += enc_int(0x40 | l[3] << 5, ric - 1 - l[1], 4) + l[2]
            else:
                b += l[1]
            cnt[l[0]] += 1
        out.append(bytes(b))
        new_off.append(new_off[-1] + len(b))
    return (np.frombuffer(b"".join(out) + bytes(16), np.uint8),
            np.array(new_off, np.uint32), top, cnt)


def tile_paths(strs, off, residue):
    s = strs.view(HSTR)
    k = len(s)
    t0 = np.arange(0, k, 64)
    t1 = np.minimum(t0 + 64, k) - 1
    wl = np.where((s["source"] & 3) % 3 == 0, s["len"], 0).astype(np.int64)
    a = residue + s["pos"][t0].astype(np.int64)
    b = residue + s["pos"][t1].astype(np.int64) + wl[t1]
    span = (b + 15) // 16 * 16 - a // 16 * 16
    o = off.astype(np.int64)
    total = o[np.minimum(t0 + 64, k)] - o[t0]
    dyn = np.add.reduceat(np.where(s["source"] == 2, s["len"], 0)
                          .astype(np.int64), t0)
    staged = span <= 3072
    fast = staged & (total + 64 <= 3072)
    nt = len(t0)
    return {"tiles": nt, "fast": round(float(fast.sum()) / nt, 4),
            "slow_staged": round(float((staged & ~fast).sum()) / nt, 4),
            "slow_unstaged": round(float((~staged).sum()) / nt, 4),
            "mean_wire_span": round(float((b - a).mean()), 1),
            "mean_out_bytes": round(float(total.mean()), 1),
            "mean_dyn_bytes": round(float(dyn.mean()), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--section", type=int, default=16)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "decode_headers_dyn", "decode_headers_dyn_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    data, off, sec_hdr = corpus(args.n, args.section)
    n, m = (len(off) - 1) // 2, len(sec_hdr) - 1
    codec = qhuff.Codec(0)
    L = qhuff.lib()
    st = torch.cuda.current_stream()
    M = qhuff.MAX_STRLEN
    wire, sec_off, kind_e, _ = codec.encode_headers_host(
        np.concatenate([data, np.zeros(16, np.uint8)]), off, sec_hdr)
    wire_bytes = len(wire)
    wire = np.concatenate([wire, np.zeros(16, np.uint8)])
    total = int(off[-1])
    _, strs_s, hdr_off_s, rc_s, kind_s, _, _ = qhuff.scan_headers_cpu(
        wire, sec_off, n)
    assert not rc_s.any() and np.array_equal(hdr_off_s, sec_hdr)

    # (b)'s batch and table
    wire_b, sec_off_b, top, cnt = with_table(wire, sec_off, strs_s, hdr_off_s,
                                             kind_s, data, off)
    wire_b_bytes = int(sec_off_b[-1])
    tdata = np.frombuffer(b"".join(a + b for a, b in top) + bytes(16), np.uint8)
    toff = np.zeros(2 * len(top) + 1, np.uint32)
    np.cumsum([len(x) for h in top for x in h], out=toff[1:])
    longest = max(len(a) + len(b) for a, b in top)
    table = (tdata, toff, 0, TABLE)
    ret, strs_b, hdr_off_b, rc_b, kind_b, _, _, did_b = \
        qhuff.scan_headers_dyn_cpu(wire_b, sec_off_b, table, None, n)
    assert ret == qhuff.OK and not rc_b.any()
    assert np.array_equal(hdr_off_b, sec_hdr)

    bound_b = qhuff.decode_headers_dyn_bound(wire_b_bytes, n, longest)
    hb = {"hdr_off": np.zeros(m + 1, np.uint32), "rc": np.zeros(m, np.int32),
          "out": np.zeros(bound_b, np.uint8),
          "off": np.zeros(2 * n + 1, np.uint32), "st": np.zeros(2 * n, np.uint8)}
    tt, keep = qhuff.dyn_table_host(*table)

    def call_host():
        rc = L.qhuff_decode_headers_dyn_host(
            codec._ctx, p(wire_b), p(sec_off_b), m, C.byref(tt), None, M, n,
            p(hb["hdr_off"]), p(hb["rc"]), None, None, None, None,
            p(hb["out"]), p(hb["off"]), p(hb["st"]), None, None)
        assert rc == qhuff.OK, rc
    call_host()
    assert not hb["rc"].any() and not hb["st"].any()
    assert np.array_equal(hb["off"], off)
    assert np.array_equal(hb["out"][:total], data)

    # device buffers
    def d8(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def d32(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    W, so = d8(wire), d32(sec_off)
    Wb, sob = d8(wire_b), d32(sec_off_b)
    T, To = d8(tdata), d32(toff)
    strs = d8(strs_s)
    strs_d = torch.empty(32 * n, dtype=torch.uint8, device=dev)
    cnt_h = torch.empty(m + 1, dtype=torch.int32, device=dev)
    rc_h = torch.empty(m, dtype=torch.int32, device=dev)
    kind, sid, hf = (torch.empty(n, dtype=torch.uint8, device=dev)
                     for _ in range(3))
    did = torch.empty(n, dtype=torch.int32, device=dev)
    out_h = torch.empty(max(bound_b, qhuff.decode_headers_bound(wire_bytes, n)),
                        dtype=torch.uint8, device=dev)
    off_h = torch.empty(2 * n + 1, dtype=torch.int32, device=dev)
    st_h = torch.empty(2 * n, dtype=torch.uint8, device=dev)

    def same():
        torch.cuda.synchronize()
        assert codec.device_error() == 0
        assert np.array_equal(off_h.cpu().numpy().view(np.uint32), off)
        assert np.array_equal(out_h[:total].cpu().numpy(), data)
        assert not st_h.any()

    def call_old():
        codec.decode_headers_into(W, strs, n, M, out_h, off_h, st_h, st)

    def call_new():
        codec.decode_headers_dyn_into(W, strs, n, M, None, 0, out_h, off_h,
                                      st_h, st)

    def call_scan():
        codec.scan_headers_dyn_into(Wb, sob, m, To, len(top), 0, TABLE, None,
                                    strs_d, n, cnt_h, rc_h, kind, sid, hf, did,
                                    st)

    def call_dec():
        codec.decode_headers_dyn_into(Wb, strs_d, n, M, T, int(toff[-1]),
                                      out_h, off_h, st_h, st)
    for fn in (call_old, call_new):
        off_h.zero_()
        fn()
        same()
    call_scan()
    off_h.zero_()
    call_dec()
    same()
    assert np.array_equal(strs_d.cpu().numpy(), strs_b)
    paths_a = tile_paths(strs_s, off, W.data_ptr() % 16)
    paths_b = tile_paths(strs_b, off, Wb.data_ptr() % 16)

    def block(fn, k, kinds):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        codec.timing(True)
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        t = codec.timing_read()
        codec.timing(False)
        per = len(kinds)
        assert [kd for kd, _ in t] == list(kinds) * k
        return [[u for _, u in t[j::per]] for j in range(per)]

    S3, D1 = (qhuff.KIND_SCAN,) * 3, (qhuff.KIND_DECODE,)
    t = {"old": [[]], "new": [[]], "scan": [[], [], []], "dec": [[]]}
    calls = (("old", call_old, D1), ("new", call_new, D1),
             ("scan", call_scan, S3), ("dec", call_dec, D1))
    for r in range(args.rounds):
        for key, fn, kinds in calls[::1 if r % 2 else -1]:
            for acc, got in zip(t[key], block(fn, args.launches, kinds)):
                acc += got
    assert codec.device_error() == 0
    th = []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        call_host()
        th.append((time.perf_counter() - t0) * 1e6)
    del keep
    med = lambda v: float(np.median(v))  # noqa: E731
    res = {
        "tool": "decode_headers_dyn_bench", "n": n, "sections": m,
        "header_bytes": total, "launches_each": len(t["old"][0]),
        "a_wire_bytes": wire_bytes,
        "a_decode_headers_us": round(med(t["old"][0]), 2),
        "a_decode_headers_dyn_us": round(med(t["new"][0]), 2),
        "a_new_over_old": round(med(t["new"][0]) / med(t["old"][0]), 3),
        "a_min_us": [round(min(t["old"][0]), 2), round(min(t["new"][0]), 2)],
        "a_paths": paths_a,
        "b_table_entries": len(top), "b_table_bytes": int(toff[-1]),
        "b_table_longest": longest, "b_wire_bytes": wire_b_bytes,
        "b_lines": {"indexed_dyn": cnt["i"], "nameref_dyn": cnt["n"],
                    "as_before": cnt["s"]},
        "b_scan_headers_dyn_us": [round(med(x), 2) for x in t["scan"]],
        "b_scan_total_us": round(sum(med(x) for x in t["scan"]), 2),
        "b_decode_headers_dyn_us": round(med(t["dec"][0]), 2),
        "b_decode_min_us": round(min(t["dec"][0]), 2),
        "b_decode_headers_dyn_host_us": round(med(th), 1),
        "b_host_min_us": round(min(th), 1), "b_host_calls": len(th),
        "b_paths": paths_b,
    }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    codec.close()


if __name__ == "__main__":
    main()
