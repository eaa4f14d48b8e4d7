"""qhuff_encode_headers_dyn measured (recorded, not asserted), on the batch of
tools/headers_bench.py -- the QIF corpus' header lists repeated to about 1M
headers, in sections of 16 -- and the table of
tools/decode_headers_dyn_bench.py: the corpus' 128 most frequent (name, value)
pairs, max_entries 128.

  (a) without a table (d = 0): the new call's launches against
      qhuff_encode_headers' on the same batch, alternated in one process --
      the lookup launch beside the old lookup launch, and the whole call
      (the sum of its launches): what the dynamic path costs when unused;
  (b) with the table: the index build, the lookup, the prefix launch, the
      encode launch and the gather's neighbours one by one, and
      qhuff_encode_headers_dyn_host beside qhuff_encode_headers_host;
  (c) the encode launch alone, (a) against (b), and the share of its 64-item
      tiles whose input span passes the 3 KB stage (one way onto the item
      kernel's out-of-line path).  The items' string offsets are the same
      with and without the table -- an indexed line's name and value still
      pass through the stage though nothing is made of them -- so that share
      is the same; what changes is the work a tile does.

Kernel times by qhuff_timing_* over blocks of warmed launches, the host calls
by a host clock.  Every timed call's result is first checked: (a) against
qhuff_encode_headers' bytes, (b) by decoding the sections again with
qhuff_decode_headers_dyn_host.  One JSON line, printed and written to
profiles/encode_headers_dyn/encode_headers_dyn_bench.json."""
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
from headers_bench import build_items, corpus, p

TABLE = 128
STAGE = 3072                             # qhuff_pipeline.h kStageCap


def past_stage(off, sec_hdr, n, m, residue):
    """the share of the encode launch's 64-item tiles whose strings span more
    than the stage (16-byte blocks, the data at address residue `residue`)"""
    _, so, _ = build_items(off, sec_hdr, np.zeros(n, np.uint8),
                           np.zeros(n, np.uint8), n, m)
    so = so.astype(np.int64) + residue
    N = len(so) - 1
    t0 = np.arange(0, N, 64)
    a, b = so[t0], so[np.minimum(t0 + 64, N)]
    span = (b + 15) // 16 * 16 - a // 16 * 16
    return len(t0), float((span > STAGE).mean()), float((b - a).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--section", type=int, default=16)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "encode_headers_dyn", "encode_headers_dyn_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    data, off, sec_hdr = corpus(args.n, args.section)
    n, m = (len(off) - 1) // 2, len(sec_hdr) - 1
    total = int(off[-1])
    data = np.concatenate([data, np.zeros(16, np.uint8)])
    codec = qhuff.Codec(0)
    L = qhuff.lib()
    st = torch.cuda.current_stream()

    # the table: the 128 most frequent (name, value) pairs
    db = data.tobytes()
    hdr = [(db[off[2 * i]:off[2 * i + 1]], db[off[2 * i + 1]:off[2 * i + 2]])
           for i in range(n)]
    top = [h for h, _ in collections.Counter(hdr).most_common(TABLE)]
    tdata = np.frombuffer(b"".join(a + b for a, b in top) + bytes(16), np.uint8)
    toff = np.zeros(2 * len(top) + 1, np.uint32)
    np.cumsum([len(x) for h in top for x in h], out=toff[1:])
    table = (tdata, toff, 0, TABLE)
    none = (None, None, 0, TABLE)

    # the results, checked once
    want_s = codec.encode_headers_host(data, off, sec_hdr)
    got_a = codec.encode_headers_dyn_host(data, off, sec_hdr, none)
    assert got_a[0] == qhuff.OK
    assert np.array_equal(got_a[1], want_s[0])
    assert np.array_equal(got_a[2], want_s[1])
    got_b = codec.encode_headers_dyn_host(data, off, sec_hdr, table)
    assert got_b[0] == qhuff.OK
    wire_b, so_b, kind_b = got_b[1], got_b[2], got_b[3]
    res = codec.decode_headers_dyn_host(
        np.concatenate([wire_b, np.zeros(16, np.uint8)]), so_b, table,
        max_hdrs=n)
    assert res[0] == qhuff.OK and not res[2].any() and not res[9].any()
    assert np.array_equal(res[1], sec_hdr) and np.array_equal(res[8], off)
    assert np.array_equal(res[7], data[:total])
    assert np.array_equal(res[3], kind_b) and np.array_equal(res[6], got_b[5])
    lines = collections.Counter(kind_b.tolist())

    def d8(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def d32(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    D, O, SH = d8(data), d32(off), d32(sec_hdr)
    T, TO = d8(tdata), d32(toff)
    bound = qhuff.encode_headers_dyn_bound(total, n, m)
    out = torch.empty(bound, dtype=torch.uint8, device=dev)
    so = torch.empty(m + 1, dtype=torch.int32, device=dev)
    kind, sid = (torch.empty(n, dtype=torch.uint8, device=dev)
                 for _ in range(2))
    did = torch.empty(n, dtype=torch.int32, device=dev)
    tab_none = qhuff.DynTable(None, None, 0, 0, TABLE)
    tab_full = qhuff.DynTable(T.data_ptr(), TO.data_ptr(), len(top), 0, TABLE)

    def call_old():
        codec.encode_headers_into(D, O, n, None, SH, m, out, so, kind, sid, st)

    def call_a():
        codec.encode_headers_dyn_into(D, O, n, None, SH, m, tab_none, None,
                                      None, out, so, kind, sid, did, st)

    def call_b():
        codec.encode_headers_dyn_into(D, O, n, None, SH, m, tab_full, None,
                                      None, out, so, kind, sid, did, st)

    def same(want_out, want_so):
        torch.cuda.synchronize()
        assert codec.device_error() == 0
        got = so.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want_so)
        assert np.array_equal(out[:int(got[-1])].cpu().numpy(), want_out)
    for fn, w in ((call_old, want_s), (call_a, want_s),
                  (call_b, (wire_b, so_b))):
        so.zero_()
        fn()
        same(w[0], w[1])

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

    H, E = qhuff.KIND_HASH, qhuff.KIND_ENCODE
    calls = (("old", call_old, (H, E)), ("a", call_a, (H, H, E)),
             ("b", call_b, (H, H, H, E)))
    t = {key: [[] for _ in kinds] for key, _, kinds in calls}
    for r in range(args.rounds):
        for key, fn, kinds in calls[::1 if r % 2 else -1]:
            for acc, got in zip(t[key], block(fn, args.launches, kinds)):
                acc += got
    assert codec.device_error() == 0

    # the host calls, alternated
    tt, keep = qhuff.dyn_table_host(*table)
    hb = {"out": np.zeros(bound, np.uint8), "so": np.zeros(m + 1, np.uint32)}

    def host_old():
        assert L.qhuff_encode_headers_host(
            codec._ctx, p(data), p(off), n, None, p(sec_hdr), m, p(hb["out"]),
            p(hb["so"]), None, None) == qhuff.OK

    def host_new():
        assert L.qhuff_encode_headers_dyn_host(
            codec._ctx, p(data), p(off), n, None, p(sec_hdr), m, C.byref(tt),
            None, None, p(hb["out"]), p(hb["so"]), None, None,
            None) == qhuff.OK
    th = {"old": [], "new": []}
    host_old()
    host_new()
    assert np.array_equal(hb["so"], so_b)
    for _ in range(args.host_reps):
        for key, fn in (("old", host_old), ("new", host_new)):
            t0 = time.perf_counter()
            fn()
            th[key].append((time.perf_counter() - t0) * 1e6)
    del keep
    med = lambda v: float(np.median(v))  # noqa: E731
    r2 = lambda v: round(med(v), 2)  # noqa: E731
    tiles, share, span = past_stage(off, sec_hdr, n, m, D.data_ptr() % 16)
    old_total = med(t["old"][0]) + med(t["old"][1])
    a_total = sum(med(x) for x in t["a"])
    b_total = sum(med(x) for x in t["b"])
    res = {
        "tool": "encode_headers_dyn_bench", "n": n, "sections": m,
        "header_bytes": total, "launches_each": len(t["old"][0]),
        "static_wire_bytes": int(want_s[1][-1]),
        "a_old_lookup_us": r2(t["old"][0]), "a_old_encode_us": r2(t["old"][1]),
        "a_old_call_us": round(old_total, 2),
        "a_dyn_lookup_us": r2(t["a"][0]), "a_dyn_prefix_us": r2(t["a"][1]),
        "a_dyn_encode_us": r2(t["a"][2]), "a_dyn_call_us": round(a_total, 2),
        "a_lookup_new_over_old": round(med(t["a"][0]) / med(t["old"][0]), 3),
        "a_call_new_over_old": round(a_total / old_total, 3),
        "b_table_entries": len(top), "b_table_bytes": int(toff[-1]),
        "b_index_slots": qhuff.dyn_index_slots(len(top)),
        "b_wire_bytes": int(so_b[-1]),
        "b_lines": {"indexed_static": lines[0], "nameref_static": lines[1],
                    "literal": lines[2], "indexed_dyn": lines[4],
                    "nameref_dyn": lines[5]},
        "b_index_us": r2(t["b"][0]), "b_lookup_us": r2(t["b"][1]),
        "b_prefix_us": r2(t["b"][2]), "b_encode_us": r2(t["b"][3]),
        "b_call_us": round(b_total, 2),
        "b_lookup_over_old_lookup": round(med(t["b"][1]) / med(t["old"][0]), 3),
        "b_encode_headers_host_us": round(med(th["old"]), 1),
        "b_encode_headers_dyn_host_us": round(med(th["new"]), 1),
        "b_host_new_over_old": round(med(th["new"]) / med(th["old"]), 3),
        "b_host_calls": len(th["new"]),
        "c_encode_tiles": tiles, "c_tiles_past_stage": round(share, 4),
        "c_mean_tile_span": round(span, 1),
        "c_encode_static_us": r2(t["old"][1]), "c_encode_dyn_us": r2(t["b"][3]),
        "c_encode_dyn_over_static": round(med(t["b"][3]) / med(t["old"][1]), 3),
    }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    codec.close()


if __name__ == "__main__":
    main()
