"""Header lists to field sections (qhuff_static_lookup, qhuff_encode_headers)
against what a caller has without them, on the QIF corpus' header lists
(tests/golden/data/fb-req.qif, netbsd.qif) repeated to about 1M headers, in
sections of 16.

Timed, after checking that (c) and (d) give the same bytes and that the
lookup's hashes are those of (h):

  (h) qhuff_xxh32_headers on the bytes                      kernel time
  (l) qhuff_static_lookup on the same bytes: the hashes,
      kind and static_id                                    kernel time
  (e) qhuff_encode_headers: its lookup launch (the items
      and their string offsets instead of the hashes) and
      its encode launch                                     kernel times
  (c) qhuff_encode_headers_host                             host clock
  (d) the same job before: qhuff_xxh32_headers_host, the
      two probes and the byte compares with numpy over
      tables the caller brings (tests/golden/
      static_lookup.json, qpack_static_table.json), two
      items a header and a section built with numpy,
      qhuff_encode_wire_host, the sections' ends gathered   host clock

(h), (l) and (e) by qhuff_timing_* over blocks of warmed launches alternated
in one process, (c) and (d) by a host clock around the synchronous calls,
also alternated.  One JSON line, printed and written to
profiles/headers/headers_bench.json."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ls-qpack_amd"))
GOLD = os.path.join(ROOT, "tests", "golden")
# (the QIF files are read by the tests' parser, so that the corpus measured
# here is the one tests/test_encode_headers.py checks)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch
import qhuff
from qpack_frames import qif_header_lists


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def corpus(n_target, per_section):
    """-> (data, off [2n + 1], sec_hdr [m + 1])"""
    hs = [h for fn in ("fb-req.qif", "netbsd.qif")
          for l in qif_header_lists(open(os.path.join(GOLD, "data", fn),
                                         "rb").read()) for h in l]
    parts = [x for h in hs for x in h]
    one = np.frombuffer(b"".join(parts), dtype=np.uint8)
    lens = np.array([len(x) for x in parts], dtype=np.int64)
    k = max(1, n_target // len(hs))
    data = np.tile(one, k)
    off = np.zeros(2 * len(hs) * k + 1, dtype=np.uint32)
    np.cumsum(np.tile(lens, k), out=off[1:])
    n = len(hs) * k
    sec_hdr = np.append(np.arange(0, n, per_section), n).astype(np.uint32)
    return data, off, sec_hdr


def spread(starts, lens):
    base = np.cumsum(lens) - lens
    return np.repeat(starts - base, lens) + np.arange(int(lens.sum()),
                                                      dtype=np.int64)


class HostLookup:
    """the lookup a caller does today on the hashes it brought back: probe,
    compare lengths, compare bytes, entry by entry with numpy"""

    def __init__(self):
        with open(os.path.join(GOLD, "static_lookup.json")) as f:
            fx = json.load(f)
        with open(os.path.join(GOLD, "qpack_static_table.json")) as f:
            self.table = [(a.encode("latin-1"), b.encode("latin-1"))
                          for a, b in json.load(f)["static_table"]]
        self.n2i = np.array(fx["name2id_plus_one"], dtype=np.int64)
        self.nv2i = np.array(fx["nameval2id_plus_one"], dtype=np.int64)

    def _match(self, data, start, length, cand, text):
        """cand[i] - 1 = candidate entry: does data[start[i] : + length[i]]
        equal text(entry)?"""
        ok = np.zeros(len(cand), dtype=bool)
        for e in np.unique(cand):
            if e == 0:
                continue
            t = np.frombuffer(text(self.table[e - 1]), dtype=np.uint8)
            idx = np.flatnonzero((cand == e) & (length == len(t)))
            if len(idx) == 0:
                continue
            if len(t) == 0:
                ok[idx] = True
                continue
            got = data[start[idx][:, None] + np.arange(len(t))[None, :]]
            ok[idx] = (got == t[None, :]).all(axis=1)
        return ok

    def __call__(self, data, off, h1, h2):
        o = off.astype(np.int64)
        a, m, b = o[0:-1:2], o[1::2], o[2::2]
        full = self.nv2i[h2 & 511]
        hit_full = self._match(data, a, b - a, full, lambda e: e[0] + e[1]) \
            & (m - a == np.array([0] + [len(e[0]) for e in self.table])[full])
        name = self.n2i[h1 & 511]
        hit_name = self._match(data, a, m - a, name, lambda e: e[0])
        kind = np.where(hit_full, 0, np.where(hit_name, 1, 2)).astype(np.uint8)
        sid = np.where(hit_full, full - 1,
                       np.where(hit_name, name - 1, 0xFF)).astype(np.uint8)
        return kind, sid


def build_items(off, sec_hdr, kind, sid, n, m):
    """two items a section prefix, two a header -> (items uint8 [8N],
    str_off uint32 [N + 1], the sections' first items)"""
    N = 2 * n + 2 * m
    sec_of = np.repeat(np.arange(m, dtype=np.int64), np.diff(sec_hdr.astype(np.int64)))
    pos = 2 * np.arange(n, dtype=np.int64) + 2 * (sec_of + 1)
    first = 2 * sec_hdr[:-1].astype(np.int64) + 2 * np.arange(m, dtype=np.int64)
    w = np.zeros((N, 2), dtype=np.uint32)        # {ival, bits word}
    so = np.zeros(N + 1, dtype=np.uint32)
    w[first, 1], w[first + 1, 1] = 8, 7
    so[first] = so[first + 1] = off[2 * sec_hdr[:-1].astype(np.int64)]
    idx, ref, lit = kind == 0, kind == 1, kind == 2
    w[pos, 0] = np.where(lit, 0, sid)
    w[pos, 1] = np.where(idx, 6 | 0xC0 << 8,
                         np.where(ref, 4 | 0x50 << 8, 3 << 16 | 0x20 << 24))
    w[pos + 1, 1] = np.where(idx, 0, 7 << 16)
    so[pos], so[pos + 1] = off[0:-1:2], off[1::2]
    so[N] = off[-1]
    return w.view(np.uint8).reshape(-1), so, np.append(first, N)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--section", type=int, default=16)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "headers", "headers_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    data, off, sec_hdr = corpus(args.n, args.section)
    n, m = (len(off) - 1) // 2, len(sec_hdr) - 1
    in_bytes = int(off[-1])
    src = np.concatenate([data, np.zeros(16, dtype=np.uint8)])
    codec = qhuff.Codec(0)
    L = qhuff.lib()
    st = torch.cuda.current_stream()
    bound = qhuff.encode_headers_bound(in_bytes, n, m)
    N = 2 * n + 2 * m

    # (c)
    out_c = np.zeros(bound, dtype=np.uint8)
    so_c = np.zeros(m + 1, dtype=np.uint32)
    kind_c, sid_c = np.zeros(n, np.uint8), np.zeros(n, np.uint8)

    def call_c():
        rc = L.qhuff_encode_headers_host(codec._ctx, p(src), p(off), n, None,
                                         p(sec_hdr), m, p(out_c), p(so_c),
                                         p(kind_c), p(sid_c))
        assert rc == qhuff.OK, rc
    call_c()
    total = int(so_c[-1])

    # (d)
    look = HostLookup()
    h1_d, h2_d = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    out_d = np.zeros(bound, dtype=np.uint8)
    oo_d = np.zeros(N + 1, dtype=np.uint32)
    res_d = {}

    def call_d():
        rc = L.qhuff_xxh32_headers_host(codec._ctx, p(src), p(off), n,
                                        qhuff.XXH_SEED, p(h1_d), p(h2_d))
        assert rc == qhuff.OK, rc
        kind, sid = look(src, off, h1_d.astype(np.int64), h2_d.astype(np.int64))
        items, so, first = build_items(off, sec_hdr, kind, sid, n, m)
        rc = L.qhuff_encode_wire_host(codec._ctx, p(src), p(so), p(items), N,
                                      p(out_d), p(oo_d))
        assert rc == qhuff.OK, rc
        res_d["kind"], res_d["sid"], res_d["sec_out"] = kind, sid, oo_d[first]
    call_d()
    assert np.array_equal(res_d["kind"], kind_c)
    assert np.array_equal(res_d["sid"], sid_c)
    assert np.array_equal(res_d["sec_out"], so_c)
    assert np.array_equal(out_d[:total], out_c[:total])

    # (h), (l), (e)
    d = torch.from_numpy(src).to(dev)
    o = torch.from_numpy(off.view(np.int32)).to(dev)
    sh = torch.from_numpy(sec_hdr.view(np.int32)).to(dev)
    h1, h2, g1, g2 = (torch.empty(n, dtype=torch.int32, device=dev)
                      for _ in range(4))
    kind, sid = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2))
    out_e = torch.empty(bound, dtype=torch.uint8, device=dev)
    so_e = torch.empty(m + 1, dtype=torch.int32, device=dev)

    def call_h():
        codec.xxh32_headers_into(d, o, n, qhuff.XXH_SEED, h1, h2, st)

    def call_l():
        codec.static_lookup_into(d, o, n, g1, g2, kind, sid, st)

    def call_e():
        codec.encode_headers_into(d, o, n, None, sh, m, out_e, so_e, kind, sid,
                                  st)
    call_h(), call_l()
    torch.cuda.synchronize()
    assert torch.equal(h1, g1) and torch.equal(h2, g2)
    assert np.array_equal(kind.cpu().numpy(), kind_c)
    call_e()
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    assert np.array_equal(so_e.cpu().numpy().view(np.uint32), so_c)
    assert np.array_equal(out_e[:total].cpu().numpy(), out_c[:total])

    def block(fn, k, kinds):
        """k timed calls of fn -> per launch kind of a call, the k times"""
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
        assert len(t) == k * per
        assert [kd for kd, _ in t] == list(kinds) * k
        return [[u for _, u in t[j::per]] for j in range(per)]

    th, tl, tel, tee = [], [], [], []
    for r in range(args.rounds):
        for which in ((0, 1, 2), (2, 1, 0))[r % 2]:
            if which == 0:
                th += block(call_h, args.launches, (qhuff.KIND_HASH,))[0]
            elif which == 1:
                tl += block(call_l, args.launches, (qhuff.KIND_HASH,))[0]
            else:
                a, b = block(call_e, args.launches,
                             (qhuff.KIND_HASH, qhuff.KIND_ENCODE))
                tel += a
                tee += b
    assert codec.device_error() == 0

    tc, td = [], []
    for r in range(args.host_reps):
        for fn, acc in ((call_c, tc), (call_d, td))[::1 if r % 2 else -1]:
            t0 = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t0) * 1e6)
    med = lambda v: float(np.median(v))
    kinds = np.bincount(kind_c, minlength=3)
    res = {
        "tool": "headers_bench", "n": n, "sections": m, "in_bytes": in_bytes,
        "wire_bytes": total, "indexed": int(kinds[0]), "nameref": int(kinds[1]),
        "literal": int(kinds[2]),
        "launches_each": len(th), "host_calls_each": len(tc),
        "h_xxh32_headers_us": round(med(th), 2),
        "l_static_lookup_us": round(med(tl), 2),
        "l_over_h": round(med(tl) / med(th), 3),
        "e_lookup_launch_us": round(med(tel), 2),
        "e_encode_launch_us": round(med(tee), 2),
        "e_lookup_over_h": round(med(tel) / med(th), 3),
        "h_min_us": round(min(th), 2), "l_min_us": round(min(tl), 2),
        "e_lookup_min_us": round(min(tel), 2),
        "c_encode_headers_host_us": round(med(tc), 1),
        "d_hash_numpy_lookup_encode_wire_host_us": round(med(td), 1),
        "c_over_d": round(med(tc) / med(td), 4),
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
