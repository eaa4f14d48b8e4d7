"""Field sections to header lists (qhuff_scan_headers, qhuff_decode_headers)
against what a caller has without them, on the batch of tools/headers_bench.py:
the QIF corpus' header lists repeated to about 1M headers, in sections of 16,
encoded by qhuff_encode_headers_host.

Timed, after checking that (c) and (d) give the same header lists and that
these are the lists that were encoded:

  (s) qhuff_scan_sections' three launches on the bytes      kernel times
  (S) qhuff_scan_headers' three launches on the same bytes  kernel times
  (w) qhuff_decode_wire on the sections' literals           kernel time
  (D) qhuff_decode_headers on the sections' headers         kernel time
  (c) qhuff_decode_headers_host                             host clock
  (d) the same job before: qhuff_decode_sections_host, then
      the header lists assembled with numpy -- the indexed
      lines found in the gaps between the literals' lines,
      the static indices read from the wire, the names and
      values gathered from the static table (tests/golden/
      qpack_static_table.json) and the decoded literals      host clock

(s), (S), (w) and (D) by qhuff_timing_* over blocks of warmed launches
alternated in one process, (c) and (d) by a host clock around the synchronous
calls, also alternated.  With them the bytes (w) and (D) write and the share
of their tiles on each path (the layout rules of qhuff_wire_impl.h and
qhuff_hdrdec_impl.h over the descriptors).  One JSON line, printed and
written to profiles/decode_headers/decode_headers_bench.json."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ls-qpack_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(ROOT, "tests", "golden")

import numpy as np
import torch
import qhuff
from headers_bench import corpus, p, spread

LIT = np.dtype([("pos", "<u4"), ("len", "<u4"), ("huffman", "u1"),
                ("prefix_bits", "u1"), ("kind", "u1"), ("hdr_len", "u1"),
                ("instr", "<u4")])
HSTR = np.dtype([("pos", "<u4"), ("len", "<u4"), ("huffman", "u1"),
                 ("source", "u1"), ("kind", "u1"), ("static_id", "u1"),
                 ("instr", "<u4")])


class HostAssembly:
    """header lists from a section's literals as a caller builds them today:
    static-only sections (no dynamic form, ids below 99), numpy throughout"""

    def __init__(self):
        with open(os.path.join(GOLD, "qpack_static_table.json")) as f:
            t = [(a.encode("latin-1"), b.encode("latin-1"))
                 for a, b in json.load(f)["static_table"]]
        self.flat = np.frombuffer(b"".join(a + b for a, b in t), np.uint8)
        nl = np.array([len(a) for a, _ in t], dtype=np.int64)
        vl = np.array([len(b) for _, b in t], dtype=np.int64)
        at = np.cumsum(nl + vl) - (nl + vl)
        self.nl, self.vl, self.n_at, self.v_at = nl, vl, at, at + nl

    def __call__(self, wire, sec_off, lits, dec, dec_off):
        lits = lits.view(LIT)
        w = wire.astype(np.int64)
        so = sec_off.astype(np.int64)
        isv = np.flatnonzero(lits["kind"] == qhuff.LIT_VALUE)
        named = np.zeros(len(isv), dtype=bool)
        named[isv > 0] = lits["kind"][isv[isv > 0] - 1] == qhuff.LIT_NAME
        start = lits["instr"][isv].astype(np.int64)
        end = lits["pos"][isv].astype(np.int64) + lits["len"][isv]
        # the bytes no literal's line and no prefix covers: indexed lines
        cov = np.zeros(len(w) + 1, dtype=np.int64)
        np.add.at(cov, start, 1)
        np.add.at(cov, end, -1)
        np.add.at(cov, so[:-1], 1)
        np.add.at(cov, so[:-1] + 2, -1)
        gap = np.cumsum(cov[:-1]) == 0
        ix = np.flatnonzero(gap & (w >= 0x80))
        ix_id = w[ix] & 0x3f
        long_ = ix_id == 63
        ix_id[long_] += w[ix[long_] + 1]
        ref_id = w[start] & 0x0f
        long_ = (ref_id == 15) & ~named
        ref_id[long_] += w[start[long_] + 1]
        # every header by its line's first byte
        at = np.concatenate([ix, start])
        order = np.argsort(at, kind="stable")
        n = len(at)
        kind = np.concatenate([np.zeros(len(ix), np.uint8),
                               np.where(named, 2, 1).astype(np.uint8)])[order]
        sid = np.concatenate([ix_id, np.where(named, 0xFF, ref_id)])[order]
        do = dec_off.astype(np.int64)
        src = np.concatenate([self.flat, dec])
        base = len(self.flat)
        sidc = np.minimum(sid, 98)
        # names: static (indexed, name reference) or the literal before the value
        nlen = np.concatenate([np.zeros(len(ix), np.int64),
                               np.where(named, do[isv] - do[isv - 1], 0)])[order]
        nsrc = np.concatenate([np.zeros(len(ix), np.int64),
                               base + do[isv - 1]])[order]
        stat_n = kind != 2
        nlen[stat_n] = self.nl[sidc[stat_n]]
        nsrc[stat_n] = self.n_at[sidc[stat_n]]
        vlen = np.concatenate([np.zeros(len(ix), np.int64),
                               do[isv + 1] - do[isv]])[order]
        vsrc = np.concatenate([np.zeros(len(ix), np.int64),
                               base + do[isv]])[order]
        stat_v = kind == 0
        vlen[stat_v] = self.vl[sidc[stat_v]]
        vsrc[stat_v] = self.v_at[sidc[stat_v]]
        lens = np.stack([nlen, vlen], axis=1).reshape(-1)
        starts = np.stack([nsrc, vsrc], axis=1).reshape(-1)
        off = np.zeros(2 * n + 1, dtype=np.uint32)
        np.cumsum(lens, out=off[1:])
        data = src[spread(starts, lens)]
        hdr_off = np.searchsorted(at[order], so).astype(np.uint32)
        return data, off, hdr_off, kind, sid.astype(np.uint8)


def tile_paths(strs, off, residue, dtype=HSTR):
    """the share of a launch's tiles (64 descriptors each) on each path, by
    the rules of qhuff_hdrdec_impl.h / qhuff_wire_impl.h: staged (wire span
    <= 3072), fast (and output + 64 <= 3072), fixed arena (no wire string
    above 66 bytes)"""
    s = strs.view(dtype)
    k = len(s)
    t0 = np.arange(0, k, 64)
    t1 = np.minimum(t0 + 64, k) - 1
    a = residue + s["pos"][t0].astype(np.int64)
    b = residue + s["pos"][t1].astype(np.int64) + s["len"][t1]
    span = (b + 15) // 16 * 16 - a // 16 * 16
    o = off.astype(np.int64)
    total = o[np.minimum(t0 + 64, k)] - o[t0]
    staged = span <= 3072
    fast = staged & (total + 64 <= 3072)
    longest = np.maximum.reduceat(s["len"].astype(np.int64), t0)
    fixed = longest <= 66
    nt = len(t0)
    return {"tiles": nt,
            "fast_fixed_arena": round(float((fast & fixed).sum()) / nt, 4),
            "fast_placed_arena": round(float((fast & ~fixed).sum()) / nt, 4),
            "slow_staged": round(float((staged & ~fast).sum()) / nt, 4),
            "slow_unstaged": round(float((~staged).sum()) / nt, 4),
            "mean_wire_span": round(float((b - a).mean()), 1),
            "mean_out_bytes": round(float(total.mean()), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--section", type=int, default=16)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "decode_headers", "decode_headers_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    data, off, sec_hdr = corpus(args.n, args.section)
    n, m = (len(off) - 1) // 2, len(sec_hdr) - 1
    codec = qhuff.Codec(0)
    L = qhuff.lib()
    st = torch.cuda.current_stream()
    wire, sec_off, kind_e, sid_e = codec.encode_headers_host(
        np.concatenate([data, np.zeros(16, np.uint8)]), off, sec_hdr)
    wire_bytes = len(wire)
    wire = np.concatenate([wire, np.zeros(16, np.uint8)])
    M = qhuff.MAX_STRLEN

    # (c)
    bound = qhuff.decode_headers_bound(wire_bytes, n)
    c = {"hdr_off": np.zeros(m + 1, np.uint32), "rc": np.zeros(m, np.int32),
         "kind": np.zeros(n, np.uint8), "sid": np.zeros(n, np.uint8),
         "hf": np.zeros(n, np.uint8), "out": np.zeros(bound, np.uint8),
         "off": np.zeros(2 * n + 1, np.uint32), "st": np.zeros(2 * n, np.uint8)}

    def call_c():
        rc = L.qhuff_decode_headers_host(
            codec._ctx, p(wire), p(sec_off), m, M, n, p(c["hdr_off"]),
            p(c["rc"]), p(c["kind"]), p(c["sid"]), p(c["hf"]), p(c["out"]),
            p(c["off"]), p(c["st"]), None, None)
        assert rc == qhuff.OK, rc
    call_c()
    total = int(c["off"][-1])
    assert not c["rc"].any() and not c["st"].any()
    assert np.array_equal(c["off"], off) and np.array_equal(c["hdr_off"], sec_hdr)
    assert np.array_equal(c["out"][:total], data)
    assert np.array_equal(c["kind"], kind_e) and np.array_equal(c["sid"], sid_e)

    # (d)
    n_lits = int((kind_e == 1).sum() + 2 * (kind_e == 2).sum())
    dl = {"lits": np.zeros(16 * n_lits, np.uint8),
          "lit_off": np.zeros(m + 1, np.uint32), "rc": np.zeros(m, np.int32),
          "used": np.zeros(m, np.uint32),
          "out": np.zeros(qhuff.decode_bound(wire_bytes, 0), np.uint8),
          "oo": np.zeros(n_lits + 1, np.uint32), "st": np.zeros(n_lits, np.uint8)}
    asm = HostAssembly()
    res_d = {}

    def call_d():
        rc = L.qhuff_decode_sections_host(
            codec._ctx, p(wire), p(sec_off), m, qhuff.SCAN_FIELD_SECTION, M,
            p(dl["lits"]), n_lits, p(dl["lit_off"]), p(dl["rc"]),
            p(dl["used"]), p(dl["out"]), p(dl["oo"]), p(dl["st"]))
        assert rc == qhuff.OK, rc
        res_d["r"] = asm(wire[:wire_bytes], sec_off, dl["lits"], dl["out"],
                         dl["oo"])
    call_d()
    d_data, d_off, d_hdr_off, d_kind, d_sid = res_d["r"]
    assert np.array_equal(d_off, off) and np.array_equal(d_data, data)
    assert np.array_equal(d_hdr_off, sec_hdr)
    assert np.array_equal(d_kind, kind_e) and np.array_equal(d_sid, sid_e)
    lit_bytes = int(dl["oo"][-1])

    # (s), (S), (w), (D)
    W = torch.from_numpy(wire).to(dev)
    so = torch.from_numpy(sec_off.view(np.int32)).to(dev)
    lits = torch.empty(16 * n_lits, dtype=torch.uint8, device=dev)
    strs = torch.empty(32 * n, dtype=torch.uint8, device=dev)
    cnt_l, cnt_h = (torch.empty(m + 1, dtype=torch.int32, device=dev)
                    for _ in range(2))
    rc_l, rc_h, used = (torch.empty(m, dtype=torch.int32, device=dev)
                        for _ in range(3))
    kind, sid, hf = (torch.empty(n, dtype=torch.uint8, device=dev)
                     for _ in range(3))
    out_w = torch.empty(qhuff.decode_bound(wire_bytes, 0), dtype=torch.uint8,
                        device=dev)
    oo_w = torch.empty(n_lits + 1, dtype=torch.int32, device=dev)
    st_w = torch.empty(n_lits, dtype=torch.uint8, device=dev)
    out_h = torch.empty(bound, dtype=torch.uint8, device=dev)
    off_h = torch.empty(2 * n + 1, dtype=torch.int32, device=dev)
    st_h = torch.empty(2 * n, dtype=torch.uint8, device=dev)

    def call_s():
        codec.scan_sections_into(W, so, m, qhuff.SCAN_FIELD_SECTION, lits,
                                 n_lits, cnt_l, rc_l, used, st)

    def call_S():
        codec.scan_headers_into(W, so, m, strs, n, cnt_h, rc_h, kind, sid, hf,
                                st)

    def call_w():
        codec.decode_wire_into(W, lits, n_lits, M, out_w, oo_w, st_w, st)

    def call_D():
        codec.decode_headers_into(W, strs, n, M, out_h, off_h, st_h, st)
    call_s(), call_S(), call_w(), call_D()
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    assert np.array_equal(off_h.cpu().numpy().view(np.uint32), off)
    assert np.array_equal(out_h[:total].cpu().numpy(), data)
    assert np.array_equal(lits.cpu().numpy(), dl["lits"])
    assert np.array_equal(out_w[:lit_bytes].cpu().numpy(),
                          dl["out"][:lit_bytes])
    paths = tile_paths(strs.cpu().numpy(), off, W.data_ptr() % 16)
    w_paths = tile_paths(dl["lits"], dl["oo"], W.data_ptr() % 16, LIT)

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
    t = {"s": [[], [], []], "S": [[], [], []], "w": [[]], "D": [[]]}
    calls = (("s", call_s, S3), ("S", call_S, S3), ("w", call_w, D1),
             ("D", call_D, D1))
    for r in range(args.rounds):
        for key, fn, kinds in calls[::1 if r % 2 else -1]:
            for acc, got in zip(t[key], block(fn, args.launches, kinds)):
                acc += got
    assert codec.device_error() == 0

    tc, td = [], []
    for r in range(args.host_reps):
        for fn, acc in ((call_c, tc), (call_d, td))[::1 if r % 2 else -1]:
            t0 = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t0) * 1e6)
    med = lambda v: float(np.median(v))  # noqa: E731
    three = lambda k: sum(med(x) for x in t[k])  # noqa: E731
    kinds_n = np.bincount(kind_e, minlength=3)
    w_written = lit_bytes + 5 * n_lits + 4
    d_written = total + 5 * 2 * n + 4
    res = {
        "tool": "decode_headers_bench", "n": n, "sections": m,
        "wire_bytes": wire_bytes, "header_bytes": total,
        "literals": n_lits, "literal_bytes": lit_bytes,
        "indexed": int(kinds_n[0]), "nameref": int(kinds_n[1]),
        "literal": int(kinds_n[2]),
        "launches_each": len(t["w"][0]), "host_calls_each": len(tc),
        "s_scan_sections_us": [round(med(x), 2) for x in t["s"]],
        "S_scan_headers_us": [round(med(x), 2) for x in t["S"]],
        "s_total_us": round(three("s"), 2), "S_total_us": round(three("S"), 2),
        "S_over_s": round(three("S") / three("s"), 3),
        "s_descriptor_bytes": 16 * n_lits,
        "S_descriptor_bytes": 32 * n + 3 * n,
        "w_decode_wire_us": round(med(t["w"][0]), 2),
        "D_decode_headers_us": round(med(t["D"][0]), 2),
        "D_over_w": round(med(t["D"][0]) / med(t["w"][0]), 3),
        "w_min_us": round(min(t["w"][0]), 2),
        "D_min_us": round(min(t["D"][0]), 2),
        "w_bytes_written": w_written, "D_bytes_written": d_written,
        "D_over_w_bytes_written": round(d_written / w_written, 3),
        "w_descriptor_bytes_read": 16 * n_lits,
        "D_descriptor_bytes_read": 32 * n,
        "w_paths": w_paths, "D_paths": paths,
        "c_decode_headers_host_us": round(med(tc), 1),
        "d_decode_sections_host_numpy_assembly_us": round(med(td), 1),
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
