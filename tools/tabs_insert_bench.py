"""Encoder-stream inserts applied to a set of dynamic tables, measured
(recorded, nothing asserted about a time): qhuff_tabs_insert_host beside
qhuff_tabs_insert_cpu on one thread, on the same input.

The set is T tables of the benches' table -- the QIF corpus' 128 most frequent
(name, value) pairs -- each exactly full (cap = the entries' size), so every
insert evicts.  Every connection's chunk holds 8 inserts, two of each kind:
literal name (Huffman), static name reference, dynamic name reference,
duplicate.  T = 1, 32 and 1,024 (1,024 x 128 entries: the arena README's
decode call reads).

Per T: the host call and the CPU form by a host clock (medians over --reps
calls, --small-reps below 1,024 tables so that the timed window is tenths of
a second, alternated, after warm-up calls), and the seven launches of one host
call by qhuff_timing_* (the dispatches' own time stamps): the scan's count,
sums and write, the decode launch, the accounting, the sums over the tables
and the copy.  The host call's arrays are first checked against the CPU
form's, all of them.  One JSON line, printed and written to
profiles/tabs_insert/tabs_insert_bench.json."""
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
import oracle_lib as O
import qhuff
import qpack_frames as Q
from headers_bench import corpus, p

TABLE = 128


def lit(first, bits, s, huff):
    pl = O.huffman_enc(s) if huff else bytes(s)
    return Q.enc_int(first | ((1 << bits) if huff else 0), len(pl), bits) + pl


def chunk(c):
    """8 inserts, two of each kind, a little different per connection"""
    v = b"value-%d" % c
    return (lit(0x40, 5, b"x-conn-%d" % (c % 97), 1) + lit(0, 7, v, 1)
            + Q.enc_int(0xc0, 1 + c % 90, 6) + lit(0, 7, v, 0)
            + Q.enc_int(0x80, 5, 6) + lit(0, 7, v, 1)       # an old entry
            + Q.enc_int(0x00, 9, 5)                         # duplicate, old
            + lit(0x40, 5, b"x-second", 0) + lit(0, 7, b"", 0)
            + Q.enc_int(0xc0, 17, 6) + lit(0, 7, b"gzip, deflate", 1)
            + Q.enc_int(0x80, 0, 6) + lit(0, 7, v, 0)       # the insert before
            + Q.enc_int(0x00, 1, 5))                        # duplicate, new


class Call:
    """one call's arrays, allocated once: the C call alone is timed"""

    def __init__(self, T, one, lens, d1, used):
        self.T = T
        off = np.zeros(2 * d1 * T + 1, np.uint32)
        np.cumsum(np.tile(lens, T), out=off[1:])
        max_cap = (used + 31) // 32 * 32
        self.tables = (np.frombuffer(one * T + bytes(16), np.uint8), off,
                       (np.arange(T + 1) * d1).astype(np.uint32),
                       np.zeros(T, np.uint32),
                       np.full(T, max_cap // 32, np.uint32))
        self.cap = np.full(T, used, np.uint32)
        self.max_cap = np.full(T, max_cap, np.uint32)
        self.lo = np.zeros(T, np.uint32)
        chunks = [chunk(c) for c in range(T)]
        self.buf = np.frombuffer(b"".join(chunks) + bytes(16), np.uint8)
        self.enc_off = np.zeros(T + 1, np.uint32)
        np.cumsum([len(x) for x in chunks], out=self.enc_off[1:])
        self.n = n = 8 * T
        self.t, self.keep = qhuff.dyn_tables_host(*self.tables)
        self.D = D = d1 * T
        self.bound = qhuff.tabs_insert_bound(int(off[-1]),
                                             int(self.enc_off[-1]), n,
                                             int(lens.reshape(-1, 2)
                                                 .sum(axis=1).max()))
        self.st = qhuff.InsState(p(self.cap), p(self.max_cap), p(self.lo), 0,
                                 0)
        self.res = []
        for _ in range(2):                  # [0] the host form's, [1] the CPU's
            a = {"rc": np.zeros(T, np.int32),
                 "consumed": np.zeros(T, np.uint32),
                 "ins_off": np.zeros(T + 1, np.uint32),
                 "ins_ref": np.zeros(n, np.uint32),
                 "ins_kind": np.zeros(n, np.uint8),
                 "ins_lo": np.zeros(n, np.uint32),
                 "out": np.zeros(self.bound, np.uint8),
                 "out_off": np.zeros(2 * (D + n) + 1, np.uint32),
                 "out_ent": np.zeros(T + 1, np.uint32),
                 "out_first": np.zeros(T, np.uint32),
                 "cap_out": np.zeros(T, np.uint32),
                 "lo_out": np.zeros(T, np.uint32)}
            sc = qhuff.InsScan(p(a["rc"]), p(a["consumed"]), p(a["ins_off"]),
                               None, None, None, None, p(a["ins_ref"]),
                               p(a["ins_kind"]), n)
            o = qhuff.InsOut(p(a["ins_lo"]), p(a["out"]), p(a["out_off"]),
                             p(a["out_ent"]), p(a["out_first"]),
                             p(a["cap_out"]), p(a["lo_out"]), self.bound,
                             D + n)
            self.res.append((a, sc, o))

    def host(self, codec):
        _, sc, o = self.res[0]
        assert qhuff.lib().qhuff_tabs_insert_host(
            codec._ctx, C.byref(self.t), C.byref(self.st), p(self.buf),
            p(self.enc_off), None, C.byref(sc), C.byref(o)) == qhuff.OK

    def cpu(self):
        _, sc, o = self.res[1]
        assert qhuff.lib().qhuff_tabs_insert_cpu(
            C.byref(self.t), C.byref(self.st), p(self.buf), p(self.enc_off),
            None, C.byref(sc), C.byref(o)) == qhuff.OK

    def check(self):
        a, b = self.res[0][0], self.res[1][0]
        assert not a["rc"].any() and int(a["ins_off"][-1]) == self.n
        assert (a["lo_out"] > 0).all()                      # it evicted
        De = int(a["out_ent"][-1])
        total = int(a["out_off"][2 * De])
        for k in a:
            if k == "out":
                assert np.array_equal(a[k][:total], b[k][:total])
            elif k == "out_off":
                assert np.array_equal(a[k][:2 * De + 1], b[k][:2 * De + 1])
            else:
                assert np.array_equal(a[k], b[k]), k
        return De, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, nargs="*", default=[1, 32, 1024])
    ap.add_argument("--reps", type=int, default=100,
                    help="timed calls at 1,024 tables and above")
    ap.add_argument("--small-reps", type=int, default=2000,
                    help="timed calls below that: a call is 0.1 ms")
    ap.add_argument("--out", default=os.path.join(
        ROOT, "profiles", "tabs_insert", "tabs_insert_bench.json"))
    args = ap.parse_args()
    data, off, _ = corpus(1 << 16, 16)
    db = data.tobytes()
    n = (len(off) - 1) // 2
    hdr = [(db[off[2 * i]:off[2 * i + 1]], db[off[2 * i + 1]:off[2 * i + 2]])
           for i in range(n)]
    top = [h for h, _ in collections.Counter(hdr).most_common(TABLE)]
    d1 = len(top)
    one = b"".join(a + b for a, b in top)
    lens = np.array([len(x) for h in top for x in h], dtype=np.int64)
    used = int(lens.sum()) + 32 * d1
    codec = qhuff.Codec(0)
    import torch
    S, Dk = qhuff.KIND_SCAN, qhuff.KIND_DECODE
    names = ("scan_count", "scan_sums", "scan_write", "decode", "account",
             "sums", "copy")
    res = {"tool": "tabs_insert_bench", "table_entries": d1,
           "table_bytes": len(one), "capacity": used, "inserts_per_chunk": 8,
           "reps": [], "tables": args.tables, "arena_bytes": [],
           "wire_bytes": [], "out_entries": [], "out_bytes": [],
           "host_call_us": [], "cpu_form_us": [], "host_over_cpu": [],
           "launch_us": {k: [] for k in names}, "launch_sum_us": []}
    for T in args.tables:
        c = Call(T, one, lens, d1, used)
        for _ in range(3):
            c.host(codec)
            c.cpu()
        De, total = c.check()
        reps = args.reps if T >= 1024 else args.small_reps
        res["reps"].append(reps)
        th, tc = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            c.host(codec)
            th.append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter()
            c.cpu()
            tc.append((time.perf_counter() - t0) * 1e6)
        # the launches of the host call, in a pass of their own
        per = [[] for _ in names]
        for _ in range(min(reps, 200)):
            codec.timing(True)
            c.host(codec)
            torch.cuda.synchronize()
            t = codec.timing_read()
            codec.timing(False)
            assert [k for k, _ in t] == [S, S, S, Dk, S, S, S], t
            for acc, (_, us) in zip(per, t):
                acc.append(us)
        assert codec.device_error() == 0
        med = lambda v: float(np.median(v))  # noqa: E731
        res["arena_bytes"].append(len(one) * T)
        res["wire_bytes"].append(int(c.enc_off[-1]))
        res["out_entries"].append(De)
        res["out_bytes"].append(total)
        res["host_call_us"].append(round(med(th), 1))
        res["cpu_form_us"].append(round(med(tc), 1))
        res["host_over_cpu"].append(round(med(th) / med(tc), 3))
        for k, v in zip(names, per):
            res["launch_us"][k].append(round(med(v), 2))
        res["launch_sum_us"].append(round(sum(med(v) for v in per), 2))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    codec.close()


if __name__ == "__main__":
    main()
