"""Literals decoded in place (qhuff_decode_wire) against the calls they stand
beside, on the 1M-string synthetic batch.

The batch is encoded on the device in QHUFF_ENC_LITERAL7 mode: that output is
a wire buffer of literals, whose descriptors are derived on the host from
out_off and each literal's first byte.  Timed, after checking that (a) and
(c) give (d)'s bytes:

  (a) qhuff_decode_wire on the wire buffer            kernel time
  (b) qhuff_decode_batch on the packed payloads of
      the same strings (the default, full kernel;
      b_lean: the lean one)                           kernel time
  (c) qhuff_decode_wire_host                          host clock
  (d) qhuff_decode_literals_ex                        host clock

(a) and (b) by qhuff_timing_* over blocks of warmed launches alternated in
one process, (c) and (d) by a host clock around the synchronous calls, also
alternated.  One JSON line, printed and written to
profiles/wire/wire_bench.json."""
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


def descriptors(wire, oo):
    """the literals of a QHUFF_ENC_LITERAL7 output: literal i is
    wire[oo[i] .. oo[i+1]), an H bit and a 7-bit prefixed length, then the
    payload -> (uint8 array of 16 * n bytes, share of Huffman literals)"""
    n = len(oo) - 1
    start = oo[:-1].astype(np.int64)
    b0 = wire[start]
    pre = b0 & 0x7f
    # (strings of at most 64 bytes: the length fits the prefix)
    assert (pre < 127).all()
    d = np.zeros(n, dtype=[("pos", "<u4"), ("len", "<u4"), ("huffman", "u1"),
                           ("prefix_bits", "u1"), ("kind", "u1"),
                           ("hdr_len", "u1"), ("instr", "<u4")])
    d["pos"] = start + 1
    d["len"] = pre
    d["huffman"] = b0 >> 7
    d["prefix_bits"] = 7
    d["kind"] = qhuff.LIT_VALUE
    d["hdr_len"] = 1
    d["instr"] = start
    assert (d["pos"].astype(np.int64) + d["len"] == oo[1:]).all()
    return d.view(np.uint8).copy(), float(d["huffman"].mean())


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wire",
                                                  "wire_bench.json"))
    args = ap.parse_args()
    n = args.n
    dev = torch.device("cuda", 0)
    data, off = qhuff.synth_batch(n)
    codec = qhuff.Codec(0)
    L = qhuff.lib()
    st = torch.cuda.current_stream()
    d = torch.from_numpy(data).to(dev)
    o = torch.from_numpy(off.view(np.int32)).to(dev)
    wire_t, woo_t = codec.encode(d, o, qhuff.ENC_LITERAL7)
    h_t, ho_t = codec.encode(d, o, qhuff.ENC_PAYLOAD)
    torch.cuda.synchronize()
    woo = woo_t.cpu().numpy().view(np.uint32)
    wire = wire_t[:int(woo[-1])].cpu().numpy()
    lits, huff_share = descriptors(wire, woo)
    assert qhuff.literals_check(lits) == (qhuff.OK, None)
    bound = qhuff.literals_bound(lits)
    hb = int(ho_t[-1].item())

    # (d): the expectation
    out_d = np.zeros(bound, dtype=np.uint8)
    oo_d = np.zeros(n + 1, dtype=np.uint32)
    st_d = np.zeros(n, dtype=np.uint8)

    def call_d():
        rc = L.qhuff_decode_literals_ex(codec._ctx, p(wire), p(lits), n, 0,
                                        p(out_d), p(oo_d), p(st_d))
        assert rc == qhuff.OK, rc
    call_d()
    assert not st_d.any() and np.array_equal(oo_d, off - off[0])
    assert np.array_equal(out_d[:int(oo_d[-1])], data)

    # (c)
    out_c = np.zeros(bound, dtype=np.uint8)
    oo_c = np.zeros(n + 1, dtype=np.uint32)
    st_c = np.ones(n, dtype=np.uint8)

    def call_c():
        rc = L.qhuff_decode_wire_host(codec._ctx, p(wire), p(lits), n, 0,
                                      p(out_c), p(oo_c), p(st_c))
        assert rc == qhuff.OK, rc
    call_c()
    assert np.array_equal(oo_c, oo_d) and not st_c.any()
    assert np.array_equal(out_c[:int(oo_c[-1])], out_d[:int(oo_d[-1])])

    # (a)
    wire_dev = wire_t[:int(woo[-1])].contiguous()
    lits_dev = torch.from_numpy(lits).to(dev)
    out_a = torch.empty(bound, dtype=torch.uint8, device=dev)
    oo_a = torch.empty(n + 1, dtype=torch.int32, device=dev)
    st_a = torch.empty(n, dtype=torch.uint8, device=dev)

    def call_a():
        codec.decode_wire_into(wire_dev, lits_dev, n, None, out_a, oo_a, st_a,
                               st)
    call_a()
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    assert np.array_equal(oo_a.cpu().numpy().view(np.uint32), oo_d)
    assert not st_a.cpu().numpy().any()
    assert np.array_equal(out_a[:int(oo_d[-1])].cpu().numpy(),
                          out_d[:int(oo_d[-1])])

    # (b)
    h = h_t[:hb].contiguous()
    out_b = torch.empty(qhuff.decode_bound(hb, n), dtype=torch.uint8,
                        device=dev)
    oo_b = torch.empty(n + 1, dtype=torch.int32, device=dev)
    st_b = torch.empty(n, dtype=torch.uint8, device=dev)

    def call_b(lean=False):
        if lean:
            codec.batch_hint(qhuff.KIND_DECODE, 0)
        codec.decode_into(h, ho_t, n, out_b, oo_b, st_b, st)

    def block(fn, k):
        """k timed launches of fn -> their kernel times (us)"""
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        codec.timing(True)
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        t = codec.timing_read()
        codec.timing(False)
        assert len(t) == k and all(kd == qhuff.KIND_DECODE for kd, _ in t)
        return [us for _, us in t]

    ta, tb, tbl = [], [], []
    for r in range(args.rounds):
        for which in ((0, 1, 2), (2, 1, 0))[r % 2]:
            if which == 0:
                ta += block(call_a, args.launches)
            elif which == 1:
                tb += block(call_b, args.launches)
            else:
                tbl += block(lambda: call_b(True), args.launches)
    assert codec.device_error() == 0

    tc, td = [], []
    for r in range(args.host_reps):
        for fn, acc in ((call_c, tc), (call_d, td))[::1 if r % 2 else -1]:
            t0 = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t0) * 1e6)
    med = lambda v: float(np.median(v))
    res = {
        "tool": "wire_bench", "n": n, "wire_bytes": int(woo[-1]),
        "payload_bytes": hb, "decoded_bytes": int(oo_d[-1]),
        "huffman_share": round(huff_share, 4),
        "launches_each": len(ta), "host_calls_each": len(tc),
        "a_decode_wire_us": round(med(ta), 2),
        "b_decode_batch_us": round(med(tb), 2),
        "b_lean_decode_batch_us": round(med(tbl), 2),
        "a_over_b": round(med(ta) / med(tb), 3),
        "a_min_us": round(min(ta), 2), "b_min_us": round(min(tb), 2),
        "c_decode_wire_host_us": round(med(tc), 1),
        "d_decode_literals_ex_us": round(med(td), 1),
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
