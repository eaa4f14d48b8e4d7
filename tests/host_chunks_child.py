"""Helper of test_host_chunks.py; not a test module.

The host path (host_batch, qhuff_hostpath.cpp) cuts a batch into one chunk
per 2^QHUFF_HOST_CHUNK_SHIFT bytes of input, and reads that shift once per
process.  With shift 16 every branch of its pipeline is reached by batches of
128 KB to 1.2 MB, but only in a process started with the variable set.  This
file holds

  * the shapes: batches defined by the input bytes of every string, so that
    the chunk plan (qhuff_host_chunks) of each is known in advance and is
    the same for encode (token bytes) and decode (Huffman bytes);
  * the case lists of the three child configurations;
  * run as a program (`host_chunks_child.py LIST SHIFT OUT`), the child
    itself: every case of the list as one host-memory call inside a guarded,
    dirty arena (test_buffer_contract.Arena), one JSON record a case written
    to OUT: return code, the SHA-256 of the output bytes, of out_off and of
    the statuses, the stray writes, the device error word.  The parent
    compares the digests with the CPU oracle's; the child computes no
    expectation.

A case that returns an error ends the child (exit status 3): nothing more is
started on a device that may have faulted."""
import functools
import hashlib
import json
import os
import sys
import time

import numpy as np

import _paths  # noqa: F401
import oracle_lib as O
import qhuff

C16 = 1 << 16               # a chunk at shift 16
C21 = 1 << 21               # a chunk at shift 21
HIGH = 0xF0000000
SLICE = 1 << 16             # strings per slice of the out_off rebase
TOKEN = np.frombuffer(qhuff.TOKEN_ALPHABET, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def six_bit_alphabet():
    """the token characters whose Huffman code has 6 bits: k of them encode
    to exactly ceil(6 k / 8) bytes"""
    a = np.array([c for c in qhuff.TOKEN_ALPHABET if O.code_of(c)[1] == 6],
                 dtype=np.uint8)
    assert len(a) >= 16
    return a


def spread(total, n, seed):
    """n lengths that sum to `total`: total / n each, neighbours moved apart
    by up to 20 bytes"""
    base, rem = divmod(int(total), n)
    ln = np.full(n, base, dtype=np.int64)
    ln[:rem] += 1
    j = min(base, 20)
    if j and n >= 2:
        d = np.random.default_rng(seed).integers(0, j + 1, n // 2)
        ln[0:2 * (n // 2):2] += d
        ln[1:2 * (n // 2):2] -= d
    assert ln.sum() == total and ln.min() >= 0
    return ln


def offsets(lens):
    off = np.zeros(len(lens) + 1, dtype=np.uint32)
    np.cumsum(lens, out=off[1:])
    return off


class Shape:
    """lens: the input bytes of every string, for encode and decode alike.
    back: in_off[0] (`in` points `back` bytes below the first string).
    garbage: a string range of the decode input made of 0xFF bytes.
    corrupt: every corrupt-th string of the decode input has its last byte
    inverted."""

    def __init__(self, name, lens, seed, shift=16, back=0, garbage=None,
                 corrupt=0):
        self.name, self.lens, self.seed = name, np.asarray(lens, np.int64), seed
        self.shift, self.back = shift, back
        self.garbage, self.corrupt = garbage, corrupt
        self.n = len(self.lens)
        self.in_bytes = int(self.lens.sum())
        self.off = offsets(self.lens)
        self._in = {}

    def inputs(self, op):
        """(data, off): off starts at 0 whatever `back` is"""
        k = "dec" if op == "dec" else "enc"
        if k not in self._in:
            rng = np.random.default_rng(self.seed)
            if k == "enc":
                data = TOKEN[rng.integers(0, len(TOKEN), self.in_bytes)]
            else:
                a = six_bit_alphabet()
                raw_off = offsets(8 * self.lens // 6)
                raw = a[rng.integers(0, len(a), int(raw_off[-1]))]
                data, off = O.encode_batch(raw, raw_off, 0)
                assert np.array_equal(off, self.off), self.name
                data = data.copy()
                if self.garbage:
                    a0, a1 = self.garbage
                    data[self.off[a0]:self.off[a1]] = 0xFF
                if self.corrupt:
                    idx = np.arange(0, self.n, self.corrupt)
                    idx = idx[self.lens[idx] > 0]
                    data[self.off[idx + 1] - 1] ^= 0xFF
            assert len(data) == self.in_bytes
            self._in[k] = np.ascontiguousarray(data)
        return self._in[k], self.off

    def call_off(self):
        """the offsets the call is given"""
        return (self.off.astype(np.int64) + self.back).astype(np.uint32)


def _uniform(name, total, n, seed, **kw):
    return Shape(name, spread(total, n, seed), seed, **kw)


def _empty_chunk(name, j, seed):
    """four chunks of 1001 strings; chunk j holds only empty strings"""
    m = 1001
    lens = np.zeros(4 * m, dtype=np.int64)
    rest = np.ones(4 * m, dtype=bool)
    rest[j * m:(j + 1) * m] = False
    lens[rest] = spread(4 * C16 + 77, 3 * m, seed)
    return Shape(name, lens, seed)


def _skewed():
    """nine chunks of 1000 strings; the first holds 90 % of the bytes"""
    total, m = 9 * C16 + 100, 1000
    head = total * 9 // 10
    lens = np.concatenate([spread(head, m, 81), spread(total - head, 8 * m, 82)])
    return Shape("skewed", lens, 8)


def _sparse():
    """200,000 strings, every 61st of 40 bytes, the others empty"""
    lens = np.zeros(200_000, dtype=np.int64)
    lens[30::61] = 40
    return Shape("sparse", lens, 9)


SMALL = 4 << 20            # host_batch: `small` up to this output bound


def up16(x):
    return (x + 15) & ~15


def bound_of(op, in_bytes, n):
    return (qhuff.decode_bound(in_bytes, n) if op == "dec"
            else qhuff.encode_bound(in_bytes, n, op))


def edge_bytes(op, n, past):
    """the most input bytes of n strings whose output bound, rounded up to
    16, is still 4 MB -- or (past) one byte more, whose rounded bound is
    4 MB + 16: from qhuff_encode_bound / qhuff_decode_bound"""
    lo, hi = 0, SMALL
    while lo < hi:                       # the last x with up16(bound) <= 4 MB
        mid = (lo + hi + 1) // 2
        if up16(bound_of(op, mid, n)) <= SMALL:
            lo = mid
        else:
            hi = mid - 1
    assert up16(bound_of(op, lo, n)) == SMALL
    assert up16(bound_of(op, lo + 1, n)) == SMALL + 16
    return lo + 1 if past else lo


def _edge(name, op, n, past):
    return _uniform(name, edge_bytes(op, n, past), n, 19 + past, shift=23)


BUILDERS = {
    # the last one-chunk (and small) call, the first two-chunk call
    "k1_top": lambda: _uniform("k1_top", 2 * C16 - 1, 3001, 1),
    "k2_bottom": lambda: _uniform("k2_bottom", 2 * C16, 3001, 2),
    # 15 chunks, 16 chunks, 17 chunks' worth capped at 16; n prime, so that
    # n * i / K is ragged
    "k15_top": lambda: _uniform("k15_top", 16 * C16 - 1, 24001, 3),
    "k16": lambda: _uniform("k16", 16 * C16, 24007, 4),
    "k16_capped": lambda: _uniform("k16_capped", 17 * C16 + 1, 25013, 5),
    # more chunks' worth of bytes than strings
    "clamp_n2": lambda: Shape("clamp_n2", [3 * C16, 3 * C16], 6),
    "clamp_n1": lambda: Shape("clamp_n1", [2 * C16], 7),
    "empty_first": lambda: _empty_chunk("empty_first", 0, 10),
    "empty_mid": lambda: _empty_chunk("empty_mid", 2, 11),
    "empty_last": lambda: _empty_chunk("empty_last", 3, 12),
    # decode: the middle chunk of three is rejected throughout
    "all_error_chunk": lambda: Shape(
        "all_error_chunk", spread(3 * C16 + 1000, 4500, 13), 13,
        garbage=(1500, 3000)),
    "skewed": _skewed,
    "sparse": _sparse,
    "offset5": lambda: _uniform("offset5", 3 * C16 + 5, 2003, 14, back=5),
    "high_offset": lambda: _uniform("high_offset", 3 * C16 + 5, 2003, 15,
                                    back=HIGH),
    "corrupt1pc": lambda: Shape("corrupt1pc", spread(4 * C16 + 9, 6007, 16),
                                16, corrupt=97),
    # shift 21: chunk copies past the copy pool's 1 MB slice
    "big4": lambda: _uniform("big4", 4 * C21, 200_003, 17, shift=21),
    "big5": lambda: _uniform("big5", 5 * C21 + 1, 250_007, 18, shift=21),
    # the default shift: either side of the 4 MB `small` threshold
    "edge_enc_small": lambda: _edge("edge_enc_small", 0, 30_011, False),
    "edge_enc_past": lambda: _edge("edge_enc_past", 0, 30_011, True),
    "edge_dec_small": lambda: _edge("edge_dec_small", "dec", 60_013, False),
    "edge_dec_past": lambda: _edge("edge_dec_past", "dec", 60_013, True),
}
SHIFT16 = [s for s in BUILDERS if s[:3] not in ("big", "edg")]
EDGES = [s for s in BUILDERS if s.startswith("edge")]
MULTI = ["k16_capped", "skewed", "empty_mid", "clamp_n2"]


@functools.lru_cache(maxsize=None)
def shape(name):
    return BUILDERS[name]()


# ---- the case lists ----------------------------------------------------------
#
# A case is "shape/op/variant".  Variants: staged; reg_in, reg_out, reg_both
# (exactly those buffers registered); registered_too_small (everything
# registered, `out` over half its bound only: it is staged); m2_staged .. m3_reg (the
# *_host_multi call over 2 or 3 contexts, nothing or everything registered).

def ops_of(name):
    """decode-only shapes; the large ones skip mode 7"""
    return {"all_error_chunk": ("dec",), "corrupt1pc": ("dec",),
            "big4": (0, "dec"), "big5": (0, "dec"),
            "edge_enc_small": (0,), "edge_enc_past": (0,),
            "edge_dec_small": ("dec",), "edge_dec_past": ("dec",),
            }.get(name, (0, 7, "dec"))


def _cases(names, variants):
    return ["%s/%s/%s" % (s, op, v) for s in names for op in ops_of(s)
            for v in variants]


SINGLE = ("staged", "reg_in", "reg_out", "reg_both")
ALL_BUFFERS = ("in", "in_off", "out", "out_off", "status")
REGISTERED = {"staged": (), "reg_in": ("in", "in_off"),
              "reg_out": ("out", "out_off", "status"),
              "reg_both": ALL_BUFFERS, "registered_too_small": ALL_BUFFERS,
              "reg": ALL_BUFFERS}
LISTS = {
    # (shift 16, default copy threads)
    "c16": _cases(SHIFT16, SINGLE) + ["k16/dec/registered_too_small"]
    + _cases(MULTI, ("m2_staged", "m2_reg", "m3_staged", "m3_reg")),
    # (shift 16, QHUFF_HOST_THREADS=1: no pool, CopyPool::run runs inline)
    "c16_t1": _cases(SHIFT16, ("staged",))
    + _cases(MULTI, ("m2_staged", "m3_staged")),
    # (shift 21, 3 copy threads: the staging memcpy is split)
    "c21_t3": _cases(["big4", "big5"], ("staged",)),
}
CONFIGS = [("c16", 16, None), ("c16_t1", 16, 1), ("c21_t3", 21, 3)]


def parse(case):
    name, op, variant = case.split("/")
    return shape(name), (op if op == "dec" else int(op)), variant


# ---- the child ---------------------------------------------------------------

def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(case, k, codecs):
    """one call in one arena -> its record"""
    import test_buffer_contract as B
    s, op, variant = parse(case)
    data, _ = s.inputs(op)
    off = s.call_off()
    n = s.n
    multi = codecs[:int(variant[1])] if variant[0] == "m" else None
    reg = REGISTERED[variant.split("_", 1)[1] if multi else variant]
    r_in, r_out = ((5, 11), (13, 2), (8, 7))[k % 3]
    specs = B.codec_specs(op, s.in_bytes, n, r_in, r_out, k)
    ar = B.Arena(specs, seed=9000 + k, guard=8192 if reg else B.GUARD)
    ar.put("in", data)
    ar.put("in_off", off)
    ar.commit(False)
    views = []
    for nm in reg:
        if nm in ar.reg and ar.reg[nm][1]:
            v = ar.view(nm)
            views.append(v[:len(v) // 2] if variant == "registered_too_small"
                         and nm == "out" else v)
    t0 = time.perf_counter()
    with qhuff.registered(*views):
        rc = B.host_codec_call(qhuff.lib(), codecs[0]._ctx, op, ar, n, s.back,
                               multi)
    secs = time.perf_counter() - t0
    rec = {"id": case, "rc": int(rc), "secs": round(secs, 4)}
    rec["dev_err"] = [c.device_error() for c in (multi or codecs[:1])]
    if rc != qhuff.OK:
        return rec
    img = ar.after()
    oo = ar.get(img, "out_off", np.uint32)
    total = int(oo[-1])
    rec["total"] = total
    rec["off"] = digest(oo)
    written = {"out_off": 4 * (n + 1)}
    if total <= ar.reg["out"][1]:
        rec["out"] = digest(ar.get(img, "out", count=total))
        written["out"] = total
    if op == "dec":
        rec["status"] = digest(ar.get(img, "status"))
        written["status"] = n
    bad = B.violations(ar.before, img, ar.reg, written, ar.guard)
    rec["stray"] = len(bad)
    rec["stray_first"] = [list(map(str, b)) for b in bad[:8]]
    return rec


def main(argv):
    which, shift, out_path = argv[1], int(argv[2]), argv[3]
    with open(out_path, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
        # first: this process cuts by the shift it was started for
        probe = offsets(spread((5 << shift) + 1, 640, 0))
        own = qhuff.host_chunks(probe, True, 0, 0)
        explicit = qhuff.host_chunks(probe, True, 0, shift)
        ok = own == explicit and len(own[0]) - 1 == 5
        emit({"id": "_shift", "rc": 0 if ok else 1, "own": own[0],
              "explicit": explicit[0],
              "threads": os.environ.get("QHUFF_HOST_THREADS")})
        if not ok:
            return 2
        codecs = [qhuff.Codec(0) for _ in range(3)]
        try:
            for k, case in enumerate(LISTS[which]):
                rec = run_case(case, k, codecs)
                emit(rec)
                if rec["rc"] or any(rec["dev_err"]):
                    return 3
        finally:
            for c in codecs:
                c.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
