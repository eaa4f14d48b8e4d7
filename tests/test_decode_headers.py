"""qhuff_scan_headers / qhuff_decode_headers and their host forms: field
sections decoded to header lists against the static table (include/qhuff.h),
the inverse of qhuff_encode_headers.

Expectations: tests/headers_decode_model.py (the reference's framing rules,
its static table and the CPU oracle's Huffman decoder), never the library.
The model itself is pinned to the reference's own vectors
(tests/golden/kat_header_blocks.json) and to headers_model, the encoder's.

CPU half: qhuff_scan_headers_cpu, the kernels' walker source on the host, and
a stand-alone program (tests/c/hdrscan_san.cpp + qhuff_frames.cpp, g++ with
ASan/UBSan).  GPU half: the device-pointer calls at data residues 0, 1 and 15
and the one-call host form."""
import ctypes as C
import functools
import json
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

import _paths  # noqa: F401
import headers_decode_model as D
import headers_model as M
import limits as L
import oracle_lib as O
import qhuff
import qpack_frames as Q
import scan_cases as S
from test_buffer_contract import FILLS, Arena
from test_encode_headers import SHAPES, corpus, shape

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = os.path.join(HERE, "golden")
MAXS = qhuff.MAX_STRLEN

FIELD_CASES = ("interop_sections", "fuzz_as_sections", "kat_blocks",
               "every_prefix_sections", "kat_int_sections", "int24_sections",
               "nonminimal_sections", "declared_sections", "alloc_clamp",
               "five_byte_sections", "skewed", "long_value", "havoc_sections")


# ---- building sections ------------------------------------------------------------

def indexed(i):
    return Q.enc_int(0xC0, i, 6)


def nameref(i, value, huffman=0, never=0):
    """value: the payload bytes as they go on the wire"""
    return Q.enc_int(0x50 | never << 5, i, 4) + S.lit(0, 7, value, huffman)


def literal(name, value, nh=0, vh=0, never=0):
    return S.lit(0x20 | never << 4, 3, name, nh) + S.lit(0, 7, value, vh)


def sec(*lines):
    return b"\0\0" + b"".join(lines)


def ordinary(rng, k):
    """k header lines of all three kinds with short token strings, Huffman
    and raw"""
    out = []
    for _ in range(k):
        s = bytes(rng.choice(L.TOKEN) for _ in range(rng.randint(1, 30)))
        n = bytes(rng.choice(L.TOKEN) for _ in range(rng.randint(1, 12)))
        x = rng.randrange(5)
        if x == 0:
            out.append(indexed(rng.randrange(99)))
        elif x == 1:
            out.append(nameref(rng.randrange(99), s, 0, rng.randrange(2)))
        elif x == 2:
            out.append(nameref(rng.randrange(99), O.huffman_enc(s), 1))
        elif x == 3:
            out.append(literal(n, O.huffman_enc(s), 0, 1, rng.randrange(2)))
        else:
            out.append(literal(O.huffman_enc(n), s, 1, 0))
    return out


@functools.lru_cache(maxsize=None)
def kat():
    with open(os.path.join(G, "kat_header_blocks.json")) as f:
        return json.load(f)["header_blocks"]


def kat_sections():
    return [bytes.fromhex(k["prefix"] + k["header"]) for k in kat()]


# ---- the model, pinned ----------------------------------------------------------------

def test_model_reference_vectors():
    """test_qpack.c:47, :64, :83, :129, :150 decode to their `headers` (:64
    and :129 with N = 1); :107 and :195 (prefix 0280) need the dynamic table"""
    seen = {}
    for k in kat():
        ln = k["source"].rsplit(":", 1)[1]
        rc, lines = D.section(bytes.fromhex(k["prefix"] + k["header"]))
        d = D.Decoded([bytes.fromhex(k["prefix"] + k["header"])])
        seen[ln] = rc
        if ln in ("107", "195"):
            assert k["prefix"] == "0280" and rc == D.ENOTSUP and d.n == 0
            continue
        want = [(bytes.fromhex(n), bytes.fromhex(v)) for n, v in k["headers"]]
        assert rc == D.OK and d.headers == want, ln
        assert not d.status.any()
        assert d.hflags.tolist() == [1 if ln in ("64", "129") else 0] * d.n
    assert seen == {"47": 0, "64": 0, "83": 0, "107": D.ENOTSUP, "129": 0,
                    "150": 0, "195": D.ENOTSUP}


@pytest.mark.parametrize("name", SHAPES)
def test_model_inverts_the_encoders_model(name):
    """decoding headers_model's bytes gives back its header list, the kinds,
    the static ids and the N bits"""
    h = shape(name)
    d = D.Decoded(h.want_sections)
    assert not d.rc.any() and not d.status.any()
    assert np.array_equal(d.hdr_off, h.sec_hdr)
    assert d.data == h.data.tobytes() and np.array_equal(d.off, h.off)
    assert np.array_equal(d.kind, h.want_kind)
    assert np.array_equal(d.static_id, h.want_id)
    fl = h.hflags if h.hflags is not None else np.zeros(h.n, np.uint8)
    # (an indexed line carries no N bit)
    assert np.array_equal(d.hflags, (fl & 1) * (h.want_kind != M.INDEXED))
    assert len(d.data) <= d.bound


def test_abi():
    with open(qhuff.HEADER) as f:
        hdr = f.read()
    for text in ("#define QHUFF_FEATURE_DECODE_HEADERS 1",
                 "#define QHUFF_ENOTSUP   (-95)", "#define QHUFF_HSTR_WIRE   0",
                 "#define QHUFF_HSTR_STATIC 1", "#define QHUFF_ABI_VERSION 7"):
        assert text in hdr
    assert (qhuff.ENOTSUP, qhuff.HSTR_WIRE, qhuff.HSTR_STATIC) == (-95, 0, 1)
    assert C.sizeof(qhuff.Hstr) == 16 == D.HSTR.itemsize
    Lb = qhuff.lib()
    for name in ("qhuff_scan_headers", "qhuff_scan_headers_host",
                 "qhuff_scan_headers_cpu", "qhuff_decode_headers",
                 "qhuff_decode_headers_host", "qhuff_decode_headers_bound"):
        assert getattr(Lb, name) and name in qhuff.EXPORTS
    for wire, n in ((0, 0), (1, 1), (4096, 64), (1 << 30, 9)):
        assert qhuff.decode_headers_bound(wire, n) == D.bound(wire, n)
    assert Lb.qhuff_abi_version() == 7


# ---- CPU: the walker through qhuff_scan_headers_cpu -------------------------------------

def check_scan(d, got, max_hdrs=None):
    ret, strs, hdr_off, rc, kind, sid, hf = got
    cap = d.n if max_hdrs is None else max_hdrs
    n = min(d.n, cap)
    assert ret == (qhuff.ERANGE if d.n > cap else qhuff.OK)
    assert np.array_equal(rc, d.rc)
    assert np.array_equal(hdr_off, d.hdr_off)
    assert np.array_equal(strs, d.str_bytes(cap))
    assert np.array_equal(kind, d.kind[:n])
    assert np.array_equal(sid, d.static_id[:n])
    assert np.array_equal(hf, d.hflags[:n])


def cpu(d, max_hdrs=None):
    buf = np.frombuffer(bytes(d.a0) + d.wire, dtype=np.uint8)
    got = qhuff.scan_headers_cpu(buf, d.sec_off,
                                 d.n if max_hdrs is None else max_hdrs)
    check_scan(d, got, max_hdrs)
    return got


def test_cpu_reference_vectors():
    d = D.Decoded(kat_sections(), a0=3)
    assert d.rc.tolist() == [0, 0, 0, D.ENOTSUP, 0, 0, D.ENOTSUP]
    cpu(d)
    for s in kat_sections():
        cpu(D.Decoded([s]))


@pytest.mark.parametrize("name", FIELD_CASES)
def test_cpu_scan_cases(name):
    mode, chunks = S.CASES[name]()
    assert mode == S.FIELD
    d = D.Decoded(chunks)
    cpu(d)
    if name == "interop_sections":
        # (encoded against a dynamic table: all but three static-only ones)
        ric = [Q.dec_int(c, 0, 8)[0] for c in chunks]
        assert all(r == D.ENOTSUP for r, x in zip(d.rc, ric) if x)
        assert (d.rc == D.ENOTSUP).sum() >= 30
    if name in ("fuzz_as_sections", "havoc_sections"):
        # a framing error stays what the host scanner says it is
        host = np.array([S.model(S.FIELD, c)[0] for c in chunks])
        assert np.array_equal(d.rc[host != 0], host[host != 0])
        assert set(d.rc.tolist()) >= {0, qhuff.ETRUNC, qhuff.EPROTO, D.ENOTSUP}


def every_static_id_sections():
    """every id as an indexed line and as a name reference: a section an id,
    then all the indexed lines in one section and all the name references in
    another"""
    secs = [sec(indexed(i), nameref(i, b"v%d" % i, 0, i & 1))
            for i in range(99)]
    return secs + [sec(*[indexed(i) for i in range(99)]),
                   sec(*[nameref(i, b"") for i in range(99)])]


def test_cpu_every_static_id():
    """every id as an indexed line and as a name reference, and the ids on
    each side of the prefix integers' boundaries"""
    d = D.Decoded(every_static_id_sections())
    assert not d.rc.any() and d.n == 4 * 99
    assert d.static_id[:8].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    cpu(d)
    for i in (62, 63):
        assert len(indexed(i)) == (1 if i < 63 else 2)
    for i in (14, 15, 16):
        assert len(Q.enc_int(0x50, i, 4)) == (1 if i < 15 else 2)
    hs = D.Decoded([sec(indexed(62), indexed(63), nameref(14, b"a"),
                        nameref(15, b"b"), nameref(16, b"c"))])
    assert hs.static_id.tolist() == [62, 63, 14, 15, 16]
    assert hs.headers[1] == D.STATIC[63] and hs.headers[3][0] == D.STATIC[15][0]
    cpu(hs)


def bad_static_id_sections():
    """ids 98, 99, 100, 2^24 - 1 and 2^24: indexed, as a name reference, and
    between two good lines"""
    secs = []
    for i in (98, 99, 100, (1 << 24) - 1, 1 << 24):
        secs += [sec(indexed(i)), sec(nameref(i, b"x")),
                 sec(indexed(1), nameref(i, b"x"), indexed(2))]
    return secs


def test_cpu_bad_static_ids():
    """ids 99, 100 and 2^24 - 1 are QHUFF_EPROTO, 2^24 the integer's own"""
    d = D.Decoded(bad_static_id_sections())
    assert d.rc.tolist() == [0] * 3 + [qhuff.EPROTO] * 12
    assert d.n == 5
    cpu(d)


DYNAMIC = {
    "indexed_t0": Q.enc_int(0x80, 3, 6),
    "nameref_t0": Q.enc_int(0x40, 3, 4) + S.lit(0, 7, b"v"),
    "indexed_post_base": Q.enc_int(0x10, 0, 4),
    "nameref_post_base": Q.enc_int(0x00, 0, 3) + S.lit(0, 7, b"v"),
}


def dynamic_form_sections():
    """each dynamic form alone, between two good lines and behind one; then
    RIC != 0 with static-only lines, and a Delta Base with its sign set
    under RIC = 0 (read and ignored)"""
    secs = []
    for form in DYNAMIC.values():
        secs += [b"\0\0" + form, sec(indexed(1), form, indexed(2)),
                 sec(literal(b"n", b"v"), form)]
    return secs + [b"\x01\x00" + indexed(17), b"\x05\x83" + nameref(1, b"/x"),
                   b"\x00\x80" + indexed(17), b"\x00\xff\x05" + indexed(17)]


def test_cpu_dynamic_forms():
    d = D.Decoded(dynamic_form_sections())
    assert d.rc.tolist() == [D.ENOTSUP] * 14 + [0, 0]
    assert d.headers == [D.STATIC[17]] * 2
    cpu(d)


TRUNC = nameref(1, b"abc")[:-1]                  # ends inside the value
PROTO = b"\xff" + b"\xff" * 10 + b"\x7f"         # an integer past 64 bits


def rc_order_cases():
    """[(section, its rc)]: one section for each pair of the order's clauses"""
    trunc, proto = TRUNC, PROTO
    notsup = DYNAMIC["indexed_t0"]
    bad = indexed(99)
    E = qhuff
    return [
        (sec(notsup, trunc), E.ETRUNC), (sec(bad, trunc), E.ETRUNC),
        (sec(notsup, proto), E.EPROTO), (sec(bad, proto), E.EPROTO),
        (b"\x01\x00" + trunc, E.ETRUNC), (b"\x01\x00" + proto, E.EPROTO),
        (sec(notsup, bad), D.ENOTSUP), (sec(bad, notsup), D.ENOTSUP),
        (b"\x01\x00" + bad, D.ENOTSUP),
        (sec(bad), E.EPROTO), (sec(indexed(1), bad, indexed(2)), E.EPROTO),
        (sec(indexed(1)), E.OK),
        # a declared length past QHUFF_MAX_STRLEN: the scanner's EPROTO
        (sec(notsup, b"\x51" + Q.enc_int(0, 65536, 7)), E.EPROTO),
        (b"\0", E.ETRUNC), (b"", E.ETRUNC), (b"\0\0", E.OK),
    ]


def test_cpu_rc_order():
    """one section for each pair of the order's clauses: the earlier wins
    wherever in the section each cause lies"""
    cases = rc_order_cases()
    d = D.Decoded([c for c, _ in cases])
    assert d.rc.tolist() == [r for _, r in cases]
    cpu(d)


@pytest.mark.parametrize("m", S.COUNTS)
def test_cpu_counts(m):
    d = D.Decoded(S.counted(m)[1])
    assert d.m == m
    cpu(d)


def test_cpu_max_hdrs():
    """max_hdrs at 0, in the middle of a section and at the count; the
    optional arrays NULL; argument errors"""
    rng = random.Random(5)
    d = D.Decoded([sec(*ordinary(rng, 7)), sec(), sec(*ordinary(rng, 9)),
                   b"\0", sec(*ordinary(rng, 4))], a0=5)
    assert d.hdr_off.tolist() == [0, 7, 7, 16, 16, 20]
    for cap in (0, 1, 7, 11, 16, 19, 20, 21):
        cpu(d, cap)
    Lb = qhuff.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    buf = np.frombuffer(bytes(d.a0) + d.wire, dtype=np.uint8)
    strs = np.full(32 * d.n + 8, 0xA5, np.uint8)
    ho, rc = np.zeros(d.m + 1, np.uint32), np.zeros(d.m, np.int32)
    assert Lb.qhuff_scan_headers_cpu(p(buf), p(d.sec_off), d.m, p(strs), d.n,
                                     p(ho), p(rc), None, None, None) == 0
    assert np.array_equal(strs[:32 * d.n], d.str_bytes())
    assert (strs[32 * d.n:] == 0xA5).all()
    E = qhuff.EINVAL
    assert Lb.qhuff_scan_headers_cpu(None, p(d.sec_off), d.m, p(strs), d.n,
                                     p(ho), p(rc), None, None, None) == E
    assert Lb.qhuff_scan_headers_cpu(p(buf), None, d.m, p(strs), d.n, p(ho),
                                     p(rc), None, None, None) == E
    assert Lb.qhuff_scan_headers_cpu(p(buf), p(d.sec_off), d.m, None, d.n,
                                     p(ho), p(rc), None, None, None) == E
    assert Lb.qhuff_scan_headers_cpu(p(buf), p(d.sec_off), d.m, p(strs), d.n,
                                     None, p(rc), None, None, None) == E
    assert Lb.qhuff_scan_headers_cpu(p(buf), p(d.sec_off), d.m, p(strs), d.n,
                                     p(ho), None, None, None, None) == E
    bad = d.sec_off.copy()
    bad[2] = bad[1] - 1
    assert Lb.qhuff_scan_headers_cpu(p(buf), p(bad), d.m, p(strs), d.n, p(ho),
                                     p(rc), None, None, None) == E
    # m = 0: hdr_off[0] alone
    ho[:] = 7
    assert Lb.qhuff_scan_headers_cpu(None, None, 0, None, 0, p(ho), None,
                                     None, None, None) == 0
    assert ho.tolist() == [0] + [7] * d.m


def _san_files(tmp_path, name, chunks):
    d = D.Decoded(chunks)
    rec, exp = str(tmp_path / (name + ".rec")), str(tmp_path / (name + ".exp"))
    with open(rec, "wb") as f:
        for c in chunks:
            f.write(struct.pack("<I", len(c)) + c)
    with open(exp, "wb") as f:
        f.write(struct.pack("<II", d.m, d.n) + d.rc.tobytes()
                + d.hdr_off.tobytes() + d.str_bytes().tobytes()
                + d.kind.tobytes() + d.static_id.tobytes()
                + d.hflags.tobytes())
    return [rec, exp], d


def test_cpu_walker_under_sanitizers(tmp_path):
    """tests/c/hdrscan_san.cpp with its own main, g++ ASan + UBSan, run as a
    child process in the inherited environment: the fuzz corpora and a seeded
    havoc of the model's own sections, packed with no padding in
    exactly-sized heap buffers"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the sanitizer build"
    exe = str(tmp_path / "hdrscan_san")
    subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-o", exe,
         os.path.join(HERE, "c", "hdrscan_san.cpp"),
         os.path.join(ROOT, "ls-qpack_amd", "csrc", "qhuff_frames.cpp")],
        check=True, timeout=300)
    own = shape("boundaries").want_sections + shape("empties").want_sections \
        + kat_sections() + [sec(*[indexed(i) for i in range(99)])]
    sets = {"fuzz": S.fuzz_payloads(), "own": own,
            "havoc": S.havoc(own, 3000, 47)}
    args, total = [], 0
    for name, chunks in sets.items():
        a, d = _san_files(tmp_path, name, chunks)
        args += a
        total += d.n
        if name == "havoc":
            assert set(d.rc.tolist()) >= {0, qhuff.ETRUNC, qhuff.EPROTO,
                                          D.ENOTSUP}
    assert total > 3000
    r = subprocess.run([exe] + args, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(r.stdout.strip().split("\n")) == len(sets)


# ---- GPU ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def codec():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    c = qhuff.Codec(0)
    yield c
    c.close()


def dev(a, pad=0):
    import torch
    a = np.array(a).view(np.uint8).reshape(-1)       # (a writable copy)
    t = torch.zeros(len(a) + pad + 16, dtype=torch.uint8, device="cuda")
    if len(a):
        t[pad:pad + len(a)] = torch.from_numpy(a).cuda()
    return t


def dev_i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def run_device(codec, d, max_len=MAXS, stream=None):
    """scan + decode on device pointers; d.a0 is the data's residue"""
    buf = dev(np.frombuffer(d.wire, dtype=np.uint8), d.a0)
    so = dev_i32(d.sec_off)
    scan = codec.scan_headers(buf, so, d.n, stream)
    dec = codec.decode_headers(buf, scan[0], d.n, max_len, stream,
                               wire_bytes=len(d.wire))
    return scan, dec, (buf, so)


def fetch_device(d, res):
    (strs, hdr_off, rc, kind, sid, hf), (out, off, st), _ = res
    off = off.cpu().numpy().view(np.uint32)
    n = d.n
    return ((qhuff.OK, strs.cpu().numpy()[:32 * n],
             hdr_off.cpu().numpy().view(np.uint32), rc.cpu().numpy(),
             kind.cpu().numpy()[:n], sid.cpu().numpy()[:n],
             hf.cpu().numpy()[:n]),
            (out[:int(off[-1])].cpu().numpy().tobytes(), off,
             st.cpu().numpy()))


def check_decode(d, got):
    out, off, st = got
    assert np.array_equal(off, d.off)
    assert np.array_equal(st, d.status)
    assert bytes(out) == d.data


def check_host(codec, sections, max_len=MAXS, also=()):
    """qhuff_decode_headers_host with hashes, and qhuff_scan_headers_host,
    against the model; the reference's hashes of the first and the last
    headers and of those with an index in `also`"""
    d = D.Decoded(sections, max_len)
    wire = np.frombuffer(d.wire, dtype=np.uint8)
    ret, hdr_off, rc, kind, sid, hf, out, off, st, h1, h2 = \
        codec.decode_headers_host(wire, d.sec_off, max_len, d.n, hashes=True)
    assert ret == qhuff.OK
    assert np.array_equal(rc, d.rc) and np.array_equal(hdr_off, d.hdr_off)
    assert np.array_equal(kind, d.kind) and np.array_equal(sid, d.static_id)
    assert np.array_equal(hf, d.hflags)
    check_decode(d, (out.tobytes(), off, st))
    # the hashes: qhuff_xxh32_headers_host on the call's own output, and the
    # reference's XXH32 of every header
    g1, g2 = codec.xxh32_headers_host(np.concatenate([out, np.zeros(16, np.uint8)]),
                                      off)
    assert np.array_equal(h1, g1) and np.array_equal(h2, g2)
    hd = d.headers
    for i in sorted(set(range(min(d.n, 40))) | set(range(max(d.n - 8, 0), d.n))
                    | set(also)):
        assert (int(h1[i]), int(h2[i])) == M.hashes(*hd[i]), i
    # and the scan's host form
    check_scan(d, codec.scan_headers_host(wire, d.sec_off, d.n))
    return d


def check_both(codec, sections, max_len=MAXS, pads=(0, 1, 15)):
    import torch
    for pad in pads:
        d = D.Decoded(sections, max_len, a0=pad)
        res = run_device(codec, d, max_len)
        torch.cuda.synchronize()
        assert codec.device_error() == 0
        scan, dec = fetch_device(d, res)
        check_scan(d, scan)
        check_decode(d, dec)
    return check_host(codec, sections, max_len)


@pytest.mark.gpu
def test_reference_vectors(codec):
    d = check_both(codec, kat_sections())
    assert d.rc.tolist() == [0, 0, 0, D.ENOTSUP, 0, 0, D.ENOTSUP]
    for s in kat_sections():
        check_both(codec, [s], pads=(0,))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHAPES)
def test_round_trip_shapes(codec, name):
    """qhuff_encode_headers_host and back: equal arrays"""
    h = shape(name)
    out, so, kind, sid = codec.encode_headers_host(h.data, h.off, h.sec_hdr,
                                                   h.hflags)
    assert out.tobytes() == h.want
    secs = [out[so[i]:so[i + 1]].tobytes() for i in range(h.m)]
    d = check_both(codec, secs)
    assert d.data == h.data.tobytes() and np.array_equal(d.off, h.off)
    assert np.array_equal(d.hdr_off, h.sec_hdr)
    assert np.array_equal(d.kind, kind) and np.array_equal(d.static_id, sid)


@pytest.mark.gpu
def test_round_trip_qif(codec):
    """the QIF header lists, one section a list: encoded, and decoded back to
    the whole header lists, names and static strings included"""
    h = corpus()
    out, so, kind, sid = codec.encode_headers_host(h.data, h.off, h.sec_hdr)
    secs = [out[so[i]:so[i + 1]].tobytes() for i in range(h.m)]
    d = check_both(codec, secs, pads=(0, 15))
    assert d.data == h.data.tobytes() and np.array_equal(d.off, h.off)
    assert np.array_equal(d.hdr_off, h.sec_hdr)
    assert np.array_equal(d.kind, kind) and np.array_equal(d.static_id, sid)
    paths = D.layout(d)
    assert any(not p["fast"] for p in paths) and any(p["fast"] for p in paths)
    assert any(not p["fixed"] for p in paths) and any(p["fixed"] for p in paths)


# ---- tile edges ---------------------------------------------------------------

LONG_VAL, LONG_NAME = 85, 73     # the 53-byte value; a 32-byte name
assert len(D.STATIC[LONG_VAL][1]) == 53 and len(D.STATIC[LONG_NAME][0]) == 32


def one_tile(d, residue=0):
    p = D.layout(d, residue)
    assert len(p) == 1
    return p[0]


@pytest.mark.gpu
def test_wire_free_tiles(codec):
    """a tile of 32 indexed lines has no wire bytes: alone, and between
    ordinary tiles"""
    rng = random.Random(11)
    free = [indexed(rng.randrange(99)) for _ in range(32)]
    d = check_both(codec, [sec(*free)])
    assert d.n == 32 and not d.strs["len"].any()
    # (its span: from its first line to its last, none of it payload)
    assert one_tile(d) == {"staged": True, "fast": True, "fixed": True,
                           "wire": len(b"".join(free[:-1])),
                           "out": len(d.data)}
    lines = ordinary(rng, 32) + free + ordinary(rng, 32) + free + free
    d = check_both(codec, [sec(*lines)])
    assert d.n == 160 and not d.strs["len"][64:128].any() \
        and not d.strs["len"][192:].any()
    # ... and cut into sections at and around the tile edges
    d = check_both(codec, [sec(*lines[:31]), sec(*lines[31:33]), sec(),
                           sec(*lines[33:64]), sec(*lines[64:])])
    assert d.n == 160


@pytest.mark.gpu
def test_static_lanes_and_33_headers(codec):
    """static strings on lanes 0, 1, 62 and 63 -- an indexed line first and
    last in the tile, a name reference there -- and 33 headers: one in the
    second tile"""
    rng = random.Random(12)
    lit30 = [literal(b"n%d" % i, O.huffman_enc(b"value-%d" % i), 0, 1)
             for i in range(30)]
    for first, last in ((indexed(LONG_VAL), indexed(LONG_NAME)),
                        (nameref(LONG_NAME, b"x"), nameref(5, b"")),
                        (indexed(0), literal(b"a", b"b"))):
        d = check_both(codec, [sec(first, *lit30, last)])
        assert d.n == 32 and d.strs["source"][0] == 1
        d = check_both(codec, [sec(first, *lit30, last, first)])
        assert d.n == 33 and len(D.layout(d)) == 2
    d = check_both(codec, [sec(*ordinary(rng, 33))])
    assert d.n == 33


def arena_tile(n, at):
    """one tile whose header `at` carries a Huffman value of n bytes, beside
    short values and the longest static value and name"""
    h = L.maxexp(n, random.Random(13 + n))
    lines = [nameref(LONG_NAME, O.huffman_enc(b"v%d" % i), 1)
             for i in range(29)]
    lines[at:at] = [nameref(LONG_NAME, h, 1)]
    lines[7:7] = [indexed(LONG_VAL), indexed(LONG_NAME)]
    return sec(*lines)


def out_tile(total):
    """one tile of `total` output bytes, 31 x 76 of them static"""
    static = 31 * 76
    return [indexed(LONG_VAL)] * 31 + [literal(b"x", bytes(
        (97 + i % 26) for i in range(total - static - 1)))]


def span_tile(span):
    """one tile (to be placed at a0 = 14: its first line on a 16-byte
    boundary) whose wire bytes span exactly `span`, its output small"""
    rng = random.Random(span)
    v = [long_codes(150, rng) for _ in range(5)]          # 563 bytes each
    head = [indexed(LONG_VAL)] + [nameref(i, x, 1) for i, x in enumerate(v)] \
        + [indexed(i) for i in range(20)] \
        + [literal(b"k", O.huffman_enc(b"v"), 0, 1)] * 4
    used = len(b"".join(head))
    # a raw value ends the span; behind it a static string, at the span's end
    fill = next(k for k in range(span) if used + len(nameref(9, bytes(k))) == span)
    lines = head + [nameref(9, bytes(fill)), indexed(LONG_NAME)]
    assert len(lines) == 32
    return sec(*lines)


def long_codes(k, rng):
    """k symbols of 30-bit codes: 4 wire bytes a decoded byte"""
    s = L.with_bits(k, 30 * k, rng)
    return O.huffman_enc(s)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [L.FIX_MAX, L.FIX_MAX + 1])
def test_arena_rule_edge(codec, n):
    """the arena rule: fixed slots iff no WIRE string of the tile has more
    than 66 payload bytes, whatever its static strings emit -- a literal of
    66 and of 67 Huffman bytes (the most either can decode to) in a tile that
    also holds the longest static value (53 bytes) and name (32)"""
    rng = random.Random(13 + n)
    h = L.maxexp(n, rng)
    for at in (0, 15, 29):
        d = check_both(codec, [arena_tile(n, at)])
        p = one_tile(d)
        assert d.n == 32 and p["fixed"] == (n == L.FIX_MAX) and p["fast"]
    # raw, and as a literal name
    lines = [literal(bytes(n), h, 0, 1), indexed(LONG_VAL),
             literal(h, b"v", 1, 0)] + [indexed(LONG_NAME)] * 29
    d = check_both(codec, [sec(*lines)])
    assert one_tile(d)["fixed"] == (n == L.FIX_MAX)


@pytest.mark.gpu
@pytest.mark.parametrize("total", [D.OUT_FAST, D.OUT_FAST + 1])
def test_out_stage_counts_static_bytes(codec, total):
    """output of 3008 and 3009 bytes, most of them static: the tile leaves
    the out stage at total + 64 > 3072 with its static bytes counted"""
    lines = out_tile(total)
    for order in (lines, lines[::-1]):
        d = check_both(codec, [sec(*order)])
        p = one_tile(d)
        assert p["out"] == total and p["staged"]
        assert p["fast"] == (total == D.OUT_FAST)
    # the same edge with Huffman wire strings beside the static ones
    rng = random.Random(total)
    hv = [L.symbols(40, rng) for _ in range(16)]
    rest = total - 16 * (40 + 32) - 15 * 76 - 1
    lines = [nameref(LONG_NAME, v, 1) for v in hv] + [indexed(LONG_VAL)] * 15 \
        + [literal(b"y", L.symbols(rest, rng), 0, 1)]
    d = check_both(codec, [sec(*lines)])
    p = one_tile(d)
    assert p["out"] == total and p["fast"] == (total == D.OUT_FAST)


@pytest.mark.gpu
@pytest.mark.parametrize("span", [3072, 3073, 3088])
def test_wire_span_edge(codec, span):
    """a tile whose wire bytes span exactly `span` from a 16-byte boundary:
    staged up to 3072, on the out-of-line path past it (3073 and 3088 round to
    the same blocks) -- static strings first, last and inside it, the output
    small either way"""
    import torch
    # (the section's prefix is two bytes: its first line on a 16-byte boundary)
    d = D.Decoded([span_tile(span)], a0=14)
    p = one_tile(d)
    assert int(d.strs["pos"][0]) == 16 and p["wire"] == span
    assert p["staged"] == (span <= 3072) and p["out"] < 2000
    res = run_device(codec, d)
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    scan, dec = fetch_device(d, res)
    check_scan(d, scan)
    check_decode(d, dec)


@pytest.mark.gpu
@pytest.mark.parametrize("huffman", [0, 1])
def test_unstaged_tile_with_static_strings(codec, huffman):
    """a 4 KB value (the tile cannot be staged) with indexed lines before and
    after it in the tile, between ordinary tiles"""
    rng = random.Random(14 + huffman)
    raw = bytes(rng.choice(L.TOKEN) for _ in range(4096 if not huffman
                                                   else 6000))
    big = O.huffman_enc(raw) if huffman else raw
    assert len(big) >= 4096 - 500 * huffman
    tile = [indexed(LONG_VAL), indexed(3)] + ordinary(rng, 12) \
        + [nameref(LONG_NAME, big, huffman)] + ordinary(rng, 12) \
        + [indexed(LONG_NAME)] * 5
    lines = ordinary(rng, 32) + tile + ordinary(rng, 32)
    d = check_both(codec, [sec(*lines)])
    assert [p["staged"] for p in D.layout(d)] == [True, False, True]
    # and as a literal line's name
    tile[14] = literal(big, b"v", huffman, 0)
    check_both(codec, [sec(*(tile + tile))], pads=(0, 15))


# ---- the length limit -------------------------------------------------------------

def sized(k, huffman, rng):
    """a payload that decodes to k bytes"""
    return L.symbols(k, rng) if huffman else bytes(rng.choice(L.TOKEN)
                                                   for _ in range(k))


@pytest.mark.gpu
@pytest.mark.parametrize("huffman", [0, 1])
def test_limit_at_max_strlen(codec, huffman):
    """max_len = QHUFF_MAX_STRLEN: a 32-byte static name with a value of
    65503 (kept) and 65504 (rejected) bytes, a 2-byte literal name with
    65533 / 65534; an indexed line is never rejected"""
    rng = random.Random(15 + huffman)
    lines = [indexed(LONG_VAL)]
    want = [(0, 0)]
    for k in (65503, 65504):
        lines.append(nameref(LONG_NAME, sized(k, huffman, rng), huffman))
        want.append((0, int(k == 65504)))
    for k in (65533, 65534):
        lines.append(literal(sized(2, huffman, rng), sized(k, huffman, rng),
                             huffman, huffman))
        want.append((0, int(k == 65534)))
    lines.append(indexed(LONG_NAME))
    want.append((0, 0))
    d = check_both(codec, [sec(*lines[:3]), sec(*lines[3:])], pads=(0, 1))
    assert d.status.reshape(-1, 2).tolist() == [list(w) for w in want]
    assert len(d.strings[3]) == 65503 and d.strings[5] == b"" \
        and len(d.strings[4]) == 32
    # no limit: everything is kept
    d = check_both(codec, [sec(*lines)], max_len=0, pads=(0,))
    assert not d.status.any()


@pytest.mark.gpu
@pytest.mark.parametrize("max_len", [1, 7, 20, 33, 60])
def test_small_limits_on_staged_tiles(codec, max_len):
    """limits small enough to reject static names and values and short
    literals on the staged path: names alone, values with their names"""
    h = shape("boundaries")
    d = check_both(codec, h.want_sections, max_len=max_len, pads=(0, 15))
    st = d.status.reshape(-1, 2)
    assert not st.all() and (max_len > 20 or (st[:, 0].any()
                                              and st[:, 1].any()))
    lines = [indexed(LONG_VAL), indexed(LONG_NAME), indexed(1),
             nameref(LONG_NAME, b"v" * 28), nameref(LONG_NAME, b"v" * 29)]
    d = check_both(codec, [sec(*lines)], max_len=60, pads=(0,))
    assert d.status.tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0, 1]


@pytest.mark.gpu
def test_rejected_strings(codec):
    """a rejected Huffman name and a rejected value: their statuses, 0 bytes,
    and the header's other string keeps its bytes -- on staged tiles and on
    one past the stage"""
    rng = random.Random(16)
    good = O.huffman_enc(b"a-good-string")
    bad = L.invalid_twin(L.symbols(23, rng))
    eos = b"\xff\xff\xff\xff"                       # the EOS code
    lines = ordinary(rng, 5) + [literal(bad, good, 1, 1),
                                literal(good, bad, 1, 1),
                                nameref(LONG_NAME, bad, 1),
                                literal(eos, b"raw", 1, 0),
                                literal(bad, eos, 1, 1), indexed(LONG_VAL)]
    d = check_both(codec, [sec(*lines)])
    assert d.status[10:].tolist() == [1, 0, 0, 1, 0, 1, 1, 0, 1, 1, 0, 0]
    assert d.strings[11] == b"a-good-string" == d.strings[12]
    assert d.strings[14] == D.STATIC[LONG_NAME][0]
    big = nameref(1, bytes(5000))
    d = check_both(codec, [sec(*(lines + [big] + lines))], pads=(0, 15))
    assert not one_tile(d)["staged"] and d.status.sum() == 12


# ---- the calls' contract ----------------------------------------------------------

def contract_sections(name):
    rng = random.Random(17)
    return {"n0m0": [], "n0m3": [sec(), sec(), sec()],
            "n33": [sec(*ordinary(rng, 20)), b"\0", sec(*ordinary(rng, 13)),
                    b"\x01\x00\xC1"]}[name]


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("name", ["n0m0", "n0m3", "n33"])
def test_buffer_contract(codec, name, host):
    """every array at its exact size in a dirty guarded arena: the expected
    bytes, and nothing else written"""
    import torch
    for k, fill in enumerate(FILLS):
        k += 3 * host
        r = (0, 1, 15)[k % 3]
        d = D.Decoded(contract_sections(name), a0=0)
        n, m = d.n, d.m
        assert (n, m) == {"n0m0": (0, 0), "n0m3": (0, 3), "n33": (33, 4)}[name]
        specs = [("buf", len(d.wire), r), ("sec_off", 4 * (m + 1), 4 * (k % 4)),
                 ("strs", 32 * n, 4 * ((k + 1) % 4)),
                 ("hdr_off", 4 * (m + 1), 4 * ((k + 2) % 4)),
                 ("rc", 4 * m, 4 * ((k + 3) % 4)), ("kind", n, (5 * k + 2) % 16),
                 ("static_id", n, (k + 9) % 16), ("hflags", n, (3 * k + 1) % 16),
                 ("out", len(d.data), (7 * k + 3) % 16),
                 ("off", 4 * (2 * n + 1), 4 * (k % 4)),
                 ("status", 2 * n, (k + 5) % 16), ("h1", 4 * n, 4 * (k % 4)),
                 ("h2", 4 * n, 4 * ((k + 1) % 4))]
        ar = Arena(specs, seed=8000 + 16 * k)
        ar.put("buf", np.frombuffer(d.wire, dtype=np.uint8))
        ar.put("sec_off", d.sec_off)
        ar.neighbours("buf", fill)
        ar.commit(not host)
        written = {"hdr_off": 4 * (m + 1), "rc": 4 * m, "kind": n,
                   "static_id": n, "hflags": n, "out": len(d.data),
                   "off": 4 * (2 * n + 1), "status": 2 * n}
        if host:
            rc = qhuff.lib().qhuff_decode_headers_host(
                codec._ctx, ar.addr("buf"), ar.addr("sec_off"), m, MAXS, n,
                ar.addr("hdr_off"), ar.addr("rc"), ar.addr("kind"),
                ar.addr("static_id"), ar.addr("hflags"), ar.addr("out"),
                ar.addr("off"), ar.addr("status"), ar.addr("h1"),
                ar.addr("h2"))
            assert rc == qhuff.OK
            written.update({"h1": 4 * n, "h2": 4 * n})
        else:
            codec.scan_headers_into(ar.ptr("buf"), ar.ptr("sec_off"), m,
                                    ar.ptr("strs"), n, ar.ptr("hdr_off"),
                                    ar.ptr("rc"), ar.ptr("kind"),
                                    ar.ptr("static_id"), ar.ptr("hflags"))
            codec.decode_headers_into(ar.ptr("buf"), ar.ptr("strs"), n, MAXS,
                                      ar.ptr("out"), ar.ptr("off"),
                                      ar.ptr("status"))
            torch.cuda.synchronize()
            assert codec.device_error() == 0
            written["strs"] = 32 * n
        img = ar.after()
        ar.check(img, written)
        assert np.array_equal(ar.get(img, "hdr_off", np.uint32), d.hdr_off)
        assert np.array_equal(ar.get(img, "rc", np.int32), d.rc)
        assert np.array_equal(ar.get(img, "kind"), d.kind)
        assert np.array_equal(ar.get(img, "static_id"), d.static_id)
        assert np.array_equal(ar.get(img, "hflags"), d.hflags)
        assert np.array_equal(ar.get(img, "off", np.uint32), d.off)
        assert np.array_equal(ar.get(img, "status"), d.status)
        assert ar.get(img, "out").tobytes() == d.data
        if not host:
            assert np.array_equal(ar.get(img, "strs"), d.str_bytes())
        elif n:
            want = [M.hashes(*hv) for hv in d.headers]
            assert ar.get(img, "h1", np.uint32).tolist() == [w[0] for w in want]
            assert ar.get(img, "h2", np.uint32).tolist() == [w[1] for w in want]


@pytest.mark.gpu
def test_argument_errors_and_erange(codec):
    """refused calls write nothing, and the context is usable afterwards"""
    rng = random.Random(18)
    secs = [sec(*ordinary(rng, 20)), sec(*ordinary(rng, 13))]
    d = D.Decoded(secs)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    buf = np.frombuffer(d.wire, dtype=np.uint8)
    n, m = d.n, d.m
    A = 0xA5
    arrs = {"hdr_off": np.full(m + 1, A, np.uint32), "rc": np.full(m, A, np.int32),
            "kind": np.full(n, A, np.uint8), "sid": np.full(n, A, np.uint8),
            "hf": np.full(n, A, np.uint8),
            "out": np.full(D.bound(len(buf), n), A, np.uint8),
            "off": np.full(2 * n + 1, A, np.uint32),
            "st": np.full(2 * n, A, np.uint8), "h1": np.full(n, A, np.uint32),
            "h2": np.full(n, A, np.uint32)}
    before = {k: v.copy() for k, v in arrs.items()}

    def call(ctx=codec._ctx, b=p(buf), so=d.sec_off, cap=n, **null):
        a = {k: (None if k in null else p(v)) for k, v in arrs.items()}
        return qhuff.lib().qhuff_decode_headers_host(
            ctx, b, p(so) if so is not None else None, m, MAXS, cap,
            a["hdr_off"], a["rc"], a["kind"], a["sid"], a["hf"], a["out"],
            a["off"], a["st"], a["h1"], a["h2"])

    E = qhuff.EINVAL
    assert call(ctx=None) == E and call(b=None) == E and call(so=None) == E
    assert call(hdr_off=0) == E and call(rc=0) == E and call(out=0) == E
    assert call(off=0) == E and call(st=0) == E
    bad = d.sec_off.copy()
    bad[1] = bad[2] + 1
    assert call(so=bad) == E
    assert call(cap=0x80000000) == qhuff.ERANGE
    assert all(np.array_equal(arrs[k], before[k]) for k in arrs)
    # n > max_hdrs: hdr_off and rc valid, nothing decoded
    assert call(cap=n - 1) == qhuff.ERANGE
    assert np.array_equal(arrs["hdr_off"], d.hdr_off)
    assert np.array_equal(arrs["rc"], d.rc)
    assert all(np.array_equal(arrs[k], before[k])
               for k in ("out", "off", "st", "h1", "h2"))
    ret, strs, ho, rc, kind, sid, hf = codec.scan_headers_host(buf, d.sec_off,
                                                               n - 3)
    check_scan(d, (ret, strs, ho, rc, kind, sid, hf), n - 3)
    assert ret == qhuff.ERANGE
    # the optional arrays NULL
    assert call(kind=0, sid=0, hf=0, h1=0, h2=0) == qhuff.OK
    assert np.array_equal(arrs["off"], d.off)
    assert np.array_equal(arrs["st"], d.status)
    assert arrs["out"][:len(d.data)].tobytes() == d.data
    assert all(np.array_equal(arrs[k], before[k])
               for k in ("kind", "sid", "hf", "h1", "h2"))
    Lb = qhuff.lib()
    assert Lb.qhuff_scan_headers(None, None, None, 0, None, 0, None, None,
                                 None, None, None, None) == E
    assert Lb.qhuff_decode_headers(None, None, None, 0, 0, None, None, None,
                                   None) == E
    assert Lb.qhuff_decode_headers(codec._ctx, None, None, 1, 0, None, None,
                                   None, None) == E
    one = np.zeros(4, np.uint32)
    assert Lb.qhuff_decode_headers(codec._ctx, p(one), p(one), 0x80000000, 0,
                                   p(one), p(one), p(one), None) == qhuff.ERANGE
    check_both(codec, secs, pads=(0,))


@pytest.mark.gpu
def test_optional_arrays_null_on_device(codec):
    import torch
    rng = random.Random(19)
    d = D.Decoded([sec(*ordinary(rng, 40))])
    buf, so = dev(np.frombuffer(d.wire, np.uint8)), dev_i32(d.sec_off)
    strs = torch.empty(32 * d.n, dtype=torch.uint8, device="cuda")
    ho = torch.empty(2, dtype=torch.int32, device="cuda")
    rc = torch.empty(1, dtype=torch.int32, device="cuda")
    codec.scan_headers_into(buf, so, 1, strs, d.n, ho, rc)
    torch.cuda.synchronize()
    assert np.array_equal(strs.cpu().numpy(), d.str_bytes())
    assert ho.cpu().numpy().tolist() == [0, d.n] and rc.item() == 0
    # a count alone: no room for any header
    codec.scan_headers_into(buf, so, 1, None, 0, ho, rc)
    torch.cuda.synchronize()
    assert ho.cpu().numpy().tolist() == [0, d.n]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 32, 33])
def test_launch_frame(codec, n):
    """the decode call at the sizes where its launch frame takes another
    path: n = 0 writes off[0] alone; 32 and 33 headers each side of the tile
    count's rounding"""
    import torch
    rng = random.Random(20 + n)
    d = D.Decoded([sec(*ordinary(rng, n))])
    assert d.n == n
    buf = dev(np.frombuffer(d.wire, np.uint8))
    strs = dev(d.str_bytes())
    full = lambda k, dt, v: torch.full((max(k, 1),), v, dtype=dt,  # noqa: E731
                                       device="cuda")
    out = full(D.bound(len(d.wire), n), torch.uint8, 0xA5)
    off = full(2 * n + 1, torch.int32, -1)
    st = full(2 * n, torch.uint8, 0xA5)
    codec.decode_headers_into(buf, strs, n, MAXS, out, off, st)
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    o = off.cpu().numpy().view(np.uint32)
    assert np.array_equal(o, d.off)
    out = out.cpu().numpy()
    assert out[:len(d.data)].tobytes() == d.data
    assert (out[len(d.data):] == 0xA5).all()
    if n == 0:
        assert (st.cpu().numpy() == 0xA5).all()
    else:
        assert np.array_equal(st.cpu().numpy(), d.status)


@pytest.mark.gpu
def test_timing_kinds(codec):
    """three scan launches, the decode launch, and the hash launch when
    hashes are asked for"""
    import torch
    rng = random.Random(21)
    secs = [sec(*ordinary(rng, 40)), sec(*ordinary(rng, 3))]
    d = D.Decoded(secs)
    wire = np.frombuffer(d.wire, np.uint8)
    K = qhuff
    codec.timing(True)
    try:
        codec.timing_read()
        res = run_device(codec, d)
        torch.cuda.synchronize()
        t = codec.timing_read()
        assert [k for k, _ in t] == [K.KIND_SCAN] * 3 + [K.KIND_DECODE]
        assert all(us > 0 for _, us in t)
        codec.decode_headers_host(wire, d.sec_off, MAXS, d.n)
        assert [k for k, _ in codec.timing_read()] \
            == [K.KIND_SCAN] * 3 + [K.KIND_DECODE]
        codec.decode_headers_host(wire, d.sec_off, MAXS, d.n, hashes=True)
        assert [k for k, _ in codec.timing_read()] \
            == [K.KIND_SCAN] * 3 + [K.KIND_DECODE, K.KIND_HASH]
    finally:
        codec.timing(False)
    check_decode(d, fetch_device(d, res)[1])


@pytest.mark.gpu
def test_two_streams(codec):
    """two scans and decodes of different sizes on two streams of one
    context, no host synchronisation between them (one scan scratch)"""
    import torch
    rng = random.Random(22)
    small = D.Decoded([sec(*ordinary(rng, 40))])
    big = D.Decoded([sec(*ordinary(rng, 16)) for _ in range(600)])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    c = qhuff.Codec(0)
    try:
        torch.cuda.synchronize()
        res = []
        for d, s in ((big, s1), (small, s2), (small, s1), (big, s2)):
            with torch.cuda.stream(s):
                res.append((d, run_device(c, d, stream=s)))
        torch.cuda.synchronize()
        assert c.device_error() == 0
        for d, r in res:
            scan, dec = fetch_device(d, r)
            check_scan(d, scan)
            check_decode(d, dec)
    finally:
        c.close()


@pytest.mark.gpu
def test_small_grid_every_wave_several_tiles():
    """a context whose grids are 1 %: every wave of the decode launch runs
    three tiles or more -- wire-free, unstaged and ordinary ones in turn"""
    import torch
    from test_hash_limits import _open
    c = _open({"QHUFF_GRID_PCT": "1"})
    try:
        W = c.grid_waves(qhuff.KIND_DECODE)
        rng = random.Random(23)
        tiles = [ordinary(rng, 32), [indexed(i) for i in range(32)],
                 ordinary(rng, 31) + [nameref(1, bytes(3300))],
                 [indexed(LONG_VAL)] * 31 + [literal(b"n", bytes(700))]]
        k = -(-(3 * W + 1) // len(tiles))
        assert 0 < W and k < 200
        secs = [sec(*t) for _ in range(k) for t in tiles]
        for _ in range(2):
            d = D.Decoded(secs)
            res = run_device(c, d)
            torch.cuda.synchronize()
            assert c.device_error() == 0
            scan, dec = fetch_device(d, res)
            check_scan(d, scan)
            check_decode(d, dec)
        p = D.layout(d)
        assert len(p) > 3 * W and [x["fast"] for x in p[:4]] \
            == [True, True, False, False]
        assert [x["staged"] for x in p[:4]] == [True, True, False, True]
    finally:
        c.close()
