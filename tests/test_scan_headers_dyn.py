"""qhuff_scan_headers_dyn on the CPU: the model (tests/headers_dyn_model.py)
against the reference's own interop files, and the walker's host form
(qhuff_scan_headers_dyn_cpu) against the model, array for array.

The anchor: the three committed interop streams replayed -- encoder-stream
inserts applied to a 256-byte table, every field section decoded in the
window it had at its place in the file -- give the header lists of the
committed QIF files exactly, all 34 sections.  Those files hold indexed
dynamic lines, post-base indexed lines and post-base name references; they
hold NO dynamic name reference with T = 0, so that form is pinned by the
constructed cases below against the model only.

The walker's clamps (windows and offsets outside the rule) are reached only
here, on the CPU, by tests/c/hdrscan_dyn_san.cpp under ASan + UBSan."""
import ctypes as C
import functools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import _paths  # noqa: F401
import headers_dyn_model as D
import qhuff
import scan_cases as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ME = 8


@functools.lru_cache(maxsize=None)
def replay(name):
    return D.Replay(name)


@functools.lru_cache(maxsize=None)
def replayed(name):
    r = replay(name)
    return D.Decoded(r.sections, r.table, r.win, max_len=0)


def table_arg(t):
    return (t.data, t.off, t.first, t.max_entries)


def cpu(d, max_hdrs=None):
    buf = np.frombuffer(bytes(d.a0) + d.wire, dtype=np.uint8)
    return qhuff.scan_headers_dyn_cpu(buf, d.sec_off, table_arg(d.table),
                                      d.sec_win,
                                      d.n if max_hdrs is None else max_hdrs)


def check_scan(d, got, max_hdrs=None):
    ret, strs, hdr_off, rc, kind, sid, hf, did = got
    n = d.n if max_hdrs is None else min(d.n, max_hdrs)
    assert ret == (qhuff.ERANGE if d.n > n else qhuff.OK)
    assert np.array_equal(rc, d.rc), (rc.tolist(), d.rc.tolist())
    assert np.array_equal(hdr_off, d.hdr_off)
    assert np.array_equal(strs, d.str_bytes(n))
    assert np.array_equal(kind, d.kind[:n])
    assert np.array_equal(sid, d.static_id[:n])
    assert np.array_equal(hf, d.hflags[:n])
    assert np.array_equal(did, d.dyn_id[:n])


# ---- the reference's own data ---------------------------------------------------

@pytest.mark.parametrize("name", sorted(D.INTEROP))
def test_replay_gives_the_qif_lists(name):
    r, d = replay(name), replayed(name)
    sections, inserts, oldest = D.INTEROP[name]
    assert (len(r.sections), len(r.entries), r.oldest) == \
        (sections, inserts, oldest)
    assert d.rc.tolist() == [D.OK] * sections        # none left out
    assert d.header_lists() == r.qif_lists(name)
    # every section but the file's first carries a Required Insert Count
    assert [s[0] != 0 for s in r.sections] == [False] + [True] * (sections - 1)
    if name == "netbsd":                             # (its encoding wraps)
        assert [s[0] for s in r.sections][-4:] == [16, 1, 2, 3]


def test_interop_line_forms():
    """what the files hold, and what they do not"""
    forms = {"indexed": 0, "post_indexed": 0, "post_nameref": 0, "nameref": 0}
    for name in D.INTEROP:
        d = replayed(name)
        for l in d.lines:
            if l.dyn is None:
                continue
            b = d.wire[l.at]
            forms["indexed" if b & 0x80 else "nameref" if b & 0x40
                  else "post_indexed" if b & 0x10 else "post_nameref"] += 1
    assert forms == {"indexed": 38, "post_indexed": 37, "post_nameref": 2,
                     "nameref": 0}


def test_abi():
    lib = qhuff.lib()
    for s in ("qhuff_scan_headers_dyn", "qhuff_scan_headers_dyn_host",
              "qhuff_scan_headers_dyn_cpu", "qhuff_decode_headers_dyn_bound",
              "qhuff_decode_headers_dyn", "qhuff_decode_headers_dyn_host"):
        assert s in qhuff.EXPORTS and getattr(lib, s)
    with open(os.path.join(ROOT, "include", "qhuff.h")) as f:
        h = f.read()
    for k, v in (("QHUFF_FEATURE_DECODE_HEADERS_DYN", "1"),
                 ("QHUFF_EBLOCKED", "(-11)"), ("QHUFF_HSTR_DYN", "2"),
                 ("QHUFF_LINE_DYN", "4"), ("QHUFF_DYN_NONE", "0xFFFFFFFFu")):
        assert "#define %s " % k in h and \
            h.split("#define %s " % k)[1].split()[0] == v
    assert (qhuff.EBLOCKED, qhuff.HSTR_DYN, qhuff.LINE_DYN, qhuff.DYN_NONE) \
        == (D.EBLOCKED, D.DYN_SRC, D.LINE_DYN, D.DYN_NONE)
    assert C.sizeof(qhuff.DynTable) == 32
    for w, n, l in ((0, 0, 0), (1000, 7, 10), (1000, 7, 76), (1000, 7, 77),
                    (5, 3, 4096)):
        assert qhuff.decode_headers_dyn_bound(w, n, l) == D.bound(w, n, l) \
            == 8 * w // 5 + max(76, l) * n + 16


@pytest.mark.parametrize("name", sorted(D.INTEROP))
def test_cpu_interop_files(name):
    d = replayed(name)
    check_scan(d, cpu(d))
    check_scan(d, cpu(d, 0), 0)


# ---- constructed ------------------------------------------------------------------

def entries(k):
    return [(b"name-%d" % i, b"value-%d" % i * (i % 3)) for i in range(k)]


T40 = D.Table(entries(40), 0, ME)


def one(section, lo, ins, table=T40):
    d = D.Decoded([section], table, [(lo, ins)])
    check_scan(d, cpu(d))
    return int(d.rc[0]), d


def named(ric, base=None, lines=b""):
    """a section with Required Insert Count ric whose first line names
    ric - 1"""
    base = ric if base is None else base
    first = D.indexed_dyn(base - ric) if base >= ric else \
        D.indexed_post(ric - 1 - base)
    return D.prefix_for(ric, base, ME) + first + lines


def test_rc_clauses_in_order():
    ok = named(10)
    assert one(ok, 4, 12)[0] == D.OK
    trunc = D.nameref_dyn(0, b"abcdef")[:-2]
    # 1. framing wins over everything after it
    assert one(D.prefix(17) + trunc, 4, 12)[0] == D.ETRUNC
    assert one(D.prefix_for(13, 13, ME) + trunc, 4, 12)[0] == D.ETRUNC
    assert one(D.prefix(17) + b"\xff" * 12, 4, 12)[0] == D.EPROTO
    # 2. the encoded count above 2 * MaxEntries, blocked or not
    assert one(D.prefix(17) + D.indexed_dyn(0), 4, 12)[0] == D.EPROTO
    assert one(D.prefix(16) + D.indexed_dyn(0), 4, 12)[0] == D.EBLOCKED
    t0 = D.Table(entries(4), 0, 0)
    assert one(D.prefix(1) + D.indexed_dyn(0), 0, 4, t0)[0] == D.EPROTO
    assert one(D.prefix(0) + D.indexed_static(1), 0, 4, t0)[0] == D.OK
    # 3. RIC <= 0; blocked wins over a bad line
    assert one(D.prefix(16) + D.indexed_dyn(0), 0, 3)[0] == D.EPROTO   # -1
    assert D.ric_of(16, 3, ME) == (D.EPROTO, -1)
    blocked = D.prefix_for(13, 13, ME)
    assert one(blocked + D.indexed_dyn(0), 4, 12)[0] == D.EBLOCKED
    assert one(blocked + D.indexed_static(99), 4, 12)[0] == D.EBLOCKED
    assert one(blocked + D.indexed_dyn(40), 4, 12)[0] == D.EBLOCKED
    # 4. the lines
    assert one(ok + D.indexed_static(99), 4, 12)[0] == D.EPROTO
    assert one(ok + D.nameref_static(99, b"v"), 4, 12)[0] == D.EPROTO
    assert one(ok + D.indexed_static(98), 4, 12)[0] == D.OK
    assert one(D.prefix(0) + D.indexed_dyn(0), 4, 12)[0] == D.EPROTO
    assert one(D.prefix(0) + D.indexed_post(0), 4, 12)[0] == D.EPROTO
    assert one(D.prefix(0, 1, 3) + D.indexed_static(5), 4, 12)[0] == D.OK
    # RIC != 0 and no line names RIC - 1
    assert one(D.prefix_for(10, 10, ME) + D.indexed_dyn(1), 4, 12)[0] \
        == D.EPROTO
    assert one(D.prefix_for(10, 10, ME) + D.indexed_static(1), 4, 12)[0] \
        == D.EPROTO
    assert one(D.prefix_for(10, 10, ME), 4, 12)[0] == D.EPROTO


def test_every_dynamic_form():
    """the four forms, N bits and Huffman values; the T = 0 name reference is
    pinned here alone (the interop files hold none)"""
    s = (D.prefix_for(10, 8, ME) + D.indexed_post(1)
         + D.indexed_dyn(0) + D.nameref_dyn(1, b"plain", never=1)
         + D.nameref_dyn(2, b"huffman value", huffman=1)
         + D.nameref_post(0, b"post", never=1) + D.nameref_post(1, b"")
         + D.indexed_static(17) + D.nameref_static(3, b"x", never=1)
         + D.literal(b"a", b"b", never=1))
    rc, d = one(s, 4, 12)
    assert rc == D.OK
    assert d.dyn_id.tolist() == [9, 7, 6, 5, 8, 9, D.DYN_NONE, D.DYN_NONE,
                                 D.DYN_NONE]
    assert d.kind.tolist() == [4, 4, 5, 5, 5, 5, 0, 1, 2]
    assert d.hflags.tolist() == [0, 0, 1, 0, 1, 0, 0, 1, 1]
    assert d.static_id.tolist() == [255] * 6 + [17, 3, 255]
    assert d.headers[2] == (b"name-6", b"plain")
    assert d.headers[3] == (b"name-5", b"huffman value")
    assert d.headers[0] == T40.entry(9)
    assert [int(x) for x in d.strs["source"][:4]] == [2, 2, 2, 2]
    assert int(d.strs["source"][5]) == D.WIRE


def test_ric_reconstruction():
    """ins on both sides of every multiple of 16 the table reaches; enc = 1,
    16, 17; RIC exactly ins, ins + 1, ins - 7, ins - 8"""
    t = D.Table(entries(70), 0, ME)
    for ins in (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65):
        lo = max(0, ins - ME)
        for enc in (1, 16, 17):
            rc, ric = D.ric_of(enc, ins, ME)
            got, _ = one(D.prefix(enc) + D.indexed_dyn(0), lo, ins, t)
            assert got == rc if rc != D.OK else got in (D.OK, D.EPROTO)
            if rc == D.OK:
                assert got == (D.OK if lo <= ric - 1 < ins else D.EPROTO)
        for delta, want in ((0, D.OK), (1, D.EBLOCKED), (-7, D.OK),
                            (-8, D.EBLOCKED)):
            ric = ins + delta
            if ric <= 0:
                continue
            # (ins - 8 == ins + 8 mod 16: the count it stands for is ahead)
            rc, got_ric = D.ric_of(D.enc_ric(ric, ME), ins, ME)
            assert rc == want
            assert got_ric == (ric if delta != -8 else ins + 8)
            got, d = one(named(ric), lo, ins, t)
            assert got == want
            if want == D.OK:
                assert d.dyn_id.tolist() == [ric - 1]


def test_delta_base_signs():
    # Base below 0: only a post-base line can reach the table
    s = D.prefix(D.enc_ric(2, ME), 1, 5)              # Base = 2 - 5 - 1 = -4
    assert one(s + D.indexed_post(5), 0, 6)[1].dyn_id.tolist() == [1]
    assert one(s + D.indexed_post(5) + D.indexed_post(4), 0, 6)[1] \
        .dyn_id.tolist() == [1, 0]
    assert one(s + D.indexed_post(5) + D.indexed_post(3), 0, 6)[0] == D.EPROTO
    assert one(s + D.indexed_post(5) + D.indexed_dyn(0), 0, 6)[0] == D.EPROTO
    # Base above ins: only a relative line can
    s = D.prefix(D.enc_ric(6, ME), 0, 3)              # Base = 9, ins = 6
    assert one(s + D.indexed_dyn(3), 0, 6)[1].dyn_id.tolist() == [5]
    assert one(s + D.indexed_dyn(3) + D.indexed_dyn(2), 0, 6)[0] == D.EPROTO
    assert one(s + D.indexed_dyn(3) + D.indexed_post(0), 0, 6)[0] == D.EPROTO
    assert one(s + D.indexed_dyn(3) + D.nameref_dyn(8, b"v"), 0, 6)[1] \
        .dyn_id.tolist() == [5, 0]
    assert one(s + D.indexed_dyn(3) + D.nameref_dyn(9, b"v"), 0, 6)[0] \
        == D.EPROTO
    # a Delta Base as large as the integer goes (two's complement)
    for sign in (0, 1):
        for delta in ((1 << 63) - 1, 1 << 63, (1 << 64) - 1):
            sec = D.prefix(D.enc_ric(6, ME), sign, delta) + D.indexed_post(0)
            one(sec, 0, 6)
            one(sec + D.indexed_dyn(0), 0, 6)


def test_window_edges():
    lo, ins = 20, 28
    base = named(ins)                                  # names ins - 1
    assert one(base, lo, ins)[1].dyn_id.tolist() == [ins - 1]
    assert one(base + D.indexed_dyn(ins - 1 - lo), lo, ins)[1] \
        .dyn_id.tolist() == [ins - 1, lo]
    assert one(base + D.indexed_dyn(ins - lo), lo, ins)[0] == D.EPROTO
    assert one(base + D.indexed_post(0), lo, ins)[0] == D.EPROTO      # ins
    assert one(base + D.nameref_dyn(ins - lo, b"v"), lo, ins)[0] == D.EPROTO
    assert one(base + D.nameref_post(0, b"v"), lo, ins)[0] == D.EPROTO
    # the same lines in a wider window are there
    assert one(base + D.indexed_dyn(ins - lo), lo - 1, ins)[0] == D.OK
    # RIC - 1 named only by a post-base line
    s = D.prefix_for(ins, ins - 1, ME) + D.indexed_post(0)
    assert one(s, lo, ins)[1].dyn_id.tolist() == [ins - 1]
    s = D.prefix_for(ins, ins - 3, ME) + D.nameref_post(2, b"v")
    assert one(s, lo, ins)[1].dyn_id.tolist() == [ins - 1]
    assert one(D.prefix_for(ins, ins - 3, ME) + D.nameref_post(1, b"v"),
               lo, ins)[0] == D.EPROTO


def test_empty_table_and_large_first():
    t = D.Table([], 0, ME)
    d = D.Decoded([D.prefix(0) + D.indexed_static(2), D.prefix(1)
                   + D.indexed_dyn(0), D.prefix(0) + D.indexed_dyn(0),
                   D.prefix(0)], t)
    assert d.sec_win is None
    check_scan(d, cpu(d))
    assert d.rc.tolist() == [D.OK, D.EPROTO, D.EPROTO, D.OK]
    # first as large as it goes: first + d = 2^32 - 1
    k = 12
    first = (1 << 32) - 1 - k
    t = D.Table(entries(k), first, ME)
    ins = first + k
    secs = [named(ins, lines=D.indexed_dyn(k - 1) + D.nameref_dyn(3, b"v")),
            named(ins, lines=D.indexed_dyn(k)),
            named(ins - 2, ins - 5, D.indexed_post(0)),
            D.prefix_for(ins, ins, ME) + D.indexed_post(0)]
    d = D.Decoded(secs, t)
    check_scan(d, cpu(d))
    assert d.rc.tolist() == [D.OK, D.EPROTO, D.OK, D.EPROTO]
    assert d.dyn_id.tolist()[:3] == [ins - 1, first, ins - 4]
    d = D.Decoded(secs, t, [(first, ins), (first + 1, ins), (first, ins - 2),
                            (first, ins - 1)])
    check_scan(d, cpu(d))
    assert d.rc.tolist() == [D.OK, D.EPROTO, D.OK, D.EBLOCKED]


def test_max_hdrs_cuts_inside_a_section():
    r = replay("fb-resp")
    d = replayed("fb-resp")
    assert d.m > 2 and d.hdr_off[1] + 1 < d.hdr_off[2]
    for cap in (0, 1, int(d.hdr_off[1]), int(d.hdr_off[1]) + 1, d.n - 1, d.n,
                d.n + 5):
        check_scan(d, cpu(d, cap), cap)
    assert r.table.d == 11


def test_cpu_argument_checks():
    d = replayed("netbsd")
    t = d.table
    buf = np.frombuffer(d.wire, dtype=np.uint8)

    def call(table, win, sec_off=d.sec_off):
        return qhuff.scan_headers_dyn_cpu(buf, sec_off, table, win, d.n)[0]

    assert call(table_arg(t), d.sec_win) == qhuff.OK
    # a broken off
    off = t.off.copy()
    off[5] = off[4] - 1
    assert call((t.data, off, 0, ME), d.sec_win) == qhuff.EINVAL
    # a broken window rule: below first, reversed, past first + d
    for s, (lo, ins) in ((0, (0, t.d + 1)), (3, (5, 4)), (2, (t.d + 1, t.d + 1))):
        win = d.sec_win.copy()
        win[2 * s:2 * s + 2] = (lo, ins)
        assert call(table_arg(t), win) == qhuff.EINVAL
    win = d.sec_win.copy() + np.uint32(7)
    assert call((t.data, t.off, 7, ME), win) == qhuff.OK
    win[0] = 6
    assert call((t.data, t.off, 7, ME), win) == qhuff.EINVAL
    # first + d past 2^32 - 1
    assert call((t.data, t.off, (1 << 32) - t.d, ME), None) == qhuff.ERANGE
    assert call((t.data, t.off, (1 << 32) - 1 - t.d, ME), None) == qhuff.OK
    # decreasing section offsets; null pointers
    bad = d.sec_off.copy()
    bad[2] = bad[1] - 1
    assert call(table_arg(t), d.sec_win, bad) == qhuff.EINVAL
    L, p = qhuff.lib(), qhuff._np_ptr
    ho, rc = np.zeros(d.m + 1, np.uint32), np.zeros(d.m, np.int32)
    tt, keep = qhuff.dyn_table_host(*table_arg(t))
    strs = np.zeros(32 * d.n, np.uint8)
    args = [p(buf), p(d.sec_off), d.m, C.byref(tt), None, p(strs), d.n, p(ho),
            p(rc), None, None, None, None]
    assert L.qhuff_scan_headers_dyn_cpu(*args) == qhuff.OK
    for i in (0, 1, 3, 5, 7, 8):
        a = list(args)
        a[i] = None
        assert L.qhuff_scan_headers_dyn_cpu(*a) == qhuff.EINVAL, i
    tn = qhuff.DynTable(None, None, t.d, 0, ME)
    a = list(args)
    a[3] = C.byref(tn)
    assert L.qhuff_scan_headers_dyn_cpu(*a) == qhuff.EINVAL
    # m = 0: hdr_off[0] alone
    ho[:] = 7
    assert L.qhuff_scan_headers_dyn_cpu(None, None, 0, C.byref(tt), None, None,
                                        0, p(ho), None, None, None, None,
                                        None) == qhuff.OK
    assert ho.tolist() == [0] + [7] * d.m


# ---- the walker under sanitizers ---------------------------------------------------

def dynamic_sections():
    """the model's own sections with dynamic lines, all in one window of T40"""
    ok = named(10)
    return [ok, ok + D.indexed_dyn(3) + D.nameref_dyn(1, b"value", never=1),
            named(12, 9, D.nameref_post(1, b"post", huffman=1)
                  + D.indexed_static(4) + D.literal(b"n", b"v")),
            D.prefix_for(13, 13, ME) + D.indexed_dyn(0),
            D.prefix(0) + D.indexed_static(2) + D.literal(b"nn", b"vv", 1, 1),
            named(8, lines=D.indexed_dyn(3)), D.prefix(17), D.prefix(0)]


def _san_files(tmp_path, name, chunks, table, win):
    wins = None if win is None else [win] * len(chunks)
    d = D.Decoded(chunks, table, wins)
    rec, exp = str(tmp_path / (name + ".rec")), str(tmp_path / (name + ".exp"))
    with open(rec, "wb") as f:
        f.write(struct.pack("<I", 0 if win is None else 1))
        for c in chunks:
            f.write(struct.pack("<I", len(c)) + c)
            if win is not None:
                f.write(struct.pack("<II", *win))
    with open(exp, "wb") as f:
        f.write(struct.pack("<II", d.m, d.n) + d.rc.tobytes()
                + d.hdr_off.tobytes() + d.str_bytes().tobytes()
                + d.kind.tobytes() + d.static_id.tobytes()
                + d.hflags.tobytes() + d.dyn_id.tobytes())
    return [rec, exp], d


def test_cpu_walker_under_sanitizers(tmp_path):
    """tests/c/hdrscan_dyn_san.cpp with its own main, g++ ASan + UBSan, run
    as a child process in the inherited environment: the fuzz payloads and a
    seeded havoc of the model's dynamic sections and of the interop files'
    sections; wire bytes, table bytes, off and sec_win in exactly-sized heap
    buffers; then the same sections under windows and offsets outside the
    rule (the walker's clamps)"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the sanitizer build"
    exe = str(tmp_path / "hdrscan_dyn_san")
    subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-o", exe,
         os.path.join(HERE, "c", "hdrscan_dyn_san.cpp"),
         os.path.join(ROOT, "ls-qpack_amd", "csrc", "qhuff_frames.cpp")],
        check=True, timeout=300)
    tab = str(tmp_path / "table")
    with open(tab, "wb") as f:
        f.write(struct.pack("<III", T40.d, T40.first, T40.max_entries)
                + T40.off.tobytes() + T40.bytes)
    own = dynamic_sections()
    interop = [s for n in sorted(D.INTEROP) for s in replay(n).sections]
    sets = {"fuzz": (S.fuzz_payloads(), None), "own": (own, (4, 12)),
            "havoc": (S.havoc(own + interop, 3000, 53), (4, 12)),
            "havoc_whole": (S.havoc(own + interop, 1000, 59), None)}
    args, total = [tab], 0
    for name, (chunks, win) in sets.items():
        a, d = _san_files(tmp_path, name, chunks, T40, win)
        args += a
        total += d.n
        if name == "havoc":
            assert set(d.rc.tolist()) >= {0, qhuff.ETRUNC, qhuff.EPROTO,
                                          qhuff.EBLOCKED}
            assert (d.dyn_id != D.DYN_NONE).sum() > 100
    assert total > 1000
    r = subprocess.run([exe] + args, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(r.stdout.strip().split("\n")) == len(sets)
