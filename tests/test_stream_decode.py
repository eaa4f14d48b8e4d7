"""qhuff_decode_stream: strings continued across chunks (include/qhuff.h).

The expectation is the oracle's resumable nibble decoder
(oq_huff_decode_full, the reference's lsqpack_huff_decode_full), driven once
per chunk per string with a state kept per string and a dst that cannot run
out.  Compared per chunk: the emitted bytes, the status (END_SRC <-> MORE)
and `eos`.  The node ids (state.state) are each decoder's own numbering and
are never compared.

The *node set*: for each symbol s and phase k the bits code('0') x (5k mod 8)
+ code(s) + code('a'), padded with ones -- 2,048 strings whose byte cuts
leave the decoder on every one of the code tree's 256 internal nodes."""
import ctypes as C
import functools
import json
import os
import random

import numpy as np
import pytest

import _paths  # noqa: F401
import oracle_lib as O
import qhuff
from qhuff import workload

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BIG = 1 << 17                    # the oracle's dst: no chunk here fills it
GUARD = 256


# ---- the oracle, one chunk at a time -----------------------------------------

_dst = C.create_string_buffer(BIG)


def fresh():
    return O.DecState(0, 0, 0)


def oracle_chunk(st, chunk, final):
    """lsqpack_huff_decode_full on one chunk -> (status as QHUFF_DEC_*, the
    bytes it emitted, eos); st is updated"""
    src = C.create_string_buffer(bytes(chunk), len(chunk) + 1)
    rv = O.lib().oq_huff_decode_full(src, len(chunk), _dst, BIG, C.byref(st),
                                     int(final))
    if rv.status == O.ERROR:
        return qhuff.DEC_ERROR, b"", None
    assert rv.status == (O.OK if final else O.END_SRC)
    assert rv.n_src == len(chunk)
    return (qhuff.DEC_OK if final else qhuff.DEC_MORE,
            C.string_at(_dst, rv.n_dst), int(st.eos))


def bits_to_bytes(bits):
    bits = bits + "1" * (-len(bits) % 8)
    return bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))


@functools.lru_cache(maxsize=None)
def code_bits(sym):
    c, n = O.code_of(sym)
    return format(c, "0%db" % n)


@functools.lru_cache(maxsize=None)
def node_set():
    out = []
    for s in range(256):
        for k in range(8):
            out.append(bits_to_bytes(code_bits(ord("0")) * ((5 * k) % 8)
                                     + code_bits(s) + code_bits(ord("a"))))
    return out


def node_set_pairs():
    """every (first piece, second piece) of every node-set string"""
    return [(s[:c], s[c:]) for s in node_set() for c in range(len(s) + 1)]


def pack(strings):
    off = np.zeros(len(strings) + 1, dtype=np.uint32)
    np.cumsum([len(s) for s in strings], out=off[1:])
    data = np.frombuffer(b"".join(strings), dtype=np.uint8).copy()
    return data, off


# ---- CPU tests ----------------------------------------------------------------

def test_symbols_and_null_arguments():
    L = qhuff.lib()
    for name in ("qhuff_decode_stream_bound", "qhuff_decode_stream",
                 "qhuff_decode_stream_host"):
        assert hasattr(L, name) and name in qhuff.EXPORTS
    assert qhuff.DEC_MORE == 2 and qhuff.STREAM_FINAL == 1
    off = np.zeros(2, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.qhuff_decode_stream(None, None, p(off), 0, None, None, None,
                                 p(off), None, None) == qhuff.EINVAL
    assert L.qhuff_decode_stream_host(None, None, p(off), 0, None, None, None,
                                      p(off), None) == qhuff.EINVAL
    for ln in (0, 1, 4, 5, 8, 66, 65535, 1 << 24):
        assert qhuff.decode_stream_bound(ln, 1) >= 8 * ln // 5 + 1
    assert qhuff.decode_stream_bound(100, 7) >= 8 * 100 // 5 + 7
    hdr = open(qhuff.HEADER).read()
    for word in ("QHUFF_FEATURE_STREAM 1", "QHUFF_DEC_MORE     2",
                 "QHUFF_STREAM_FINAL 1"):
        assert word in hdr
    assert "#define QHUFF_ABI_VERSION 7" in hdr


def test_harness_self_check():
    """the node set reaches all 256 oracle states after the first piece, and
    the two pieces' outputs concatenate to the complete-string decode"""
    strs = node_set()
    assert len(strs) == 2048 and max(len(s) for s in strs) <= 9
    pairs = node_set_pairs()
    assert len(pairs) == 13362
    states = set()
    whole = {s: O.huff_decode(s, full=True) for s in set(strs)}
    for a, b in pairs:
        st = fresh()
        s1, o1, _ = oracle_chunk(st, a, False)
        assert s1 == qhuff.DEC_MORE
        states.add(int(st.state))
        s2, o2, _ = oracle_chunk(st, b, True)
        assert s2 == qhuff.DEC_OK
        assert whole[a + b] == (O.OK, o1 + o2)
    assert states == set(range(256))


# ---- GPU harness ----------------------------------------------------------------

@pytest.fixture(scope="module")
def codec():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a GPU")
    c = qhuff.Codec(0)
    yield c
    c.close()


def gpu_round(codec, chunks, state, flags, host=False):
    """one launch -> (per-chunk bytes, status, new state)"""
    import torch
    data, off = pack(chunks)
    n = len(chunks)
    if host:
        out, oo, status, st = codec.decode_stream_host(data, off, state, flags)
        out = np.asarray(out)
    else:
        d = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda")
        if len(data):
            d[:len(data)] = torch.from_numpy(data).cuda()
        o = torch.from_numpy(off.astype(np.int64)).to(torch.int32).cuda()
        st = torch.from_numpy(np.ascontiguousarray(state)).cuda()
        fl = None if flags is None else torch.from_numpy(flags).cuda()
        out, oo, status, st = codec.decode_stream(d, o, st, fl)
        torch.cuda.synchronize()
        assert codec.device_error() == 0
        oo = oo.cpu().numpy().view(np.uint32)
        out = out[:int(oo[-1])].cpu().numpy()
        status = status.cpu().numpy()
        st = st.cpu().numpy()
    assert oo[0] == 0 and len(oo) == n + 1
    raw = out.tobytes()
    return ([raw[oo[i]:oo[i + 1]] for i in range(n)], np.asarray(status),
            np.array(st[:n]), oo)


def run_rounds(codec, rounds, host=False, null_flags_when_none_final=True):
    """rounds: per launch (chunks, finals) over the same n strings.  Every
    chunk against the oracle.  A string that ended (final, or ERROR) starts
    afresh in both decoders with its next chunk.  Returns the statuses."""
    n = len(rounds[0][0])
    ost = [fresh() for _ in range(n)]
    gst = np.zeros((max(n, 1), 2), dtype=np.uint8)
    seen = []
    for chunks, finals in rounds:
        assert len(chunks) == n and len(finals) == n
        flags = np.array([qhuff.STREAM_FINAL if f else 0 for f in finals],
                         dtype=np.uint8)
        if not any(finals) and null_flags_when_none_final:
            flags = None
        elif n == 0:
            flags = np.zeros(1, dtype=np.uint8)
        outs, status, gst2, oo = gpu_round(codec, chunks, gst, flags, host)
        gst = np.zeros((max(n, 1), 2), dtype=np.uint8)
        gst[:n] = gst2
        pos = 0
        for i in range(n):
            ws, wo, we = oracle_chunk(ost[i], chunks[i], finals[i])
            assert status[i] == ws, (i, chunks[i].hex(), finals[i])
            assert outs[i] == wo, (i, chunks[i].hex(), finals[i])
            assert oo[i] == pos
            pos += len(wo)
            if ws != qhuff.DEC_ERROR:
                assert gst[i, 1] == we, (i, chunks[i].hex(), finals[i])
            if ws != qhuff.DEC_MORE:
                ost[i] = fresh()
                gst[i] = 0
        assert oo[n] == pos
        seen.append(status.copy())
    return seen


def two_rounds(pairs):
    return [([a for a, _ in pairs], [False] * len(pairs)),
            ([b for _, b in pairs], [True] * len(pairs))]


def load_kats():
    with open(os.path.join(G, "kat_huff_decode.json")) as f:
        kat = json.load(f)["decode_ok"]
    return sorted((bytes.fromhex(k["huff"]) for k in kat), key=len)


def encoded(strings):
    data, off = pack(strings)
    h, ho = O.encode_batch(data, off, 0)
    raw = h.tobytes()
    return [raw[ho[i]:ho[i + 1]] for i in range(len(strings))]


def token_payloads(n, seed, lo=8, hi=64):
    data, off = qhuff.synth_batch(n, seed=seed, min_len=lo, max_len=hi)
    raw = data.tobytes()
    return encoded([raw[off[i]:off[i + 1]] for i in range(n)])


# ---- GPU tests ------------------------------------------------------------------

@pytest.mark.gpu
def test_node_set(codec):
    """every internal node saved by one launch and resumed by the next"""
    st = run_rounds(codec, two_rounds(node_set_pairs()))
    assert (st[0] == qhuff.DEC_MORE).all() and (st[1] == qhuff.DEC_OK).all()


STAGE = 3072                     # a tile's staged input bytes, at most


@pytest.mark.gpu
def test_node_set_past_the_stage(codec):
    """the node set on tiles past the stage: 63 pairs to a tile of 64, the
    64th string a long payload whose two pieces each exceed the stage, so
    every chunk of both launches is sized and decoded from global memory
    (stop on a code past the chunk's end, resume on a pending code)"""
    rng = random.Random(63)
    long_ = encoded([bytes(rng.choice(qhuff.TOKEN_ALPHABET)
                           for _ in range(11000))])[0]
    assert len(long_) >= 3100
    room = len(long_) - 2 * (STAGE + 1)
    assert room >= 255
    nodes = node_set_pairs()
    pairs = []
    for t, i in enumerate(range(0, len(nodes), 63)):
        cut = STAGE + 1 + (37 * t) % (room + 1)
        pairs += nodes[i:i + 63] + [(long_[:cut], long_[cut:])]
    tiles = -(-len(pairs) // 64)
    assert tiles == 213
    rounds = two_rounds(pairs)
    for chunks, _ in rounds:
        _, off = pack(chunks)
        for t in range(tiles):
            lo, hi = 64 * t, min(64 * t + 64, len(chunks))
            assert int(off[hi]) - int(off[lo]) > STAGE
    st = run_rounds(codec, rounds)
    assert (st[0] == qhuff.DEC_MORE).all() and (st[1] == qhuff.DEC_OK).all()


@pytest.mark.gpu
def test_kats_at_every_cut(codec):
    k17, k283, k2807 = load_kats()
    assert (len(k17), len(k283), len(k2807)) == (17, 283, 2807)
    pairs = [(k[:c], k[c:]) for k in (k17, k283) for c in range(len(k) + 1)]
    rng = random.Random(2807)
    pairs += [(k2807[:c], k2807[c:])
              for c in sorted(rng.sample(range(len(k2807) + 1), 64))]
    st = run_rounds(codec, two_rounds(pairs))
    assert (st[1] == qhuff.DEC_OK).all()


@pytest.mark.gpu
def test_many_small_pieces(codec):
    """1-byte chunks over successive launches: a 30-bit code spans 4-5
    chunks (a state leads to a state with no output); a quarter of the
    chunks are empty, and half of the strings end on an empty final chunk"""
    rng = random.Random(5)
    strs = node_set() + token_payloads(2000, seed=5, lo=4, hi=32)
    plans = []
    for s in strs:
        plan = []
        for b in s:
            while rng.random() < 0.25:
                plan.append((b"", False))
            plan.append((bytes([b]), False))
        if rng.random() < 0.5:
            plan.append((b"", True))
        else:
            plan[-1] = (plan[-1][0], True)
        plans.append(plan)
    depth = max(len(p) for p in plans)
    rounds = []
    for r in range(depth):
        row = [p[r] if r < len(p) else (b"", False) for p in plans]
        rounds.append(([c for c, _ in row], [f for _, f in row]))
    seen = run_rounds(codec, rounds)
    ends = sum(int((s != qhuff.DEC_MORE).sum()) for s in seen)
    assert ends == len(strs)
    assert all((s != qhuff.DEC_ERROR).all() for s in seen)


@pytest.mark.gpu
def test_errors(codec):
    rng = random.Random(6)
    ones3 = bits_to_bytes(code_bits(ord("0")) + "111")       # ends 3 ones deep
    cases = [
        [(b"\xff\xff\xff", False), (b"\xff", False)],   # EOS, not final
        [(b"\xff", False), (b"", True)],                # 8 ones
        [(b"\xfe", False), (b"", True)],
        [(ones3, False), (b"\xff", True)],              # 11 ones
        [(ones3, False), (b"", True)],                  # 3 ones: accepted
        [(b"\xff\xff\xff\xff", False), (b"", False)],   # EOS in one chunk
        [(b"\xff\xff", False), (b"\xff\xfc", True)],
    ]
    for _ in range(5000):
        s = bytes(rng.randrange(256) for _ in range(rng.randint(1, 24)))
        c = rng.randint(0, len(s))
        cases.append([(s[:c], False), (s[c:], True)])
    rounds = [([c[r][0] for c in cases], [c[r][1] for c in cases])
              for r in range(2)]
    st = run_rounds(codec, rounds)
    E, M, K = qhuff.DEC_ERROR, qhuff.DEC_MORE, qhuff.DEC_OK
    assert [int(x) for x in st[0][:7]] == [M] * 5 + [E, M]
    assert [int(x) for x in st[1][:2]] == [E, E]
    assert [int(x) for x in st[1][3:5]] == [E, K]
    assert (st[1] == E).sum() > 1000 and (st[1] == K).sum() > 10


def _invalid_1pc(strs, seed):
    rng = random.Random(seed)
    out = []
    for s in strs:
        if s and rng.random() < 0.01:
            s = s[:-1] + bytes([s[-1] ^ (1 << rng.randrange(8))])
        out.append(s)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_equals_decode_batch_when_all_final(codec, n):
    """zeroed states, every flag FINAL: qhuff_decode_batch's bytes, out_off
    and statuses"""
    import torch
    tok = token_payloads(n, seed=70 + n)
    dc, oc = workload.alphabet_c(n, seed=71 + n)
    rc = dc.tobytes()
    alc = encoded([rc[oc[i]:oc[i + 1]] for i in range(n)])
    for strs in (tok, alc, _invalid_1pc(tok, n)):
        data, off = pack(strs)
        d = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda")
        if len(data):
            d[:len(data)] = torch.from_numpy(data).cuda()
        o = torch.from_numpy(off.astype(np.int64)).to(torch.int32).cuda()
        w_out, w_off, w_st = codec.decode(d, o)
        fl = torch.full((max(n, 1),), qhuff.STREAM_FINAL, dtype=torch.uint8,
                        device="cuda")
        g_out, g_off, g_st, state = codec.decode_stream(d, o, None, fl)
        torch.cuda.synchronize()
        assert codec.device_error() == 0
        assert torch.equal(g_off, w_off)
        assert torch.equal(g_st, w_st)
        tot = int(w_off[-1].item())
        assert torch.equal(g_out[:tot], w_out[:tot])
        if n == 4097:
            assert (w_st == 0).sum() > 4000


@functools.lru_cache(maxsize=None)
def payload_65535():
    """a valid encoded string of exactly 65,535 bytes"""
    rng = random.Random(65535)
    alpha = qhuff.TOKEN_ALPHABET
    lens = workload.RFC_LEN
    s, bits, cap = bytearray(), 0, 8 * 65535
    while cap - bits >= 5:
        b = rng.choice(alpha)
        if bits + lens[b] > cap:
            b = ord("0")                     # 5 bits
        s.append(b)
        bits += int(lens[b])
    h = O.huffman_enc(bytes(s))
    assert len(h) == 65535
    return h


@pytest.mark.gpu
def test_shapes(codec):
    rng = random.Random(8)

    def long_tok(lo):
        return encoded([bytes(rng.choice(qhuff.TOKEN_ALPHABET)
                              for _ in range(lo))])[0]
    # 64 chunks x 100 B: a tile past the 3 KB stage
    strs = [long_tok(170 + i) for i in range(64)]
    assert min(len(s) for s in strs) > 100
    run_rounds(codec, two_rounds([(s[:100], s[100:]) for s in strs]))
    # chunks of 129 B and 300 B among short ones
    pairs = []
    for i in range(130):
        s = long_tok(500 + i)
        cut = (129, 300, rng.randint(0, 40))[i % 3]
        pairs.append((s[:cut], s[cut:]))
    run_rounds(codec, two_rounds(pairs))
    # one 65,535-byte payload at four cuts
    h = payload_65535()
    st = run_rounds(codec, two_rounds([(h[:c], h[c:])
                                       for c in (1, 3071, 3073, 65534)]))
    assert (st[1] == qhuff.DEC_OK).all()
    # 64 empty chunks: not final (flags = NULL), then final
    st = run_rounds(codec, [([b""] * 64, [False] * 64),
                            ([b""] * 64, [True] * 64)])
    assert (st[0] == qhuff.DEC_MORE).all() and (st[1] == qhuff.DEC_OK).all()
    # final and non-final chunks in one batch; flags given, and flags = NULL
    toks = token_payloads(300, seed=88)
    first = [(s, True) if i % 3 == 0 else (s[:len(s) // 2], False)
             for i, s in enumerate(toks)]
    second = [(b"", False) if i % 3 == 0 else (s[len(s) // 2:], i % 3 == 1)
              for i, s in enumerate(toks)]
    third = [(b"", i % 3 == 2) for i in range(len(toks))]
    rounds = [([c for c, _ in r], [f for _, f in r])
              for r in (first, second, third)]
    run_rounds(codec, rounds)
    none_final = [([s[:5] for s in toks], [False] * len(toks)),
                  ([s[5:9] for s in toks], [False] * len(toks))]
    run_rounds(codec, none_final, null_flags_when_none_final=True)
    run_rounds(codec, none_final, null_flags_when_none_final=False)


def stage_edge_tile(longest, content):
    """64 second chunks that are one staged tile of exactly 3072 bytes, all
    5-bit codes behind a state 4 bits into code('0') (first pieces as
    worst_case_batch): each fills floor((8 * len - 1) / 5) + 1 bytes, the
    most a chunk can.  longest 65: ten chunks at kStreamFixMaxLen, the
    fixed arena's limit; 66: ten more a byte past it, and the 3 * lane
    variable arena packed to 3072 bytes of input.  content "zeros": code('0')
    throughout (not final: the bits rarely end on a symbol); "f5": random
    5-bit symbols, so that a misplaced byte shows, final with ones for
    padding on every other chunk.  -> (first, second, finals)"""
    rng = random.Random(longest)
    lens = ([66] * 10 + [65] * 10 + [40] * 42 + [41] * 2 if longest == 66
            else [65] * 20 + [40] * 32 + [41] * 12)
    assert sum(lens) == 3072 and max(lens) == longest and len(lens) == 64
    rng.shuffle(lens)
    f5 = [s for s in range(256) if O.code_of(s)[1] == 5]
    assert bytes(f5) == b"012aceiost"
    second, finals = [], []
    for i, ln in enumerate(lens):
        if content == "zeros":
            second.append(b"\0" * ln)
            finals.append(False)
            continue
        k = (8 * ln - 1) // 5
        bits = rng.choice("01") + "".join(code_bits(rng.choice(f5))
                                          for _ in range(k))
        c = bits_to_bytes(bits)
        assert len(c) == ln and 8 * ln - len(bits) < 5
        second.append(c)
        finals.append(i % 2 == 0)
    return [b"\0\0\0"] * 64, second, finals


@pytest.mark.gpu
@pytest.mark.parametrize("content", ["zeros", "f5"])
@pytest.mark.parametrize("longest", [65, 66])
def test_stage_edge_tile(codec, longest, content):
    """a staged tile of exactly 3072 bytes whose every chunk decodes to the
    bound, with chunks at (65) and past (66) the fixed arena's limit"""
    first, second, finals = stage_edge_tile(longest, content)
    total = 0
    for a, b, f in zip(first, second, finals):
        st = fresh()
        assert oracle_chunk(st, a, False)[:2] == (qhuff.DEC_MORE, b"0000")
        ws, wo, _ = oracle_chunk(st, b, f)
        assert ws == (qhuff.DEC_OK if f else qhuff.DEC_MORE)
        assert len(wo) == (8 * len(b) - 1) // 5 + 1
        total += len(wo)
    assert total > 8 * 3072 // 5                 # more than 8/5 of the stage
    st = run_rounds(codec, [(first, [False] * 64), (second, finals)])
    assert (st[0] == qhuff.DEC_MORE).all()
    assert (st[1] == [qhuff.DEC_OK if f else qhuff.DEC_MORE
                      for f in finals]).all()


# ---- the buffer contract ---------------------------------------------------------

def carve(specs):
    """(name, bytes, residue mod 16) in order -> {name: (start, bytes)} and
    the arena's size: GUARD bytes either side of every buffer"""
    reg, pos = {}, 0
    for name, nbytes, res in specs:
        pos += GUARD
        pos += (res - pos) % 16
        reg[name] = (pos, int(nbytes))
        pos += int(nbytes) + GUARD
    return reg, pos + 16


def worst_case_batch():
    """chunks that fill floor(8 * len / 5) + 1 bytes: the state 4 bits into
    code('0'), then bytes that are all 5-bit codes (code('0') is five zero
    bits: zero bytes)"""
    assert code_bits(ord("0")) == "00000"
    lens = [28] * 64 + [64] * 20 + [0] * 44 + [66] * 20 + [0] * 44 \
        + [67] * 40 + [0] * 24 + [65, 8, 1, 2, 3, 99]
    first = [b"\0\0\0" if ln else b"" for ln in lens]    # "0000" + 4 bits
    second = [b"\0" * ln for ln in lens]
    return lens, first, second


@pytest.mark.gpu
@pytest.mark.parametrize("res", [1, 15])
@pytest.mark.parametrize("host", [False, True])
def test_buffer_contract(codec, res, host):
    """every buffer at its exact size in a dirty arena, byte buffers at
    residue `res` mod 16 (uint32 arrays at 4 or 12): guards, inputs, flags
    and the bytes of out past out_off[n] unchanged; the worst-case chunks
    fill the bound exactly"""
    import torch
    lens, first, second = worst_case_batch()
    n = len(lens)
    ost = [fresh() for _ in range(n)]
    for i in range(n):
        assert oracle_chunk(ost[i], first[i], False)[0] == qhuff.DEC_MORE
    # the states of the first pieces, from the library itself
    _, st1, state, _ = gpu_round(codec, first, np.zeros((n, 2), np.uint8), None)
    assert (st1 == qhuff.DEC_MORE).all()
    data, off = pack(second)
    off = off + 7                                   # in_off[0] != 0
    # final where the zero bits end on a symbol (accepted), and on a few
    # chunks where they do not (ERROR: 0 bytes)
    flags = np.array([1 if (i % 2 and (8 * ln - 1) % 5 == 0) or i % 16 == 5
                      or (ln == 0 and i % 2) else 0
                      for i, ln in enumerate(lens)], dtype=np.uint8)
    bound = qhuff.decode_stream_bound(len(data), n)
    assert bound == 8 * len(data) // 5 + n + 16
    r4 = 4 if res == 1 else 12
    specs = [("in", len(data), res), ("in_off", 4 * (n + 1), r4),
             ("state", 2 * n, res), ("flags", n, res), ("out", bound, res),
             ("out_off", 4 * (n + 1), r4), ("status", n, res)]
    reg, size = carve(specs)
    before = np.random.default_rng(res).integers(0, 256, size, dtype=np.uint8)

    def put(name, a):
        s, nb = reg[name]
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        assert len(b) == nb
        before[s:s + nb] = b
    put("in", data)
    put("in_off", off.astype(np.uint32))
    put("state", state)
    put("flags", flags)
    if host:
        mem = np.empty(size + 16, dtype=np.uint8)
        sh = (-mem.ctypes.data) % 16
        arena = mem[sh:sh + size]
        arena[:] = before
        base = arena.ctypes.data
    else:
        dev = torch.from_numpy(before).cuda()
        base = dev.data_ptr()
    assert base % 16 == 0
    a = lambda name, back=0: C.c_void_p(base + reg[name][0] - back)
    L = qhuff.lib()
    if host:
        rc = L.qhuff_decode_stream_host(
            codec._ctx, a("in", 7), a("in_off"), n, a("state"), a("flags"),
            a("out"), a("out_off"), a("status"))
        after = arena.copy()
    else:
        rc = L.qhuff_decode_stream(
            codec._ctx, a("in", 7), a("in_off"), n, a("state"), a("flags"),
            a("out"), a("out_off"), a("status"),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        after = dev.cpu().numpy()
    assert rc == 0 and codec.device_error() == 0
    get = lambda name, dt: after[reg[name][0]:reg[name][0]
                                 + reg[name][1]].view(dt)
    oo = get("out_off", np.uint32)
    status = get("status", np.uint8)
    out = get("out", np.uint8)
    gstate = get("state", np.uint8).reshape(n, 2)
    pos = 0
    for i in range(n):
        ws, wo, we = oracle_chunk(ost[i], second[i], bool(flags[i]))
        assert status[i] == ws
        assert oo[i] == pos
        assert out[pos:pos + len(wo)].tobytes() == wo
        if ws != qhuff.DEC_ERROR:
            assert gstate[i, 1] == we
            if lens[i] % 5:
                assert len(wo) == 8 * lens[i] // 5 + 1      # the bound, exactly
        pos += len(wo)
    assert oo[n] == pos
    may = np.zeros(size, dtype=bool)
    for name, w in (("out", pos), ("out_off", 4 * (n + 1)), ("status", n),
                    ("state", 2 * n)):
        may[reg[name][0]:reg[name][0] + w] = True
    bad = np.flatnonzero((before != after) & ~may)
    assert len(bad) == 0, [(int(i), [k for k, (s, nb) in reg.items()
                                     if s - GUARD <= i < s + nb + GUARD])
                           for i in bad[:8]]


@pytest.mark.gpu
def test_host_entry(codec):
    """the node set through qhuff_decode_stream_host"""
    st = run_rounds(codec, two_rounds(node_set_pairs()), host=True)
    assert (st[0] == qhuff.DEC_MORE).all() and (st[1] == qhuff.DEC_OK).all()
