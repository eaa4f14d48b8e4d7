"""What the five device-pointer tile calls share around their launch
(qhuff_host.cpp): qhuff_encode_batch, qhuff_decode_batch, qhuff_decode_stream,
qhuff_decode_wire and qhuff_encode_wire at the sizes where that code takes
another path (n = 0: out_off[0] alone is written; 64 and 65: each side of
the tile count's rounding), back to back on two streams of one context, with
launch timing on, and around the batch calls' kernel-variant state.

Expectations never come from the library: oracle_lib.encode_batch /
decode_batch for the batch calls, the oracle's resumable decoder one chunk at
a time for the stream call (test_stream_decode.oracle_chunk), its
complete-string decode of each Huffman payload for the wire call
(test_wire_decode.test_counts) and qpack_frames.enc_int +
oracle_lib.enc_enc_str per item for encode_wire
(test_encode_wire.item_bytes)."""
import functools
import os
import random

import numpy as np
import pytest

import _paths  # noqa: F401
import oracle_lib as O
import qhuff
import qpack_frames as Q
from test_encode_wire import item, item_bytes
from test_stream_decode import fresh, oracle_chunk
from test_wire_decode import lit

SIZES = (0, 1, 64, 65)
SENTINEL = 0xA5
E, D = qhuff.KIND_ENCODE, qhuff.KIND_DECODE
CALLS = ("encode", "decode", "stream", "wire", "encwire")
KINDS = {"encode": E, "decode": D, "stream": D, "wire": D, "encwire": E}


def pack(strings):
    off = np.zeros(len(strings) + 1, dtype=np.uint32)
    np.cumsum([len(s) for s in strings], out=off[1:])
    return np.frombuffer(b"".join(strings), dtype=np.uint8).copy(), off


class Case:
    """n strings of 1-8 token bytes, the inputs of the five calls over them
    and what each call has to return: want[call] = (per-string bytes,
    statuses or None, stream states or None)"""

    def __init__(self, n):
        rng = random.Random(7000 + n)
        self.n = n
        self.strings = [bytes(rng.choice(qhuff.TOKEN_ALPHABET)
                              for _ in range(rng.randint(1, 8)))
                        for _ in range(n)]
        self.data, self.off = pack(self.strings)
        # the Huffman payloads: what encode returns, what the decodes read
        self.huff, self.huff_off = O.encode_batch(self.data, self.off, 0)
        raw = self.huff.tobytes()
        payloads = [raw[self.huff_off[i]:self.huff_off[i + 1]]
                    for i in range(n)]
        d_out, d_off, d_st = O.decode_batch(self.huff, self.huff_off)
        assert not d_st.any() and np.array_equal(d_off, self.off)
        assert np.array_equal(d_out, self.data)
        chunks = [oracle_chunk(fresh(), p, True) for p in payloads]
        assert [c[1] for c in chunks] == self.strings
        # every third item an instruction's integer in front of its literal
        self.items = [item(i, 4, 0x50, 7, 0) if i % 3 == 0
                      else item(str_bits=7, str_first=0) for i in range(n)]
        assert qhuff.items_check(self.items) == (qhuff.OK, None)
        wire = [item_bytes(it, s) for it, s in zip(self.items, self.strings)]
        self.wire, self.wire_off = pack(wire)
        # the literals of that output, where they lie in it
        self.lits = []
        for i, (it, s, w) in enumerate(zip(self.items, self.strings, wire)):
            at = len(Q.enc_int(it.int_first, it.ival, 4)) if it.int_bits else 0
            assert len(w) - at - 1 < 127            # a one-byte length
            huffman = w[at] >> 7
            payload = w[at + 1:]
            if huffman:
                assert O.huff_decode(payload) == (O.OK, s)
            else:
                assert payload == s
            self.lits.append(lit(int(self.wire_off[i]) + at + 1, payload,
                                 huffman))
        assert qhuff.literals_check(self.lits) == (qhuff.OK, None)
        assert n < 64 or 0 < sum(l.huffman for l in self.lits) < n
        ok = [qhuff.DEC_OK] * n
        self.want = {
            "encode": (payloads, None, None),
            "decode": (self.strings, ok, None),
            "stream": (self.strings, [c[0] for c in chunks],
                       [c[2] for c in chunks]),
            "wire": (self.strings, ok, None),
            "encwire": (wire, None, None),
        }

    def bound(self, call):
        n = self.n
        return {"encode": qhuff.encode_bound(len(self.data), n, 0),
                "decode": qhuff.decode_bound(len(self.huff), n),
                "stream": qhuff.decode_stream_bound(len(self.huff), n),
                "wire": qhuff.literals_bound(self.lits),
                "encwire": qhuff.encode_wire_bound(len(self.data), n)}[call]


@functools.lru_cache(maxsize=None)
def case(n):
    return Case(n)


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
    """a device copy of a numpy array (never empty), pad zero bytes behind"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    t = torch.zeros(max(a.size + pad, 1), dtype=torch.from_numpy(a).dtype,
                    device="cuda")
    if a.size:
        t[:a.size] = torch.from_numpy(a).cuda()
    return t


class Inputs:
    """a case's inputs on the device, uploaded once per test"""

    def __init__(self, cs):
        self.cs = cs
        self.data, self.off = dev(cs.data, 16), dev(cs.off)
        self.huff, self.huff_off = dev(cs.huff, 16), dev(cs.huff_off)
        self.wire = dev(cs.wire, 16)
        self.lits = dev(qhuff.literals_array(cs.lits))
        self.items = dev(qhuff.items_array(cs.items))
        self.flags = dev(np.full(max(cs.n, 1), qhuff.STREAM_FINAL, np.uint8))


class Outputs:
    """sentinel-filled results of one call"""

    def __init__(self, cs, call):
        import torch
        full = lambda k, dt: torch.full((max(k, 1),), SENTINEL, dtype=dt,
                                        device="cuda")
        self.call, self.cs = call, cs
        self.out = full(cs.bound(call), torch.uint8)
        self.out_off = torch.full((cs.n + 1,), -1, dtype=torch.int32,
                                  device="cuda")
        self.status = full(cs.n, torch.uint8)
        self.state = torch.zeros((max(cs.n, 1), 2), dtype=torch.uint8,
                                 device="cuda")


def launch(codec, inp, res, stream=None, src=None):
    """one call into res; src: the Outputs of an encode (for decode) or of an
    encode_wire (for wire) whose device output this call reads"""
    n, call = inp.cs.n, res.call
    if call == "encode":
        codec.encode_into(inp.data, inp.off, n, 0, res.out, res.out_off,
                          stream)
    elif call == "decode":
        assert src is None or src.call == "encode"
        codec.decode_into(src.out if src else inp.huff,
                          src.out_off if src else inp.huff_off, n, res.out,
                          res.out_off, res.status, stream)
    elif call == "stream":
        codec.decode_stream_into(inp.huff, inp.huff_off, n, res.state,
                                 inp.flags, res.out, res.out_off, res.status,
                                 stream)
    elif call == "wire":
        assert src is None or src.call == "encwire"
        codec.decode_wire_into(src.out if src else inp.wire, inp.lits, n,
                               None, res.out, res.out_off, res.status, stream)
    else:
        assert call == "encwire"
        codec.encode_wire_into(inp.data, inp.off, inp.items, n, res.out,
                               res.out_off, stream)


def check(res):
    """a finished call's results against the case's expectation"""
    cs, n = res.cs, res.cs.n
    outs, status, eos = cs.want[res.call]
    oo = res.out_off.cpu().numpy().view(np.uint32)
    out = res.out.cpu().numpy()
    want_off = np.zeros(n + 1, dtype=np.uint32)
    np.cumsum([len(o) for o in outs], out=want_off[1:])
    assert np.array_equal(oo, want_off), res.call
    assert out[:int(oo[-1])].tobytes() == b"".join(outs), res.call
    if n == 0:
        assert oo[0] == 0
        assert (out == SENTINEL).all(), res.call
        assert (res.status.cpu().numpy() == SENTINEL).all(), res.call
    if status is not None:
        assert [int(s) for s in res.status.cpu().numpy()[:n]] == status, \
            res.call
    if eos is not None:
        assert [int(e) for e in res.state.cpu().numpy()[:n, 1]] == eos


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_sizes(codec, n):
    import torch
    inp = Inputs(case(n))
    for call in CALLS:
        res = Outputs(inp.cs, call)
        launch(codec, inp, res)
        torch.cuda.synchronize()
        assert codec.device_error() == 0
        check(res)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_two_streams(codec, n):
    """the calls alternately on two streams, no host synchronisation between
    them: a decode reads the encode's output, a decode_wire the
    encode_wire's, each launched on the other stream -- ordered by the
    context alone"""
    import torch
    inp = Inputs(case(n))
    s = [torch.cuda.Stream(), torch.cuda.Stream()]
    plan = [("encode", None), ("decode", 0), ("encwire", None), ("wire", 2),
            ("stream", None)] * 2
    plan = [(c, None if k is None else k + 5 * (i // 5))
            for i, (c, k) in enumerate(plan)]
    res = [Outputs(inp.cs, call) for call, _ in plan]
    torch.cuda.synchronize()             # the inputs and the sentinels
    for i, (call, k) in enumerate(plan):
        # (five calls a round: the second round's streams are swapped)
        launch(codec, inp, res[i], s[i % 2], None if k is None else res[k])
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    for r in res:
        check(r)


def _each_call(codec, inp):
    for call in CALLS:
        launch(codec, inp, Outputs(inp.cs, call))


@pytest.mark.gpu
def test_timing(codec):
    import torch
    inp, empty = Inputs(case(65)), Inputs(case(0))
    kinds = [KINDS[c] for c in CALLS]
    assert kinds == [E, D, D, D, E]
    codec.timing(True)
    try:
        codec.timing_read()
        _each_call(codec, inp)
        _each_call(codec, empty)         # (n = 0: no launch, no record)
        torch.cuda.synchronize()
        t = codec.timing_read()
        assert [k for k, _ in t] == kinds
        assert all(us > 0 for _, us in t)
        # every second launch of each kind, counted from the call
        codec.timing(True, every=2)
        _each_call(codec, inp)
        _each_call(codec, inp)
        torch.cuda.synchronize()
        t = codec.timing_read()
        seen, want = {E: 0, D: 0}, []
        for k in kinds * 2:
            if seen[k] % 2 == 0:
                want.append(k)
            seen[k] += 1
        assert want == [E, D, D, E, D]
        assert [k for k, _ in t] == want
        assert all(us > 0 for _, us in t)
    finally:
        codec.timing(False)
    assert codec.device_error() == 0
    _each_call(codec, inp)
    torch.cuda.synchronize()
    assert codec.timing_read() == []


@pytest.mark.gpu
def test_variant_state(codec):
    """the stream, wire and encode_wire calls leave the batch calls' variant
    of the last launch and a pending hint as they are"""
    import torch
    pin = {"lean": 0, "full": 1}.get(os.environ.get("QHUFF_KERNELS"))
    lean, full = (0, 1) if pin is None else (pin, pin)
    inp = Inputs(case(65))
    lean_calls = ("stream", "wire", "encwire")
    batch = {E: "encode", D: "decode"}

    def run(call):
        res = Outputs(inp.cs, call)
        launch(codec, inp, res)
        torch.cuda.synchronize()
        check(res)

    for kind in (E, D):
        # a hinted batch launch: the lean kernel, not the default
        codec.batch_hint(kind, 0)
        run(batch[kind])
        assert codec.kernel_variant(kind) == lean
    for call in lean_calls:
        run(call)
        assert codec.kernel_variant(E) == lean
        assert codec.kernel_variant(D) == lean
    for kind in (E, D):
        run(batch[kind])                 # no hint: the full kernel
        assert codec.kernel_variant(kind) == full
        codec.batch_hint(kind, 0)
    for call in lean_calls:
        run(call)
        assert codec.kernel_variant(E) == full
        assert codec.kernel_variant(D) == full
    for kind in (E, D):
        run(batch[kind])                 # the hint from before the lean calls
        assert codec.kernel_variant(kind) == lean
        run(batch[kind])                 # and it applied to that launch only
        assert codec.kernel_variant(kind) == full
    assert codec.device_error() == 0
