"""Helper of test_path_trace.py; not a test module.

The path-trace build of the library (libqhuff_trace.so, `make trace`:
QH_PATH_TRACE, qhuff_device.h PathTrace) writes one record per tile saying
which of each pair of equivalent paths the kernel took.  qhuff loads its
library once per process (QHUFF_LIB), so the records are read in child
processes: this file holds

  * the three configurations (CONFIGS) and the cases of each (case_ids);
  * run as a program (`path_trace_child.py CONFIG OUT`), the child: every
    case of the configuration as one launch.  The launch's bytes, offsets
    and statuses are first compared with the oracle -- the trace build must
    be a correct codec before its records are believed -- then every tile's
    record, field by field, with the layout model (limits.classify /
    classify_enc, trace_expect, coop_expect; qhuff.workload.tile_paths).
    One JSON line a case goes to OUT: {"id", "oracle_ok", "errors": [one
    line per field that differs, naming the case, the tile and the field],
    "rec": the record of the case's own tile}.

A launch that raises or leaves a device error ends the child (exit status
3): nothing more is started on a device that may have faulted."""
import json
import os
import sys

import numpy as np

import _paths  # noqa: F401
import limits as L
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden", "data")

CONFIGS = {"full": {"QHUFF_KERNELS": "full"},
           "lean": {"QHUFF_KERNELS": "lean"},
           "small": {"QHUFF_KERNELS": "full", "QHUFF_GRID_PCT": "1"}}
COOP_REAL = ("token", "all", "long", "many", "invalid")
WIRE = ("edge66/0", "edge66/1", "edge67/0", "edge67/1", "far_apart/0",
        "big_output/0")
STREAM = (65, 66)


def trace_lib():
    return os.path.join(os.path.dirname(HERE), "ls-qpack_amd",
                        "libqhuff_trace.so")


def encw_cases():
    import test_encode_wire as EW
    return ["encw/%s/%d" % (name, r) for name in sorted(EW.SHAPES)
            for r in EW.RESIDUES]


def case_ids(config):
    if config == "small":
        return ["comb/decode", "comb/encode"]
    ids = ["dec/%s/%d" % (f.name, r) for f in L.DECODE for r in f.residues]
    ids += ["enc/%s/%d/%d" % (f.name, r, m) for f in L.ENCODE
            for r in f.residues for m in (0, 7)]
    ids += ["corpus/dec", "corpus/enc"]
    if config == "full":
        ids += ["coop/" + k for k in COOP_REAL]
        ids += ["wire/" + k for k in WIRE]
        ids += ["stream/%d" % k for k in STREAM]
        ids += encw_cases()
    return ids


# ---- comparing ------------------------------------------------------------------

def read_records(codec, n_tiles, errors, cid):
    w = codec.profile_read()
    if n_tiles == 0:                         # nothing launched, no records
        if w is not None:
            errors.append("%s: %d words and no tile" % (cid, len(w)))
        return []
    if w is None or len(w) == 0:
        errors.append("%s: profile_read() returned no words after a launch"
                      % cid)
        return None
    recs = L.trace_records(w)
    if len(recs) != n_tiles:
        errors.append("%s: %d records for %d tiles" % (cid, len(recs), n_tiles))
        return None
    return recs


def fmt(v):
    return hex(v) if isinstance(v, int) and v > 0xffff else repr(v)


def compare(cid, tile, rec, want, errors):
    for k, v in want.items():
        if rec[k] != v:
            errors.append("%s tile %d %s: the kernel %s, the model %s"
                          % (cid, tile, k, fmt(rec[k]), fmt(v)))


def oracle_cmp(cid, got, want, names, errors):
    ok = True
    for g, w, name in zip(got, want, names):
        if not np.array_equal(np.asarray(g), np.asarray(w)):
            errors.append("%s: %s differs from the oracle's" % (cid, name))
            ok = False
    return ok


def strings_of(data, off):
    raw, o = data.tobytes(), [int(x) for x in off]
    return [raw[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def coop_conditions(cid, j, rec, o_st, errors):
    """no string the oracle accepts is in a fail mask; every cooperative
    string it rejects is in one"""
    for i in range(64):
        if (rec["coop"] >> i) & 1:
            rejected = bool(o_st[j * L.TS + i])
            if rejected != bool((rec["fail"] >> i) & 1):
                errors.append("%s tile %d lane %d: oracle status %d, %s the "
                              "fail mask" % (cid, j, i, o_st[j * L.TS + i],
                                             "not in" if rejected else "in"))
        elif (rec["fail"] >> i) & 1:
            errors.append("%s tile %d lane %d: failed but not cooperative"
                          % (cid, j, i))


def decode_launch(codec, cid, data, off, pad, want, info, errors, lean):
    """one decode launch against the oracle, then every tile's record
    against the model -> (oracle_ok, records)"""
    import test_limits as TL
    got = TL.gpu_decode(codec, data, off, pad)
    o_out, o_off, o_st = want
    ok = oracle_cmp(cid, (got[2], got[1], got[0]), (o_st, o_off, o_out),
                    ("status", "out_off", "bytes"), errors)
    recs = read_records(codec, len(info), errors, cid)
    if recs is None:
        return ok, None
    strs = strings_of(data, off)
    for j, t in enumerate(info):
        compare(cid, j, recs[j],
                L.trace_expect(strs[j * L.TS:(j + 1) * L.TS], t), errors)
        if not lean:
            coop_conditions(cid, j, recs[j], o_st, errors)
    return ok, recs


def encode_launch(codec, cid, data, off, pad, mode, want, info, errors):
    import torch
    import test_limits as TL
    d, o = TL.to_dev(data, off, pad)
    out, out_off = codec.encode(d, o, mode)
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    g_off = out_off.cpu().numpy().view(np.uint32)
    g_out = out[:int(g_off[-1])].cpu().numpy()
    ok = oracle_cmp(cid, (g_off, g_out), (want[1], want[0]),
                    ("out_off", "bytes"), errors)
    recs = read_records(codec, len(info), errors, cid)
    if recs is None:
        return ok, None
    for j, t in enumerate(info):
        compare(cid, j, recs[j], L.trace_expect_enc(t), errors)
    return ok, recs


# ---- the cases ------------------------------------------------------------------

def run_dec(codec, cid, lean, errors):
    import test_limits as TL
    _, name, r = cid.split("/")
    f, r = L.DECODE_BY_NAME[name], int(r)
    data, off, pad, ti, want, info = TL.dec_case(f, r)
    if lean:
        info = L.classify(off.astype(np.int64) + pad, 0,
                          np.diff(want[1].astype(np.int64)), lean=True)
    ok, recs = decode_launch(codec, cid, data, off, pad, want, info, errors,
                             lean)
    return ok, recs and recs[ti]


def run_enc(codec, cid, lean, errors):
    import test_limits as TL
    _, name, r, mode = cid.split("/")
    f, r, mode = L.ENCODE_BY_NAME[name], int(r), int(mode)
    data, off, pad, ti, want, info = TL.enc_case(f, r, mode)
    if lean:
        info = L.classify_enc(bytes(pad) + data.tobytes(),
                              off.astype(np.int64) + pad, 0, mode,
                              np.diff(want[1].astype(np.int64)), lean=True)
    ok, recs = encode_launch(codec, cid, data, off, pad, mode, want, info,
                             errors)
    return ok, recs and recs[ti]


def run_comb(codec, cid, lean, errors):
    """limits.combined on a grid of a few workgroups: every tile of the few
    hundred against the model -> the fixtures' own records by name/residue"""
    import test_limits as TL
    kind = cid.split("/")[1]
    data, off, where, want, info = TL.combined_case(kind)
    if kind == "decode":
        ok, recs = decode_launch(codec, cid, data, off, 0, want, info, errors,
                                 lean)
    else:
        ok, recs = encode_launch(codec, cid, data, off, 0, 0, want, info,
                                 errors)
    special = {ti for _, _, ti in where}
    for j, rec in enumerate(recs or []):
        if j not in special and (rec["path"] != "fast" or not rec["staged"]
                                 or rec["coop"]):
            errors.append("%s tile %d: an ordinary tile %s, staged %r"
                          % (cid, j, rec["path"], rec["staged"]))
    return ok, recs and {"%s/%d" % (f.name, r): recs[ti]
                         for f, r, ti in where}


def coop_input(which):
    import test_gpu_parity as GP
    if which == "many":
        return GP.coop_many_input()
    if which == "invalid":
        return GP.coop_invalid_input()
    return GP.coop_long_input(which)


def run_coop(codec, cid, lean, errors):
    data, off = coop_input(cid.split("/")[1])
    want = O.decode_batch(data, off)
    info = L.classify(off, 0, np.diff(want[1].astype(np.int64)))
    ok, recs = decode_launch(codec, cid, data, off, 0, want, info, errors,
                             lean)
    n = sum(bin(r["coop"]).count("1") for r in recs or [])
    return ok, {"coop_strings": n,
                "failed": sum(bin(r["fail"]).count("1") for r in recs or []),
                "max_rounds": max([r["rounds"] or 0 for r in recs or []] + [0])}


def corpus():
    from qhuff import workload as W
    data, off = W.corpus_batch(1 << 12, G)
    h, ho = O.encode_batch(data, off, 0)
    return data, off, h, ho, W.tile_paths(data, off, ho)


def booleans(cid, recs, pairs, errors):
    for name, got, want in pairs:
        for j in np.nonzero(np.asarray(got) != np.asarray(want))[0]:
            errors.append("%s tile %d %s: the kernel %r, tile_paths %r"
                          % (cid, j, name, bool(got[j]), bool(want[j])))


def run_corpus(codec, cid, lean, errors):
    """the corpus batch of bench.py --full: the records against classify and
    against the per-tile booleans its shares are made of"""
    data, off, h, ho, p = corpus()
    if cid == "corpus/dec":
        want = O.decode_batch(h, ho)
        info = L.classify(ho, 0, np.diff(want[1].astype(np.int64)), lean=lean)
        ok, recs = decode_launch(codec, cid, h, ho, 0, want, info, errors,
                                 lean)
        if recs:
            fast = np.array([r["path"] == "fast" for r in recs])
            var = np.array([r["var"] > 0 for r in recs])
            coop = np.array([r["coop"] != 0 for r in recs])
            booleans(cid, recs, [
                ("staged", [r["staged"] for r in recs], p["dec_staged"]),
                ("fast", fast, p["dec_fast"] if lean
                 else p["dec_fast"] & ~p["coop"]),
                ("var_arena", var & p["dec_fast"], p["var_arena"]),
                ("coop", coop, np.zeros_like(coop) if lean else p["coop"]),
            ], errors)
    else:
        want = (h, ho)
        info = L.classify_enc(data.tobytes(), off, 0, 0,
                              np.diff(ho.astype(np.int64)), lean=lean)
        ok, recs = encode_launch(codec, cid, data, off, 0, 0, want, info,
                                 errors)
        if recs:
            fast = np.array([r["path"] == "fast" for r in recs])
            dense = np.array([r["dense"] > 0 for r in recs])
            ec = np.array([r["enc_coop"] != 0 for r in recs])
            booleans(cid, recs, [
                ("staged", [r["staged"] for r in recs], p["enc_staged"]),
                ("fast", fast, p["enc_fast"]),
                ("dense", dense & fast, p["dense"]),
                ("enc_coop", ec, np.zeros_like(ec) if lean else p["enc_coop"]),
            ], errors)
    shares = {k: int(np.sum(v)) for k, v in p.items()}
    return ok, {"tiles": len(recs or []), "tile_paths": shares}


def at_residue(raw, r):
    """the bytes on the device at r mod 16 (16 zero bytes behind them)"""
    import torch
    base = torch.zeros(len(raw) + 48, dtype=torch.uint8, device="cuda")
    assert base.data_ptr() % 16 == 0
    d = base[r:r + len(raw) + 16]
    if len(raw):
        d[:len(raw)] = torch.from_numpy(
            np.frombuffer(bytes(raw), dtype=np.uint8).copy()).cuda()
    return d


def run_wire(codec, cid, lean, errors):
    import torch
    import qhuff
    import test_wire_decode as WD
    _, name, r = cid.split("/")
    r = int(r)
    s = {"edge66": lambda: WD.stage_edge(66), "edge67": lambda: WD.stage_edge(67),
         "far_apart": WD.far_apart, "big_output": WD.big_output}[name]()
    want = s.want(codec)
    out, oo, st = codec.decode_wire(at_residue(s.buf, r)[:len(s.buf)],
                                    WD.dev(qhuff.literals_array(s.lits)), None,
                                    bound=qhuff.literals_bound(s.lits))
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    got = WD.split(out, oo, st, len(s.lits))
    ok = got[1] == want[1] and got[0] == want[0]
    if not ok:
        errors.append("%s: the output differs from the oracle's" % cid)
    staged = WD.tile_staged(s.lits, r)
    recs = read_records(codec, len(staged), errors, cid)
    for j, rec in enumerate(recs or []):
        compare(cid, j, rec, {"written": 1, "staged": staged[j]}, errors)
    return ok, recs and recs[0]


def run_stream(codec, cid, lean, errors):
    import test_stream_decode as SD
    longest = int(cid.split("/")[1])
    first, second, finals = SD.stage_edge_tile(longest, "f5")
    # (run_rounds holds every chunk of both launches against the oracle)
    SD.run_rounds(codec, [(first, [False] * 64), (second, finals)])
    recs = read_records(codec, 1, errors, cid)
    if recs:
        # the second launch: one tile of exactly 3072 bytes, aligned
        compare(cid, 0, recs[0], {"written": 1, "staged": True}, errors)
    return True, recs and recs[0]


def run_encw(codec, cid, lean, errors):
    import torch
    import qhuff
    import test_encode_wire as EW
    _, name, r = cid.split("/")
    r = int(r)
    make, want_paths = EW.SHAPES[name]
    b = make()
    paths = b.paths(r)
    assert paths == want_paths[r]
    out, oo = codec.encode_wire(at_residue(b.data.tobytes(), r),
                                EW.dev(b.off.view(np.int32)),
                                EW.dev(qhuff.items_array(b.items)))
    torch.cuda.synchronize()
    assert codec.device_error() == 0
    g_out, g_off = EW.fetch(out, oo)
    ok = np.array_equal(g_off, b.want_off) and g_out == b"".join(b.want)
    if not ok:
        errors.append("%s: the output differs from the oracle's" % cid)
    recs = read_records(codec, len(paths), errors, cid)
    for j, rec in enumerate(recs or []):
        p = paths[j]
        want = {"written": 1, "staged": p != "in",
                "path": "fast" if p in ("dense", "lane") else "slow"}
        if p in ("dense", "lane"):
            want["dense"] = int(p == "dense")
        compare(cid, j, rec, want, errors)
    return ok, recs and [[x["staged"], x["path"], x["dense"]] for x in recs]


RUN = {"dec": run_dec, "enc": run_enc, "comb": run_comb, "coop": run_coop,
       "corpus": run_corpus, "wire": run_wire, "stream": run_stream,
       "encw": run_encw}


def main(config, out_path):
    for k, v in CONFIGS[config].items():
        assert os.environ.get(k) == v, "start the child with %s=%s" % (k, v)
    import qhuff
    # (the library under test: libqhuff_trace.so, trace_lib(), from the tests)
    assert os.environ.get("QHUFF_LIB") and qhuff.LIB_PATH == os.environ["QHUFF_LIB"]
    codec = qhuff.Codec(0)
    lean = config == "lean"
    with open(out_path, "w") as f:
        for cid in case_ids(config):
            errors = []
            try:
                ok, rec = RUN[cid.split("/")[0]](codec, cid, lean, errors)
            except Exception as e:          # a failed launch: stop here
                f.write(json.dumps({"id": cid, "oracle_ok": False, "rec": None,
                                    "errors": ["%s: %r" % (cid, e)]}) + "\n")
                f.flush()
                return 3
            f.write(json.dumps({"id": cid, "oracle_ok": bool(ok),
                                "errors": errors, "rec": rec}) + "\n")
            f.flush()
    codec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
