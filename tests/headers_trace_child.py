"""Helper of test_decode_headers_trace.py; not a test module.

The path-trace build of the library (libqhuff_trace.so, `make trace`) writes
one record a tile saying which path the kernel took.  qhuff loads its library
once per process (QHUFF_LIB), so the records of qhuff_decode_headers are read
in a child process: run as a program (`headers_trace_child.py OUT`), every
case of cases() is one scan + decode; its results are first compared with the
model -- the trace build must be correct before its records are believed --
and one JSON line a case goes to OUT: {"id", "ok", "tiles": [{"staged",
"path", "units", "var"}]}.

A launch that raises or leaves a device error ends the child (exit status
3): nothing more is started on a device that may have faulted."""
import json
import os
import random
import sys

import numpy as np

import _paths  # noqa: F401
import headers_decode_model as D
import limits as L

HERE = os.path.dirname(os.path.abspath(__file__))


def trace_lib():
    return os.path.join(os.path.dirname(HERE), "ls-qpack_amd",
                        "libqhuff_trace.so")


def cases():
    """{id: (sections, a0)}: the tiles on each side of the decode kernel's
    three comparisons, a wire-free tile and an unstaged one"""
    import test_decode_headers as T
    rng = random.Random(31)
    out = {"wire_free": ([T.sec(*[T.indexed(i) for i in range(32)])], 0),
           "unstaged": ([T.sec(T.indexed(T.LONG_VAL), *T.ordinary(rng, 29),
                               T.nameref(T.LONG_NAME, bytes(4096)),
                               T.indexed(T.LONG_NAME))], 0),
           "three_tiles": ([T.sec(*T.ordinary(rng, 70))], 5)}
    for n in (L.FIX_MAX, L.FIX_MAX + 1):
        out["arena%d" % n] = ([T.arena_tile(n, 15)], 0)
    for total in (D.OUT_FAST, D.OUT_FAST + 1):
        out["out%d" % total] = ([T.sec(*T.out_tile(total))], 0)
    for span in (3072, 3073):
        out["span%d" % span] = ([T.span_tile(span)], 14)
    return out


def expect(d):
    """the records D.layout() predicts for d's tiles (the buffer's base is
    16-byte aligned): place() runs once on a staged tile and not at all on
    an unstaged one"""
    return [{"staged": p["staged"], "path": "fast" if p["fast"] else "slow",
             "units": int(p["staged"]),
             "var": int(p["staged"] and not p["fixed"])}
            for p in D.layout(d)]


def main(out_path):
    import torch
    import qhuff
    import test_decode_headers as T
    assert os.path.samefile(qhuff.LIB_PATH, trace_lib())
    codec = qhuff.Codec(0)
    with open(out_path, "w") as f:
        for cid, (secs, a0) in cases().items():
            d = D.Decoded(secs, a0=a0)
            try:
                res = T.run_device(codec, d)
                torch.cuda.synchronize()
                if codec.device_error() != 0:
                    raise RuntimeError("device error")
                rec = L.trace_records(codec.profile_read())
                scan, dec = T.fetch_device(d, res)
            except Exception as e:                   # noqa: BLE001
                print("%s: %r" % (cid, e), file=sys.stderr)
                sys.exit(3)
            ok = True
            try:
                T.check_scan(d, scan)
                T.check_decode(d, dec)
            except AssertionError:
                ok = False
            f.write(json.dumps({"id": cid, "ok": ok, "tiles": [
                {k: r[k] for k in ("staged", "path", "units", "var")}
                for r in rec]}) + "\n")
            f.flush()
    codec.close()


if __name__ == "__main__":
    main(sys.argv[1])
