"""Helper of test_decode_headers_dyn_trace.py; not a test module.

headers_trace_child.py for qhuff_decode_headers_dyn: run as a program
(`headers_dyn_trace_child.py OUT`) under the path-trace build of the library
(QHUFF_LIB = libqhuff_trace.so), every case of cases() is one scan + decode
against the model, then one JSON line goes to OUT: {"id", "ok", "tiles":
[{"staged", "path", "units", "var", "dyn"}]} -- "dyn" the record's word 6, the
tile's output bytes that came from the table.

A launch that raises or leaves a device error ends the child (exit status
3): nothing more is started on a device that may have faulted."""
import json
import os
import random
import sys

import numpy as np

import _paths  # noqa: F401
import headers_dyn_model as D
import limits as L

HERE = os.path.dirname(os.path.abspath(__file__))


def trace_lib():
    return os.path.join(os.path.dirname(HERE), "ls-qpack_amd",
                        "libqhuff_trace.so")


def cases():
    """{id: (sections, entries, a0, table pad)}: the out stage's edge reached
    by dynamic bytes alone, the 4 KB entry, a tile of 64 table strings and a
    mixed batch of three tiles"""
    import test_decode_headers_dyn as T
    rng = random.Random(81)
    out = {}
    for total in (D.OUT_FAST, D.OUT_FAST + 1):
        ents = [(T.pat(47, i), T.pat(47 + (i == 9 and total > D.OUT_FAST),
                                     i + 50)) for i in range(32)]
        s = D.prefix_for(32, 32, 64) + b"".join(D.indexed_dyn(i)
                                                for i in range(32))
        out["out%d" % total] = ([s], ents, 0, 0)
    big = T.len_entries(big=True)
    k = len(big)
    out["entry4k"] = ([T.one_section(big, T.mixed_lines(T.len_entries(), 20, rng)
                                     + [D.indexed_dyn(k - 1 - 4)])], big, 3, 1)
    ents = T.len_entries()
    out["dyn64"] = ([T.one_section(ents, [D.indexed_dyn(len(ents) - 1 - i % 4)
                                          for i in range(31)])], ents, 0, 15)
    out["three_tiles"] = ([T.one_section(ents, T.mixed_lines(ents, 70, rng))],
                          ents, 5, 7)
    return out


def model(case):
    secs, ents, a0, pad = case
    return D.Decoded(secs, D.Table(ents, 0, 64, pad=pad), a0=a0)


def expect(d):
    """the records D.layout() predicts for d's tiles"""
    return [{"staged": p["staged"], "path": "fast" if p["fast"] else "slow",
             "units": int(p["staged"]),
             "var": int(p["staged"] and not p["fixed"]), "dyn": p["dyn"]}
            for p in D.layout(d, d.a0)]


def main(out_path):
    import qhuff
    import test_decode_headers_dyn as T
    assert os.path.samefile(qhuff.LIB_PATH, trace_lib())
    codec = qhuff.Codec(0)
    with open(out_path, "w") as f:
        for cid, case in cases().items():
            d = model(case)
            try:
                scan, dec = T.run_device(codec, d)
                words = codec.profile_read()
            except Exception as e:                   # noqa: BLE001
                print("%s: %r" % (cid, e), file=sys.stderr)
                sys.exit(3)
            rec = L.trace_records(words)
            dyn = np.asarray(words, dtype=np.uint64) \
                .reshape(-1, L.TRACE_WORDS)[:, 6]
            ok = True
            try:
                T.check_scan(d, scan)
                T.check_decode(d, dec)
            except AssertionError:
                ok = False
            f.write(json.dumps({"id": cid, "ok": ok, "tiles": [
                dict({k: r[k] for k in ("staged", "path", "units", "var")},
                     dyn=int(x)) for r, x in zip(rec, dyn)]}) + "\n")
            f.flush()
    codec.close()


if __name__ == "__main__":
    main(sys.argv[1])
