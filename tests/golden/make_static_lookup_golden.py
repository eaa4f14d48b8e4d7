#!/usr/bin/env python3
"""Regenerate tests/golden/static_lookup.json from the reference's lsqpack.c
(run where the reference's source tree exists).

Nothing here executes reference code: lsqpack.c is read as TEXT and the
initializer data of the four arrays of its static lookup (lsqpack.c:629-716)
is extracted as numbers, as make_golden.py does for static_table[]:

  name2id_plus_one[512]      [slot] = id + 1 (designated initializers)
  nameval2id_plus_one[512]
  name_hashes[99]            XXH32(name, LSQPACK_XXH_SEED) of every entry
  nameval_hashes[99]         XXH32(value, seed = the name's hash)

MANIFEST.sha256 is make_golden.py's and is left alone.
Usage: python tests/golden/make_static_lookup_golden.py REF_ROOT
(REF_ROOT: the reference's source tree, the directory that holds lsqpack.c)
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = sys.argv[1]


def array_body(text, name):
    """(text between the braces of `name[...] = { ... };`, first line)"""
    m = re.search(r"\b%s\s*\[[^\]]*\]\s*=\s*\{" % re.escape(name), text)
    assert m, name
    end = text.index("};", m.end())
    return text[m.end():end], text.count("\n", 0, m.start()) + 1


def designated(text, name, size):
    body, line = array_body(text, name)
    out = [0] * size
    pairs = re.findall(r"\[\s*(\d+)\s*\]\s*=\s*(\d+)", body)
    assert re.sub(r"\[\s*\d+\s*\]\s*=\s*\d+|[\s,]", "", body) == ""
    for slot, v in pairs:
        assert out[int(slot)] == 0
        out[int(slot)] = int(v)
    return out, line


def listed(text, name):
    body, line = array_body(text, name)
    vals = re.findall(r"0[xX]([0-9A-Fa-f]+)[uU]?", body)
    assert re.sub(r"0[xX][0-9A-Fa-f]+[uU]?|[\s,]", "", body) == ""
    return [int(v, 16) for v in vals], line


def main():
    path = os.path.join(REF, "lsqpack.c")
    text = open(path, encoding="latin-1").read()
    width = {}
    for k in ("XXH_NAME_WIDTH", "XXH_NAMEVAL_WIDTH", "XXH_NAME_SHIFT",
              "XXH_NAMEVAL_SHIFT", "LSQPACK_XXH_SEED"):
        width[k] = int(re.search(r"#define\s+%s\s+(\d+)" % k, text).group(1))
    n2i, l0 = designated(text, "name2id_plus_one", 1 << width["XXH_NAME_WIDTH"])
    nv2i, _ = designated(text, "nameval2id_plus_one",
                         1 << width["XXH_NAMEVAL_WIDTH"])
    nh, _ = listed(text, "name_hashes")
    nvh, l1 = listed(text, "nameval_hashes")
    assert len(nh) == len(nvh) == 99
    out = {"source": "lsqpack.c:%d-%d" % (l0, l1 + (len(nvh) + 4) // 5 + 2),
           "seed": width["LSQPACK_XXH_SEED"],
           "name_width": width["XXH_NAME_WIDTH"],
           "name_shift": width["XXH_NAME_SHIFT"],
           "nameval_width": width["XXH_NAMEVAL_WIDTH"],
           "nameval_shift": width["XXH_NAMEVAL_SHIFT"],
           "name2id_plus_one": n2i, "nameval2id_plus_one": nv2i,
           "name_hashes": nh, "nameval_hashes": nvh}
    with open(os.path.join(HERE, "static_lookup.json"), "w") as fp:
        json.dump(out, fp, indent=None, sort_keys=True,
                  separators=(",", ": "))
        fp.write("\n")
    print("wrote static_lookup.json:", out["source"])


if __name__ == "__main__":
    main()
