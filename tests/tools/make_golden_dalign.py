#!/usr/bin/env python
"""Golden vectors for the device form of ocda_go on the shapes of tests/dalign_cases.py (anchors on the sequences' ends and on the 2-bit words'
boundaries, unrelated sequences, long indels, sizes around min_align_size, reached ends, the trim, equal diagonals, the read's reverse strand),
generated from the REFERENCE's own ocda_go (oracle/_ref/librescue_ref.so = oracle/rescue_ref_shim.c over the reference objects).  Committed is data
only: tests/golden/dalign_cases.json - per case its name and parameters (the tests rebuild the sequences from tests/dalign_cases.py's seed), 64-bit
FNV hashes of the two sequences and what the reference returned: the return value, the four end points, the difference count and the identity.

    python tests/tools/make_golden_dalign.py
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import dalign_cases, test_rescue as T  # noqa: E402
from oracle import oracle_api as ora  # noqa: E402


def main():
    if not os.path.exists(T.REF):
        sys.exit("oracle/_ref is missing: run `make -C oracle ref` in the build container")
    ref = C.CDLL(T.REF)
    out = []
    for c in dalign_cases.shape_cases():
        q = dalign_cases.query_of(c)
        o, ident = (C.c_int * 6)(), C.c_double()
        r = ref.ref_ocda_go(T.ptr(q), c["qs"], len(q), T.ptr(c["tmpl"]), c["ts"], len(c["tmpl"]), C.c_double(c["error"]), c["min_size"], o, C.byref(ident))
        rec = {k: c[k] for k in ("name", "qdir", "qs", "ts", "error", "min_size")}
        rec.update({"ret": r, "out": list(o)[:5], "ident": ident.value if r else 0.0, "read_fnv": ora.fnv64(bytes(c["read"])), "tmpl_fnv": ora.fnv64(bytes(c["tmpl"]))})
        out.append(rec)
    with open(os.path.join(ROOT, "tests", "golden", "dalign_cases.json"), "w") as f:
        json.dump({"cases": out}, f, indent=0, sort_keys=True)
    print(len(out), "cases,", sum(c["ret"] for c in out), "aligned")


if __name__ == "__main__":
    main()
