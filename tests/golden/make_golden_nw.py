#!/usr/bin/env python
"""Golden vectors for the device form of edlib_go on the shapes of tests/nw_cases.py (word and stripe boundaries, the leaf limit from both sides, a
split with one word of rows, every reject rule on either side of its threshold, the read's reverse strand), generated from the REFERENCE's own
edlib_go (oracle/_ref/librescue_ref.so = oracle/rescue_ref_shim.c over the reference objects).  Committed is data only: tests/golden/nw_cases.json -
per case its name and parameters (the tests rebuild the sequences from tests/nw_cases.py's seeds) and what the reference returned: end points,
distance, columns, identity and 64-bit FNV hashes of the two alignment strings.

    python tests/golden/make_golden_nw.py
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import nw_cases, test_rescue as T  # noqa: E402
from oracle import oracle_api as ora  # noqa: E402


def main():
    if not os.path.exists(T.REF):
        sys.exit("oracle/_ref is missing: run `make -C oracle ref` in the build container")
    ref = C.CDLL(T.REF)
    out = []
    for c in nw_cases.shape_cases():
        q = nw_cases.query_of(c)
        cap = (c["qt"] - c["qf"]) + (c["tt"] - c["tf"]) + 16
        o, ident = (C.c_int * 6)(), C.c_double()
        qa, ta = C.create_string_buffer(cap), C.create_string_buffer(cap)
        r = ref.ref_edlib_go(T.ptr(q), c["qf"], c["qt"], T.ptr(c["tmpl"]), c["tf"], c["tt"], C.c_double(c["error"]), c["tol"], c["min_size"], o, C.byref(ident), qa, ta, cap)
        rec = {k: c[k] for k in ("name", "qdir", "qf", "qt", "tf", "tt", "error", "tol", "min_size")}
        rec.update({"ret": r, "read_fnv": ora.fnv64(bytes(c["read"])), "tmpl_fnv": ora.fnv64(bytes(c["tmpl"]))})
        if r:
            rec.update({"out": list(o), "ident": ident.value, "qaln": ora.fnv64(qa.value), "taln": ora.fnv64(ta.value)})
        out.append(rec)
    with open(os.path.join(ROOT, "tests", "golden", "nw_cases.json"), "w") as f:
        json.dump({"cases": out}, f, indent=0, sort_keys=True)
    print(len(out), "cases,", sum(c["ret"] for c in out), "aligned")


if __name__ == "__main__":
    main()
