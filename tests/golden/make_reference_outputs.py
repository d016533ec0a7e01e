"""Writes tests/golden/reference_lib_outputs.json: what the reference's own libraries answer for the
inputs of the three reference-library tests in tests/test_oracle.py.

Needs oracle/_ref (libsais_ref.so, librefutils.so), which `make -C oracle` builds from the reference
checkout.  The suffix arrays and id streams are recorded as SHA-256 of their int32 bytes (the largest
suffix array has 300,000 entries); the character classes, decoded code points and parsed vocabulary
words are recorded as they are.
Run:  python tests/golden/make_reference_outputs.py
"""
import ctypes as C
import hashlib
import json
import os
import sys

here = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(here))

import oracle_lib as O  # noqa: E402
import test_oracle as T  # noqa: E402

if not (os.path.exists(O.LIBSAIS_REF) and os.path.exists(O.REFUTILS)):
    raise SystemExit("oracle/_ref is not built (make -C oracle with the reference checkout present)")

out = {"source": "the reference's libsais.c, utils.cpp and utf8.cpp, built by oracle/Makefile into oracle/_ref",
       "suffix_array": [], "encode_libsais": None, "utils": None}
assert O.use_libsais(True)
for n, k, S in T._sa_inputs():
    out["suffix_array"].append({"n": n, "k": k, "s_sha256": T._sha(S), "sa_sha256": T._sha(O.suffix_array(S, k))})
s, vocab = T._libsais_encode_input()
ids = O.encode(s, vocab)
O.use_libsais(False)
out["encode_libsais"] = {"input_sha256": hashlib.sha256(("\n".join([s] + vocab)).encode()).hexdigest(),
                         "n_ids": len(ids), "ids_sha256": T._sha(ids)}
out["utils"] = T.ref_utils_outputs(C.CDLL(O.REFUTILS))

with open(os.path.join(here, "reference_lib_outputs.json"), "w") as f:
    json.dump(out, f, separators=(",", ":"))
    f.write("\n")
