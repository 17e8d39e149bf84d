"""Writes tests/golden/pmax_digests.json: the digest (tests/refresh_cases.py digest: A, P, R and the marks of
every level) of the hierarchies tests/test_interp_pmax.py builds with the cap on the entries per row of P
off.  They were recorded with the library of the commit before the cap existed (SSS_AMG_LIB names that
build), so that "off" stays what the setup gave then.

    python tests/golden/make_pmax_digests.py
"""
import json
import os
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent.parent), str(HERE.parent)]
os.environ.pop("SSS_SETUP_PMAX", None)

import amg_amd as A  # noqa: E402
import pmax_cases as PC  # noqa: E402
import pmis_restatement as R  # noqa: E402
import refresh_cases as RC  # noqa: E402
from conftest import quiet_ctx  # noqa: E402

out = {}
M = R.matrix(PC.HIER_MATRIX)
for cs, interp in PC.HIER:
    with quiet_ctx():
        H = A.Hierarchy(M, R.pars(cs, interp))
    out[PC.hier_key(cs, interp)] = RC.digest(H)
    H.close()
(HERE / "pmax_digests.json").write_text(json.dumps(out, indent=1) + "\n")
print(json.dumps(out, indent=1))
