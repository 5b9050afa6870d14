"""Record tests/golden/label_op_refusals.json: the return code and the edt_hip_last_error() text of every case of
tests/test_label_op_refusals_cpu.py, as the library named by EDT_HIP_LIB (default: the in-tree build) answers them.  Run it
against the library of the commit whose refusals are the contract:

    EDT_HIP_LIB=/path/to/libedt_hip.so python tests/golden/make_golden_refusals.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("EDT_HIP_ALLOW_NO_DEVICE", "1")   # (no case needs a device)

import conftest  # noqa: E402,F401  (puts the package on sys.path)
import test_label_op_refusals_cpu as t  # noqa: E402
from edt import _lib  # noqa: E402

rows = t.record(_lib.load())
with open(t.TABLE, "w") as f:
    f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
print(t.TABLE, len(rows), "refusals from", _lib.LIB_PATH)
