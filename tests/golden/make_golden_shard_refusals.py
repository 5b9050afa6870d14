"""Record tests/golden/shard_refusals.json: what the library named by EDT_HIP_LIB (default: the in-tree build) answers to the
calls of tests/test_shard_refusals.py.  Run it against the library of the commit whose refusals are the contract:

    EDT_HIP_LIB=/path/to/libedt_hip.so python tests/golden/make_golden_shard_refusals.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conftest  # noqa: E402,F401  (puts the package on sys.path)
import test_shard_refusals as t  # noqa: E402

for name in t.ENV + ("EDT_HIP_DEBUG_MODE",):
    os.environ.pop(name, None)
from edt import _lib  # noqa: E402

rows = t.answers(_lib.load())
with open(t.TABLE, "w") as f:
    f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
print(t.TABLE, len(rows), "answers from", _lib.LIB_PATH)
