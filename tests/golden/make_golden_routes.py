"""Record tests/golden/transform_routes.json: what the library named by EDT_HIP_LIB (default: the in-tree build) answers to
edt_hip_transform_route for the calls of tests/test_transform_routes_cpu.py.  The table in the repository was recorded from the
commit before that query existed, through a probe in its dispatcher (README.md here describes it):

    EDT_HIP_LIB=/path/to/probed/libedt_hip.so python tests/golden/make_golden_routes.py

Cases that set an environment hook are answered by a child process each hook, started with the hook set: a library may read
the environment once.  The script refuses to write a table that would be an empty check (coverage_gaps)."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conftest  # noqa: E402,F401  (puts the package on sys.path)
import test_transform_routes_cpu as t  # noqa: E402

hook = sys.argv[1] if len(sys.argv) > 1 else None
for name in t.ENV + ("EDT_HIP_DEBUG_MODE",):
    if name != hook:
        os.environ.pop(name, None)
from edt import _lib  # noqa: E402

cases = t.route_cases()
mine = [i for i, c in enumerate(cases) if c[12] == hook]
got = dict(zip(mine, t.answers(_lib.load(), [cases[i] for i in mine])))
if hook:  # (a child: its answers to the parent)
    json.dump(sorted(got.items()), sys.stdout)
    sys.exit(0)
for name in t.ENV:
    env = dict(os.environ, **{name: t.ENV_VALUES[name]})
    out = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=env, check=True, capture_output=True, text=True).stdout
    got.update((int(i), a) for i, a in json.loads(out))
rows = [got[i] for i in range(len(cases))]
gaps = t.coverage_gaps(rows)
if gaps:
    sys.exit(f"not written -- no recorded row has: {gaps}")
unique = sorted({json.dumps(r) for r in rows})
index = {a: i for i, a in enumerate(unique)}
with open(t.TABLE, "w") as f:
    f.write('{"cases_sha256": "%s",\n"fields": %s,\n"answers": [\n%s\n],\n"rows": [\n' % (t.digest(cases), json.dumps(t.FIELDS), ",\n".join(unique)))
    idx = [str(index[json.dumps(r)]) for r in rows]
    f.write(",\n".join(",".join(idx[i:i + 40]) for i in range(0, len(idx), 40)) + "\n]}\n")
print(t.TABLE, len(rows), "rows,", len(unique), "distinct answers from", _lib.LIB_PATH)
