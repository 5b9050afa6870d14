"""Record tests/golden/python_calls.json: what the numpy layer of the ``edt`` package does with the calls of
tests/test_python_boundary_cpu.py: boundary_cases() -- the exception it raises, or every call it makes into the library and
the type, dtype, shape and memory order of what it returns.  Only public functions of ``edt`` are called, with the recording
stand-in of that test module in place of ``edt._lib.load``, so the script runs against any checkout of the package: the
table in the repository was recorded from the commit BEFORE edt/_args.py existed,

    python tests/golden/make_golden_python_calls.py /path/to/that/checkout/euclidean-distance-transform-3d_amd

(with EDT_HIP_LIB naming a built library if that checkout has none: the import still loads it).  Without an argument the
package of this tree is recorded.  The script refuses to write a table that would be an empty check (coverage_gaps)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conftest  # noqa: E402,F401  (puts the package on sys.path)
import test_python_boundary_cpu as t  # noqa: E402

if len(sys.argv) > 1:
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
import edt  # noqa: E402

cases = t.boundary_cases(t.library_names(edt))
rows = [t.answer(edt, c) for c in cases]
gaps = t.coverage_gaps(cases, rows)
if gaps:
    sys.exit(f"not written -- no recorded row has: {gaps}")
unique = sorted({json.dumps(r) for r in rows})
index = {a: i for i, a in enumerate(unique)}
with open(t.TABLE, "w") as f:
    f.write('{"cases_sha256": "%s",\n"answers": [\n%s\n],\n"rows": [\n' % (t.digest(cases), ",\n".join(unique)))
    idx = [str(index[json.dumps(r)]) for r in rows]
    f.write(",\n".join(",".join(idx[i:i + 40]) for i in range(0, len(idx), 40)) + "\n]}\n")
print(t.TABLE, len(rows), "rows,", len(unique), "distinct answers from", os.path.dirname(edt.__file__))
