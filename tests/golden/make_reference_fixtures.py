"""tests/golden/make_reference_fixtures.py -- regenerates the fixtures that stand in for the reference checkout.

    python tests/golden/make_reference_fixtures.py <path to a checkout of the reference repository>

Writes two data files next to this script, so that the tests which check the project against the
reference's shipped files run from a clean checkout of this repository alone:

- reference_models.json: for every model file under the reference's model/ directory, its path there,
  the SHA-256 of its bytes, and the lines in which it differs from what em_io.em_write makes of the
  packed copy under models/ (trailing blanks on the boundary lines).  tests/test_reference_files.py
  rebuilds each shipped file byte for byte from models/ with these lines and checks the digest.
- reference_matlab_functions.txt: the names of the functions and methods the reference's .m files
  define, one per line (tests/test_host.py, test_matlab_files_call_only_functions_that_exist).
"""
import glob
import hashlib
import json
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from em_model_manned_bayes_amd import em_io  # noqa: E402

FUN_RE = r"function\s+(?:\[?([^=\n]*?)\]?\s*=\s*)?([A-Za-z_]\w*)\s*(?:\(([^)]*)\))?"


def main(ref):
    models, tmp = [], tempfile.mkdtemp(prefix="emgpu_reffix_")
    for f in sorted(glob.glob(os.path.join(ref, "model", "**", "*.txt"), recursive=True)):
        stem = os.path.splitext(os.path.basename(f))[0]
        shipped = open(f, "rb").read()
        written = open(em_io.materialize_model(stem, tmp), "rb").read()
        a, b = shipped.decode("ascii").split("\n"), written.decode("ascii").split("\n")
        assert len(a) == len(b), (f, len(a), len(b))
        models.append({"path": os.path.relpath(f, os.path.join(ref, "model")).replace(os.sep, "/"), "stem": stem,
                       "sha256": hashlib.sha256(shipped).hexdigest(),
                       "lines": [[i, x] for i, (x, y) in enumerate(zip(a, b)) if x != y]})
    with open(os.path.join(HERE, "reference_models.json"), "w") as fh:
        json.dump(models, fh, indent=1)
        fh.write("\n")
    names = set()
    for f in glob.glob(os.path.join(ref, "code", "matlab", "**", "*.m"), recursive=True):
        names.add(os.path.basename(f)[:-2])
        names |= {m.group(2) for m in re.finditer(FUN_RE, open(f, errors="ignore").read())}
    with open(os.path.join(HERE, "reference_matlab_functions.txt"), "w") as fh:
        fh.write("\n".join(sorted(names)) + "\n")
    print("%d model files, %d MATLAB names" % (len(models), len(names)))


if __name__ == "__main__":
    main(sys.argv[1])
