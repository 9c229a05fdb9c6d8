"""Record the result files of the five solvers' run_method (tests/solver_file_cases.py) on the GPU:

    python tools/record_solver_files.py [--out tests/golden/solver_files_parent.json]

Writes {case: {relative path: text}} - the text of every metric file; time and memory files, and image files, by name only (null).
tests/test_gpu_solver_files.py compares a run of the working tree against a recording made on the commit BEFORE a change to the
solvers' host code.  Run it twice there: two byte-identical recordings let the test assert text equality.  Only the package's public
API is used, so the tool runs unchanged on an older commit.
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import solver_file_cases as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "solver_files_parent.json"))
    out = ap.parse_args().out
    net = S.new_model()
    rec = {}
    for name in S.CASES:
        with tempfile.TemporaryDirectory() as tmp:
            S.run_case(name, net, tmp)
            rec[name] = S.collect(tmp)
        print(f"{name}: {len(rec[name])} files")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
