#!/usr/bin/env python3
"""CPU only: runs a build of tools/finish_host_standalone.cpp (see its head for the sanitizer build line) over the checker's scenes and
compares every hash it prints with the checker's (tests/_finish_ref.py, hashes).  Any sanitizer report on stderr counts as a failure.

  python tools/finish_host_standalone_check.py ./finish_host_standalone [DIRECTORY FOR THE CASE FILES]
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import _finish_ref as F  # noqa: E402
import _linearize_ref as R  # noqa: E402
import _optimize_ref as O  # noqa: E402


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    exe, out = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    bad = 0
    for name in O.SCENES:
        job, frames = F.scene(name)
        path = os.path.join(out, f"finish_{name}.bin")
        F.write_case(path, R.W, R.H, job, frames)
        for its, force in ((6, 0), (0, 0), (6, 1)):
            p = subprocess.run([exe, path, str(its), str(force)], capture_output=True, text=True, env=env)
            loop, fin = F.run(job, frames, its, dict(force_accept=force))
            ok = p.returncode == 0 and not p.stderr.strip() and json.loads(p.stdout) == F.hashes(loop, fin)
            print(name, its, force, "ok" if ok else "MISMATCH OR REPORT", p.stderr[-600:])
            bad += not ok
    print("reports or mismatches:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
