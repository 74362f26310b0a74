#!/usr/bin/env python3
"""CPU only: runs a build of tools/nullspace_host_standalone.cpp (see its head for the sanitizer build line) over the checker's scenes
and compares every hash it prints with the checker's (tests/_nullspace_ref.py).  Any sanitizer report on stderr counts as a failure.

  python tools/nullspace_host_standalone_check.py ./nullspace_host_standalone [DIRECTORY FOR THE CASE FILES]
"""
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import _nullspace_ref as NR  # noqa: E402


def fnv1a(b):
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    exe, out = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    bad = 0
    for name in NR.POSE_SCENES + NR.GIVEN_SCENES:
        job, exp = NR.scene(name), NR.expected(name)
        ev = np.ascontiguousarray(job["world_to_cam_eval"], np.float64).reshape(-1, 7)
        path = os.path.join(out, f"nullspace_{name}.bin")
        with open(path, "wb") as f:
            fn = job.get("frame_null_in")
            f.write(struct.pack("ii", len(ev), 0 if fn is None else 1) + ev.tobytes() + np.ascontiguousarray(job["state_zero"], np.float64).tobytes()
                    + np.ascontiguousarray(job["exposure"], np.float32).tobytes() + (b"" if fn is None else np.ascontiguousarray(fn, np.float64).tobytes()))
        p = subprocess.run([exe, path], capture_output=True, text=True, env=env)
        want = {k: f"{fnv1a(np.ascontiguousarray(exp[k], np.float64).tobytes()):016x}" for k in ("null_basis", "null_pinv", "sing", "frame_null", "null_x0_pre")}
        want.update(rank=exp["rank"], flags=exp["flags"], forms_equal=1, refusal=1)
        ok = p.returncode == 0 and not p.stderr.strip() and json.loads(p.stdout) == want
        print(name, "ok" if ok else "MISMATCH OR REPORT", p.stderr[-600:])
        bad += not ok
    print("reports or mismatches:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
