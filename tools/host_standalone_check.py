#!/usr/bin/env python3
"""CPU only: runs the sanitizer builds of the stand-alone programs tools/*_host_standalone.cpp (the build line is in each source's head)
over the scenes of every checker that has a `hashes` function -- step, marginalize, finish, nullspace, rescale and admit -- and compares every value a
program prints with the checker's.  Any text on stderr, a sanitizer report for one, counts as a failure.

  python tools/host_standalone_check.py DIRECTORY_OF_THE_BUILT_PROGRAMS [DIRECTORY FOR THE CASE FILES] [PROGRAM ...]

A program that is not in the directory is reported and counts as a failure; name programs (step, marginalize, finish, nullspace, rescale, admit) to
run those alone.
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import _admit_ref as AR  # noqa: E402
import _finish_ref as F  # noqa: E402
import _linearize_ref as R  # noqa: E402
import _marginalize_ref as M  # noqa: E402
import _nullspace_ref as NR  # noqa: E402
import _optimize_ref as O  # noqa: E402
import _rescale_ref as RR  # noqa: E402
import _step_ref as T  # noqa: E402


# per program: (label, write the case file at a path, further arguments, what the program must print)
def step_cases():
    for name in T.SCENES:
        job, frames, exp = T.expected(name)
        yield name, lambda path, job=job, frames=frames: T.write_case(path, R.W, R.H, job, frames), (), T.hashes(exp)


def marginalize_cases():
    for name in M.SCENES:
        job, frames, exp = M.case(name)
        yield name, lambda path, job=job, frames=frames: M.write_case(path, R.W, R.H, job, frames), (), M.hashes(exp)


def finish_cases():
    for name in O.SCENES:
        job, frames = F.scene(name)
        for its, force in ((6, 0), (0, 0), (6, 1)):
            loop, fin = F.run(job, frames, its, dict(force_accept=force))
            yield f"{name} {its} {force}", lambda path, job=job, frames=frames: F.write_case(path, R.W, R.H, job, frames), (its, force), F.hashes(loop, fin)


def nullspace_cases():
    for name in NR.POSE_SCENES + NR.GIVEN_SCENES:
        yield name, lambda path, job=NR.scene(name): NR.write_case(path, job), (), NR.hashes(NR.expected(name))


def rescale_cases():
    for name, job in sorted(RR.scenes().items()):
        yield name, lambda path, job=job: RR.write_case(path, job), (), dict(RR.hashes(RR.rescale(job)), forms_equal=1, refusal=1)


def admit_cases():
    jobs = dict(AR.scenes(), **{"chain_" + k: AR.chain_scene(k) for k in AR.CHAINS})
    for name, job in sorted(jobs.items()):
        yield name, lambda path, job=job: AR.write_case(path, job), (), dict(AR.hashes(AR.admit(job)), forms_equal=1, refusal=1)


PROGRAMS = dict(step=step_cases, marginalize=marginalize_cases, finish=finish_cases, nullspace=nullspace_cases, rescale=rescale_cases, admit=admit_cases)


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    bins, out = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    bad = 0
    for program in sys.argv[3:] or PROGRAMS:
        exe = os.path.join(bins, f"{program}_host_standalone")
        if not os.path.exists(exe):
            print(program, "NOT BUILT:", exe)
            bad += 1
            continue
        for label, write, args, want in PROGRAMS[program]():
            path = os.path.join(out, f"{program}_{label.split()[0]}.bin")
            write(path)
            p = subprocess.run([exe, path] + [str(a) for a in args], capture_output=True, text=True, env=env)
            ok = p.returncode == 0 and not p.stderr.strip() and json.loads(p.stdout) == want
            print(program, label, "ok" if ok else "MISMATCH OR REPORT", p.stderr[-600:])
            bad += not ok
    print("reports or mismatches:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
