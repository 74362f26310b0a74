#!/usr/bin/env python3
"""Writes the fixture of tests/test_eval_trip_edges.py: form 0's outputs (dsm_diag_single_eval), full and residual-only, of every case of
tests/_trip_edges.py as raw bytes, from the library that is built in the tree.  It is run ONCE, with the library of the commit a change
to the evaluation loop is compared against; the tests never run it.  Before a record is kept every other form that applies must have
produced the same bytes (what tests/test_eval_forms_f64.py asserts), so form 0 stands for all of them.
    python tools/record_eval_trip_edges.py OUT.npz        (needs a GPU)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _trip_edges as E  # noqa: E402
from _gn_checks import TABLES, trackers  # noqa: E402
from _scenes import _photometry  # noqa: E402
from direct_stereo_slam_amd.tracker import Context  # noqa: E402


def main():
    out_path = sys.argv[1]
    ctx = Context(0)
    records = {}
    for name in E.SCENES:
        sc = E.scene(name)
        ref_aff, ref_exp, _ = _photometry(sc)
        trks = trackers(ctx, sc)
        for lvl in (0, 1):
            for n in E.counts_of(name, lvl):
                tpl = E.template_of(sc, lvl, n)
                for t, trk in zip(TABLES, trks):
                    trk.setCoarseTrackingRef(0, ref_aff, ref_exp, *tpl)
                    forms = (0, 1, 2, 3) if trk.reduction_geometry(lvl, n)[2] <= 1 else (0, 1, 2)
                    for kind in ("pose", "scale"):
                        for ro in (False, True):
                            outs = [E.evaluate(trk, kind, lvl, sc, ro, form) for form in forms]
                            got = [E.bits(o[:1] if ro else o) for o in outs]  # (residual-only: rs is what the forms share bit for bit)
                            assert all(g == got[0] for g in got), ("the forms differ", name, kind, lvl, t, n, ro)
                            records[E.key(name, kind, lvl, t, n, ro)] = E.bits(outs[0])
        for trk in trks:
            trk.close()
    np.savez_compressed(out_path, **E.pack(records))
    print(len(records), "records ->", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
