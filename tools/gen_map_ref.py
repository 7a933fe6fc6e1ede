#!/usr/bin/env python3
"""Generates tests/golden/map_ref/*.npz: what the REFERENCE's own Frame::isInFrustum, Frame::isInFrustum_l (with
MapPoint::PredictScale and the searches behind them), LocalMapping::CreateNewMapPoints (with ComputeF12 and KeyFrame::UnprojectStereo;
one camera and two) and MapPoint / MapLine::ComputeDistinctiveDescriptors return for every case of tests/helpers_map_ref.py.

Runs oracle/_ref/pli_ref_map (those definitions cut out of the reference's sources at build time and compiled where they lie against
the stand-in of oracle/ref_recipe/map_shim; built by oracle/Makefile only where the reference tree exists) once per case and stores
the case's input tables beside everything the driver records.  Then prints the exits the restatements take over the corpus.  With a
program as argument (a checked build) it only compares that program's answers with the committed fixtures.  Dev-time only.  The
fixtures are inputs of this project's own making and recorded results of that program; no reference source is stored.  The files'
bytes depend on their arrays alone: a second run reproduces them.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers_map_ref as H

if len(sys.argv) > 1:
    for c in H.CASES:
        a, want = H.load_fixture(c.name)
        got = H.run_reference(c.bag(a), sys.argv[1])
        assert sorted(got) == sorted(want), c.name
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (c.name, k)
    print("%s reproduces all %d fixtures" % (sys.argv[1], len(H.CASES)))
    sys.exit(0)
if not os.path.exists(H.REF_EXE):
    sys.exit("oracle/_ref/pli_ref_map absent (make -C oracle ref_map, with the reference tree present): fixtures not regenerated")
os.makedirs(H.GOLD_DIR, exist_ok=True)
for stale in sorted(set(os.listdir(H.GOLD_DIR)) - {c.name + ".npz" for c in H.CASES}):
    os.remove(os.path.join(H.GOLD_DIR, stale))
total = 0
for c in H.CASES:
    a = c.arrays()
    res = {H.CALL: H.run_reference(c.bag(a))}
    if c.fn == "new_map_points":
        res["f64"] = c.judge(a, res[H.CALL])
        print("   least libm margin %.1f ulps, %d rejected pairs" % (res["f64"]["libm_margin_ulps"][0], len(res["f64"]["rejected_exit"])))
    H.save_fixture(c.name, a, res)
    size = os.path.getsize(H.fixture_path(c.name))
    total += size
    print("%-36s %-15s %7d bytes" % (c.name, c.fn, size))
print("total %d bytes in %d files" % (total, len(H.CASES)))
assert total <= (1 << 20), total
H._FIX.clear()
print("\nexits taken over the corpus (the restatements on the fixtures' inputs):")
for fn, ex in H.exit_counts().items():
    print("  %-15s %s" % (fn, ", ".join("%s %d" % kv for kv in sorted(ex.items()))))
