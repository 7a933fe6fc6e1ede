#!/usr/bin/env python3
"""Generates tests/golden/match_ref/*.npz: what the REFERENCE's own ORBmatcher searches return for every case of
tests/helpers_match_ref.py.

Runs oracle/_ref/pli_ref_match (the reference's src/ORBmatcher.cc, src/CameraModels/Pinhole.cpp and
Thirdparty/DBoW2/DBoW2/FeatureVector.cpp compiled where they lie against the stand-in of oracle/ref_recipe/match_shim; built by
oracle/Makefile only where the reference tree exists) once per call of every case and stores the case's input tables beside
everything the caller of the reference function can see.  Then prints, per function, how often each exit of the restatement's EXITS
was taken over the corpus.  Dev-time only.  The fixtures are inputs of this project's own making and recorded results of that
program; no reference source is stored.  The files' bytes depend on their arrays alone: a second run reproduces them.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers_match_ref as H

if not os.path.exists(H.REF_EXE):
    sys.exit("oracle/_ref/pli_ref_match absent (make -C oracle ref_match, with the reference tree present): fixtures not regenerated")
os.makedirs(H.GOLD_DIR, exist_ok=True)
for stale in sorted(set(os.listdir(H.GOLD_DIR)) - {c.name + ".npz" for c in H.CASES}):
    os.remove(os.path.join(H.GOLD_DIR, stale))
total = 0
for c in H.CASES:
    a = c.arrays()
    results = {call: H.run_reference(c.bag(a, call)) for call in c.calls}
    H.save_fixture(c.name, a, results)
    size = os.path.getsize(H.fixture_path(c.name))
    total += size
    print("%-32s %-7s %3d calls %7d bytes" % (c.name, c.fn, len(c.calls), size))
print("total %d bytes in %d files" % (total, len(H.CASES)))
assert total <= (1 << 20) + (1 << 16), total
H._FIX.clear()
print("\nexits taken over the corpus (scalar restatements on the fixtures' inputs):")
for fn, ex in H.exit_counts().items():
    names = next(c.exits for c in H.CASES if c.fn == fn)
    if names:
        print("  %-7s %s" % (fn, ", ".join("%s %d" % (k, ex[k]) for k in names)))
