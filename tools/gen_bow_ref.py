#!/usr/bin/env python3
"""Generates tests/golden/bow_ref/*.npz: what the REFERENCE's own DBoW2 answers for every case of tests/helpers_bow_ref.py.

Runs oracle/_ref/pli_ref_bow (the reference's Thirdparty/DBoW2 compiled where it lies; built by oracle/Makefile only where the
reference tree exists) once per case and levelsup and stores the tree arrays, the features, the per-feature rows and, where no
feature left its node id unset, the BowVector and the FeatureVector.  Dev-time only.  The fixtures are recorded results of that
program; no reference source is stored.  Prints, per case and levelsup, the features with an unset node id and the ties counted.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers_bow_ref as H

exe = os.path.join(ROOT, "oracle", "_ref", "pli_ref_bow")
if not os.path.exists(exe):
    sys.exit("oracle/_ref/pli_ref_bow absent (make -C oracle, with the reference tree present): fixtures not regenerated")
for c in H.CASES:
    arrays = H.generate(exe, c)
    H.save_fixture(c.name, arrays)
    size = os.path.getsize(H.fixture_path(c.name))
    assert size <= 200 * 1024, (c.name, size)
    tree = H.Tree(*H.vocabulary_of(arrays))
    ties = [tree.classify(f)[1] for f in arrays["feat"]]
    print("%-22s %5d nodes, %5d words, %5d features, %3d with a tie, %7d bytes" % (
        c.name, len(arrays["parent"]), int(arrays["nwords"]), len(arrays["feat"]), sum(1 for t in ties if t), size))
    for ls in arrays["levelsups"].tolist():
        at = sum(1 for t in ties if c.L - ls in t)
        print("    levelsup %d: %4d node ids unset, %3d ties at the recorded level, set-level maps %s" % (
            ls, int((arrays["node_%d" % ls] == H.UNSET).sum()), at, "recorded" if arrays["det_%d" % ls] else "indeterminate"))
