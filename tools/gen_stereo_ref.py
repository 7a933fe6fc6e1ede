#!/usr/bin/env python3
"""Generates tests/golden/stereo_ref/*.npz and manifest.json: what the REFERENCE's own stereo matchers, LineMatcher and
Frame::GetFeaturesInArea return for every case of tests/helpers_stereo_ref.py.

Runs oracle/_ref/pli_ref_stereo (built by oracle/Makefile only where the reference tree exists) once per case and stores the case's
inputs beside the recorded results.  A reference run that throws or aborts stops the generation.  Then counts, from the labels of
tests/helpers_matchers.py alone, how often every exit and branch is reached over the reference cases, and asserts the corpus
conditions.  With a second argument, that program (a checked build, say) is run instead and its results are only compared with the
committed fixtures.  Dev-time only.  The fixtures are inputs of this project's own making and recorded results; no reference
source is stored.  The files' bytes depend on their arrays alone: a second run reproduces them.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers_stereo_ref as S
from oracle import pyoracle

pyoracle.lib()
exe = sys.argv[1] if len(sys.argv) > 1 else S.REF_EXE
if not os.path.exists(exe):
    sys.exit("%s absent (make -C oracle ref_stereo, with the reference tree present): fixtures not regenerated" % exe)
if len(sys.argv) > 1:
    differ = S.generate(pyoracle, exe, write=False)
    print("compared %d cases against the committed fixtures: %s" % (len(S.fixture_names()), differ or "all equal"))
    sys.exit(1 if differ else 0)
S.generate(pyoracle)
total = 0
for n in S.fixture_names():
    size = os.path.getsize(S.fixture_path(n))
    total += size
    print("%-40s %8d bytes" % (n, size))
print("total %d bytes in %d files" % (total, len(S.fixture_names())))
print(json.dumps(S.manifest(), indent=1, sort_keys=True))
assert total <= (1 << 20), total
