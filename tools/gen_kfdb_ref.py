#!/usr/bin/env python3
"""Generates tests/golden/kfdb_ref/*.npz: what the REFERENCE's own KeyFrameDatabase answers for every world of tests/helpers_kfdb.py.

    tools/gen_kfdb_ref.py [REFERENCE_TREE]          (default: $PLI_REFERENCE, else ../reference beside this repository)

Dev-time only.  Compiles tools/pin/kfdb/kfdb_ref_main.cpp with the reference's src/KeyFrameDatabase.cc and Thirdparty/DBoW2 where they
lie, unmodified (tools/pin/kfdb/standins.h is force-included: stand-in KeyFrame / Frame / Map classes of our own), into a temporary
directory OUTSIDE the tree, replays each world and stores the recorded answers.  build(), smoke() and the tests never run that
program; only the .npz files are committed, and they hold no reference source.

Before a fixture is written the corpus is checked, on the reference's answers, for what can go wrong (the numbered list of
tests/test_kfdb_cpu.py's module docstring).  The events inside the two functions (a neighbour replaces pBestKF, the duplicate filter
drops an entry, a stale score enters accScore, a connected keyframe would have held the maximum) cannot be read off the reference's
return values; they are counted by the restatement of tests/helpers_kfdb.py AFTER it has been found equal to the reference's answers
in every recorded value.
"""
import collections
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers_bow_ref as B
import helpers_kfdb as H


def build(ref, outdir):
    exe = os.path.join(outdir, "pli_ref_kfdb")
    pin = os.path.join(ROOT, "tools", "pin", "kfdb")
    dbow = os.path.join(ref, "Thirdparty", "DBoW2")
    srcs = [os.path.join(pin, "kfdb_ref_main.cpp"), os.path.join(ref, "src", "KeyFrameDatabase.cc")]
    srcs += [os.path.join(dbow, "DBoW2", f) for f in ("FORB.cpp", "BowVector.cpp", "FeatureVector.cpp", "ScoringObject.cpp")]
    srcs += [os.path.join(dbow, "DUtils", f) for f in ("Random.cpp", "Timestamp.cpp")]
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++14", "-w", "-include", os.path.join(pin, "standins.h"),
                           "-I", os.path.join(pin, "shim"), "-I", os.path.join(ROOT, "oracle", "ref_recipe", "bow_shim"),
                           "-I", ref, "-I", os.path.join(ref, "include"), "-I", dbow, "-o", exe] + srcs)
    return exe


def run(exe, world, workdir):
    req = H.make_world(world)
    voc, reqf, rspf = (os.path.join(workdir, n) for n in ("voc.txt", "request", "response"))
    with open(voc, "w", newline="") as f:
        f.write(B.vocabulary_text(*req["voc"]))
    with open(reqf, "wb") as f:
        f.write(H.request_bytes(req, voc))
    subprocess.run([exe, reqf, rspf], check=True, timeout=300)
    return H.fixture_arrays(req, H.parse_response(open(rspf, "rb").read(), req))


def bits(x):
    return np.float64(x).view(np.uint64)


def check_corpus(fixes):
    """The assertions on the reference's answers; prints the figures."""
    events = collections.Counter()
    cand2 = nothing = first_tie = loop_full = 0
    sizes, pairs, desc_changed, swap_changed, straddle = set(), 0, 0, 0, 0
    for name, fix in fixes.items():
        got = H.replay(fix, events=events)
        d = H.differences(fix, got)
        assert not d, (name, "the restatement differs from the reference", d[:8])
        queries = [op for op in fix["ops"].tolist() if op[0] in (H.OP_RELOC, H.OP_NBEST)]
        for j, op in enumerate(queries):
            nl = fix["loop_off"][j + 1] - fix["loop_off"][j]
            nm = fix["merge_off"][j + 1] - fix["merge_off"][j]
            cand2 += (nl + nm) >= 2
            nothing += int(fix["common"][j].sum() == 0)
            loop_full += op[0] == H.OP_NBEST and nl == op[2] and nm < op[2]
        sizes |= set(np.diff(fix["kf_bow_off"]).tolist())
        # 5: two keyframes with the same first shared word whose add order differs from their id order
        def on_query(j, db, qw, qv):
            nonlocal first_tie
            c, f, _ = H.answers(qw, qv, db.slots())
            live = [s for s in range(len(c)) if c[s] > 0]
            for a in live:
                for b in live:
                    if a != b and f[a] == f[b] and (db.slot_seq[a] < db.slot_seq[b]) != (db.slot_kf[a].mnId < db.slot_kf[b].mnId):
                        first_tie += 1
                        return
        H.replay(fix, on_query=on_query)
        for j, i, qw, qv, kw, kv in H.score_pairs(fix):
            want = fix["score"][j, i]
            assert bits(H.score(qw, qv, kw, kv)) == bits(want), (name, j, i, "score restatement")
            assert len(H.shared_words(qw, kw)[0]) == fix["common"][j, i], (name, j, i, "shared words")
            pairs += 1
            desc_changed += bits(H.score(qw, qv, kw, kv, "descending_sum")) != bits(want)
            swap_changed += bits(H.score(qw, qv, kw, kv, "swapped_arguments")) != bits(want)
            _, ik = H.shared_words(qw, kw)
            straddle += len(ik) >= 2 and any(a // 64 != b // 64 for a, b in zip(ik[:-1], ik[1:]))
    print("queries with >= 2 candidates: %d; pBestKF replaced by a neighbour: %d; duplicates dropped: %d; stale scores added: %d"
          % (cand2, events["neighbour_best"], events["duplicate"], events["stale"]))
    print("same first word, add order != id order: %d; connected keyframe above the maximum: %d; loop full, merge not: %d; "
          "queries sharing nothing: %d; ties in the sorted list: %d" % (first_tie, events["connected_max"], loop_full, nothing, events["tie"]))
    print("keyframe sizes: %s" % sorted(sizes))
    print("pairs: %d, across a chunk boundary: %d, bits change with a descending sum: %.1f %%, with swapped arguments: %.1f %%"
          % (pairs, straddle, 100.0 * desc_changed / pairs, 100.0 * swap_changed / pairs))
    assert cand2 >= 1 and events["neighbour_best"] >= 1 and events["duplicate"] >= 1 and events["stale"] >= 1          # 1-4
    assert first_tie >= 1 and events["connected_max"] >= 1 and loop_full >= 1 and nothing >= 1                          # 5-8
    assert {1, 63, 64, 65, 128, 129} <= sizes and straddle >= 1                                                         # 9, 10
    assert desc_changed >= 0.2 * pairs and swap_changed >= 0.2 * pairs                                                  # 11, 12


def main():
    here_ref = os.environ.get("PLI_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")
    ref = sys.argv[1] if len(sys.argv) > 1 else here_ref
    if not os.path.exists(os.path.join(ref, "src", "KeyFrameDatabase.cc")):
        sys.exit("no reference tree at %s: fixtures not regenerated" % ref)
    fixes = {}
    with tempfile.TemporaryDirectory() as d:
        exe = build(ref, d)
        for world in H.WORLDS:
            fixes[world.name] = run(exe, world, d)
    check_corpus(fixes)
    os.makedirs(H.GOLD_DIR, exist_ok=True)
    for name, arrays in fixes.items():
        np.savez_compressed(H.fixture_path(name), **arrays)
        size = os.path.getsize(H.fixture_path(name))
        assert size <= 200 * 1024, (name, size)
        print("%-14s %3d keyframes, %2d queries, %7d bytes" % (name, len(arrays["kf_id"]), len(arrays["score"]), size))


if __name__ == "__main__":
    main()
