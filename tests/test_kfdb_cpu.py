"""The keyframe database's place-recognition queries on the CPU: the plain Python restatement of tests/helpers_kfdb.py (DBoW2's L1
score, and DetectRelocalizationCandidates / DetectNBestCandidates rebuilt from the per-slot answers of one device query) against the
REFERENCE's own recorded answers (tests/golden/kfdb_ref/, tools/gen_kfdb_ref.py), bit for bit; every mutant of the restatement shows
in at least one recorded value; the header declares the entry points and capi.py binds them.

What the corpus must exercise (asserted by the generator on the reference's answers, re-asserted here where the fixtures suffice):
 1 a query with two or more candidates           2 a neighbour replaces pBestKF          3 the duplicate filter drops an entry
 4 a stale score changes accScore                5 same first word, add order != id order 6 a connected keyframe above the maximum
 7 vpLoopCand full while vpMergeCand is not      8 a query that shares nothing            9 keyframes of 1, 63, 64, 65, 128, 129 words
10 shared words on both sides of a chunk of 64  11 >= 20 % of the pairs change with a descending sum
12 >= 20 % change with swapped arguments
"""
import collections
import os
import re

import numpy as np
import pytest

import helpers_kfdb as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [w.name for w in H.WORLDS]


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", NAMES)
def test_the_score_restatement_equals_the_reference_bit_for_bit(name):
    fix = H.load_fixture(name)
    nq, nkf = fix["score"].shape
    assert 30 <= nkf <= 60 and 6 <= nq
    for j, i, qw, qv, kw, kv in H.score_pairs(fix):
        got = H.score(qw, qv, kw, kv)
        assert bits(got) == bits(fix["score"][j, i]), (j, i, got, fix["score"][j, i])
        assert np.float32(got).tobytes() == fix["score_f32"][j, i].tobytes()
        assert len(H.shared_words(qw, kw)[0]) == fix["common"][j, i]
    assert np.signbit(fix["score"][fix["common"] == 0]).all() and (fix["score"][fix["common"] == 0] == 0).all()      # -0.0


@pytest.mark.parametrize("name", NAMES)
def test_the_two_functions_equal_the_reference_in_candidates_and_members(name):
    fix = H.load_fixture(name)
    events = collections.Counter()
    got = H.replay(fix, events=events)
    assert H.differences(fix, got) == []
    assert min(events[k] for k in ("neighbour_best", "duplicate", "stale", "connected_max", "loop_full_merge_not", "tie")) >= 1, events


def test_the_corpus_holds_the_sizes_and_the_orders_that_can_go_wrong():
    sizes, pairs, desc, swap, straddle, nothing, many = set(), 0, 0, 0, 0, 0, 0
    for name in NAMES:
        fix = H.load_fixture(name)
        sizes |= set(np.diff(fix["kf_bow_off"]).tolist())
        nothing += int((fix["common"].sum(axis=1) == 0).sum())
        many += int(((np.diff(fix["loop_off"]) + np.diff(fix["merge_off"])) >= 2).sum())
        for j, i, qw, qv, kw, kv in H.score_pairs(fix):
            pairs += 1
            desc += bits(H.score(qw, qv, kw, kv, "descending_sum")) != bits(fix["score"][j, i])
            swap += bits(H.score(qw, qv, kw, kv, "swapped_arguments")) != bits(fix["score"][j, i])
            ik = H.shared_words(qw, kw)[1]
            straddle += len(ik) >= 2 and ik[0] // 64 != ik[-1] // 64
    assert {1, 63, 64, 65, 128, 129} <= sizes
    assert nothing >= 1 and many >= 1 and straddle >= 1
    assert desc >= 0.2 * pairs and swap >= 0.2 * pairs, (pairs, desc, swap)


@pytest.mark.parametrize("mut", H.MUTANTS)
def test_every_mutant_differs_from_the_fixtures(mut):
    seen = []
    for name in NAMES:
        fix = H.load_fixture(name)
        if mut in ("descending_sum", "swapped_arguments", "float_accumulator"):
            seen += [1 for j, i, qw, qv, kw, kv in H.score_pairs(fix) if bits(H.score(qw, qv, kw, kv, mut)) != bits(fix["score"][j, i])]
        seen += H.differences(fix, H.replay(fix, mut=mut))
    assert seen, "the fixtures do not see the mutant %s" % mut


def test_a_bad_keyframe_in_the_sorted_list_is_an_error_and_a_second_add_too():
    fix = H.load_fixture(NAMES[0])
    maps, kfs = H.stubs_of(fix)
    db = H.Database()
    for kf in kfs[:20]:
        db.add(kf)
    with pytest.raises(ValueError):
        db.add(kfs[3])
    for kf in kfs[:20]:
        kf.bad = True
    with pytest.raises(H.BadKeyFrame):
        db.detect_n_best_candidates(kfs[25], 3)


def test_the_answers_of_free_and_empty_slots():
    w, v = np.array([3, 9], np.uint32), np.array([0.25, 0.75])
    c, f, s = H.answers(w, v, [None, (np.zeros(0, np.uint32), np.zeros(0)), (np.array([9], np.uint32), np.array([1.0]))])
    assert c.tolist() == [0, 0, 1] and f.tolist() == [-1, -1, 1]
    assert np.signbit(s[:2]).all() and (s[:2] == 0).all() and s[2] == 0.75


def test_the_header_declares_the_keyframe_database_and_capi_binds_it():
    src = open(os.path.join(ROOT, "include", "pli_frontend.h")).read()
    from pli_slam_amd import capi
    for fn in ("create", "destroy", "add", "erase", "clear", "stats", "query"):
        assert re.search(r"\bpli_kfdb_%s\(" % fn, src), fn
        assert "pli_kfdb_" + fn in capi._PROTOS
        assert hasattr(capi.lib(), "pli_kfdb_" + fn)
    assert "#define PLI_KFDB_QUERY_MAX_WAVES %d" % capi.KFDB_QUERY_MAX_WAVES in src
    assert "#define PLI_BOW_MAX_FEATURES %d" % capi.BOW_MAX_FEATURES in src
    fields = re.search(r"struct pli_kfdb_stats \{(.*?)\};", src, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"(\w+);", fields) == [n for n, _ in capi.KfdbStats._fields_]
    from pli_slam_amd.frontend import Frontend
    for fn in ("create", "destroy", "add", "erase", "clear", "stats", "query"):
        assert callable(getattr(Frontend, "kfdb_" + fn))


def test_the_fixtures_are_small():
    for name in NAMES:
        assert os.path.getsize(H.fixture_path(name)) <= 200 * 1024
