"""Pins the oracle's bag-of-words transform to the reference's own Thirdparty/DBoW2.

tests/golden/bow_ref/*.npz hold what DBoW2::TemplatedVocabulary<cv::Mat, FORB> itself answered for every case of
tests/helpers_bow_ref.py: the reference's files compiled where they lie against oracle/ref_recipe/bow_shim/, the vocabulary loaded
by its own loadFromTextFile, run by oracle/_ref/pli_ref_bow (tools/gen_bow_ref.py).  What is pinned: the order of the children, the
nearest child with the first winning a tie, the word ids in file order, the weights, the level whose node is recorded, the
BowVector's accumulation and L1 normalisation and the FeatureVector.  Every comparison is byte equality over every feature of every
case and levelsup.

Where the reference's descent never stores a node id (helpers_bow_ref.UNSET in the fixtures, see the helper), the oracle and the
device answer 0: this project's rule, stated in oracle/match_oracle.hpp and DESIGN.md.
"""
import os

import numpy as np
import pytest

import helpers_bow_ref as H

REF_EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "pli_ref_bow")
needs_ref = pytest.mark.skipif(not os.path.exists(REF_EXE), reason="oracle/_ref/pli_ref_bow is built only where the reference tree exists")

# transform(features, ...) sums the L1 norm over the map, in word order; summed feature by feature it rounds differently here
L1_ORDER_CASE, L1_ORDER_LEVELSUP = "complete_k10_L3_s2", 4


def _cases_levelsups(determinate_only=False):
    for c in H.CASES:
        fix = H.load_fixture(c.name)
        for ls in fix["levelsups"].tolist():
            if not determinate_only or fix["det_%d" % ls]:
                yield c, fix, ls


@pytest.fixture(scope="module")
def trees():
    return {c.name: H.Tree(*H.vocabulary_of(H.load_fixture(c.name))) for c in H.CASES}


@pytest.fixture(scope="module")
def classes(trees):
    """{case: [(path, tie levels)] per feature}, from the plain numpy descent."""
    return {c.name: [trees[c.name].classify(f) for f in H.load_fixture(c.name)["feat"]] for c in H.CASES}


def test_corpus_has_the_required_cases():
    assert sorted(os.listdir(H.GOLD_DIR)) == sorted(c.name + ".npz" for c in H.CASES)
    assert all(c.k <= 20 for c in H.CASES)                                      # loadFromTextFile refuses more (:1371)
    shapes = {(c.k, c.L, c.seed, c.ragged) for c in H.CASES}
    assert shapes >= {(10, 4, 1, True), (10, 3, 2, False), (3, 6, 3, True), (20, 2, 4, False)}
    assert any(c.stop_fraction == 0.3 for c in H.CASES) and any(c.L == 1 for c in H.CASES)
    for c in H.CASES:
        fix = H.load_fixture(c.name)
        assert 300 <= len(fix["feat"]) <= 1500
        assert set(fix["kind"].tolist()) == {H.KIND_NODE, H.KIND_PERTURBED, H.KIND_RANDOM, H.KIND_TIE}
        assert set(fix["levelsups"].tolist()) == {4, 1, 0, 9, c.L}
        assert os.path.getsize(H.fixture_path(c.name)) < 200 * 1024


def test_fixture_conditions(trees, classes):
    """The corpus is only worth anything if it reaches the places where a descent goes wrong; counted from the fixtures alone."""
    assert len(H.RAGGED) == 2
    for name in H.RAGGED:
        fix = H.load_fixture(name)
        assert int((fix["node_1"] == H.UNSET).sum()) >= 50, name
        assert int((fix["node_0"] == H.UNSET).sum()) >= 50, name
    tied = at_recorded = stopped = 0
    for c in H.CASES:
        fix = H.load_fixture(c.name)
        for path, ties in classes[c.name]:
            tied += bool(ties)
            at_recorded += any(c.L - ls in ties for ls in fix["levelsups"].tolist())
        stopped += int((fix["weight_4"] == 0).sum())
    assert tied >= 50 and at_recorded >= 20 and stopped >= 30, (tied, at_recorded, stopped)
    single = [c.name for c in H.CASES if any(len(ch) == 1 for ch in trees[c.name].children)]
    assert single, "no vocabulary has an inner node with a single child"
    # a set-level map is recorded exactly where no node id is unset, and both kinds occur
    det = [bool(fix["det_%d" % ls]) == (not (fix["node_%d" % ls] == H.UNSET).any()) for _, fix, ls in _cases_levelsups()]
    assert all(det)
    assert any(not fix["det_%d" % ls] for _, fix, ls in _cases_levelsups()) and any(fix["det_%d" % ls] for _, fix, ls in _cases_levelsups())


@needs_ref
@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c.name)
def test_live_reference_equals_fixture(case):
    """Regenerated twice from the seeds and the reference's program: every array equals the committed one byte for byte."""
    fix = H.load_fixture(case.name)
    for run in range(2):
        got = H.generate(REF_EXE, case)
        assert sorted(got) == sorted(fix), (run, sorted(set(got) ^ set(fix)))
        for key in fix:
            a, b = np.asarray(got[key]), fix[key]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (case.name, run, key)


@needs_ref
def test_final_newline_quirk():
    """loadFromTextFile reads `while(!f.eof())` (:1390): a file that ends in a newline gets one phantom node more, which counts
    as a word.  A known answer of the reference, pinned so that nobody writes a fixture with a final newline."""
    fix = H.load_fixture("complete_k20_L2_s4")
    voc, feat = H.vocabulary_of(fix), fix["feat"][:4]
    plain = H.run_reference(REF_EXE, H.vocabulary_text(*voc), feat, 0)
    quirk = H.run_reference(REF_EXE, H.vocabulary_text(*voc, final_newline=True), feat, 0)
    assert plain["nwords"] == int(fix["nwords"]) == int(fix["is_leaf"].sum())
    assert quirk["nwords"] == plain["nwords"] + 1


def test_numpy_descent_equals_reference_fixture(trees):
    """The classifier itself: it reproduces the reference, UNSET included, so what it counts above is what the reference did."""
    for c, fix, ls in _cases_levelsups():
        word, weight, node = trees[c.name].rows(fix["feat"], ls)
        assert word.tobytes() == fix["word_%d" % ls].tobytes() and weight.tobytes() == fix["weight_%d" % ls].tobytes(), (c.name, ls)
        assert node.tobytes() == fix["node_%d" % ls].tobytes(), (c.name, ls)
        if fix["det_%d" % ls]:
            assert H.check_maps(fix, ls, *H.set_level(word, weight, node)) is None, (c.name, ls)


@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c.name)
def test_oracle_equals_reference_fixture(oracle, case):
    fix = H.load_fixture(case.name)
    voc = oracle.Vocabulary(*H.vocabulary_of(fix))
    for ls in fix["levelsups"].tolist():
        word, weight, node = voc.descend(fix["feat"], ls)
        assert H.check_rows(fix, ls, word, weight, node) is None, (case.name, ls, H.check_rows(fix, ls, word, weight, node))
        assert np.array_equal(node, H.expected_device_node(fix, ls))
        if fix["det_%d" % ls]:
            bw, bv = voc.bow_vector(fix["feat"], ls)
            fn, fi = voc.feature_vector(fix["feat"], ls)
            assert H.check_maps(fix, ls, bw, bv, fn, fi) is None, (case.name, ls, H.check_maps(fix, ls, bw, bv, fn, fi))


# ------------------------------------------------------------------------------------------------ the comparison can fail
def _rejected_rows(fix, ls, tree, **kw):
    word, weight, node = tree.rows(fix["feat"], ls, **kw)
    node = np.where(node == H.UNSET, 0, node)                                   # the answer the oracle and the device would give
    return H.check_rows(fix, ls, word, weight, node)


def test_check_rejects_last_child_winning_a_tie(classes):
    for c in H.CASES:
        fix = H.load_fixture(c.name)
        assert any(t for _, t in classes[c.name])
        mutant = H.Tree(*H.vocabulary_of(fix), tie="last")
        assert _rejected_rows(fix, 0, mutant) == "word id", c.name


def test_check_rejects_word_ids_numbered_by_node_id():
    for c in H.CASES:
        fix = H.load_fixture(c.name)
        mutant = H.Tree(*H.vocabulary_of(fix), word_order="node")
        assert _rejected_rows(fix, 4, mutant) == "word id", c.name


def test_check_rejects_node_id_one_level_too_deep(trees):
    for c in H.CASES:
        fix = H.load_fixture(c.name)
        hit = [ls for ls in fix["levelsups"].tolist() if 0 < c.L - ls < c.L]
        assert hit or c.L == 1, c.name                                          # L = 1 has no level below the recorded one
        for ls in hit:
            assert _rejected_rows(fix, ls, trees[c.name]) is None
            assert _rejected_rows(fix, ls, trees[c.name], nid_shift=1) in ("node id", "node id where the reference writes none"), (c.name, ls)


def test_check_rejects_stopped_feature_kept_in_feature_vector(trees):
    rejected = 0
    for c, fix, ls in _cases_levelsups(determinate_only=True):
        rows = trees[c.name].rows(fix["feat"], ls)
        assert H.check_maps(fix, ls, *H.set_level(*rows)) is None
        if (rows[1] == 0).any():
            assert H.check_maps(fix, ls, *H.set_level(*rows, keep_stopped=True)) in ("fv_node", "fv_index"), (c.name, ls)
            rejected += 1
    assert rejected >= 6


def test_check_rejects_l1_norm_in_feature_order(trees):
    fix = H.load_fixture(L1_ORDER_CASE)
    assert fix["det_%d" % L1_ORDER_LEVELSUP]
    rows = trees[L1_ORDER_CASE].rows(fix["feat"], L1_ORDER_LEVELSUP)
    assert H.check_maps(fix, L1_ORDER_LEVELSUP, *H.set_level(*rows)) is None
    assert H.check_maps(fix, L1_ORDER_LEVELSUP, *H.set_level(*rows, norm_order="feature")) == "bow_val"
