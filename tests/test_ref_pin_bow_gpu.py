"""The device's vocabulary descent (k_bow_descend behind pli_bow_transform) against the reference's own recorded DBoW2 answers
(tests/golden/bow_ref, see tests/test_ref_pin_bow.py and tests/helpers_bow_ref.py), not against the oracle: word id, weight bits
and node id of every feature of every case and levelsup, with 0 where the reference's descent never stores a node id (this
project's rule).  ORB and LBD rows go through the same kernel as 32-byte rows, so the fixtures' byte rows stand for both.
One tree with k = 70 is held to the oracle only, because the reference's loader refuses k > 20: it exercises the `c += 64` stride
of the kernel's child loop.  Reads only the fixtures, the helper and the oracle library.
"""
import numpy as np
import pytest

import helpers_bow_ref as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    fe = Frontend(capi.default_config(128, 96, orb_nfeatures=100, lsd_nfeatures=0))
    yield fe
    fe.close()


def _accumulate(word, wt, node):
    """The caller's accumulation of test_bow_vocabulary_descent (BowVector::addWeight in feature order, L1 norm in word order),
    with FeatureVector::addFeature beside it."""
    bow, fv = {}, {}
    for i, (w_, v_, n_) in enumerate(zip(word.tolist(), wt.tolist(), node.tolist())):
        if v_ > 0:
            bow[w_] = bow.get(w_, 0.0) + v_
            fv.setdefault(n_, []).append(i)
    norm = 0.0
    for w_ in sorted(bow):
        norm += abs(bow[w_])
    vals = [bow[w_] / norm for w_ in sorted(bow)]
    return (np.array(sorted(bow), np.uint32), np.array(vals, np.float64),
            np.array([n_ for n_ in sorted(fv) for _ in fv[n_]], np.uint32), np.array([i for n_ in sorted(fv) for i in fv[n_]], np.uint32))


@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c.name)
def test_device_equals_reference_fixture(gpu, case):
    fe = gpu
    fix = H.load_fixture(case.name)
    feat = fix["feat"]
    gv = fe.vocab_create(*H.vocabulary_of(fix))
    for ls in fix["levelsups"].tolist():
        word, wt, node = fe.bow_transform(gv, feat, ls)
        assert H.check_rows(fix, ls, word, wt, node) is None, (case.name, ls, H.check_rows(fix, ls, word, wt, node))
        assert np.array_equal(node, H.expected_device_node(fix, ls)), (case.name, ls)
        if fix["det_%d" % ls]:
            assert H.check_maps(fix, ls, *_accumulate(word, wt, node)) is None, (case.name, ls)
    # batch edges of the kernel, against the fixture rows
    ls = 1
    want = (fix["word_%d" % ls].astype(np.int32), fix["weight_%d" % ls], H.expected_device_node(fix, ls))
    for i in (0, len(feat) - 1):                                                # n = 1
        got = fe.bow_transform(gv, feat[i:i + 1], ls)
        assert all(g.shape == (1,) and g.tobytes() == w[i:i + 1].tobytes() for g, w in zip(got, want)), (case.name, i)
    assert all(len(g) == 0 for g in fe.bow_transform(gv, feat[:0], ls))         # n = 0
    cut = len(feat) // 3 + 1                                                    # one call and two calls
    halves = [fe.bow_transform(gv, feat[:cut], ls), fe.bow_transform(gv, feat[cut:], ls)]
    for j, w in enumerate(want):
        assert np.concatenate([halves[0][j], halves[1][j]]).tobytes() == w.tobytes(), (case.name, j)
    fe.vocab_destroy(gv)


def _even_distance(a, b):
    """b with one bit flipped where needed, so that a and b differ in an even number of bits."""
    if H.hamming(a, b) % 2:
        b = b.copy()
        b[0] ^= 1
    return b


def _wide_tree(k=70, seed=11):
    """k = 70, L = 2: 70 random children of the root, 70 perturbed copies under each.  The pairs at child positions (0, 64) and
    (63, 69) of every inner node differ in an even number of bits, so a feature can sit exactly between them."""
    rng = np.random.default_rng(seed)
    pairs = ((0, 64), (63, 69))
    top = rng.integers(0, 256, (k, 32), dtype=np.uint8)
    for a, b in pairs:
        top[b] = _even_distance(top[a], top[b])
    parent, is_leaf, desc, weight = [0] * k, [0] * k, list(top), [0.0] * k
    for p in range(k):
        ch = np.repeat(top[p][None], k, axis=0)
        for c in range(k):
            for bit in rng.integers(0, 256, 24):
                ch[c, bit >> 3] ^= np.uint8(1 << (bit & 7))
        for a, b in pairs:
            ch[b] = _even_distance(ch[a], ch[b])
        parent += [p + 1] * k; is_leaf += [1] * k; desc += list(ch)
        weight += [0.0 if rng.random() < 0.05 else float(rng.uniform(0.5, 9.0)) for _ in range(k)]
    return (k, 2, np.array(parent, np.int32), np.array(is_leaf, np.uint8), np.stack(desc).astype(np.uint8), np.array(weight, np.float64)), pairs


def test_wide_tree_child_loop_stride(gpu):
    """k = 70 > 64: a lane of the wave takes children c and c + 64.  Ties between child positions 0 / 64 (the same lane) and
    63 / 69 (the last lane against a second-trip lane), at both levels; the first must win.  Held to the oracle, and the plain
    numpy descent confirms that the ties are where they were placed."""
    from oracle import pyoracle as po
    fe = gpu
    voc, pairs = _wide_tree()
    tree = H.Tree(*voc)
    rng = np.random.default_rng(12)
    feats, placed = [], []
    for p in [0] + [int(x) for x in tree.children[0][[0, 5, 63, 64, 69]]]:     # the root and five level-1 nodes
        ch = tree.children[p]
        assert len(ch) == 70
        for a, b in pairs:
            f = H.tie_feature(tree.desc[ch[a]], tree.desc[ch[b]], rng)
            assert f is not None
            d = H.hamming(tree.desc[ch], f)
            assert np.array_equal(np.flatnonzero(d == d.min()), [a, b]), (p, a, b)
            placed.append((len(feats), int(tree.level[p]) + 1, int(ch[a])))
            feats.append(f)
    feats = np.vstack([np.stack(feats), voc[4][rng.integers(0, len(voc[4]), 150)], rng.integers(0, 256, (150, 32), dtype=np.uint8)])
    for i, level, first in placed:                                               # the descent reaches the tie and takes the first
        path, ties = tree.classify(feats[i])
        assert level in ties and path[level - 1] == first, (i, level, path)
    ov = po.Vocabulary(*voc)
    gv = fe.vocab_create(*voc)
    for ls in (0, 1, 2, 9):
        word, wt, node = fe.bow_transform(gv, feats, ls)
        oword, owt, onode = ov.descend(feats, ls)
        nword, nwt, nnode = tree.rows(feats, ls)
        assert np.array_equal(word, oword) and wt.tobytes() == owt.tobytes() and np.array_equal(node, onode), ls
        assert np.array_equal(word, nword.astype(np.int32)) and wt.tobytes() == nwt.tobytes() and np.array_equal(node, nnode.astype(np.int32)), ls
    fe.vocab_destroy(gv)
