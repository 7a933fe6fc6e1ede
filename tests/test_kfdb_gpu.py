"""The keyframe database on the device (pli_kfdb_*, k_kfdb_query) through Frontend: the recorded worlds of tests/golden/kfdb_ref
replayed operation by operation, with common / first / score of every slot (free ones included) equal to the reference's recorded
answers and to the restatement of tests/helpers_kfdb.py byte for byte, and the two whole functions run on the device's answers equal
to the reference's candidates and members; the launch's grid edges; the arena's growth, rebuild and slot reuse; the argument errors.
"""
import numpy as np
import pytest

import helpers_kfdb as H

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


def same_bytes(got, want):
    return all(np.asarray(g).dtype == np.asarray(w).dtype and np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


def vector(rng, n, nwords=1 << 20):
    """A BowVector of n words with values of mixed magnitude, normalised like DBoW2's."""
    w = np.sort(rng.choice(nwords, n, replace=False)).astype(np.uint32)
    v = rng.uniform(0.5, 9.0, n) * rng.choice([1, 1, 2, 40], n)
    return w, v / v.sum() if n else v


@pytest.mark.parametrize("name", [w.name for w in H.WORLDS])
def test_the_recorded_sequence_equals_the_reference_and_the_restatement(gpu, name):
    fe, fix = gpu, H.load_fixture(name)
    maps, kfs = H.stubs_of(fix)
    db, h = H.Database(), fe.kfdb_create()
    db.answers_fn = lambda qw, qv: fe.kfdb_query(h, qw, qv, len(db.slot_kf))
    out, j = [], 0
    try:
        for kind, a, b, c in fix["ops"].tolist():
            if kind == H.OP_ADD:
                assert fe.kfdb_add(h, kfs[a].words, kfs[a].values) == db.add(kfs[a])
            elif kind == H.OP_ERASE:
                fe.kfdb_erase(h, db.erase(kfs[a]))
            elif kind == H.OP_CLEAR_MAP:
                for s in db.clear_map(maps[a]):
                    fe.kfdb_erase(h, s)
            elif kind == H.OP_CLEAR:
                db.clear(); fe.kfdb_clear(h)
            else:
                qw, qv = H.query_bow(fix, j)
                got = fe.kfdb_query(h, qw, qv, len(db.slot_kf))
                assert same_bytes(got, H.answers(qw, qv, db.slots())), (name, j)
                assert same_bytes(got, fe.kfdb_query(h, qw, qv)), (name, j, "two queries in a row differ")
                for s, kf in enumerate(db.slot_kf):
                    if kf is None:
                        assert got[0][s] == 0 and got[1][s] == -1 and got[2][s] == 0 and np.signbit(got[2][s])
                    else:
                        assert got[0][s] == fix["common"][j, kf.index], (name, j, s)
                        assert got[2][s].tobytes() == fix["score"][j, kf.index].tobytes(), (name, j, s, got[2][s], fix["score"][j, kf.index])
                if kind == H.OP_RELOC:
                    loop, merge = db.detect_relocalization_candidates(a, qw, qv, maps[b]), []
                else:
                    loop, merge = db.detect_n_best_candidates(kfs[a], b)
                out.append({"loop": [k.mnId for k in loop], "merge": [k.mnId for k in merge], "members": [k.members() for k in kfs]})
                j += 1
        assert H.differences(fix, out) == []
    finally:
        fe.kfdb_destroy(h)


def test_grid_edges_one_word_keyframes_and_the_largest_vectors(gpu):
    """More slots than four rounds of the launch's waves hold, by three; one keyframe and one query of PLI_BOW_MAX_FEATURES words
    (every chunk of 64 full, the staged query at its 32 KiB); queries of no word and of one word."""
    from pli_slam_amd import capi
    fe, rng = gpu, np.random.default_rng(5)
    n = 4 * capi.KFDB_QUERY_MAX_WAVES + 3
    big_w, big_v = vector(rng, capi.BOW_MAX_FEATURES, 3 * capi.BOW_MAX_FEATURES)
    q_w, q_v = vector(rng, capi.BOW_MAX_FEATURES, 3 * capi.BOW_MAX_FEATURES)
    ones = rng.integers(0, 3 * capi.BOW_MAX_FEATURES, n).astype(np.uint32)
    slots = [(ones[i:i + 1], np.ones(1)) for i in range(n)] + [(big_w, big_v)]
    h = fe.kfdb_create()
    try:
        for s, (w, v) in enumerate(slots):
            assert fe.kfdb_add(h, w, v) == s
        assert fe.kfdb_stats(h)["slot_high_water"] == n + 1
        for qw, qv in ((q_w, q_v), (q_w[:0], q_v[:0]), (big_w[100:101], np.ones(1)), (ones[n - 1:n], np.ones(1))):
            got = fe.kfdb_query(h, qw, qv)
            want = H.answers(qw, qv, slots)
            assert same_bytes(got, want), len(qw)
        assert fe.kfdb_query(h, q_w, q_v)[0][n] > 1000          # the two large vectors share thousands of words
    finally:
        fe.kfdb_destroy(h)


def test_growth_rebuild_slot_reuse_and_clear(gpu):
    fe, rng = gpu, np.random.default_rng(6)
    h = fe.kfdb_create()
    slots = []
    qw, qv = vector(rng, 900, 4000)

    def check():
        st = fe.kfdb_stats(h)
        assert st["slot_high_water"] == len(slots) and st["live_keyframes"] == sum(s is not None for s in slots)
        assert st["live_words"] == sum(len(s[0]) for s in slots if s is not None) <= st["arena_words"] <= st["arena_capacity"]
        assert same_bytes(fe.kfdb_query(h, qw, qv, len(slots)), H.answers(qw, qv, slots))
        return st

    def add():
        kf = vector(rng, int(rng.integers(700, 1300)), 4000)
        s = fe.kfdb_add(h, *kf)
        free = [i for i, x in enumerate(slots) if x is None]
        assert s == (free[0] if free else len(slots))             # the smallest free slot
        if s == len(slots):
            slots.append(kf)
        else:
            slots[s] = kf
        return check()

    try:
        st = check()
        cap0 = st["arena_capacity"]
        while st["growths"] == 0:
            assert len(slots) < 200
            st = add()
        assert st["arena_capacity"] == 2 * cap0 and st["rebuilds"] == 0
        if len(slots) % 2 == 0:
            st = add()
        for s in range(0, len(slots), 2):                         # every other keyframe, the larger half of them
            fe.kfdb_erase(h, s)
            slots[s] = None
            st = check()
        for s in range(1, len(slots), 2):                         # (their sizes differ: until the holes exceed half of the words)
            if 2 * (st["arena_words"] - st["live_words"]) > st["arena_words"]:
                break
            fe.kfdb_erase(h, s)
            slots[s] = None
            st = check()
        assert 2 * (st["arena_words"] - st["live_words"]) > st["arena_words"] and st["rebuilds"] == 0
        nadd = 0
        while st["rebuilds"] == 0:
            assert nadd < 4
            st = add(); nadd += 1
        assert nadd == 1 and st["arena_words"] == st["live_words"]        # the next add rebuilt: no holes
        for _ in range(5):                                         # free slots are handed out again, smallest first
            st = add()
        assert st["rebuilds"] == 1 and st["slot_high_water"] == len(slots)
        fe.kfdb_clear(h)
        slots.clear()
        st = check()
        assert st["slot_high_water"] == 0 and st["arena_words"] == 0
        c, f, s = fe.kfdb_query(h, qw, qv)
        assert len(c) == len(f) == len(s) == 0
        add(); add()
    finally:
        fe.kfdb_destroy(h)


def test_argument_errors_leave_the_database_unchanged(gpu):
    from pli_slam_amd import capi
    fe, rng = gpu, np.random.default_rng(7)
    h = fe.kfdb_create()
    try:
        slots = [vector(rng, 50, 500) for _ in range(3)]
        for kf in slots:
            fe.kfdb_add(h, *kf)
        fe.kfdb_erase(h, 1)
        slots[1] = None
        qw, qv = vector(rng, 200, 500)
        before = (fe.kfdb_stats(h), fe.kfdb_query(h, qw, qv))
        big = np.arange(capi.BOW_MAX_FEATURES + 1, dtype=np.uint32)
        bad = [
            (-3, lambda: fe.kfdb_add(h, big, np.ones(len(big)))),
            (-3, lambda: fe.kfdb_query(h, big, np.ones(len(big)))),
            (-1, lambda: fe.kfdb_add(h, np.array([5, 3, 9], np.uint32), np.ones(3))),
            (-1, lambda: fe.kfdb_add(h, np.array([3, 5, 5], np.uint32), np.ones(3))),
            (-1, lambda: fe.kfdb_query(h, np.array([5, 3], np.uint32), np.ones(2))),
            (-1, lambda: fe.kfdb_query(h, np.array([4, 4], np.uint32), np.ones(2))),
            (-1, lambda: fe.kfdb_query(h, qw, qv, 2)),
            (-1, lambda: fe.kfdb_query(h, qw, qv, 4)),
            (-1, lambda: fe.kfdb_erase(h, 1)),
            (-1, lambda: fe.kfdb_erase(h, 3)),
            (-1, lambda: fe.kfdb_erase(h, -1)),
        ]
        for status, call in bad:
            with pytest.raises(capi.PliError) as e:
                call()
            assert e.value.status == status, (status, str(e.value))
            after = (fe.kfdb_stats(h), fe.kfdb_query(h, qw, qv))
            assert after[0] == before[0] and same_bytes(after[1], before[1])
        assert same_bytes(before[1], H.answers(qw, qv, slots))
        assert fe.kfdb_add(h, np.zeros(0, np.uint32), np.zeros(0)) == 1          # an empty keyframe is valid, in the freed slot
        slots[1] = (np.zeros(0, np.uint32), np.zeros(0))
        assert same_bytes(fe.kfdb_query(h, qw, qv), H.answers(qw, qv, slots))
    finally:
        fe.kfdb_destroy(h)
