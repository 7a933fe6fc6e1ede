"""The yardsticks of pli_distinctive_descriptors agree with each other and with answers worked out by hand, and their random inputs
exercise what they claim (ties for the least median, winners other than row 0); the Python mirror declares the entry.  No GPU."""
import numpy as np
import pytest

import helpers_distinctive as H

FLIPS = (0.05, 0.15, 0.5)


@pytest.fixture(scope="module")
def random_groups():
    """400 tracks of 3..39 rows per flip rate, with the restatement's answer for each."""
    out = {}
    for flip in FLIPS:
        rng = np.random.default_rng(int(flip * 1000) + 7)
        groups = [H.track(rng, int(rng.integers(3, 40)), flip) for _ in range(400)]
        out[flip] = [(g, H.restated_point(g)) for g in groups]
    return out


@pytest.mark.parametrize("flip", FLIPS)
def test_the_three_definitions_agree_on_random_tracks(random_groups, flip):
    for g, want in random_groups[flip]:
        assert H.restated_line(g) == want, len(g)
        assert H.independent(g) == want, len(g)


@pytest.mark.parametrize("flip", FLIPS)
def test_the_random_tracks_have_ties_and_winners_other_than_row_0(random_groups, flip):
    """On the restatement alone: a generator without ties would not test the strict `<`, one whose winner is always row 0 would pass
    a kernel that answers 0."""
    answers = [want for _, want in random_groups[flip]]
    ties = sum(1 for _, m, med in answers if med.count(m) > 1)
    moved = sum(1 for b, _, _ in answers if b != 0)
    print("flip %.2f: %d of %d groups tie for the least median, %d have BestIdx != 0" % (flip, ties, len(answers), moved))
    assert ties >= 0.10 * len(answers), ties
    assert moved >= 0.50 * len(answers), moved


@pytest.mark.parametrize("name", sorted(H.hand_groups()))
def test_hand_groups(name):
    g, want = H.hand_groups()[name]
    for fn in (H.restated_point, H.restated_line, H.independent):
        assert fn(g) == want, (name, fn.__name__)


def test_hand_groups_say_what_they_claim():
    hg = H.hand_groups()
    assert hg["one"][1][:2] == (0, 0) and hg["two"][1][:2] == (0, 0)
    assert 256 in hg["complement"][1][2] and 256 in hg["complement_median"][1][2]
    b, m, med = hg["tie"][1]
    assert med.count(m) >= 2 and b == med.index(m) and b != 0 and med[0] > m


def test_empty_groups_have_no_answer():
    best, bm, rows = H.expected([np.zeros((0, 32), np.uint8), H.hand_groups()["three"][0]])
    assert best.tolist() == [-1, 0] and bm.tolist() == [H.INT_MAX, 3] and rows.tolist() == [3, 3, 5]


def test_the_python_mirror_declares_the_entry():
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    assert "pli_distinctive_descriptors" in capi._PROTOS
    assert callable(getattr(Frontend, "distinctive_descriptors", None))
    assert capi.DISTINCTIVE_MAX_OBS == 2048
    assert hasattr(capi.lib(), "pli_distinctive_descriptors") and hasattr(capi.lib(dev=True), "pli_distinctive_descriptors")
