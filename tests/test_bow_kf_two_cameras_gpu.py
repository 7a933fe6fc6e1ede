"""pli_search_by_bow_kf on the MI355X fed the tables that PliORBmatcherTwoCameras::SearchByBoW(pKF1, pKF2, vpMatches12) gathers
for keyframes of two cameras (rows idx >= mvKeysUn.size() with valid = 0 and angle 0) equals the literal restatement of
ORBmatcher.cc:823-963 with its two `continue`s (tests/test_bow_kf_two_cameras_cpu.py), for mvKeysUn.size() equal to 0, NLeft and
N on either side."""
import numpy as np
import pytest

from pli_slam_amd import capi
from test_bow_kf_two_cameras_cpu import cases, masked, search_literal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd.frontend import Frontend
    f = Frontend(capi.default_config(752, 480), dev=False)
    yield f
    f.close()


def test_the_device_fed_the_masks_equals_the_literal_restatement(fe):
    total = 0
    for kf1, kfs in cases():
        for ratio, ori in ((0.75, True), (0.7, False)):
            m, n = fe.search_by_bow_kf(*masked(kf1), [masked(kf) for kf in kfs], nnratio=ratio, check_orientation=ori)
            for k, kf2 in enumerate(kfs):
                want_m, want_n = search_literal(kf1, kf2, ratio, ori)
                assert np.array_equal(m[k], want_m) and n[k] == want_n, (k, int((m[k] != want_m).sum()), n[k], want_n)
                total += want_n
    assert total > 0
