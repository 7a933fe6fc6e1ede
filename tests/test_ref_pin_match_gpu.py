"""The device's matcher searches against the reference's own recorded answers (tests/golden/match_ref, see
tests/test_ref_pin_match.py and tests/helpers_match_ref.py), not against the restatements: for every case the Frontend call of the
function - search_local_map, search_by_projection, search_by_projection_reloc, search_by_projection_sim3 in both projection forms,
search_by_bow, search_by_bow_kf, search_for_initialization (single calls and the chain), search_for_triangulation (bOnlyStereo and
bCoarse both ways) and fuse_search with reproj_gate both ways - equals what src/ORBmatcher.cc returned, exactly.

The batched entry points are called twice: once with every keyframe / candidate / neighbour of the case in ONE call, which is what
the kernels add over the reference, and once per reference call; both must equal the K single calls the fixtures recorded.
Reads only the fixtures and the helper.
"""
import numpy as np
import pytest

import helpers_match_ref as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    f = Frontend(capi.default_config(752, 480), dev=False)
    assert f.cfg.orb_nlevels == H.FU.NLEVELS
    yield f
    f.close()


@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c.name)
def test_device_equals_reference_fixture(fe, case):
    a, results = H.load_fixture(case.name)
    got = case.device(fe, a, case.calls)
    assert sorted(got) == sorted(case.calls)
    for call in case.calls:
        want = case.expected(a, call, results[call])
        batched, single = got[call]
        assert H.same(want, single), (case.name, call, "a call of its own")
        assert H.same(want, batched), (case.name, call, "one call over the whole case")
