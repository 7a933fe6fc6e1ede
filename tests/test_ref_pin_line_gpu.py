"""The device's line chain against the reference's own recorded outputs (tests/golden/line_ref, see tests/test_ref_pin_line.py and
tests/helpers_line_ref.py), not against the oracle: key-line construction, the top-N cut and the LBD bytes, through
Frontend.line_extract on both eyes and, as frame 1 of a two-frame batch whose frame 0 is a different image, batch_run_host.

Byte equality, per field with row indices; no tolerance.  Rows must match in place except inside the tie groups of the cases that
helpers_line_ref names (the device sorts stably, the reference with std::sort): the same rule as on the CPU.

The fixtures were produced with the float overloads of atan2 and cos / sin (both of the reference's programs agree on that), so the
contexts set PLI_PARITY_TRIG_F32_KEYLINE, and PLI_PARITY_TRIG_F32_LBD set is the value that must reproduce the LBD bytes.  With
PLI_PARITY_TRIG_F32_LBD clear no program of the reference corresponds: the key lines must still be the fixture's, and the rows whose 32
bytes differ are printed, not asserted.  Reads only the fixtures and the helper.
"""
import collections

import numpy as np
import pytest

import helpers_line_ref as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    return capi, Frontend


def _groups():
    """Image cases by configuration, so that each context is created once: [((W, H, nfeatures, min_line_length), [Case, ...])]."""
    g = collections.OrderedDict()
    for c in H.IMAGE_CASES:
        h, w = c.image().shape
        g.setdefault((w, h, c.nfeatures, c.min_line_length), []).append(c)
    return list(g.items())


def _check(case, fix, kl, desc, what, bytes_asserted):
    msgs, moved_inside, moved_straddle = H.compare_with_ties(case, fix, kl, desc, with_desc=bytes_asserted)
    if not bytes_asserted:
        differing = [m for m in H.compare_with_ties(case, fix, kl, desc)[0] if m.startswith("descriptor bytes")]
        print("%s: %s" % (what, differing or "the 32 bytes equal the fixture's in every row outside tie groups"))
    assert not msgs, "%s differs from the reference's fixture: %s" % (what, msgs)
    if case.name not in H.TIE_INSIDE + H.TIE_STRADDLE:
        assert kl.tobytes() == fix["kl"].tobytes(), what
    return moved_inside, moved_straddle


@pytest.mark.parametrize("lbd_f32", [True, False], ids=["lbd_f32_set", "lbd_f32_clear"])
@pytest.mark.parametrize("group", _groups(), ids=lambda g: "%dx%d_n%d_mll%g" % g[0])
def test_device_equals_reference_fixture(gpu, group, lbd_f32):
    capi, Frontend = gpu
    (w, h, nfeatures, mll), cases = group
    cfg = capi.default_config(w, h, lsd_nfeatures=nfeatures, min_line_length=mll, orb_nfeatures=100, orb_nlevels=2, max_frames=2)
    assert cfg.parity_flags & (capi.PARITY_TRIG_F32_LBD | capi.PARITY_TRIG_F32_KEYLINE) == 0        # the defaults stay clear
    cfg.parity_flags |= capi.PARITY_TRIG_F32_KEYLINE | (capi.PARITY_TRIG_F32_LBD if lbd_f32 else 0)
    fe = Frontend(cfg)
    for c in cases:
        img = c.image()
        fix = H.load_fixture(c.name)
        for eye in (0, 1):
            n, kl, desc = fe.line_extract(eye, img)
            assert n == len(fix["kl"]), (c.name, "key-line count", n, len(fix["kl"]))
            moved = _check(c, fix, kl, desc, "%s line_extract eye %d" % (c.name, eye), lbd_f32)
        other = np.ascontiguousarray(255 - img[::-1, ::-1])
        assert not np.array_equal(other, img)
        recs = fe.batch_run_host(np.stack([np.stack([other, other]), np.stack([img, other])]), stages=capi.RUN_LINES)
        assert _check(c, fix, recs[1]["klL"], recs[1]["ldescL"], c.name + " batch_run_host frame 1", lbd_f32) == moved
        assert recs[1]["klR"].tobytes() == recs[0]["klL"].tobytes() and np.array_equal(recs[1]["ldescR"], recs[0]["ldescL"])
        if c.name in H.TIE_INSIDE + H.TIE_STRADDLE:
            print("%s: %d rows differ inside kept tie groups, %d from the straddling group on" % ((c.name,) + moved))
    fe.close()
