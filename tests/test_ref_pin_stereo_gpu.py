"""The stereo kernels and the descriptor matchers against the RECORDED RESULTS of the reference's own compiled text
(tests/golden/stereo_ref/, see tests/test_ref_pin_stereo.py and tests/helpers_stereo_ref.py), bit for bit.

k_stereo_points, k_stereo_median and k_stereo_lines get every `points` and `lines` fixture through the constructed-table route of
tests/helpers_stereo_gpu.py: one context per distinct configuration, four frames per call with a different case per frame, one
single-frame call, the line matcher in both launch forms (kl_cap < 192 in one launch, kl_cap >= 192 sliced).  uright, depth, disp, le,
counts[4] and counts[5] are compared with the fixtures; the DBG_STEREO_SAD values and best indices with what the labelled restatement
of tests/helpers_matchers.py says.  pli_match_lines, pli_match_nnr, pli_hamming_knn2, pli_descriptor_distance and the line half of
pli_batch_track are compared with the `nnr`, `match` and `dist` fixtures.  Rows that had to be removed before a case went to the
reference stay covered by tests/test_independent_matchers_gpu.py.  Nothing here reads anything but tests/golden/.
"""
import numpy as np
import pytest

import helpers_matchers as hm
import helpers_stereo_ref as S
from helpers_stereo_gpu import device, group_key, make_frontend, run_batch

pytestmark = pytest.mark.gpu

NAMES = S.fixture_names()
STEREO = [n for n in NAMES if n.startswith(("points_", "lines_"))]


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle


@pytest.fixture(scope="module")
def gpu():
    return device()


@pytest.fixture(scope="module")
def cases(gpu, po):
    """Every points / lines fixture as a case with the device's Config, and what the labelled restatement expects of DBG_STEREO_SAD."""
    out = []
    for name in STEREO:
        c, ref = S.case_of_fixture(name, gpu.capi.Config, None)
        c["ref"] = ref
        if name.startswith("points_"):
            cp, _ = S.case_of_fixture(name, po.Config, po)              # the oracle's pyramids, for the restatement alone
            c["best_idx"], c["sad"] = hm.run_points(cp)[2:4]
        out.append(c)
    return out


def check(c, got):
    rec, sad, bidx = got
    ref, name = c["ref"], c["name"]
    if name.startswith("points_"):
        n = len(c["kpL"])
        for what, a, b in (("uright", rec["uright"], ref["uright"]), ("depth", rec["depth"], ref["depth"]),
                           ("best index", bidx[:n], c["best_idx"]), ("SAD", sad[:n], c["sad"])):
            bad = np.flatnonzero(a.view(np.int32) != b.view(np.int32))
            assert bad.size == 0, "%s: %s differs from the reference at left keypoints %s" % (name, what, bad[:5])
        assert rec["counts"][4] == int((ref["uright"] >= 0).sum()), name
    else:
        assert rec["disp"].tobytes() == ref["disp"].tobytes(), "%s: disp differs from the reference at left lines %s" % (
            name, np.flatnonzero((rec["disp"] != ref["disp"]).any(1))[:5])
        assert rec["le"].dtype == np.float64 and rec["le"].tobytes() == ref["le"].tobytes(), "%s: le differs from the reference" % name
        assert rec["counts"][5] == int((ref["disp"][:, 0] >= 0).sum()), name


@pytest.mark.parametrize("lsd_nfeatures,sliced", [(160, False), (256, True)])
def test_stereo_kernels_equal_the_reference_fixtures(gpu, cases, lsd_nfeatures, sliced):
    groups = {}
    for c in cases:
        groups.setdefault(group_key(c), []).append(c)
    ncase = 0
    for group in groups.values():
        fe = make_frontend(gpu, group[0], 4, lsd_nfeatures, orb_nfeatures=500)
        assert (fe.kl_cap >= 192) == sliced, fe.kl_cap
        for i in range(0, len(group), 4):
            chunk = group[i:i + 4]
            for c, got in zip(chunk, run_batch(gpu, fe, chunk)):
                check(c, got)
                ncase += 1
        check(group[-1], run_batch(gpu, fe, [group[-1]])[0])          # one frame per call
        if len(group) > 1:                                              # and the same tables in another frame slot than before
            rev = group[:4][::-1]
            for c, got in zip(rev, run_batch(gpu, fe, rev)):
                check(c, got)
        fe.close()
    print("fixtures compared on the device: %d in %d contexts" % (ncase, len(groups)))
    assert ncase == len(STEREO) and sum(n.startswith("points_") for n in STEREO) >= 20 and sum(n.startswith("lines_") for n in STEREO) >= 15


def test_descriptor_matchers_equal_the_reference_fixtures(gpu):
    fe = gpu.Frontend(gpu.capi.default_config(128, 128))
    n_nnr = n_match = 0
    for name in NAMES:
        if not name.startswith(("nnr_", "match_")):
            continue
        ins, ref = S.load_fixture(name)
        d1, d2 = S.descriptor_inputs(name)
        nnr = float(ins["params"][0])
        if name.startswith("match_") and ins["params"][1] != 0:
            n, m = fe.match(d1, d2, nnr)                     # pli_match_lines: bestLRMatches both ways
            n_match += 1
        else:
            n, m = fe.match_nnr(d1, d2, nnr)                 # matchNNR, and match() with bestLRMatches off
            n_nnr += 1
        assert n == int(ref["ret"][0]) and m.tobytes() == ref["m12"].tobytes(), name
        idx, dist = fe.knn2(d1, d2)                          # an accepted match is the nearest train row, the lower one of equals
        ok = ref["m12"] >= 0
        if name.startswith("nnr_"):
            assert np.array_equal(idx[ok, 0], ref["m12"][ok]), name
            rej = ~ok                                        # and a rejected one failed the float test on the two distances
            assert not (dist[rej, 0].astype(np.float32) < dist[rej, 1].astype(np.float32) * np.float32(nnr)).any(), name
    for name in NAMES:
        if name.startswith("dist_"):
            ins, ref = S.load_fixture(name)
            assert fe.descriptor_distance(ins["a"], ins["b"]).tobytes() == ref["out"].tobytes(), name
    print("fixtures compared on the device: %d nnr, %d match, 2 dist" % (n_nnr, n_match))
    assert n_nnr >= 30 and n_match >= 9
    fe.close()


def test_track_line_matches_equal_a_match_fixture(gpu):
    """pli_batch_track on a two-frame batch: the left line descriptors of frame 0 and frame 1 are d1 and d2 of one `match` fixture
    (bestLRMatches on), so matches_12 of frame 1 against frame 0 is that fixture's result."""
    torch, capi = gpu.torch, gpu.capi
    name = "match_low_entropy_0.9_lr1"
    ins, ref = S.load_fixture(name)
    d1, d2 = S.descriptor_inputs(name)
    W, H, F = 128, 128, 2
    cfg = capi.default_config(W, H, orb_nfeatures=200, lsd_nfeatures=160, max_frames=F)
    fe = gpu.Frontend(cfg)
    assert max(len(d1), len(d2)) <= fe.kl_cap
    Y = fe.layout
    imgs = np.full((F, 2, H, W), 100, np.uint8)
    dimg = torch.from_numpy(imgs).cuda()
    dtab = torch.zeros(fe.table_bytes(F), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fe.batch_run_device(F, dimg.data_ptr(), dimg.data_ptr() + W * H, W, 2 * W * H, dtab.data_ptr(), stages=capi.RUN_ALL)
    fe.sync()
    tab = dtab.cpu().numpy().copy()
    for f, d in enumerate((d1, d2)):
        rec = tab[f * Y.record_bytes:(f + 1) * Y.record_bytes]
        counts = rec[Y.off_counts:Y.off_counts + 32].view(np.int32)
        counts[:6] = (0, 0, len(d), 0, 0, 0)
        rec[Y.off_ldesc[0]:Y.off_ldesc[0] + d.size] = np.ascontiguousarray(d).ravel()
    dtab.copy_(torch.from_numpy(tab))
    poses = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(-1), F)
    d_poses = torch.from_numpy(poses).cuda()
    tl = fe.track_layout()
    d_track = torch.zeros(F * tl.record_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fe.batch_track_device(F, dtab.data_ptr(), d_poses.data_ptr(), fe.track_params(nnr_lines=float(ins["params"][0])), d_track.data_ptr())
    fe.sync()
    tr = fe.parse_track(d_track.cpu().numpy(), 1)
    assert tr["counts"][2] == len(d1) and tr["counts"][3] == int(ref["ret"][0])
    assert tr["lines"].tobytes() == ref["m12"].tobytes()
    assert int(ref["ret"][0]) >= 5
    fe.close()
