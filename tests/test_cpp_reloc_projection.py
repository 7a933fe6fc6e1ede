"""The C++ SearchByProjection(Frame, KeyFrame, sAlreadyFound, th, ORBdist) adapters, executed (-m gpu):
tests/cpp/reloc_projection_harness.cpp runs the reference's signature of PliORBmatcher::SearchByProjection (ORBmatcher.cc:2325-2447)
candidate by candidate with the two settings of Tracking.cc:4290 / :4304, the batch form once, and the two successive calls of
:4290 / :4304 on one frame, on stub Frame / KeyFrame / MapPoint types: mvpMapPoints partly filled at entry, NULL and bad points in
the keyframe's list, a non-empty sAlreadyFound.  The containers equal the restatement of tests/test_reloc_projection_cpu.py.  The
level_ratio table and the poses are the ones the adapter built with this host's compiler (dumped), since its log(float) and its
-Rcw.t()*tcw need not be Python's to the last bit."""
import os
import subprocess

import numpy as np
import pytest

from test_fuse_search_cpu import CAM, NLEVELS
from test_reloc_projection_cpu import Cand, reloc_case, reloc_search_fast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")


def build(outdir):
    exe = os.path.join(outdir, "reloc_projection_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-pthread", "-I", ROOT, "-I",
                        os.path.join(ROOT, "tests", "stubs"), os.path.join(ROOT, "tests", "cpp", "reloc_projection_harness.cpp"),
                        LIB, "-Wl,-rpath," + os.path.dirname(LIB), "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def make_world(rng, ncand, nmp=300, nfeat=300):
    """reloc_case as containers: one pool (the candidates' lists one after the other, then three points that only hold frame
    rows); candidate k's list = its pool indices, -1 where the scene's state is NULL; bad points are bad in the pool; the points the
    scene calls already found are in sAlreadyFound, with the holders of the rows occupied at entry.
    -> fr, pool, pdesc, [(Cand, mp, found, entry)]"""
    fr, cands, states = reloc_case(rng, ncand, nmp, nfeat)
    pool = np.concatenate([cd.points for cd in cands] + [cands[0].points[:3]])
    pdesc = np.concatenate([cd.descs for cd in cands] + [cands[0].descs[:3]])
    holders = len(pool) - 3 + np.arange(3)
    pool["valid"] = 1
    per = []
    for k, (cd, st) in enumerate(zip(cands, states)):
        idx = (k * nmp + np.arange(nmp)).astype(np.int32)
        pool["valid"][idx[st == 1]] = 0                                  # isBad()
        mp = np.where(st == 0, -1, idx).astype(np.int32)                 # NULL
        entry = np.where(cd.occupied != 0, holders[rng.integers(0, 3, nfeat)], -1).astype(np.int32)
        found = np.unique(np.concatenate([idx[st == 2], entry[entry >= 0]])).astype(np.int32)
        per.append((cd, mp, found, entry))
    return fr, pool, pdesc, per


def write_input(path, world):
    fr, pool, pdesc, per = world
    with open(path, "wb") as f:
        f.write(np.array([len(per), len(pool), len(fr.x)], np.int32).tobytes())
        f.write(np.array(list(CAM), np.float32).tobytes())
        f.write(pool.tobytes() + np.ascontiguousarray(pdesc).tobytes())
        f.write(fr.x.tobytes() + fr.y.tobytes() + fr.octave.astype(np.int32).tobytes() + fr.angle.tobytes() +
                np.ascontiguousarray(fr.desc).tobytes())
        for cd, mp, found, entry in per:
            T = np.eye(4, dtype=np.float32)
            T[:3, :3], T[:3, 3] = cd.pose[:9].reshape(3, 3), cd.pose[9:12]
            f.write(np.array([len(mp), len(found)], np.int32).tobytes() + T.tobytes() + mp.tobytes() + cd.angles.tobytes() +
                    found.tobytes() + entry.tobytes())


def expected(world, k, pose, th, orb_dist, lr, entry=None, found=None):
    """-> nmatches, mvpMapPoints (pool indices) after candidate k's call"""
    fr, pool, pdesc, per = world
    cd, mp, found0, entry0 = per[k]
    entry = entry0 if entry is None else entry
    found = set((found0 if found is None else found).tolist())
    pts = pool[np.maximum(mp, 0)].copy()
    pts["valid"] = [(m >= 0 and pool["valid"][m] != 0 and m not in found) for m in mp.tolist()]
    c = Cand(pts, pdesc[np.maximum(mp, 0)], cd.angles, pose, (entry >= 0).astype(np.uint8))
    rows, _, n = reloc_search_fast(c, fr, CAM, th, orb_dist, True, lr)
    out = entry.copy()
    out[rows >= 0] = mp[rows[rows >= 0]]
    return n, out


@pytest.mark.gpu
def test_both_adapter_forms_equal_the_restatement(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    exe = build(str(tmp_path))
    for seed, ncand in ((61, 3), (62, 1)):
        world = make_world(np.random.default_rng(seed), ncand)
        inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
        write_input(inp, world)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        raw = np.fromfile(outp, np.int32)
        nf = len(world[0].x)
        tail = raw[ncand * (2 * (1 + nf) + (1 + nf) + (2 + nf)):].view(np.float32)
        lr, poses = tail[:NLEVELS - 1], tail[NLEVELS - 1:].reshape(ncand, 15)
        assert (np.diff(lr) > 0).all() and abs(lr[1] - 1.2) < 1e-5
        at, total = 0, 0
        for k in range(ncand):
            assert np.array_equal(poses[k][:12], world[3][k][0].pose[:12])               # Rcw and tcw are copied
            assert np.abs(poses[k][12:] - world[3][k][0].pose[12:]).max() < 1e-5
            for th, orb_dist in ((10.0, 100), (3.0, 64)):
                want = expected(world, k, poses[k], th, orb_dist, lr)
                assert raw[at] == want[0] and np.array_equal(raw[at + 1:at + 1 + nf], want[1]), ("single", k, th)
                assert (want[1] != world[3][k][3]).sum() == want[0]
                total += want[0]
                at += 1 + nf
        for k in range(ncand):                        # the batch form
            want = expected(world, k, poses[k], 10.0, 100, lr)
            assert raw[at] == want[0] and np.array_equal(raw[at + 1:at + 1 + nf], want[1]), ("batch", k)
            at += 1 + nf
        for k in range(ncand):                        # :4290, sFound from mvpMapPoints, :4304 on the same frame
            n1, mid = expected(world, k, poses[k], 10.0, 100, lr)
            n2, fin = expected(world, k, poses[k], 3.0, 64, lr, entry=mid, found=np.unique(mid[mid >= 0]))
            assert (raw[at], raw[at + 1]) == (n1, n2) and np.array_equal(raw[at + 2:at + 2 + nf], fin), ("replay", k)
            at += 2 + nf
        assert total > 30 * ncand, "the case matches nothing"


def test_reloc_projection_harness_builds_and_fails_loudly_without_a_device(tmp_path):
    """Here (no GPU) the extractor call throws pli::Error(PLI_ERR_NO_DEVICE) and the harness exits with 1; on the GPU box the
    same program runs.  Either way it builds and links against the product library."""
    import torch
    exe = build(str(tmp_path))
    world = make_world(np.random.default_rng(1), 2, 60, 50)
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, world)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
