"""The C++ SearchForInitialization adapter and the local-map SearchByProjection(Frame&, vector<MapPoint*>, ...) member, executed
(-m gpu): tests/cpp/init_search_harness.cpp runs PliORBmatcher::SearchForInitialization (ORBmatcher.cc:706-821) for frame 0 against
three later frames with mvbPrevMatched carried as Tracking.cc:2072-2110 does, and the local-map member (ORBmatcher.cc:44-143,
Tracking.cc:3854) on a frame with rows occupied at entry, bad points, points out of view and far points, on stub Frame / KeyFrame /
MapPoint types; it also calls every other SearchByProjection form once, so the build proves that no overload became ambiguous.  The
containers equal the restatements: tests/test_init_search_cpu.py and helpers_matchers.search_local_map."""
import os
import subprocess

import numpy as np
import pytest

from helpers_matchers import PROJ_QUERY_DT, search_local_map
from test_init_search_cpu import BOUNDS, chain, chain_scene, flip, init_search_fast, keypoints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")
f32 = np.float32
NNRATIO_LOCAL = 0.8                                       # ORBmatcher matcher(0.8) of Tracking::SearchLocalPoints
POINT_DT = np.dtype([("in_view", "<i4"), ("bad", "<i4"), ("nobs", "<i4"), ("level", "<i4"), ("depth", "<f4"), ("view_cos", "<f4"),
                     ("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("desc", "u1", (32,))])


def build(outdir):
    exe = os.path.join(outdir, "init_search_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-pthread", "-I", ROOT, "-I",
                        os.path.join(ROOT, "tests", "stubs"), os.path.join(ROOT, "tests", "cpp", "init_search_harness.cpp"),
                        LIB, "-Wl,-rpath," + os.path.dirname(LIB), "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def scale_factors(n=8):
    sf = [f32(1.0)]
    for _ in range(n - 1):
        sf.append(f32(sf[-1] * f32(1.2)))
    return np.array(sf, f32)


def make_world(rng, npool=300, cut=None):
    """chain_scene's four frames; on the last one: uright for a third of the rows, 15 % of the rows held at entry (some by points
    without observations, which do not occupy), and a local map of npool points aimed at its keypoints."""
    t1, frames = chain_scene()
    tabs = [t1] + list(frames)
    if cut:
        tabs = [t._replace(x=t.x[:cut], y=t.y[:cut], octave=t.octave[:cut], desc=t.desc[:cut], angle=t.angle[:cut]) for t in tabs]
    last = tabs[-1]
    nf = len(last.x)
    uright = np.where(rng.random(nf) < 0.33, last.x - rng.uniform(1, 30, nf), -1.0).astype(f32)
    pool = np.zeros(npool, POINT_DT)
    j = rng.integers(0, nf, npool)
    pool["in_view"] = rng.random(npool) < 0.85
    pool["bad"] = rng.random(npool) < 0.1
    pool["level"] = last.octave[j] + (rng.random(npool) < 0.4)
    pool["depth"] = rng.uniform(1, 70, npool)
    pool["view_cos"] = rng.uniform(0.995, 1.0, npool)
    pool["proj_x"] = last.x[j] + rng.uniform(-2.5, 2.5, npool)
    pool["proj_y"] = last.y[j] + rng.uniform(-2.5, 2.5, npool)
    pool["proj_xr"] = np.where(uright[j] > 0, uright[j] + rng.uniform(-4, 4, npool), pool["proj_x"] - 5)
    pool["desc"] = np.stack([flip(rng, last.desc[k], int(rng.integers(0, 120))) for k in j])
    searching = (pool["in_view"] != 0) & (pool["bad"] == 0)
    pool["nobs"] = np.where(searching, rng.integers(1, 5, npool), rng.integers(0, 3, npool))
    entry = np.where(rng.random(nf) < 0.15, rng.integers(0, npool, nf), -1).astype(np.int32)
    return tabs, uright, entry, pool


def write_input(path, world, window=100, nnratio=0.9, th=3, b_far=1, th_far=50.0):
    tabs, uright, entry, pool = world
    with open(path, "wb") as f:
        f.write(np.array([len(tabs), window, b_far, len(pool)], np.int32).tobytes())
        f.write(np.array(list(BOUNDS) + [nnratio, th, th_far], f32).tobytes() + scale_factors().tobytes())
        for k, t in enumerate(tabs):
            n = len(t.x)
            lastone = k == len(tabs) - 1
            f.write(np.array([n], np.int32).tobytes() + t.x.tobytes() + t.y.tobytes() + t.octave.astype(np.int32).tobytes() +
                    t.angle.tobytes() + np.ascontiguousarray(t.desc).tobytes() +
                    (uright if lastone else np.full(n, -1, f32)).tobytes() + (entry if lastone else np.full(n, -1, np.int32)).tobytes())
        f.write(pool.tobytes())


def expected_local_map(world, th=3, b_far=1, th_far=50.0):
    """-> nmatches, mvpMapPoints (pool indices) as the adapter leaves them: the gates of ORBmatcher.cc:53-62, RadiusByViewingCos
    (:216-222) times th, the query of pli_search_local_map's header, cur_occupied from the rows whose point has observations."""
    tabs, uright, entry, pool = world
    last = tabs[-1]
    sf = scale_factors()
    q = np.zeros(len(pool), PROJ_QUERY_DT)
    valid = (pool["in_view"] != 0) & (pool["bad"] == 0)
    if b_far:
        valid &= ~(pool["depth"] > f32(th_far))
    r = np.where(pool["view_cos"] > 0.998, f32(2.5), f32(4.0)).astype(f32)
    if f32(th) != 1.0:
        r = (r * f32(th)).astype(f32)
    q["u"], q["v"], q["ur"] = pool["proj_x"], pool["proj_y"], pool["proj_xr"]
    q["radius"] = (r * sf[pool["level"]]).astype(f32)
    q["min_level"], q["max_level"] = pool["level"] - 1, pool["level"]
    q["valid"] = valid
    occupied = np.array([e >= 0 and pool["nobs"][e] > 0 for e in entry.tolist()], np.uint8)
    n, best, _ = search_local_map(q, pool["desc"], keypoints(last), last.desc, uright, occupied, BOUNDS, NNRATIO_LOCAL)
    out = entry.copy()
    for i in np.flatnonzero(best >= 0):
        out[best[i]] = i
    return n, out, int(valid.sum())


@pytest.mark.gpu
def test_the_adapters_equal_the_restatements(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    exe = build(str(tmp_path))
    world = make_world(np.random.default_rng(71))
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, world)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    raw = np.fromfile(outp, np.int32)
    tabs = world[0]
    n1 = len(tabs[0].x)
    at = 0
    want = chain(init_search_fast, tabs[0], tabs[1:], window=100, nnratio=0.9)
    for k, (_, m12, nm, prev) in enumerate(want):
        assert raw[at] == nm and np.array_equal(raw[at + 1:at + 1 + n1], m12), ("SearchForInitialization", k)
        assert raw[at + 1 + n1:at + 1 + 3 * n1].view(f32).tobytes() == prev.tobytes(), ("vbPrevMatched", k)
        assert nm > 30
        at += 1 + 3 * n1
    n, out, nvalid = expected_local_map(world)
    nf = len(tabs[-1].x)
    assert raw[at] == n and np.array_equal(raw[at + 1:at + 1 + nf], out), "the local map"
    assert at + 1 + nf == len(raw)
    assert n > 40 and nvalid < len(world[3]) - 60, (n, nvalid)


def test_the_local_map_case_is_not_vacuous():
    """On the CPU: the case has bad points, points out of view, far points, rows held at entry with and without observations, and
    matches that land on rows held by a point without observations."""
    world = make_world(np.random.default_rng(71))
    _, _, entry, pool = world
    n, out, nvalid = expected_local_map(world)
    n2, _, nvalid2 = expected_local_map(world, b_far=0)
    held = entry >= 0
    with_obs = np.array([e >= 0 and pool["nobs"][e] > 0 for e in entry.tolist()])
    assert n > 40 and nvalid2 > nvalid and n2 > n
    assert (pool["bad"] != 0).sum() > 10 and (pool["in_view"] == 0).sum() > 10
    assert with_obs.sum() > 10 and (held & ~with_obs).sum() > 3
    assert (out[with_obs] == entry[with_obs]).all()                           # occupied rows are never written
    assert not ((pool["in_view"] != 0) & (pool["bad"] == 0) & (pool["nobs"] == 0)).any()


def test_init_search_harness_builds_and_fails_loudly_without_a_device(tmp_path):
    """Here (no GPU) the extractor call throws pli::Error(PLI_ERR_NO_DEVICE) and the harness exits with 1; on the GPU box the
    same program runs.  Either way it builds - every SearchByProjection overload resolves - and links against the product library."""
    import torch
    exe = build(str(tmp_path))
    world = make_world(np.random.default_rng(1), 40, cut=60)
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, world)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
