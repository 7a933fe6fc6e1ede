"""The C++ ComputeDistinctiveDescriptors adapters, executed: tests/cpp/distinctive_harness.cpp calls
PliComputeDistinctiveDescriptorsOfPoints / OfLines (pli_slam_amd/adapters/orbslam_map_features.hpp) on stub KeyFrame / MapPoint /
MapLine types with std::map observations; from the observation order the harness actually iterated, the descriptor every feature
ended with equals the row the restatements of MapPoint.cc:330-359 / MapLine.cc:278-312 (tests/helpers_distinctive.py) choose."""
import os
import subprocess

import numpy as np
import pytest

import helpers_distinctive as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")
UNTOUCHED = np.full(32, 0xAB, np.uint8)
NULL, GOOD, BAD = 0, 1, 2


def build(outdir):
    exe = os.path.join(outdir, "distinctive_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", ROOT, "-I", os.path.join(ROOT, "tests", "stubs"),
                        os.path.join(ROOT, "tests", "cpp", "distinctive_harness.cpp"), LIB, "-Wl,-rpath," + os.path.dirname(LIB),
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def keyframes(rng, nkf, n, bad_every=0):
    """(bad, mDescriptors, mDescriptors_l) per keyframe: the rows of feature f are noisy copies of a per-feature base, so that a
    track has a real median structure."""
    base = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    base_l = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    out = []
    for k in range(nkf):
        rate = 0.15 * rng.uniform(0.3, 1.5)
        out.append((bool(bad_every and k % bad_every == bad_every - 1),
                    np.stack([H.flip_bits(rng, d, rate) for d in base]), np.stack([H.flip_bits(rng, d, rate) for d in base_l])))
    return out


def write_input(path, kfs, batches):
    i32 = lambda *v: np.array(v, np.int32).tobytes()
    with open(path, "wb") as f:
        f.write(i32(len(kfs)))
        for bad, d, dl in kfs:
            f.write(i32(int(bad), len(d)) + np.ascontiguousarray(d, np.uint8).tobytes() + i32(len(dl)) + np.ascontiguousarray(dl, np.uint8).tobytes())
        f.write(i32(len(batches)))
        for lines, device, feats in batches:
            f.write(i32(int(lines), int(device), len(feats)))
            for kind, obs in feats:
                f.write(i32(kind, len(obs)) + b"".join(i32(k, idx) for k, idx in obs))


def read_output(path, batches):
    raw = np.fromfile(path, np.uint8)
    at = 0

    def ints(n):
        nonlocal at
        v = raw[at:at + 4 * n].view(np.int32).copy()
        at += 4 * n
        return v

    out = []
    for _, _, feats in batches:
        ret = int(ints(1)[0])
        rows = []
        for _ in feats:
            calls, nobs = ints(2).tolist()
            order = ints(2 * nobs).reshape(nobs, 2).tolist()
            rows.append((calls, order, raw[at:at + 32].copy()))
            at += 32
        out.append((ret, rows))
    assert at == len(raw)
    return out


def verify(kfs, batches, got):
    """Every feature against the restatement on the order the harness iterated; returns the device-group count per batch."""
    counts = []
    for (lines, _, feats), (ret, rows) in zip(batches, got):
        sent = 0
        for p, ((kind, obs), (calls, order, desc)) in enumerate(zip(feats, rows)):
            assert sorted(map(tuple, order)) == sorted(dict(obs).items()), p           # the feature's own observations, in the map's order
            live = [(k, i) for k, i in order if not kfs[k][0]]
            if kind != GOOD or not live:
                assert calls == 0 and np.array_equal(desc, UNTOUCHED), (p, kind, calls)
                continue
            group = np.stack([kfs[k][2 if lines else 1][i] for k, i in live])
            best = (H.restated_line if lines else H.restated_point)(group)[0]
            assert calls == 1 and np.array_equal(desc, group[best]), (p, len(group), best)
            sent += len(group) >= 3
        assert ret == sent, (ret, sent)
        counts.append(sent)
    return counts


def observations(rng, nkf, n, lo, hi):
    """A track: the feature index of rng.integers(lo, hi) distinct keyframes."""
    return [(int(k), int(rng.integers(0, n))) for k in rng.choice(nkf, int(rng.integers(lo, hi)), replace=False)]


def small_batch(rng, nkf, n, lines):
    """Groups of one or two live rows only, with a NULL and a bad feature among them."""
    good = [k for k in range(nkf)]
    feats = [(GOOD, [(good[int(k)], int(rng.integers(0, n))) for k in rng.choice(len(good), int(rng.integers(1, 3)), replace=False)])
             for _ in range(20)]
    return (lines, 0, feats + [(NULL, []), (BAD, observations(rng, nkf, n, 1, 3))])


def test_groups_of_one_and_two_rows_need_no_device(tmp_path):
    """Without any extractor there is no device context, so a device call would throw: the batch returns 0 and every descriptor is
    the first live observation's row.  Runs here (no GPU) and on the GPU box alike."""
    exe = build(str(tmp_path))
    rng = np.random.default_rng(5)
    kfs = keyframes(rng, 12, 30)
    batches = [small_batch(rng, 12, 30, 0), small_batch(rng, 12, 30, 1)]
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, kfs, batches)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = read_output(outp, batches)
    assert verify(kfs, batches, got) == [0, 0]
    for (lines, _, feats), (_, rows) in zip(batches, got):
        for (kind, _), (calls, order, desc) in zip(feats, rows):
            if kind == GOOD:
                k, i = order[0]
                assert np.array_equal(desc, kfs[k][2 if lines else 1][i])


def mixed_batches(rng, nkf, n):
    points = [(GOOD, observations(rng, nkf, n, 1, nkf + 1)) for _ in range(120)]
    points += [(NULL, []), (BAD, observations(rng, nkf, n, 3, 9)), (GOOD, []),                    # NULL, bad, no observations
               (GOOD, [(k, 3) for k in range(nkf) if k % 4 == 3]),                                # every observing keyframe bad
               (GOOD, [(k, 5) for k in range(nkf)])]                                              # seen by every keyframe, bad ones skipped
    rng.shuffle(points)
    lines = [(GOOD, observations(rng, nkf, n, 1, nkf + 1)) for _ in range(60)] + [(NULL, []), (BAD, observations(rng, nkf, n, 3, 9))]
    return [(0, 1, points), (1, 1, lines), small_batch(rng, nkf, n, 0)]


@pytest.mark.gpu
def test_distinctive_adapters_equal_the_restatement(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    exe = build(str(tmp_path))
    rng = np.random.default_rng(6)
    kfs = keyframes(rng, 80, 40, bad_every=4)
    batches = mixed_batches(rng, 80, 40)
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, kfs, batches)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    counts = verify(kfs, batches, read_output(outp, batches))
    assert counts[0] > 60 and counts[1] > 30 and counts[2] == 0, counts


def test_distinctive_harness_builds_and_fails_loudly_without_a_device(tmp_path):
    """Here (no GPU) the extractor call throws pli::Error(PLI_ERR_NO_DEVICE) and the harness exits with 1; on the GPU box the same
    program runs.  Either way it builds and links against the product library."""
    import torch
    exe = build(str(tmp_path))
    rng = np.random.default_rng(7)
    kfs = keyframes(rng, 8, 10)
    batches = [(0, 1, [(GOOD, observations(rng, 8, 10, 3, 8)) for _ in range(5)])]
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, kfs, batches)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
        verify(kfs, batches, read_output(outp, batches))
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)
