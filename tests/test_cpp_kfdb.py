"""The C++ keyframe database adapter (pli_slam_amd/adapters/orbslam_keyframe_database.hpp), executed: tests/cpp/kfdb_harness.cpp runs
PliKeyFrameDatabase on stub KeyFrame / Frame / Map types over a recorded world of tests/golden/kfdb_ref; the candidates and the six
members of every keyframe after every query equal the REFERENCE's recorded answers; a second add() and a bad keyframe in the sorted
list of DetectNBestCandidates throw std::logic_error.  On the device (-m gpu) against the product library; here against
tests/cpp/mock_pli_kfdb.cpp, as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import struct
import subprocess

import numpy as np
import pytest

import helpers_kfdb as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pli_slam_amd", "csrc", "libpli_frontend.so")
HARNESS = os.path.join(ROOT, "tests", "cpp", "kfdb_harness.cpp")


def build(outdir):
    exe = os.path.join(outdir, "kfdb_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", ROOT, HARNESS, LIB, "-Wl,-rpath," + os.path.dirname(LIB),
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def write_input(path, fix, asks=5):
    row = lambda off, flat, i: flat[off[i]:off[i + 1]]
    b = struct.pack("<i", len(fix["map_bad"])) + fix["map_bad"].tobytes()
    nkf = len(fix["kf_id"])
    b += struct.pack("<i", nkf)
    for i in range(nkf):
        w, v = row(fix["kf_bow_off"], fix["kf_bow_word"], i), row(fix["kf_bow_off"], fix["kf_bow_val"], i)
        b += struct.pack("<qii", int(fix["kf_id"][i]), int(fix["kf_map"][i]), len(w)) + w.astype("<u4").tobytes() + v.astype("<f8").tobytes()
        for off, flat in ((fix["cov_off"], fix["cov_idx"]), (fix["conn_off"], fix["conn_idx"])):
            lst = row(off, flat, i)
            b += struct.pack("<i", len(lst)) + lst.astype("<i4").tobytes()
    ops = fix["ops"].tolist()
    queries = [(j, op) for j, op in enumerate(o for o in ops if o[0] in (H.OP_RELOC, H.OP_NBEST))]
    b += struct.pack("<i", len(queries))
    for j, _ in queries:
        w, v = H.query_bow(fix, j)
        b += struct.pack("<i", len(w)) + w.astype("<u4").tobytes() + v.astype("<f8").tobytes()
    b += struct.pack("<i", len(ops))
    j = 0
    for kind, a, bb, c in ops:
        b += struct.pack("<iqii", kind, a, bb, j if kind == H.OP_RELOC else 0)      # the query's BowVector by its position among the queries
        j += kind in (H.OP_RELOC, H.OP_NBEST)
    b += struct.pack("<i", asks)
    with open(path, "wb") as f:
        f.write(b)


def read_output(path, fix):
    raw = open(path, "rb").read()
    nkf = len(fix["kf_id"])
    mem_dt = np.dtype([("rq", "<u8"), ("rw", "<i4"), ("rs", "<f4"), ("pq", "<u8"), ("pw", "<i4"), ("ps", "<f4")])
    o, out = 0, []
    while o < len(raw):
        lists = []
        for _ in range(2):
            (n,) = struct.unpack_from("<i", raw, o); o += 4
            lists.append(np.frombuffer(raw, "<i8", n, o).tolist()); o += 8 * n
        m = np.frombuffer(raw, mem_dt, nkf, o); o += mem_dt.itemsize * nkf
        out.append({"loop": lists[0], "merge": lists[1], "members": [tuple(r) for r in m.tolist()]})
    return out


def run_and_compare(exe, tmp_path, env=None):
    for name in [w.name for w in H.WORLDS]:
        fix = H.load_fixture(name)
        inp, outp = str(tmp_path / ("in_" + name)), str(tmp_path / ("out_" + name))
        write_input(inp, fix)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "kfdb_harness: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
            (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
        got = read_output(outp, fix)
        assert len(got) == len(fix["score"])
        assert H.differences(fix, got) == [], name


@pytest.mark.gpu
def test_the_adapter_replays_the_recorded_worlds_on_the_device(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    run_and_compare(build(str(tmp_path)), tmp_path)


def test_kfdb_harness_builds_and_fails_loudly_without_a_device(tmp_path):
    """Here (no GPU) creating the context throws pli::Error(PLI_ERR_NO_DEVICE) and the harness exits with 1; on the GPU box the same
    program runs.  Either way it builds and links against the product library."""
    import torch
    exe = build(str(tmp_path))
    fix = H.load_fixture(H.WORLDS[0].name)
    inp, outp = str(tmp_path / "in"), str(tmp_path / "out")
    write_input(inp, fix)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)


def test_the_adapter_on_the_mock_library_under_address_and_ub_sanitizers(tmp_path):
    """Host only: the harness, a stand-alone program with its own main, built with -fsanitize=address,undefined against
    tests/cpp/mock_pli_kfdb.cpp (the database in plain host code) and run here: the recorded worlds replay to the reference's answers, the
    two std::logic_error cases throw, and neither sanitizer reports anything."""
    exe = str(tmp_path / "kfdb_harness_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-pthread", "-I", ROOT,
                        HARNESS, os.path.join(ROOT, "tests", "cpp", "mock_pli_kfdb.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=66", UBSAN_OPTIONS="print_stacktrace=1")
    run_and_compare(exe, tmp_path, env=env)
