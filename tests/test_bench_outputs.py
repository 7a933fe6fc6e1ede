"""bench.py's plain line, its --full line and --dump-outputs.  CPU: make_images gives the pairs synth.make_stereo_pair gives, and
dump_outputs writes back exactly the records it was handed (records of the oracle's frames packed into a table of a hand-made layout).
-m gpu: a plain run prints the headline keys and nothing of --full, --full adds its legs, and two runs with the same arguments dump the
same outputs, which equal the oracle's frame."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("roofline", "lsd_rounds", "cpu_baseline", "parity", "single_pair", "host_inclusive", "large_batch")


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in os.listdir(d) if n.endswith(".npy")}


def _fields(a):
    return np.stack([a[n_].astype(np.float32) for n_ in a.dtype.names], 1)


def _check_against(out, i, t):
    """Frame i of a dump (split by its counts) against the named arrays `t` of one record."""
    c = out["counts"].astype(np.int64)
    assert np.array_equal(c[i, :4], t["counts"][:4])       # table sizes (4, 5: stereo matches, compared below by their arrays)
    lo = c[:i].sum(axis=0)
    for eye, k in ((0, "L"), (1, "R")):
        a, b = lo[eye], lo[eye] + c[i, eye]
        la, lb = lo[2 + eye], lo[2 + eye] + c[i, 2 + eye]
        assert np.array_equal(out["kp" + k][a:b], _fields(t["kp" + k]))
        assert np.array_equal(out["desc" + k][a:b], t["desc" + k].astype(np.float32))
        assert np.array_equal(out["kl" + k][la:lb], _fields(t["kl" + k]))
        assert np.array_equal(out["ldesc" + k][la:lb], t["ldesc" + k].astype(np.float32))
    a, b, la, lb = lo[0], lo[0] + c[i, 0], lo[2], lo[2] + c[i, 2]
    assert np.array_equal(out["uright"][a:b], t["uright"]) and np.array_equal(out["depth"][a:b], t["depth"])
    assert np.array_equal(out["disp"][la:lb], t["disp"]) and np.array_equal(out["le"][la:lb], t["le"])


def _oracle_record(po, cfg, L, R):
    fr = po.Frame(po.Config.from_buffer_copy(bytes(cfg)))
    t = {"counts": np.zeros(8, np.int32)}
    for eye, k, img in ((0, "L", L), (1, "R", R)):
        n, t["kp" + k], t["desc" + k] = fr.orb_extract(eye, img)
        m, t["kl" + k], t["ldesc" + k] = fr.line_extract(eye, img)
        t["counts"][eye], t["counts"][2 + eye] = n, m
    t["uright"], t["depth"], _, _ = fr.stereo_points()
    t["disp"], t["le"], _ = fr.stereo_lines()
    return t


def test_make_images_are_the_seeded_synthetic_pairs():
    bench = _bench()
    from pli_slam_amd import synth
    W, H = 188, 120
    for config, rank, world, nuniq in ((0, 0, 1, 5), (0, 1, 2, 3), (3, 1, 2, 3)):
        got = bench.make_images(SimpleNamespace(real_images=False, config=config), rank, world, nuniq, W, H)
        if config == 3:
            want = [synth.make_stereo_pair(100, W, H, t=rank * nuniq + t_) for t_ in range(nuniq)]
        else:
            want = [synth.make_stereo_pair(s_, W, H) for s_ in range(rank * nuniq, rank * nuniq + nuniq)]
        assert got.dtype == np.uint8 and np.array_equal(got, np.stack([np.stack(p) for p in want]))


def test_dump_outputs_writes_back_the_records(tmp_path, oracle, monkeypatch):
    bench = _bench()
    import torch
    from pli_slam_amd import capi
    from pli_slam_amd.frontend import Frontend
    W, H, F = 376, 240, 5
    cfg = capi.default_config(W, H, orb_nfeatures=500, lsd_nfeatures=60, max_frames=1)
    images = bench.make_images(SimpleNamespace(real_images=False, config=0), 0, 1, F, W, H)
    truth = [_oracle_record(oracle, cfg, images[f, 0], images[f, 1]) for f in range(F)]
    # a table layout of our own (64-byte aligned sections, room for 700 keypoints / 80 keylines per eye), filled with the oracle's records
    Y = capi.TableLayout()
    Y.kp_cap, Y.kl_cap = 700, 80
    end = [0]

    def take(nbytes):
        end[0] += (nbytes + 63) // 64 * 64
        return end[0] - (nbytes + 63) // 64 * 64
    Y.off_counts = take(32)
    for e in range(2):
        Y.off_kp[e], Y.off_desc[e], Y.off_kl[e], Y.off_ldesc[e] = take(24 * 700), take(32 * 700), take(68 * 80), take(32 * 80)
    Y.off_uright, Y.off_depth, Y.off_disp, Y.off_le = take(4 * 700), take(4 * 700), take(8 * 80), take(24 * 80)
    Y.record_bytes = end[0]
    table = np.zeros(F * Y.record_bytes, np.uint8)
    for f, t in enumerate(truth):
        rec = table[f * Y.record_bytes:(f + 1) * Y.record_bytes]

        def put(off, a):
            b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            rec[off:off + b.size] = b
        put(Y.off_counts, t["counts"])
        for e, k in ((0, "L"), (1, "R")):
            put(Y.off_kp[e], t["kp" + k]), put(Y.off_desc[e], t["desc" + k]), put(Y.off_kl[e], t["kl" + k]), put(Y.off_ldesc[e], t["ldesc" + k])
        put(Y.off_uright, t["uright"]), put(Y.off_depth, t["depth"]), put(Y.off_disp, t["disp"]), put(Y.off_le, t["le"])
    fe = SimpleNamespace(layout=Y)
    fe.parse_record = lambda tab, i: Frontend.parse_record(fe, tab, i)
    for cap in (64, 3):                  # every frame, then a seeded sample of 3 of the 5
        monkeypatch.setattr(bench, "DUMP_FRAMES", cap)
        d = str(tmp_path / ("cap%d" % cap))
        bench.dump_outputs(fe, torch.from_numpy(table), F, None, 0, d)
        out = _load(d)
        assert all(a.dtype in (np.float32, np.float64) for a in out.values())
        frames = out["frames"].astype(np.int64)
        assert len(frames) == min(F, cap) and np.all(np.diff(frames) > 0) and frames.max() < F
        for i, f in enumerate(frames):
            _check_against(out, i, truth[f])
    assert sum(c[0] for c in (t["counts"] for t in truth)) > 0


def run_bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", *args], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_line_and_its_dump_repeat_and_equal_the_oracle(tmp_path, oracle):
    from pli_slam_amd import capi, synth
    runs = []
    for r in range(2):
        d = str(tmp_path / ("run%d" % r))
        line = run_bench("--steps", "3", "--warmup", "1", "--frames-per-gpu", "8", "--dump-outputs", d)
        for k in HEADLINE:
            assert k in line, k
        assert not any(k in line for k in FULL_ONLY), sorted(line)
        assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(8 * 1e3 / line["ms_per_step"])
        runs.append(_load(d))
    a, b = runs
    assert sorted(a) == sorted(b) and all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.array_equal(a["frames"], np.arange(8))
    cfg = capi.default_config(752, 480, orb_nfeatures=1200, lsd_nfeatures=100, max_frames=8)      # as bench.py configures it
    L, R = synth.make_stereo_pair(5, 752, 480)
    _check_against(a, 5, _oracle_record(oracle, cfg, L, R))


@pytest.mark.gpu
def test_plain_config3_dump_carries_the_track(tmp_path):
    d = str(tmp_path / "c3")
    line = run_bench("--config", "3", "--frames-per-gpu", "4", "--steps", "1", "--warmup", "1", "--dump-outputs", d)
    assert line["steps"] == 1 and "roofline" not in line
    out = _load(d)
    tc = out["track_counts"].astype(np.int64)
    assert tc.shape == (4, 4) and len(out["track_best"]) == tc[:, 0].sum() and len(out["track_lines"]) == tc[:, 2].sum()
    assert (out["track_best"] >= 0).sum() > 0


@pytest.mark.gpu
def test_full_line_adds_profile_parity_and_legs():
    line = run_bench("--steps", "2", "--warmup", "1", "--frames-per-gpu", "8", "--full", "--cpu-baseline-seconds", "2", "--no-large-batch-leg")
    for k in HEADLINE + ("roofline", "lsd_rounds", "cpu_baseline", "parity", "single_pair", "host_inclusive"):
        assert k in line, k
    assert line["parity"]["ok"] is True and line["value"] > 0
    rf = line["roofline"]
    assert rf["kernel"] and rf["kernel_ms_per_step"] and rf["kernel_launches_per_step"] > 0
