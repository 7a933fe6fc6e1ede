"""Yardsticks and inputs for pli_distinctive_descriptors (MapPoint / MapLine::ComputeDistinctiveDescriptors).

restated_point / restated_line follow the reference's statements one by one (MapPoint.cc:330-359, MapLine.cc:278-312); independent is
the definition alone, written another way.  All three return (BestIdx, BestMedian, [median_i]) as exact integers for a group of
N >= 1 descriptors, an (N, 32) uint8 array in the order of the reference's vDescriptors.

The two restatements take `mut`, a set of deliberate misreadings that tests/test_ref_pin_map.py wants the fixtures of the reference's
own compiled code to reject (MUTANTS): "median_half" takes the median at index N / 2, "pick_le" lets a later row with an equal
median win (<= in the pick).
"""
import numpy as np

INT_MAX = 2147483647
MUTANTS = ("median_half", "pick_le")
POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int32)


def descriptor_distance(a, b):
    """ORBmatcher::DescriptorDistance / cv::norm(a, b, NORM_HAMMING) of two 32-byte rows: the number of differing bits."""
    return int(POPCOUNT[a ^ b].sum())


def restated_point(group, mut=()):
    group = np.asarray(group, np.uint8).reshape(-1, 32)
    N = len(group)                                                        # const size_t N = vDescriptors.size();
    Distances = [[np.float32(0)] * N for _ in range(N)]                   # float Distances[N][N];
    for i in range(N):
        Distances[i][i] = np.float32(0)
        for j in range(i + 1, N):
            distij = descriptor_distance(group[i], group[j])
            Distances[i][j] = np.float32(distij)
            Distances[j][i] = np.float32(distij)
    BestMedian = INT_MAX
    BestIdx = 0
    medians = []
    for i in range(N):
        vDists = [int(v) for v in Distances[i]]                           # vector<int> vDists(Distances[i], Distances[i] + N);
        vDists = sorted(vDists)
        median = vDists[N // 2 if "median_half" in mut else int(0.5 * (N - 1))]
        medians.append(median)
        if (median <= BestMedian) if "pick_le" in mut else (median < BestMedian):
            BestMedian = median
            BestIdx = i
    return BestIdx, BestMedian, medians


def restated_line(group, mut=()):
    group = np.asarray(group, np.uint8).reshape(-1, 32)
    NL = len(group)
    Distances = [[np.float32(0)] * NL for _ in range(NL)]                 # Distances.resize(NL, vector<float>(NL, 0));
    for i in range(NL):
        Distances[i][i] = np.float32(0)
        for j in range(NL):                                               # j from 0: every pair twice, the diagonal recomputed
            distij = descriptor_distance(group[i], group[j])
            Distances[i][j] = np.float32(distij)
            Distances[j][i] = np.float32(distij)
    BestMedian = INT_MAX
    BestIdx = 0
    medians = []
    for i in range(NL):
        vDists = sorted(int(v) for v in Distances[i])
        median = vDists[NL // 2 if "median_half" in mut else int(0.5 * (NL - 1))]
        medians.append(median)
        if (median <= BestMedian) if "pick_le" in mut else (median < BestMedian):
            BestMedian = median
            BestIdx = i
    return BestIdx, BestMedian, medians


def independent(group):
    """The definition: the lower median of every row of the Hamming matrix, then the lexicographic minimum of (median, i)."""
    group = np.asarray(group, np.uint8).reshape(-1, 32)
    n = len(group)
    med = np.empty(n, np.int64)
    for lo in range(0, n, 256):                                           # (row blocks: the table lookup of 2048 x 2048 x 32 at once is 128 MiB)
        d = POPCOUNT[group[lo:lo + 256, None, :] ^ group[None, :, :]].sum(axis=2)
        med[lo:lo + 256] = np.partition(d, (n - 1) // 2, axis=1)[:, (n - 1) // 2]
    m, i = min((int(m), i) for i, m in enumerate(med))
    return i, m, [int(v) for v in med]


def expected(groups, fn=independent):
    """(best, best_median, row_median) of a whole call as the entry point returns them: -1 / INT32_MAX for an empty group."""
    best, bm, rows = [], [], []
    for g in groups:
        if len(g) == 0:
            best.append(-1); bm.append(INT_MAX)
            continue
        b, m, r = fn(g)
        best.append(b); bm.append(m); rows += r
    return np.array(best, np.int32), np.array(bm, np.int32), np.array(rows, np.int32)


# ---- inputs ----
def flip_bits(rng, desc, rate):
    mask = np.packbits(rng.random(256) < rate)
    return desc ^ mask


def track(rng, n, flip):
    """One feature's track: a base descriptor seen n times, every observation with its own bit-flip rate flip * U(0.3, 1.5)."""
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    return np.stack([flip_bits(rng, base, flip * rng.uniform(0.3, 1.5)) for _ in range(n)]) if n else np.zeros((0, 32), np.uint8)


def with_bits(*bits):
    d = np.zeros(32, np.uint8)
    for b in bits:
        d[b >> 3] |= 1 << (b & 7)
    return d


def first_bits(k):
    return with_bits(*range(k))


def complement_pairs(n):
    """A descriptor and its complement, repeated to n rows."""
    a = np.arange(32, dtype=np.uint8) * 7 + 3
    return np.stack([a if i % 2 == 0 else ~a for i in range(n)])


# name -> (group, (BestIdx, BestMedian, medians) worked out by hand)
def hand_groups():
    a = np.arange(32, dtype=np.uint8)
    out = {}
    out["one"] = (a[None], (0, 0, [0]))
    out["two"] = (np.stack([a, ~a]), (0, 0, [0, 0]))                     # the median index of N = 2 is 0: the diagonal's zero
    # weights 0, 3, 8 on nested bit sets: D = [[0 3 8] [3 0 5] [8 5 0]], the medians (index 1 of 3) are 3, 3, 5
    out["three"] = (np.stack([first_bits(0), first_bits(3), first_bits(8)]), (0, 3, [3, 3, 5]))
    # a, ~a, ~a: row 0 = [0 256 256] -> 256; rows 1, 2 = [256 0 0] -> 0
    out["complement"] = (np.stack([a, ~a, ~a]), (1, 0, [256, 0, 0]))
    # a and its complement alone in three rows a, ~a, a: row 1 = [256 0 256] -> 256
    out["complement_median"] = (np.stack([a, ~a, a]), (0, 0, [0, 256, 0]))
    out["identical"] = (np.stack([a] * 7), (0, 0, [0] * 7))
    # weights 20, 2, 4, 3 on nested bit sets (N = 4, median index 1: the nearest other row):
    # row 0 -> 16 (to row 2), row 1 -> 1 (to row 3), row 2 -> 1 (to row 3), row 3 -> 1: rows 1, 2, 3 tie, the earliest wins, row 0 loses
    out["tie"] = (np.stack([first_bits(20), first_bits(2), first_bits(4), first_bits(3)]), (1, 1, [16, 1, 1, 1]))
    return out
