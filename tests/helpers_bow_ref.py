"""Corpus of the bag-of-words pin (tests/test_ref_pin_bow.py, tests/test_ref_pin_bow_gpu.py).

Every case is a vocabulary tree and a feature set, both generated from seeds.  tests/golden/bow_ref/<name>.npz holds the tree
arrays, the features and what the reference's own DBoW2 answered for them (oracle/_ref/pli_ref_bow, built by oracle/Makefile from
the reference tree): per levelsup the per-feature rows (word id, weight, node id) of the protected
TemplatedVocabulary::transform(feature, id, weight, &nid, levelsup), and the BowVector and FeatureVector of
transform(features, BowVector, FeatureVector, levelsup) where they are determinate.

The node id is not always written by the reference: the set-level transform declares `NodeId nid;` uninitialised
(TemplatedVocabulary.h:1163) and the descent stores it only for nid_level <= 0 (:1239) or at level L - levelsup (:1263).  The driver
presets 0xFFFFFFFF (UNSET), the fixtures keep it, and the set-level maps are recorded only for a (case, levelsup) without one.

The vocabulary goes to the reference as a text file in ORBvoc.txt form WITHOUT a final newline: loadFromTextFile reads
`while(!f.eof())` (:1390), so a trailing newline makes it parse one more, empty, line into a phantom node.

`Tree.rows` is a plain numpy descent used to classify features (ties, unset node ids) and to carry the mutants of the CPU test; it
follows the reference's walk loop (:1244-1266), one child at a time with a strict `<`.
"""
import collections
import os
import struct
import subprocess
import tempfile

import numpy as np

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bow_ref")
UNSET = 0xFFFFFFFF
KIND_NODE, KIND_PERTURBED, KIND_RANDOM, KIND_TIE = 0, 1, 2, 3

# single_child: inner nodes (by position among the inner nodes of their level) that keep only their first child
Case = collections.namedtuple("Case", "name k L seed ragged stop_fraction single_child")

CASES = [
    Case("ragged_k10_L4_s1", 10, 4, 1, True, 0.05, ()),
    Case("complete_k10_L3_s2", 10, 3, 2, False, 0.05, ()),
    Case("ragged_k3_L6_s3", 3, 6, 3, True, 0.05, ()),
    Case("complete_k20_L2_s4", 20, 2, 4, False, 0.05, ()),
    Case("stopped_k6_L3_s5", 6, 3, 5, True, 0.3, ((1, 1), (2, 3))),      # (level, position among that level's inner nodes)
    Case("flat_k12_L1_s6", 12, 1, 6, False, 0.05, ()),
]
CASE_BY_NAME = {c.name: c for c in CASES}
RAGGED = [c.name for c in CASES if c.ragged and not c.single_child]


def levelsups(L):
    """4, 1, 0, 9 and L itself, each once."""
    out = []
    for ls in (4, 1, 0, 9, L):
        if ls not in out:
            out.append(ls)
    return out


_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.int64)


def hamming(a, b):
    """Hamming distance of 32-byte rows (broadcasting)."""
    return _POP[np.bitwise_xor(a, b)].sum(axis=-1)


# ------------------------------------------------------------------------------------------------------------ vocabularies
def _levels(parent):
    lvl = np.zeros(len(parent) + 1, np.int64)
    for i, p in enumerate(parent):
        lvl[i + 1] = lvl[p] + 1
    return lvl


def _keep_first_child(arrays, picks):
    """Removes every child but the first (with its subtree) of the picked inner nodes; node order is kept."""
    k, L, parent, is_leaf, desc, weight = arrays
    lvl = _levels(parent)
    inner = {}
    for i in range(len(parent)):
        if not is_leaf[i]:
            inner.setdefault(int(lvl[i + 1]), []).append(i + 1)
    only = {inner[level][pos] for level, pos in picks}
    removed = np.zeros(len(parent) + 1, bool)
    seen = set()
    for i, p in enumerate(parent):
        if removed[p] or (p in only and p in seen):
            removed[i + 1] = True
        seen.add(int(p))
    keep = ~removed[1:]
    newid = np.cumsum(~removed) - 1                                       # root stays 0
    return (k, L, newid[parent[keep]].astype(np.int32), is_leaf[keep].copy(), desc[keep].copy(), weight[keep].copy())


def make_vocabulary(case):
    from pli_slam_amd import synth
    arrays = synth.make_vocabulary(case.k, case.L, case.seed, case.ragged, case.stop_fraction)
    if case.single_child:
        arrays = _keep_first_child(arrays, case.single_child)
    return arrays


def vocabulary_text(k, L, parent, is_leaf, desc, weight, final_newline=False):
    """ORBvoc.txt form: 'k L scoring weighting' (L1_NORM = 0, TF_IDF = 0), then 'parent is_leaf 32 bytes weight' per node."""
    lines = ["%d %d 0 0" % (k, L)]
    for i in range(len(parent)):
        lines.append("%d %d %s %s" % (parent[i], is_leaf[i], " ".join(str(int(b)) for b in desc[i]), repr(float(weight[i]))))
    return "\n".join(lines) + ("\n" if final_newline else "")


class Tree:
    """The plain numpy statement of the descent.  Mutants: tie='last' (the last of equally near children wins),
    word_order='node' (word id = node id), nid_shift=1 in rows() (node id taken one level too deep)."""

    def __init__(self, k, L, parent, is_leaf, desc, weight, tie="first", word_order="leaf"):
        n = len(parent)
        self.k, self.L, self.tie = int(k), int(L), tie
        self.desc = np.vstack([np.zeros((1, 32), np.uint8), np.asarray(desc, np.uint8)])
        self.weight = np.concatenate([[0.0], np.asarray(weight, np.float64)])
        ch = [[] for _ in range(n + 1)]
        for i, p in enumerate(parent):
            ch[int(p)].append(i + 1)                                      # children in file order (:1404)
        self.children = [np.array(c, np.int64) for c in ch]
        self.level = _levels(parent)
        self.word = np.full(n + 1, -1, np.int64)
        leaves = np.flatnonzero(np.asarray(is_leaf) > 0) + 1
        self.word[leaves] = np.arange(len(leaves)) if word_order == "leaf" else leaves   # word ids in file order (:1420-1427)
        self.nwords = len(leaves)

    def walk(self, f, start=0):
        """[(node chosen, positions of the children at the minimum distance)] per level below `start`."""
        out, cur = [], start
        while len(self.children[cur]):
            ch = self.children[cur]
            d = hamming(self.desc[ch], f)
            best, best_d = 0, d[0]
            for j in range(1, len(ch)):                                   # :1252-1261
                if d[j] < best_d or (self.tie == "last" and d[j] == best_d):
                    best, best_d = j, d[j]
            cur = int(ch[best])
            out.append((cur, np.flatnonzero(d == d.min())))
        return out

    def leaf_of(self, f, start):
        w = self.walk(f, start)
        return w[-1][0] if w else start

    def classify(self, f):
        """(path of node ids, levels (1-based) at which two or more children tie at the minimum and the first and the last of
        them lead to different words)."""
        cur, path, ties = 0, [], []
        for node, mins in self.walk(f):
            if len(mins) >= 2:
                ch = self.children[cur]
                if self.word[self.leaf_of(f, int(ch[mins[0]]))] != self.word[self.leaf_of(f, int(ch[mins[-1]]))]:
                    ties.append(len(path) + 1)
            path.append(node)
            cur = node
        return path, ties

    def rows(self, feat, levelsup, nid_shift=0):
        """(word uint32, weight float64, node uint32 with UNSET where the reference's descent never stores one)."""
        n = len(feat)
        word, weight, node = np.zeros(n, np.uint32), np.zeros(n, np.float64), np.full(n, UNSET, np.uint32)
        nid_level = self.L - levelsup
        for i in range(n):
            path = [p for p, _ in self.walk(feat[i])]
            word[i], weight[i] = self.word[path[-1]], self.weight[path[-1]]
            if nid_level <= 0:
                node[i] = 0                                               # :1239
            elif nid_level + nid_shift <= len(path):
                node[i] = path[nid_level + nid_shift - 1]                 # :1263
        return word, weight, node


def set_level(word, weight, node, norm_order="word", keep_stopped=False):
    """transform(features, BowVector, FeatureVector, levelsup) (:1157-1205) from per-feature rows: addWeight in feature order,
    L1 norm in word order.  -> (bow words uint32, bow values float64, fv nodes uint32, fv feature indices uint32), the maps in
    key order.  Mutants: norm_order='feature' (the norm summed feature by feature), keep_stopped (a stopped word's feature stays
    in the FeatureVector)."""
    bow, fv = {}, {}
    for i, (w, v, nd) in enumerate(zip(word.tolist(), weight.tolist(), node.tolist())):
        if v > 0:
            bow[w] = bow[w] + v if w in bow else v
        if v > 0 or keep_stopped:
            fv.setdefault(nd, []).append(i)
    norm = 0.0
    if norm_order == "word":
        for w in sorted(bow):
            norm += abs(bow[w])
    else:
        for v in weight.tolist():
            if v > 0:
                norm += abs(v)
    words = sorted(bow)
    vals = [bow[w] / norm if norm > 0.0 else bow[w] for w in words]
    fn = [nd for nd in sorted(fv) for _ in fv[nd]]
    fi = [i for nd in sorted(fv) for i in fv[nd]]
    return np.array(words, np.uint32), np.array(vals, np.float64), np.array(fn, np.uint32), np.array(fi, np.uint32)


# ---------------------------------------------------------------------------------------------------------------- features
def tie_feature(a, b, rng):
    """Sibling a with half of the bits flipped in which a and b differ: equidistant from both.  None for an odd count."""
    diff = np.flatnonzero(np.unpackbits(np.bitwise_xor(a, b)))
    if len(diff) % 2:
        return None
    bits = np.unpackbits(a)
    flip = rng.choice(diff, len(diff) // 2, replace=False) if len(diff) else diff
    bits[flip] ^= 1
    return np.packbits(bits)


def make_features(case, arrays):
    """(features (n, 32) uint8, kind (n,) uint8)."""
    k, L, parent, is_leaf, desc, weight = arrays
    rng = np.random.default_rng(1000 + case.seed)
    tree = Tree(*arrays)
    n = len(parent)
    lvl = tree.level[1:]
    feats, kinds = [], []
    # node descriptors themselves: every word that ends above the last level (its node id is never stored at levelsup 0, and
    # above level L - 1 not at levelsup 1 either), then any node
    leaf_lvl = np.where(np.asarray(is_leaf) > 0, lvl, L)
    shallow, mid = np.flatnonzero(leaf_lvl <= L - 2), np.flatnonzero(leaf_lvl == L - 1)
    nodes = np.concatenate([shallow[:40], mid[:60], rng.choice(n, min(n, 160), replace=False)]).astype(np.int64)
    feats.append(desc[nodes]); kinds += [KIND_NODE] * len(nodes)
    # ... with one byte perturbed: such words again, several times each (a ragged tree has few of them), then any node
    again = [np.resize(g, m) for g, m in ((shallow, 90), (mid, 90)) if len(g)]
    pert = desc[np.concatenate(again + [rng.choice(n, min(n, 160), replace=False)]).astype(np.int64)].copy()
    pert[np.arange(len(pert)), rng.integers(0, 32, len(pert))] ^= rng.integers(1, 256, len(pert)).astype(np.uint8)
    feats.append(pert); kinds += [KIND_PERTURBED] * len(pert)
    # uniform random bytes
    feats.append(rng.integers(0, 256, (200, 32), dtype=np.uint8)); kinds += [KIND_RANDOM] * 200
    # constructed ties between sibling pairs, at every level
    ties = []
    per_level = max(40, 240 // L)
    for level in range(1, L + 1):
        parents = [p for p in range(n + 1) if tree.level[p] == level - 1 and len(tree.children[p]) >= 2]
        got = tries = 0
        while parents and got < per_level and tries < 40 * per_level:
            tries += 1
            ch = tree.children[parents[int(rng.integers(0, len(parents)))]]
            ia, ib = sorted(rng.choice(len(ch), 2, replace=False).tolist())
            f = tie_feature(tree.desc[ch[ia]], tree.desc[ch[ib]], rng)
            if f is None:
                continue
            d = hamming(tree.desc[ch], f)
            if d[ia] == d[ib] == d.min() and (d == d.min()).sum() == 2:   # nearer to the pair than to the other siblings
                ties.append(f)
                got += 1
    if ties:
        feats.append(np.stack(ties)); kinds += [KIND_TIE] * len(ties)
    return np.ascontiguousarray(np.vstack(feats), np.uint8), np.array(kinds, np.uint8)


# -------------------------------------------------------------------------------------------- the reference's own program
def run_reference(exe, text, feat, levelsup):
    """One run of oracle/_ref/pli_ref_bow as a child process -> {"nwords", "word", "weight", "node", "determinate", and when
    determinate "bow_word", "bow_val", "fv_node", "fv_index" (the FeatureVector as (node, feature index) pairs in map order)}."""
    feat = np.ascontiguousarray(feat, np.uint8)
    n = len(feat)
    with tempfile.TemporaryDirectory() as d:
        voc, req, rsp = os.path.join(d, "voc.txt"), os.path.join(d, "request"), os.path.join(d, "response")
        with open(voc, "w", newline="") as f:
            f.write(text)
        path = voc.encode()
        with open(req, "wb") as f:
            f.write(struct.pack("<i", len(path)) + path + struct.pack("<ii", levelsup, n) + feat.tobytes())
        subprocess.run([exe, req, rsp], check=True, timeout=120)
        raw = open(rsp, "rb").read()
    nwords, n2, det = struct.unpack_from("<iii", raw, 0)
    assert n2 == n
    o = 12
    out = {"nwords": nwords, "determinate": bool(det)}
    out["word"] = np.frombuffer(raw, "<u4", n, o).copy(); o += 4 * n
    out["weight"] = np.frombuffer(raw, "<f8", n, o).copy(); o += 8 * n
    out["node"] = np.frombuffer(raw, "<u4", n, o).copy(); o += 4 * n
    if det:
        (nb,) = struct.unpack_from("<i", raw, o); o += 4
        bow = np.frombuffer(raw, np.dtype([("w", "<u4"), ("v", "<f8")]), nb, o); o += 12 * nb
        out["bow_word"], out["bow_val"] = bow["w"].copy(), bow["v"].copy()
        (nf,) = struct.unpack_from("<i", raw, o); o += 4
        fn, fi = [], []
        for _ in range(nf):
            nd, cnt = struct.unpack_from("<Ii", raw, o); o += 8
            fi.append(np.frombuffer(raw, "<u4", cnt, o)); o += 4 * cnt
            fn.append(np.full(cnt, nd, np.uint32))
        out["fv_node"] = np.concatenate(fn) if fn else np.zeros(0, np.uint32)
        out["fv_index"] = np.concatenate(fi).astype(np.uint32) if fi else np.zeros(0, np.uint32)
    assert o == len(raw)
    return out


ROW_KEYS = ("word", "weight", "node")
MAP_KEYS = ("bow_word", "bow_val", "fv_node", "fv_index")


def generate(exe, case):
    """The fixture's arrays {name: array}, from the seeds and the reference's program."""
    arrays = make_vocabulary(case)
    k, L, parent, is_leaf, desc, weight = arrays
    feat, kind = make_features(case, arrays)
    text = vocabulary_text(*arrays)
    out = {"k": np.int32(k), "L": np.int32(L), "parent": parent, "is_leaf": is_leaf, "desc": desc, "weight": weight,
           "feat": feat, "kind": kind, "levelsups": np.array(levelsups(L), np.int32)}
    for ls in levelsups(L):
        r = run_reference(exe, text, feat, ls)
        out["nwords"] = np.int32(r["nwords"])
        out["det_%d" % ls] = np.uint8(r["determinate"])
        for key in ROW_KEYS + (MAP_KEYS if r["determinate"] else ()):
            out["%s_%d" % (key, ls)] = r[key]
    return out


def fixture_path(name):
    return os.path.join(GOLD_DIR, name + ".npz")


def save_fixture(name, arrays):
    os.makedirs(GOLD_DIR, exist_ok=True)
    np.savez_compressed(fixture_path(name), **arrays)


_loaded = {}


def load_fixture(name):
    """{name: array} as generate() returns it; loaded once, read-only."""
    if name not in _loaded:
        z = np.load(fixture_path(name))
        d = {}
        for key in z.files:
            d[key] = z[key]
            d[key].setflags(write=False)
        _loaded[name] = d
    return _loaded[name]


def vocabulary_of(fix):
    return int(fix["k"]), int(fix["L"]), fix["parent"], fix["is_leaf"], fix["desc"], fix["weight"]


def expected_device_node(fix, ls):
    """The reference's node ids as int32, with this project's rule where the reference wrote none: 0."""
    node = fix["node_%d" % ls]
    return np.where(node == UNSET, 0, node).astype(np.int32)


# ----------------------------------------------------------------------------------------------------------------- checks
def check_rows(fix, ls, word, weight, node):
    """None when (word, weight, node) equal the reference's rows for levelsup `ls` (word id, weight bits, node id wherever the
    reference wrote one, 0 wherever it did not), else what differs."""
    rnode = fix["node_%d" % ls]
    if not np.array_equal(np.asarray(word).astype(np.int64), fix["word_%d" % ls].astype(np.int64)):
        return "word id"
    if np.asarray(weight, np.float64).tobytes() != fix["weight_%d" % ls].tobytes():
        return "weight bits"
    node = np.asarray(node).astype(np.int64)
    if not np.array_equal(node[rnode != UNSET], rnode[rnode != UNSET].astype(np.int64)):
        return "node id"
    if np.any(node[rnode == UNSET] != 0):
        return "node id where the reference writes none"
    return None


def check_maps(fix, ls, bow_word, bow_val, fv_node, fv_index):
    """None when the BowVector and the FeatureVector equal the recorded ones byte for byte, else what differs."""
    got = {"bow_word": np.asarray(bow_word, np.uint32), "bow_val": np.asarray(bow_val, np.float64),
           "fv_node": np.asarray(fv_node, np.uint32), "fv_index": np.asarray(fv_index, np.uint32)}
    for key in MAP_KEYS:
        if got[key].tobytes() != fix["%s_%d" % (key, ls)].tobytes():
            return key
    return None
