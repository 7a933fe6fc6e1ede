"""Corpus, fixtures and plain Python restatement of the keyframe database's place-recognition queries
(tests/test_kfdb_cpu.py, tests/test_kfdb_gpu.py, tests/test_cpp_kfdb.py).

A fixture tests/golden/kfdb_ref/<name>.npz is a "world": a vocabulary (synth.make_vocabulary), 40-odd keyframes in two maps with
covisibility lists and connected sets, an operation list (add in an order that is not the id order, erase, clearMap, clear, and the
two queries, all in sequence on ONE database) and what the REFERENCE's own code answered: tools/gen_kfdb_ref.py compiles the
reference's src/KeyFrameDatabase.cc and Thirdparty/DBoW2 where they lie (tools/pin/kfdb/), replays the world and records
  * every keyframe's and every query's BowVector (the reference's transform),
  * per (query, keyframe of the world): the shared words and vocabulary.score(query, keyframe) as the double and as the float the
    database stores,
  * per query: the returned candidates in order and the six members of every keyframe after the call.

Features are node descriptors of the vocabulary (stored as node indices), chosen by word with the descent of
tests/helpers_bow_ref.py, which is pinned to the reference's.

The restatement is written the way the adapter works (pli_slam_amd/adapters/orbslam_keyframe_database.hpp): from the per-slot answers
of one pli_kfdb_query call (common, first, score) and the add sequence of the slots it rebuilds lKFsSharingWords and then replays the
reference's statements on the keyframes' members.  `mut` names ONE deliberate deviation (MUTANTS); each must show in the fixtures.
"""
import collections
import os
import struct

import numpy as np

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kfdb_ref")
LEVELSUP = 4
# Times a keyframe sees a word.  Swapping the score's two arguments changes a term only where one value is more than three times
# the other (otherwise fabs(vi - wi) - fabs(vi) and fabs(vi - wi) - fabs(wi) are both exact), and the change survives the sum only
# where the sum stays small beside that value: a few words seen very often, the rest once or twice.
REPEATS = (1, 1, 2, 40)
OP_ADD, OP_ERASE, OP_RELOC, OP_NBEST, OP_CLEAR_MAP, OP_CLEAR = range(6)
MUTANTS = ("descending_sum", "swapped_arguments", "float_accumulator", "ge_at_min_common_words", "fresh_scores", "slot_order",
           "connected_in_maximum", "map_filter_before_gate", "unstable_sort")

World = collections.namedtuple("World", "name seed bad_merge_map")
WORLDS = [World("world_a_s11", 11, False), World("world_b_s12", 12, True)]
WORLD_BY_NAME = {w.name: w for w in WORLDS}


# ------------------------------------------------------------------------------------------------------------------ score
def shared_words(qw, kw):
    """(indices in the query, indices in the keyframe) of the shared words, ascending."""
    _, iq, ik = np.intersect1d(np.asarray(qw, np.uint32), np.asarray(kw, np.uint32), assume_unique=True, return_indices=True)
    return iq, ik


def score(qw, qv, kw, kv, mut=None):
    """L1Scoring::score(query, keyframe) (ScoringObject.cpp:23-68) as its double: the sum in ascending word order of
    fabs(vi - wi) - fabs(vi) - fabs(wi), vi the query's value, evaluated left to right; then -sum / 2.0."""
    iq, ik = shared_words(qw, kw)
    pairs = list(zip(np.asarray(qv, np.float64)[iq].tolist(), np.asarray(kv, np.float64)[ik].tolist()))
    if mut == "descending_sum":
        pairs.reverse()
    acc = np.float32(0) if mut == "float_accumulator" else 0.0
    for vi, wi in pairs:
        if mut == "swapped_arguments":
            vi, wi = wi, vi
        term = abs(vi - wi) - abs(vi) - abs(wi)
        acc = np.float32(acc + np.float32(term)) if mut == "float_accumulator" else acc + term
    return -float(acc) / 2.0


def answers(qw, qv, slots, mut=None):
    """What pli_kfdb_query answers: slots = per slot (words, values) or None for a free one ->
    (common int32, first int32, score float64); a free slot and an empty keyframe give 0, -1, -0.0."""
    n = len(slots)
    common, first, sc = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.full(n, -0.0, np.float64)
    for s, kf in enumerate(slots):
        if kf is None:
            continue
        iq, _ = shared_words(qw, kf[0])
        common[s] = len(iq)
        if len(iq):
            first[s] = iq[0]
        sc[s] = score(qw, qv, kf[0], kf[1], mut)
    return common, first, sc


# ----------------------------------------------------------------------------------------------------- the two functions
class Map:
    def __init__(self, index, bad):
        self.index, self.bad = index, bool(bad)


class KeyFrame:
    """The members KeyFrameDatabase.cc touches, with KeyFrame.cc's initial values."""

    def __init__(self, index, mn_id, kmap, words, values):
        self.index, self.mnId, self.map = index, int(mn_id), kmap
        self.words, self.values = np.asarray(words, np.uint32), np.asarray(values, np.float64)
        self.cov, self.conn, self.bad = [], set(), False
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = 0, 0, np.float32(0)
        self.mnPlaceRecognitionQuery, self.mnPlaceRecognitionWords, self.mPlaceRecognitionScore = 0, 0, np.float32(0)

    def members(self):
        return (self.mnRelocQuery, self.mnRelocWords, np.float32(self.mRelocScore), self.mnPlaceRecognitionQuery,
                self.mnPlaceRecognitionWords, np.float32(self.mPlaceRecognitionScore))


class BadKeyFrame(Exception):
    """The reference loops for ever on a bad keyframe in the sorted list (KeyFrameDatabase.cc:929); the adapter throws."""


class Database:
    """slot -> keyframe with an add sequence number per slot, as the adapter keeps them; the device side is `answers`."""

    def __init__(self, answers_fn=None):
        self.slot_kf, self.slot_seq, self.next_seq = [], [], 0
        self.answers_fn = answers_fn              # (qw, qv) -> (common, first, score) of the device; None: the restatement

    def add(self, kf):
        if kf in self.slot_kf:
            raise ValueError("the keyframe is already in the database")
        free = [s for s, k in enumerate(self.slot_kf) if k is None]
        s = free[0] if free else len(self.slot_kf)       # the smallest free slot, as pli_kfdb_add hands them out
        if s == len(self.slot_kf):
            self.slot_kf.append(None); self.slot_seq.append(0)
        self.slot_kf[s], self.slot_seq[s] = kf, self.next_seq
        self.next_seq += 1
        return s

    def erase(self, kf):
        if kf in self.slot_kf:
            s = self.slot_kf.index(kf)
            self.slot_kf[s] = None
            return s
        return -1

    def clear(self):
        self.slot_kf, self.slot_seq = [], []

    def clear_map(self, kmap):
        return [self.erase(kf) for kf in list(self.slot_kf) if kf is not None and kf.map is kmap]

    def slots(self):
        return [None if kf is None else (kf.words, kf.values) for kf in self.slot_kf]

    def _query(self, qw, qv, mut):
        if self.answers_fn is not None:
            return self.answers_fn(qw, qv)
        return answers(qw, qv, self.slots(), mut if mut in ("descending_sum", "swapped_arguments", "float_accumulator") else None)

    def _sharing(self, common, first, mut):
        live = [s for s, kf in enumerate(self.slot_kf) if kf is not None and common[s] > 0]
        return sorted(live) if mut == "slot_order" else sorted(live, key=lambda s: (first[s], self.slot_seq[s]))

    def detect_relocalization_candidates(self, f_id, qw, qv, kmap, mut=None, events=None):
        """KeyFrameDatabase::DetectRelocalizationCandidates (:977-1089) -> the candidates in order."""
        common, first, sc = self._query(qw, qv, mut)
        sharing = []
        for s in self._sharing(common, first, mut):
            kf = self.slot_kf[s]
            if kf.mnRelocQuery != f_id:
                kf.mnRelocWords = 0
                kf.mnRelocQuery = f_id
                sharing.append((kf, s))
            kf.mnRelocWords += int(common[s])
        if not sharing:
            return []
        max_common = max([0] + [kf.mnRelocWords for kf, _ in sharing])
        min_common = int(np.float32(max_common) * np.float32(0.8))
        scored = []
        for kf, s in sharing:
            if kf.mnRelocWords > min_common or (mut == "ge_at_min_common_words" and kf.mnRelocWords == min_common):
                si = np.float32(sc[s])
                kf.mRelocScore = si
                scored.append((si, kf))
        if not scored:
            return []
        fresh = {kf: si for si, kf in scored}
        acc_list, best_acc = [], np.float32(0)
        for si, kf in scored:
            best, acc, best_kf = si, si, kf
            for kf2 in kf.cov[:10]:
                if kf2.mnRelocQuery != f_id:
                    continue
                s2 = kf2.mRelocScore
                if mut == "fresh_scores":
                    s2 = fresh.get(kf2, np.float32(0))
                elif events is not None and kf2 not in fresh and s2 != 0:
                    events["stale"] += 1
                acc = np.float32(acc + s2)
                if s2 > best:
                    best_kf, best = kf2, s2
                    if events is not None:
                        events["neighbour_best"] += 1
            acc_list.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        if mut == "map_filter_before_gate":                      # the gate taken over the keyframes of the map only
            acc_list = [(acc, kf) for acc, kf in acc_list if kf.map is kmap]
            best_acc = max([np.float32(0)] + [acc for acc, _ in acc_list])
        retain = np.float32(np.float32(0.75) * best_acc)
        out, seen = [], set()
        for acc, kf in acc_list:
            if acc > retain:
                if kf.map is not kmap:
                    continue
                if kf not in seen:
                    out.append(kf); seen.add(kf)
                elif events is not None:
                    events["duplicate"] += 1
        return out

    def detect_n_best_candidates(self, pkf, n_num, mut=None, events=None):
        """KeyFrameDatabase::DetectNBestCandidates (:806-974) -> (vpLoopCand, vpMergeCand)."""
        common, first, sc = self._query(pkf.words, pkf.values, mut)
        qid = pkf.mnId
        sharing, connected_words = [], []
        for s in self._sharing(common, first, mut):
            kf = self.slot_kf[s]
            if kf.mnPlaceRecognitionQuery != qid:
                if kf in pkf.conn:
                    kf.mnPlaceRecognitionWords = 1            # reset at every shared word, then ++
                    connected_words.append(int(common[s]))
                    continue
                kf.mnPlaceRecognitionWords = 0
                kf.mnPlaceRecognitionQuery = qid
                sharing.append((kf, s))
            kf.mnPlaceRecognitionWords += int(common[s])
        if not sharing:
            return [], []
        max_common = max([0] + [kf.mnPlaceRecognitionWords for kf, _ in sharing])
        if events is not None and connected_words and max(connected_words) > max_common:
            events["connected_max"] += 1
        if mut == "connected_in_maximum":
            max_common = max([max_common] + connected_words)
        min_common = int(np.float32(max_common) * np.float32(0.8))
        scored = []
        for kf, s in sharing:
            if kf.mnPlaceRecognitionWords > min_common or (mut == "ge_at_min_common_words" and kf.mnPlaceRecognitionWords == min_common):
                si = np.float32(sc[s])
                kf.mPlaceRecognitionScore = si
                scored.append((si, kf))
        if not scored:
            return [], []
        fresh = {kf: si for si, kf in scored}
        acc_list = []
        for si, kf in scored:
            best, acc, best_kf = si, si, kf
            for kf2 in kf.cov[:10]:
                if kf2.mnPlaceRecognitionQuery != qid:
                    continue
                s2 = kf2.mPlaceRecognitionScore
                if mut == "fresh_scores":
                    s2 = fresh.get(kf2, np.float32(0))
                elif events is not None and kf2 not in fresh and s2 != 0:
                    events["stale"] += 1
                acc = np.float32(acc + s2)
                if s2 > best:
                    best_kf, best = kf2, s2
                    if events is not None:
                        events["neighbour_best"] += 1
            acc_list.append((acc, best_kf))
        if mut == "unstable_sort":                               # equal scores change places
            acc_list = sorted(reversed(acc_list), key=lambda e: -float(e[0]))
        else:                                                    # list::sort is stable; compFirst: a.first > b.first
            acc_list = sorted(acc_list, key=lambda e: -float(e[0]))
        if events is not None and any(a[0] == b[0] and a[1] is not b[1] for a, b in zip(acc_list, acc_list[1:])):
            events["tie"] += 1
        loop, merge, seen = [], [], set()
        i = 0
        while i < len(acc_list) and (len(loop) < n_num or len(merge) < n_num):
            kf = acc_list[i][1]
            if kf.bad:
                raise BadKeyFrame(kf.mnId)
            if kf not in seen:
                if pkf.map is kf.map and len(loop) < n_num:
                    loop.append(kf)
                elif pkf.map is not kf.map and len(merge) < n_num and not kf.map.bad:
                    merge.append(kf)
                seen.add(kf)
            elif events is not None:
                events["duplicate"] += 1
            i += 1
        if events is not None and len(loop) == n_num and len(merge) < n_num:
            events["loop_full_merge_not"] += 1
        return loop, merge


# ----------------------------------------------------------------------------------------------------------------- worlds
def _vocabulary(world):
    from pli_slam_amd import synth
    return synth.make_vocabulary(10, 3, world.seed, False, 0.05)


def make_world(world):
    """The request of one world: {"voc": (k, L, parent, is_leaf, desc, weight), "kf_id", "kf_map", "map_bad", "kf_feat": [node
    indices per keyframe], "cov", "conn" (lists of keyframe indices), "ops": [(kind, a, b, c)], "q_feat": [node indices per
    relocalisation query]}.  A feature is the descriptor of vocabulary node `index` (row of desc)."""
    import helpers_bow_ref as B
    voc = _vocabulary(world)
    k, L, parent, is_leaf, desc, weight = voc
    tree = B.Tree(*voc)
    rng = np.random.default_rng(7000 + world.seed)
    leaves = np.flatnonzero(is_leaf > 0)
    w, wt, _ = tree.rows(desc[leaves], LEVELSUP)
    by_word = {}
    for node, word, val in zip(leaves.tolist(), w.tolist(), wt.tolist()):
        if val > 0 and word not in by_word:
            by_word[word] = node                                  # one feature per word: the node whose descriptor lands in it
    words = rng.permutation(sorted(by_word)).tolist()
    take = lambda n: [words.pop() for _ in range(n)]
    pool = take(40)                                               # words any keyframe may hold
    nowhere = take(30)                                            # words no keyframe holds
    loc = [take(50) for _ in range(4)] + [take(150)]              # the words of five locations; the last is the large one
    # (location, map) of every place; the keyframes of a place see each other
    places = [(0, 0), (0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (3, 1), (0, 0), (4, 0)]
    feats = lambda ws, reps: [by_word[x] for x, r in zip(ws, reps) for _ in range(int(r))]

    def draw(location, keep_lo, npool):
        ws = [x for x in loc[location] if rng.random() < rng.uniform(keep_lo, 1.0)]
        ws += rng.choice(pool, npool, replace=False).tolist()
        return feats(ws, rng.choice(REPEATS, len(ws)))

    kf_feat, kf_place = [], []
    for p, (location, _) in enumerate(places[:7]):
        for _ in range(5):
            kf_feat.append(draw(location, 0.9, 24)); kf_place.append(p)
    twin = draw(0, 0.95, 24)                                      # place 7: two identical keyframes that see only each other
    kf_feat += [twin, list(twin)]; kf_place += [7, 7]
    big = loc[4]
    for n in (1, 63, 64, 65, 128, 129):                           # place 8: exact word counts around the chunk of 64
        ws = big[:n] if n > 1 else big[70:71]
        kf_feat.append(feats(ws, rng.choice(REPEATS, len(ws)))); kf_place.append(8)
    nkf = len(kf_feat)
    ids = rng.permutation(np.arange(1, nkf + 40))[:nkf].astype(np.int64)
    ids[3] = 0                                                     # an id that equals the members' initial query id
    kf_map = np.array([places[p][1] for p in kf_place], np.int32)
    cov, conn = [], []
    for i in range(nkf):
        same = [j for j in range(nkf) if j != i and kf_place[j] == kf_place[i]]
        order = rng.permutation(same).tolist()
        if kf_place[i] in (3, 4):                                  # links across places: neighbours that share few words
            order = order[:2] + [int(j) for j in rng.choice([j for j in range(nkf) if kf_place[j] in (0, 1, 2)], 3, replace=False)] + order[2:]
        if kf_place[i] == 0:                                       # the first visit also sees the second: nine neighbours
            order = order + [j for j in range(nkf) if kf_place[j] == 1]
        if kf_place[i] == 2:                                       # the other map's visit: lists of 0 to 4 neighbours
            order = order[:i % 5]
        if kf_place[i] == 8:                                       # a long list: GetBestCovisibilityKeyFrames(10) cuts it
            order = order + [int(j) for j in rng.choice([j for j in range(nkf) if kf_place[j] != 8], 8, replace=False)]
        cov.append(order); conn.append(sorted(order))
    late = [5, 27, 13]                                              # keyframes that query as DetectNBestCandidates before they are added
    add_order = [int(i) for i in rng.permutation(nkf) if i not in late]
    q_feat = [draw(0, 0.9, 24), draw(0, 0.9, 24), draw(1, 0.9, 24), feats(nowhere[:20], [1] * 20), draw(4, 0.6, 24),
              draw(0, 0.9, 24), draw(2, 0.9, 24), draw(0, 0.9, 24)]
    ops = [(OP_ADD, i, 0, 0) for i in add_order[:30]]
    ops += [(OP_RELOC, 0, 0, 0)]                                   # frame id 0: the id every keyframe already stores
    ops += [(OP_RELOC, 5, 0, 1)]
    ops += [(OP_ERASE, add_order[2], 0, 0), (OP_ERASE, add_order[11], 0, 0)]
    ops += [(OP_ADD, i, 0, 0) for i in add_order[30:]]
    ops += [(OP_RELOC, 6, 0, 2)]                                   # location 1: its keyframes list neighbours scored by query 5 only
    ops += [(OP_NBEST, 5, 3, 0), (OP_ADD, 5, 0, 0)]
    ops += [(OP_ADD, add_order[2], 0, 0)]                          # back in, in another place of the add order
    ops += [(OP_RELOC, 7, 1, 3)]                                   # shares nothing
    ops += [(OP_NBEST, 27, 2, 0), (OP_ADD, 27, 0, 0)]            # the only visit of its location: its connected keyframes share most
    ops += [(OP_RELOC, 8, 0, 4)]                                   # the large location
    ops += [(OP_NBEST, 3, 3, 0)]                                   # the keyframe with id 0 asks
    ops += [(OP_NBEST, 13, 2, 0), (OP_ADD, 13, 0, 0)]
    ops += [(OP_RELOC, 5, 0, 5)]                                   # a frame id seen before
    ops += [(OP_ERASE, add_order[20], 0, 0), (OP_NBEST, 13, 40, 0), (OP_RELOC, 11, 1, 7)]      # ... and location 0 asked for in the other map
    if world.bad_merge_map:
        ops += [(OP_CLEAR_MAP, 1, 0, 0), (OP_RELOC, 9, 0, 6), (OP_CLEAR, 0, 0, 0), (OP_RELOC, 10, 0, 1)]
    else:
        ops += [(OP_RELOC, 9, 1, 6), (OP_CLEAR_MAP, 0, 0, 0), (OP_RELOC, 10, 0, 1)]
    return {"voc": voc, "kf_id": ids, "kf_map": kf_map, "map_bad": np.array([0, 1 if world.bad_merge_map else 0], np.uint8),
            "kf_feat": kf_feat, "cov": cov, "conn": conn, "ops": ops, "q_feat": q_feat}


def _ragged(lists, dtype):
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, dtype).reshape(-1) for x in lists]) if lists and off[-1] else np.zeros(0, dtype)
    return off, flat.astype(dtype)


def request_bytes(req, voc_path):
    desc = req["voc"][4]
    feat = lambda nodes: struct.pack("<i", len(nodes)) + np.ascontiguousarray(desc[np.asarray(nodes, np.int64)], np.uint8).tobytes()
    path = voc_path.encode()
    b = struct.pack("<i", len(path)) + path + struct.pack("<i", LEVELSUP)
    b += struct.pack("<i", len(req["map_bad"])) + req["map_bad"].tobytes()
    b += struct.pack("<i", len(req["kf_id"]))
    for i in range(len(req["kf_id"])):
        b += struct.pack("<qi", int(req["kf_id"][i]), int(req["kf_map"][i])) + feat(req["kf_feat"][i])
        for lst in (req["cov"][i], req["conn"][i]):
            b += struct.pack("<i", len(lst)) + np.asarray(lst, "<i4").tobytes()
    b += struct.pack("<i", len(req["ops"]))
    for kind, a, bb, c in req["ops"]:
        if kind in (OP_ADD, OP_ERASE, OP_CLEAR_MAP):
            b += struct.pack("<ii", kind, a)
        elif kind == OP_CLEAR:
            b += struct.pack("<i", kind)
        elif kind == OP_RELOC:
            b += struct.pack("<iqi", kind, a, bb) + feat(req["q_feat"][c])
        else:
            b += struct.pack("<iii", kind, a, bb)
    return b


def parse_response(raw, req):
    """The reference program's answer -> the recorded arrays of the fixture."""
    nkf = len(req["kf_id"])
    o = 0
    (nwords,) = struct.unpack_from("<i", raw, o); o += 4
    bow_dt = np.dtype([("w", "<u4"), ("v", "<f8")])

    def bow():
        nonlocal o
        (n,) = struct.unpack_from("<i", raw, o); o += 4
        a = np.frombuffer(raw, bow_dt, n, o); o += 12 * n
        return a["w"].copy(), a["v"].copy()

    def ids():
        nonlocal o
        (n,) = struct.unpack_from("<i", raw, o); o += 4
        a = np.frombuffer(raw, "<i8", n, o).copy(); o += 8 * n
        return a

    kfb = [bow() for _ in range(nkf)]
    mem_dt = np.dtype([("rq", "<u8"), ("rw", "<i4"), ("rs", "<f4"), ("pq", "<u8"), ("pw", "<i4"), ("ps", "<f4")])
    qb, common, sc, loop, merge, mem = [], [], [], [], [], []
    for kind, *_ in req["ops"]:
        if kind not in (OP_RELOC, OP_NBEST):
            continue
        qb.append(bow())
        common.append(np.frombuffer(raw, "<i4", nkf, o).copy()); o += 4 * nkf
        sc.append(np.frombuffer(raw, "<f8", nkf, o).copy()); o += 8 * nkf
        loop.append(ids()); merge.append(ids())
        mem.append(np.frombuffer(raw, mem_dt, nkf, o).copy()); o += mem_dt.itemsize * nkf
    assert o == len(raw), (o, len(raw))
    out = {"nwords": np.int32(nwords)}
    out["kf_bow_off"], out["kf_bow_word"] = _ragged([w for w, _ in kfb], np.uint32)
    _, out["kf_bow_val"] = _ragged([v for _, v in kfb], np.float64)
    out["q_bow_off"], out["q_bow_word"] = _ragged([w for w, _ in qb], np.uint32)
    _, out["q_bow_val"] = _ragged([v for _, v in qb], np.float64)
    out["common"] = np.stack(common).astype(np.int32)
    out["score"] = np.stack(sc).astype(np.float64)
    out["score_f32"] = out["score"].astype(np.float32)
    out["loop_off"], out["loop_id"] = _ragged(loop, np.int64)
    out["merge_off"], out["merge_id"] = _ragged(merge, np.int64)
    m = np.stack(mem)
    for key in mem_dt.names:
        out["mem_" + key] = np.ascontiguousarray(m[key])
    return out


def fixture_arrays(req, rec):
    k, L, parent, is_leaf, desc, weight = req["voc"]
    out = {"k": np.int32(k), "L": np.int32(L), "parent": parent, "is_leaf": is_leaf, "desc": desc, "weight": weight,
           "kf_id": req["kf_id"], "kf_map": req["kf_map"], "map_bad": req["map_bad"], "ops": np.array(req["ops"], np.int64)}
    out["kf_feat_off"], out["kf_feat_node"] = _ragged(req["kf_feat"], np.int32)
    out["q_feat_off"], out["q_feat_node"] = _ragged(req["q_feat"], np.int32)
    out["cov_off"], out["cov_idx"] = _ragged(req["cov"], np.int32)
    out["conn_off"], out["conn_idx"] = _ragged(req["conn"], np.int32)
    out.update(rec)
    return out


def fixture_path(name):
    return os.path.join(GOLD_DIR, name + ".npz")


_loaded = {}


def load_fixture(name):
    """{name: array}; loaded once, read-only."""
    if name not in _loaded:
        z = np.load(fixture_path(name))
        d = {}
        for key in z.files:
            d[key] = z[key]
            d[key].setflags(write=False)
        _loaded[name] = d
    return _loaded[name]


def _row(off, flat, i):
    return flat[off[i]:off[i + 1]]


def stubs_of(fix):
    """(maps, keyframes) of a fixture as fresh stub objects holding the recorded BowVectors."""
    maps = [Map(i, b) for i, b in enumerate(fix["map_bad"].tolist())]
    kfs = [KeyFrame(i, fix["kf_id"][i], maps[int(fix["kf_map"][i])], _row(fix["kf_bow_off"], fix["kf_bow_word"], i),
                    _row(fix["kf_bow_off"], fix["kf_bow_val"], i)) for i in range(len(fix["kf_id"]))]
    for i, kf in enumerate(kfs):
        kf.cov = [kfs[j] for j in _row(fix["cov_off"], fix["cov_idx"], i).tolist()]
        kf.conn = {kfs[j] for j in _row(fix["conn_off"], fix["conn_idx"], i).tolist()}
    return maps, kfs


def query_bow(fix, j):
    return _row(fix["q_bow_off"], fix["q_bow_word"], j), _row(fix["q_bow_off"], fix["q_bow_val"], j)


def replay(fix, mut=None, events=None, answers_fn=None, on_query=None):
    """Replays the fixture's operations on the restatement -> per query {"loop": ids, "merge": ids, "members": rows of six per
    keyframe}.  answers_fn(db, qw, qv) replaces the restated device answers; on_query(j, db, qw, qv) sees every query first."""
    maps, kfs = stubs_of(fix)
    db = Database()
    if answers_fn is not None:
        db.answers_fn = lambda qw, qv: answers_fn(db, qw, qv)
    out, j = [], 0
    for kind, a, b, c in fix["ops"].tolist():
        if kind == OP_ADD:
            db.add(kfs[a])
        elif kind == OP_ERASE:
            db.erase(kfs[a])
        elif kind == OP_CLEAR_MAP:
            db.clear_map(maps[a])
        elif kind == OP_CLEAR:
            db.clear()
        else:
            qw, qv = query_bow(fix, j)
            if on_query is not None:
                on_query(j, db, qw, qv)
            if kind == OP_RELOC:
                loop, merge = db.detect_relocalization_candidates(a, qw, qv, maps[b], mut, events), []
            else:
                assert np.array_equal(qw, kfs[a].words)
                loop, merge = db.detect_n_best_candidates(kfs[a], b, mut, events)
            out.append({"loop": [k.mnId for k in loop], "merge": [k.mnId for k in merge], "members": [k.members() for k in kfs]})
            j += 1
    return out


MEMBER_KEYS = ("mem_rq", "mem_rw", "mem_rs", "mem_pq", "mem_pw", "mem_ps")


def differences(fix, got):
    """What of a replay differs from the recorded answers: [(query, what)]; empty when all is equal, floats by their bits."""
    diffs = []
    for j, g in enumerate(got):
        if g["loop"] != _row(fix["loop_off"], fix["loop_id"], j).tolist():
            diffs.append((j, "loop candidates"))
        if g["merge"] != _row(fix["merge_off"], fix["merge_id"], j).tolist():
            diffs.append((j, "merge candidates"))
        cols = list(zip(*g["members"]))
        for key, col in zip(MEMBER_KEYS, cols):
            want = fix[key][j]
            if np.asarray(col, want.dtype).tobytes() != want.tobytes():
                diffs.append((j, key))
    return diffs


def score_pairs(fix):
    """Every recorded (query, keyframe) pair: (j, i, query words, query values, keyframe words, keyframe values)."""
    nq, nkf = fix["score"].shape
    for j in range(nq):
        qw, qv = query_bow(fix, j)
        for i in range(nkf):
            yield j, i, qw, qv, _row(fix["kf_bow_off"], fix["kf_bow_word"], i), _row(fix["kf_bow_off"], fix["kf_bow_val"], i)
