"""Links on the host (include/finito_amd.h: LINKS, fin_records_links, fin_link_hash; fin_links_host.cpp): the MODEL -- plain Python written from the
header's definition, which tests/test_links.py, test_links_table.py and test_cli_links.py hold the device and the CLI to --, the host twin against it, the Python
helpers, and the stand-alone sanitizer program.  Every comparison is exact; nothing here needs a GPU."""
import bisect
import os
import subprocess

import numpy as np
import pytest

import finito_amd as fa
from tests.test_fragments_host import build, mate
from tests.test_records import brute_expand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
class Model:
    """counts: {(g_a, g_b): count} with g_a <= g_b, over the transitions whose ends lie in the index; outside: the transitions with an end outside it (not counted);
    both_ways: the keys met as (lower place, higher place) and the other way round, in read order"""

    def __init__(self, pairs, nks, ends):
        self.ends = [int(e) for e in ends]
        self.starts = [0] + self.ends[:-1]
        total, nu = self.ends[-1], len(self.ends)
        self.counts, self.outside, self.same_unitig_jumps = {}, 0, 0
        seen_up, seen_down = set(), set()
        p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist()
        at = 0
        for nk in np.asarray(nks, dtype=np.int64).tolist():
            for i in range(at + 1, at + nk):   # slot 0 of a read never makes a transition
                (ua, oa), (ub, ob) = p[i - 1], p[i]
                if ua == -1 or ub == -1:
                    continue
                if ua == ub and abs(ob - oa) == 1:
                    continue   # straight, either way
                if not (0 <= ua < nu and 0 <= ub < nu):
                    self.outside += 1
                    continue
                ga, gb = self.starts[ua] + oa, self.starts[ub] + ob
                if not (0 <= ga < total and 0 <= gb < total):
                    self.outside += 1
                    continue
                key = (min(ga, gb), max(ga, gb))
                self.counts[key] = self.counts.get(key, 0) + 1
                (seen_up if ga <= gb else seen_down).add(key)
                if ua == ub:
                    self.same_unitig_jumps += 1
            at += nk
        assert at == len(p)
        self.both_ways = seen_up & seen_down
        self.transitions = sum(self.counts.values())
        self.n_distinct = len(self.counts)
        self.n_self = sum(1 for a, b in self.counts if a == b)

    def end_of(self, g):
        u = bisect.bisect_right(self.ends, g)
        return u, g - self.starts[u]

    def table(self, min_count=1):
        keep = sorted(key for key, c in self.counts.items() if c >= max(min_count, 1))
        out = np.zeros(len(keep), dtype=fa.LINK_DTYPE)
        for i, key in enumerate(keep):
            out[i] = self.end_of(key[0]) + self.end_of(key[1]) + (self.counts[key],)
        return out


def assert_table(got, m, what="", min_count=1, times=1):
    """a downloaded LinkTable against the model (every count `times` times the model's)"""
    want = m.table(-(-min_count // times))
    want["count"] *= np.uint64(times)
    assert got.links.dtype == fa.LINK_DTYPE and got.links.shape == want.shape, "%s: %d links, model %d" % (what, len(got.links), len(want))
    bad = np.nonzero(got.links != want)[0]
    assert len(bad) == 0, "%s: %d links differ, first %d: got %s, model %s" % (what, len(bad), bad[0], got.links[bad[0]], want[bad[0]])
    assert (got.transitions, got.n_distinct, got.n_self) == (times * m.transitions, m.n_distinct, m.n_self), "%s: counters %s, model %s" % (
        what, (got.transitions, got.n_distinct, got.n_self), (times * m.transitions, m.n_distinct, m.n_self))


# ---- hand-made reads ------------------------------------------------------------------------------------------------------------------------
K = 5
ENDS = np.cumsum([300, 40, 500, K, K + 1, 5000]).astype(np.int64)


def wandering_reads(rng, ends, k, n, max_nk=70):
    """n reads as build() takes them: searched reads that step up and down, repeat a pair, jump to one of a few places of every unitig and have absent slots;
    kind-1 records with positions; kind-2 reads; reads without k-mers"""
    lens = np.diff(np.concatenate([[0], ends]))
    out = []
    for _ in range(n):
        t = rng.random()
        if t < 0.08:
            out.append(("none", int(rng.integers(1, 10))))
        elif t < 0.12:
            out.append(("scan", []))
        elif t < 0.3:
            nk = int(rng.integers(1, 40))
            Es = sorted(int(x) for x in rng.integers(0, nk + k - 1, int(rng.integers(0, 4))))
            out.append(mate(int(np.argmax(lens)), int(rng.integers(0, 1000)), nk, bool(rng.integers(0, 2)), "rec", Es))
        else:
            slots, prev = [], None
            for _ in range(int(rng.integers(1, max_nk + 1))):
                w = int(rng.integers(0, 12))
                if w == 0:
                    cur = (-1, -1)
                elif w == 1 or prev is None or prev[0] < 0:
                    u = int(rng.integers(0, len(lens)))
                    cur = (u, int(rng.integers(0, min(6, lens[u] - k + 1))))
                elif w == 2:
                    cur = prev
                elif w < 8 and prev[1] + 1 <= lens[prev[0]] - k:
                    cur = (prev[0], prev[1] + 1)
                elif prev[1] >= 1:
                    cur = (prev[0], prev[1] - 1)
                else:
                    cur = (prev[0], prev[1] + 1) if prev[1] + 1 <= lens[prev[0]] - k else prev
                slots.append(cur); prev = cur
            out.append(("scan", slots))
    return out


def test_the_twin_against_the_model_at_one_and_four_threads():
    rng = np.random.default_rng(4290)
    recs, stream = build(wandering_reads(rng, ENDS, K, 5000))
    nks = recs["nk"].astype(np.int64)
    m = Model(brute_expand(recs, stream, K), nks, ENDS)
    assert m.n_distinct >= 200 and m.n_self >= 5 and len(m.both_ways) >= 50 and m.same_unitig_jumps >= 50 and m.outside == 0
    assert max(m.counts.values()) >= 40 and min(m.counts.values()) == 1
    assert all((recs["meta"] >> 16 == kind).sum() >= 8 for kind in (0, 1, 2))
    for threads in (1, 4):
        for mc in (0, 1, 2, 40, 10**9):
            assert_table(fa.records_links(recs, stream, K, ENDS, mc, threads), m, "threads %d, min_count %d" % (threads, mc), mc)
    assert len(m.table(40)) >= 1 and len(m.table(10**9)) == 0
    empty = fa.records_links(recs[:0], stream[:0], K, ENDS)
    assert len(empty.links) == 0 and (empty.transitions, empty.n_distinct, empty.n_self) == (0, 0, 0)


def test_the_rule_by_hand():
    """each clause of the definition on a read of its own"""
    cases = {
        "a step of +1 and a step of -1 are straight": ([(0, 5), (0, 6), (0, 5), (0, 6)], {}),
        "a repeated pair is a self link": ([(0, 7), (0, 7)], {(7, 7): 1}),
        "a step of two is a jump inside the unitig": ([(0, 7), (0, 9)], {(7, 9): 1}),
        "the pair is unordered": ([(2, 3), (0, 4), (2, 3)], {(4, 343): 2}),
        "an absent slot between two found ones": ([(0, 7), (-1, -1), (2, 3)], {}),
        "slot 0 makes none": ([(1, 1)], {}),
        "the last k-mer of a unitig to the first of the next": ([(0, 295), (1, 0)], {(295, 300): 1}),
        "the same offset in another unitig": ([(0, 4), (1, 4), (1, 5)], {(4, 304): 1}),
    }
    for name, (slots, want) in cases.items():
        recs, stream = build([("scan", slots)])
        m = Model(brute_expand(recs, stream, K), recs["nk"], ENDS)
        assert m.counts == want, name
        assert_table(fa.records_links(recs, stream, K, ENDS), m, name)
    # the last slot of one read and the first of the next never meet; a kind-1 record with gaps and a kind-2 read make none
    recs, stream = build([("scan", [(0, 7)]), ("scan", [(2, 3)]), mate(2, 10, 30, True, "rec", (3, 20)), ("none", 4), ("scan", [(0, 1), (2, 2)])])
    m = Model(brute_expand(recs, stream, K), recs["nk"], ENDS)
    assert m.counts == {(1, 342): 1}
    assert_table(fa.records_links(recs, stream, K, ENDS), m, "read boundaries, records")


def test_the_twin_refuses_what_the_header_says():
    good = [("scan", [(0, 7), (2, 3)])]
    for name, slots in {"a unitig number at n_unitigs": [(0, 7), (len(ENDS), 0)], "a place at total_len": [(0, 7), (len(ENDS) - 1, 5000)]}.items():
        recs, stream = build(good + [("scan", slots)])
        m = Model(brute_expand(recs, stream, K), recs["nk"], ENDS)
        assert m.outside == 1 and m.transitions == 1, name
        with pytest.raises(fa.FinitoError) as e:
            fa.records_links(recs, stream, K, ENDS)
        assert e.value.code == fa.FIN_EINVAL, name
    recs, stream = build(good + [("scan", [(len(ENDS), 0), (len(ENDS), 1)])])   # outside, but straight: no transition looks at it
    assert fa.records_links(recs, stream, K, ENDS).transitions == 1
    recs, stream = build(good)
    with pytest.raises(fa.FinitoError):
        fa.records_links(recs, stream[:1], K, ENDS)
    with pytest.raises(fa.FinitoError):
        fa.records_links(recs, stream, K, ENDS[::-1])


def test_link_hash_mirrors_the_library():
    L = fa.lib()
    rng = np.random.default_rng(7)
    for key in [0, 1, (1 << 64) - 2, (5 << 32) | 9] + [int(x) for x in rng.integers(0, 1 << 63, 200)]:
        assert fa.link_hash(key) == L.fin_link_hash(key)
    assert fa.link_hash(1) == 0x5692161D100B05E5


def test_unitig_edges_classes_every_end():
    k = 4
    ends = np.cumsum([10, k, 7, k, 12])            # unitigs 1 and 3 hold one k-mer each
    rows = [(0, 6, 1, 0, 5),      # E -> B: an edge
            (0, 6, 2, 0, 2),      # E -> S: an edge
            (1, 0, 3, 0, 1),      # B -> B: an edge
            (2, 3, 2, 3, 4),      # E -> E, a self link at a unitig's last k-mer: an edge by its ends
            (0, 3, 2, 0, 7),      # I -> S: a jump
            (0, 4, 2, 0, 1),      # I -> S again: summed with the one above
            (2, 1, 4, 8, 3),      # I -> E: a jump
            (4, 0, 4, 5, 9)]      # S -> I: a jump inside one unitig
    t = fa.LinkTable(np.array(rows, dtype=fa.LINK_DTYPE), 32, 8, 1)
    e = t.unitig_edges(ends, k)
    want = [(0, b"E", 1, b"B", 5), (0, b"E", 2, b"S", 2), (0, b"I", 2, b"S", 8), (1, b"B", 3, b"B", 1), (2, b"E", 2, b"E", 4), (2, b"I", 4, b"E", 3), (4, b"S", 4, b"I", 9)]
    assert e.edges.dtype == fa.LINK_EDGE_DTYPE and e.edges.tolist() == want
    assert (e.n_edge, e.n_jump) == (12, 20) and e.n_edge + e.n_jump == t.transitions
    with pytest.raises(fa.FinitoError):
        fa.LinkTable(np.array([(9, 0, 9, 1, 1)], dtype=fa.LINK_DTYPE), 1, 1, 0).unitig_edges(ends, k)
    empty = fa.LinkTable(np.zeros(0, dtype=fa.LINK_DTYPE), 0, 0, 0).unitig_edges(ends, k)
    assert len(empty.edges) == 0 and (empty.n_edge, empty.n_jump) == (0, 0)


def test_links_merge_adds_two_tables():
    rng = np.random.default_rng(4291)
    halves = [build(wandering_reads(rng, ENDS, K, 700)) for _ in range(2)]
    tabs = [fa.records_links(r, s, K, ENDS) for r, s in halves]
    recs, stream = np.concatenate([halves[0][0], halves[1][0]]), np.concatenate([halves[0][1], halves[1][1]])
    m = Model(brute_expand(recs, stream, K), recs["nk"], ENDS)
    shared = set(map(tuple, tabs[0].links[["u_a", "off_a", "u_b", "off_b"]].tolist())) & set(map(tuple, tabs[1].links[["u_a", "off_a", "u_b", "off_b"]].tolist()))
    assert len(shared) >= 20 and len(shared) < min(len(t.links) for t in tabs)
    assert_table(fa.links_merge(*tabs), m, "merged")
    assert_table(fa.links_merge(tabs[1], tabs[0]), m, "merged, the other way round")
    none = fa.LinkTable(np.zeros(0, dtype=fa.LINK_DTYPE), 0, 0, 0)
    assert_table(fa.links_merge(tabs[0], none), Model(brute_expand(*halves[0], K), halves[0][0]["nk"], ENDS), "merged with an empty table")


def test_the_sanitizer_program_builds_and_passes(tmp_path):
    """tools/asan_links.cpp: the twin under ASan + UBSan as a stand-alone program on the CPU -- nothing is loaded into Python; the sanitizers' runtimes are
    linked into the program itself, so it does not matter what else the loader brings"""
    exe = str(tmp_path / "asan_links")
    src = ["tools/asan_links.cpp", "finito_amd/csrc/fin_links_host.cpp", "finito_amd/csrc/fin_records_host.cpp", "finito_amd/csrc/fin_taxa_host.cpp"]
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-std=c++17", "-fopenmp", "-o", exe] + src, cwd=ROOT)
    r = subprocess.run([exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and not r.stderr.strip(), r.stderr[-2000:]
