"""The constructed colliders of the compact k-mer table (fin_format.h: FinDevIndex::kt3), without a GPU: the Python restatements of fin_mix64, fin_kt3_fold,
fin_kt3_hash and fin_kt3_bucket (tests/util.py) held against the header itself through a small host program, the inverse of the finaliser, what colliders_of and
control_of promise, and -- per case of tests/test_kmer_table_collisions.py -- what the case presupposes, asserted with the faithful oracle on the CPU.

Everything here rests on fin_mix64 being a bijection.  A hash without an inverse needs another way to make colliders."""
import os
import subprocess

import numpy as np
import pytest

from tests.util import (COLLISION_KS, _collision_try, KT3_TAG_BITS, collision_case, collision_case_problems, collision_scenarios, colliders_of, control_of, default_cbf_m, kmer_words,
                        kt3_bucket, kt3_hash, mix64, prepass_middle_start, random_genome, rc, unmix64, words_kmer)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = (1 << KT3_TAG_BITS) - 1

# reads lines "n_buckets w0 w1 ..." (hexadecimal key words) and prints "hash bucket" of each: one word: fin_mix64 alone and fin_kt3_hash(k0, 0); two: fin_kt3_hash and
# the folded form; more: the folded form, as fin_kernel_b.hip and fin_prepass.hip (look_ktabN_at) make it
PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "fin_format.h"
int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        uint64_t w[8]; int n = 0; char* p = line;
        const uint32_t nb = (uint32_t)strtoull(p, &p, 16);
        for (;;) { char* e; const uint64_t v = strtoull(p, &e, 16); if (e == p || n == 8) break; w[n++] = v; p = e; }
        uint64_t key = w[0];
        for (int j = 1; j < n; j++) key = fin_kt3_fold(key, w[j], (uint32_t)j);
        const uint64_t h = fin_mix64(key);
        if (n <= 2 && h != fin_kt3_hash(w[0], n == 2 ? w[1] : 0ull)) { printf("the two-word form and the folded form differ\n"); return 1; }
        printf("%016llx %08x %08x\n", (unsigned long long)h, fin_kt3_bucket(h, nb), (unsigned)(h & FIN_KT3_TAGMASK));
    }
    return 0;
}
"""


def test_restatements_against_the_header(tmp_path):
    """hash, bucket and tag of a few hundred keys of 1, 2, 4 and 7 words -- random ones, words of zeros (a run of A adds nothing), all ones -- as the header computes
    them, exactly"""
    src = tmp_path / "kt3_header.cpp"; exe = tmp_path / "kt3_header"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "finito_amd", "csrc"), "-o", str(exe), str(src)])
    rng = np.random.default_rng(30)
    keys = []
    for n in (1, 2, 4, 7):
        for i in range(120):
            w = [int(x) for x in rng.integers(0, 1 << 64, n, dtype=np.uint64)]
            if i % 10 == 0: w[int(rng.integers(0, n))] = 0
            if i % 17 == 0: w[-1] = 0
            if i == 3: w = [(1 << 64) - 1] * n
            if i == 4: w = [0] * n
            keys.append((int(rng.choice([1, 16, 1000, 12345, (1 << 32) - 1])) if i % 3 else int(rng.integers(1, 1 << 32)), w))
    text = "".join("%x %s\n" % (nb, " ".join("%x" % x for x in w)) for nb, w in keys)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == len(keys)
    for (nb, w), line in zip(keys, lines):
        h = kt3_hash(w)
        assert line == "%016x %08x %08x" % (h, kt3_bucket(h, nb), h & TAG), (nb, w, line)
        if len(w) == 1:
            assert h == mix64(w[0])


def test_the_finaliser_has_an_inverse():
    rng = np.random.default_rng(31)
    for x in [0, 1, (1 << 64) - 1, 1 << 63, 1 << 29, 1 << 32] + [int(v) for v in rng.integers(0, 1 << 64, 2000, dtype=np.uint64)]:
        assert unmix64(mix64(x)) == x and mix64(unmix64(x)) == x


def test_key_words_pack_the_first_base_into_the_low_bits():
    assert kmer_words("C" + "A" * 30) == [1] and kmer_words("A" * 31 + "T" + "G") == [3 << 62, 2]
    rng = np.random.default_rng(32)
    for k in COLLISION_KS:
        q = random_genome(rng, k)
        w = kmer_words(q)
        assert len(w) == (k + 31) // 32 and words_kmer(w, k) == q and all(x < 1 << 64 for x in w) and w[-1] < 1 << (2 * ((k - 1) % 32 + 1))


@pytest.mark.parametrize("k", (31, 32, 47, 63, 64, 100, 127, 200))
def test_colliders_and_controls(k):
    """the shared bits, the kept key words, validity, and the yield: three of three from k = 32 on; at k = 31 (a first word must lie below 2^62) at least 40 % of the
    victims must have a collider -- a condition on the inputs the cases draw from; this test's 2000 victims: 1106, 55.3 %"""
    rng = np.random.default_rng(3300 + k)
    n = 2000 if k == 31 else 200
    with_one = 0
    for _ in range(n):
        y = random_genome(rng, k)
        wy = kmer_words(y); h = kt3_hash(wy)
        cs = colliders_of(y)
        with_one += bool(cs)
        assert len(cs) == 3 or k == 31
        assert len(set(cs)) == len(cs)
        for x in cs + [control_of(y)]:
            wx = kmer_words(x); hx = kt3_hash(wx)
            assert len(x) == k and set(x) <= set("ACGT") and x != y and wx[1:] == wy[1:]
            assert hx >> 32 == h >> 32
            for nb in (1, 7, 4096, 1000003, (1 << 32) - 1):
                assert kt3_bucket(hx, nb) == kt3_bucket(h, nb)
        assert all(kt3_hash(kmer_words(x)) & TAG == h & TAG for x in cs)
        assert {(kt3_hash(kmer_words(x)) ^ h) >> KT3_TAG_BITS for x in cs} <= {1, 2, 3}   # (they differ from the victim in hash bits 30 and 31 only)
        assert kt3_hash(kmer_words(control_of(y))) & TAG != h & TAG
    if k == 31:
        print("k = 31: %d of %d victims have a collider" % (with_one, n))
        assert with_one >= 0.4 * n
    else:
        assert with_one == n


CASES = [(k, s) for k in COLLISION_KS for s in collision_scenarios(k)]


@pytest.mark.parametrize("k,scenario", CASES)
def test_what_a_case_presupposes(k, scenario):
    """the oracle finds no absent collider and no control k-mer on either strand, every present collider at its own place, every victim as its scenario says (at its
    own place; scenario 5: at a place that does not spell it); the reads carry the members where their kind says; the generator is deterministic"""
    c = collision_case(k, scenario)
    assert collision_case_problems(c) == []
    # (sizes: the issue asks for indexes of a few kb and reads of at most 300 bases.  Every absent collider and every control k-mer brings two unitigs of k bases, so
    #  the largest text, scenario 1 at k = 200, has 28 644 bases; and a read that splices a k-mer between two stretches with a k-mer each has more than 3 k bases:
    #  beyond 300 from k = 100 on, 644 at k = 200.  k <= 64: no read is longer than the 256 bases the fast path takes)
    assert len(c.text) <= 30000 and len(c.reads) <= 300 and len(c.reads) == len(c.control_reads) == len(c.kinds)
    assert max(len(r) for r in c.reads) <= (256 if k <= 64 else 3 * k + 100)
    assert all(len(cs) == (3 if k >= 32 and scenario in (1, 2) else len(cs)) and len(cs) >= 1 for _, cs in c.groups)
    members = set(c.control)
    assert members and not members & set(c.control.values())
    n_differ = 0
    for r, q, (what, kind, rev) in zip(c.reads, c.control_reads, c.kinds):
        assert len(r) == len(q) and len(r) >= k
        n_differ += r != q
        f = rc(r) if rev else r
        here = [i for i in range(len(f) - k + 1) if f[i:i + k] in members]
        assert here, (what, kind)
        if kind in ("first", "whole", "twice"):
            assert here[0] == 0
        if kind in ("last", "whole", "twice"):
            assert here[-1] == len(f) - k
        if kind == "middle":
            assert here == [prepass_middle_start(len(f), k)] and 0 < here[0] < len(f) - k
        if kind == "twice":
            assert len(here) >= 2   # (more: the stretch between them may hold a victim that is a member itself)
    assert n_differ == len(c.reads)
    merged, fwd = c.expected["reads"]
    assert merged.shape == fwd.shape == (sum(len(r) - k + 1 for r in c.reads), 2)
    at = 0
    for r, (what, kind, rev) in zip(c.reads, c.kinds):
        n = len(r) - k + 1
        f = rc(r) if rev else r
        for i in range(n):
            m = f[i:i + k]
            slot = n - 1 - i if rev else i
            if m in members and m not in c.present and m not in [v for v, _ in c.groups]:
                assert merged[at + slot, 0] == -1, "an absent collider, found"
            elif m in members:
                assert merged[at + slot, 0] >= 0, "a member that is in the index, not found"
        if what == "member":   # reads along the unitigs of the present colliders and around their victims: every k-mer is found
            assert (merged[at:at + n, 0] >= 0).all()
        at += n
    if scenario == 1:
        assert len(c.first_reads) == sum(len(cs) for _, cs in c.groups) >= 20
    if scenario == 2:
        assert c.where["text_first"] == k - 1 and c.where["text_last"] == len(c.text) - 1
        assert c.where["unitig_first"] - k + 1 in [0] + list(c.ends) and c.where["unitig_last"] + 1 in list(c.ends)
        if k == 31:
            assert ((c.where["one_window"] - k + 1) & 63) + k <= 64 < ((c.where["two_windows"] - k + 1) & 63) + k
    if scenario == 3:
        assert max(len(cs) for _, cs in c.groups) == (3 if k >= 32 else 1) and c.present == {x for _, cs in c.groups for x in cs}
    if scenario == 4:
        assert default_cbf_m(k) == 20 and len(c.runs) == len(c.groups)
    if scenario == 5:
        assert c.present and any(x not in c.present for _, cs in c.groups for x in cs)
    again = _collision_try(k, scenario, c.seed)
    assert again.reads == c.reads and again.control_reads == c.control_reads and again.unitigs == c.unitigs
