"""The equivalence-class table (fin_eqclasses.hip) where probes wrap and tables are small, the parts that need no GPU: Python mirrors of the table's hash
arithmetic written from the definitions in the kernel file's header (ec_mix, ec_word_hash, the row hash, ec_tag, ec_home), a sequential model of the table
(claim, compare, serial pass), the case generator table_cases() that picks rows by rejection sampling against the mirror, and the guards: every case is
asserted to have exactly the property it is named for -- "this claim probe crosses the table's end", "this serial window wraps", "this table is smaller than a
window", "the limit is met in the serial pass" -- so that a case cannot lose its property silently.

The model chooses inputs and proves guards.  It is NEVER the expectation of a download: that stays tests/test_eqclasses_host.py::classes_of_rows (np.unique).
The mirror is tied to the device by tests/test_eqclasses_table.py, which asserts the model's number of rows through the serial pass against stats()[3], exact,
wherever a case's first add holds one row per tag (the owner): from then on a row goes through the serial pass iff it is not its tag's owner row."""
import numpy as np
import pytest

from tests.test_eqclasses_host import assert_classes, classes_of_rows

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


# ---- the mirrors: Python integers, reduced to 64 bits after every add and multiply ----------------------------------------------------------
def ec_mix(x):
    x ^= x >> 30; x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27; x = x * 0x94D049BB133111EB & M64
    return x ^ (x >> 31)


def ec_word_hash(word, i):
    return ec_mix((word + (i + 1) * GOLD) & M64)


def row_hash(row):
    h = 0
    for i, word in enumerate(row):
        h ^= ec_word_hash(int(word), i)
    return h


def ec_tag(h, tag_bits):
    t = h & ((1 << tag_bits) - 1)
    return t if t else 1


def ec_home(tag, lg):
    return (tag * GOLD & M64) >> (64 - lg)


def lg_of(max_classes):
    """the table has 2^lg slots: the power of two >= 2 max_classes, at least 2"""
    lg = 1
    while (1 << lg) < 2 * max_classes:
        lg += 1
    return lg


# the same in numpy's uint64 arrays (their arithmetic wraps), for the rejection sampling; test_the_array_mirror_is_the_integer_mirror holds them together
def _mix(x):
    x = x ^ (x >> np.uint64(30)); x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27)); x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def row_hashes(rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    h = np.zeros(len(rows), dtype=np.uint64)
    for i in range(rows.shape[1]):
        h ^= _mix(rows[:, i] + np.uint64((i + 1) * GOLD & M64))
    return h


def tags_of(rows, tag_bits):
    t = row_hashes(rows) & np.uint64((1 << tag_bits) - 1)
    t[t == 0] = 1
    return t


def homes_of(tags, lg):
    return ((np.asarray(tags, dtype=np.uint64) * np.uint64(GOLD)) >> np.uint64(64 - lg)).astype(np.int64)


# ---- the sequential model -------------------------------------------------------------------------------------------------------------------
class Report:
    """what one add did in the model"""

    def __init__(self):
        self.serial = 0                  # rows through the serial pass (the add's collision list)
        self.claim_wrapped = False       # a claim-pass probe went from slot slots - 1 to slot 0
        self.start_wrapped = False       # a serial probe started behind a candidate in the last slot: (cand + 1) & mask is 0
        self.window_wrapped = False      # the serial pass went from the table's last window to window 0: s = (b + width) & mask is 0
        self.partial_then_zero = False   # ... and the look it left was a partial one (it began inside the last window)
        self.met_foreign = False         # a serial probe passed a slot held by another tag
        self.limit_claim = False         # the claim pass saw more than max_classes classes, or a probe chain as long as the table
        self.limit_serial = False        # the serial pass saw them
        self.full = False                # a serial probe looked at `slots` slots and found neither its row nor an empty slot


class TableModel:
    """the table of fin_eqclasses.hip, one row after the other: linear probing from the tag's home, a candidate is the first slot with the same tag, full-row
    compare behind it, the serial pass window by window as the kernel takes them"""

    def __init__(self, max_classes, tag_bits, W):
        self.max_classes, self.tag_bits, self.W = max_classes, tag_bits, W
        self.lg = lg_of(max_classes)
        self.slots = 1 << self.lg
        self.tags = [0] * self.slots
        self.rows = [None] * self.slots
        self.counts = [0] * self.slots
        self.classes = 0
        self.unaligned = 0

    def occupied(self):
        return {s for s in range(self.slots) if self.tags[s]}

    def contents(self):
        """(rows, reads, unaligned) in classes_of_rows' form -- to check the model itself"""
        occ = sorted(self.occupied(), key=lambda s: self.rows[s])
        rows = np.array([self.rows[s] for s in occ], dtype=np.uint64).reshape(len(occ), self.W)
        return rows, np.array([self.counts[s] for s in occ], dtype=np.uint64), self.unaligned

    def add(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, self.W)
        slots, mask, width = self.slots, self.slots - 1, min(64, self.slots)
        rep = Report()
        keys = [tuple(int(x) for x in r) for r in rows]
        tags = [int(t) for t in tags_of(rows, self.tag_bits)] if len(rows) else []
        slot_of = []
        for key, tag in zip(keys, tags):                       # pass 1: claim a slot or find the candidate
            if not any(key):
                self.unaligned += 1; slot_of.append(None)
                continue
            s, got = ec_home(tag, self.lg), None
            for _ in range(slots):
                if self.tags[s] == 0:
                    self.tags[s], self.rows[s], got = tag, key, s
                    self.classes += 1
                    if self.classes > self.max_classes:
                        rep.limit_claim = True
                    break
                if self.tags[s] == tag:
                    got = s
                    break
                if s == mask:
                    rep.claim_wrapped = True
                s = (s + 1) & mask
            if got is None:
                rep.limit_claim = True
            slot_of.append(got)
        coll = []
        for i, (key, s) in enumerate(zip(keys, slot_of)):      # pass 2: compare with the candidate
            if s is None:
                continue
            if self.rows[s] == key:
                self.counts[s] += 1
            else:
                coll.append(i)
        for i in coll:                                         # pass 3: go on behind the candidate, a window at a time
            key, cand = keys[i], slot_of[i]
            tag = self.tags[cand]
            if cand == mask:
                rep.start_wrapped = True
            s, probed, done = (cand + 1) & mask, 0, False
            while probed < slots and not done:
                b = s & ~(width - 1)
                for sq in range(s, b + width):
                    t = self.tags[sq]
                    if t == 0:
                        self.tags[sq], self.rows[sq], self.counts[sq], done = tag, key, 1, True
                        self.classes += 1
                    elif t == tag:
                        if self.rows[sq] == key:
                            self.counts[sq] += 1; done = True
                    else:
                        rep.met_foreign = True
                    if done:
                        break
                if not done and b + width == slots:
                    rep.window_wrapped = True
                    if s != b:
                        rep.partial_then_zero = True
                probed += b + width - s
                s = (b + width) & mask
            if not done:
                rep.full = True
        rep.serial = len(coll)
        if rep.full or (self.classes > self.max_classes and not rep.limit_claim):
            rep.limit_serial = True
        return rep


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """adds: uint64[n, W] each, added in turn.  owners_fixed: the first add holds one row per tag, so every later add's path through the table is determined"""

    def __init__(self, group, name, max_classes, tag_bits, W, adds, owners_fixed, **more):
        self.group, self.name, self.max_classes, self.tag_bits, self.W, self.adds, self.owners_fixed = group, name, max_classes, tag_bits, W, adds, owners_fixed
        self.n_colors = 64 * W
        self.slots = 1 << lg_of(max_classes)
        self.__dict__.update(more)
        self._run = None

    def run(self):
        """(the model after every add, the adds' reports), made once"""
        if self._run is None:
            m = TableModel(self.max_classes, self.tag_bits, self.W)
            self._run = m, [m.add(a) for a in self.adds]
        return self._run

    def serial_after(self):
        """the model's stats()[3] after each add"""
        return [int(x) for x in np.cumsum([r.serial for r in self.run()[1]])]

    def __repr__(self):
        return self.name


def draw_rows(rng, W, n, tag_bits, lg, keep=None, avoid=()):
    """n distinct non-empty rows (none of them in `avoid`) whose (tags, homes) by the mirror pass `keep`"""
    out, seen = [], {bytes(np.ascontiguousarray(r, dtype=np.uint64).tobytes()) for r in avoid}
    while len(out) < n:
        cand = rng.integers(1, M64, size=(4096, W), dtype=np.uint64, endpoint=True)
        if keep is not None:
            t = tags_of(cand, tag_bits)
            cand = cand[keep(t, homes_of(t, lg))]
        for row in cand:
            if row.tobytes() not in seen and len(out) < n:
                seen.add(row.tobytes()); out.append(row)
    return np.array(out, dtype=np.uint64).reshape(n, W)


def with_dups(rng, rows, n_total):
    """n_total rows: every row of `rows` at least once, shuffled"""
    n = len(rows)
    return rows[np.concatenate([np.arange(n), rng.integers(0, n, n_total - n)])][rng.permutation(n_total)]


def owners_of(rows, tag_bits):
    """the first row of every tag"""
    _, first = np.unique(tags_of(rows, tag_bits), return_index=True)
    return rows[np.sort(first)]


def chain_rows(rng, max_classes, tag_bits, W, main_tag, n_chain, through):
    """an owner of main_tag, n_chain more rows of that tag and, with `through`, one row each of the other tags whose home lies in the n_chain slots behind
    main_tag's home -- they hold slots in the middle of the chain"""
    lg = lg_of(max_classes)
    mask = (1 << lg) - 1
    home = ec_home(main_tag, lg)
    same = draw_rows(rng, W, n_chain + 1, tag_bits, lg, lambda t, h: t == main_tag)
    others = np.zeros((0, W), dtype=np.uint64)
    if through:
        inside = [t for t in range(1, 1 << tag_bits) if t != main_tag and 0 < ((ec_home(t, lg) - home) & mask) <= n_chain]
        others = np.concatenate([draw_rows(rng, W, 1, tag_bits, lg, lambda t, h, want=want: t == want) for want in inside] or [others])
    return same[:1], same[1:], others


def table_cases(rng):
    cases = []
    # 1. the claim pass across the table's end: full-width tags, homes among the last three slots, more rows than there are slots behind the home
    for max_classes in (4, 32, 64, 128):
        for W in (1, 2, 64):
            lg = lg_of(max_classes)
            n = 4 if max_classes == 4 else 6
            rows = draw_rows(rng, W, n, 63, lg, lambda t, h, lg=lg: h >= (1 << lg) - 3)
            name = "claim wrap, %d slots, W=%d" % (1 << lg, W)
            cases.append(Case("claim_wrap", name + ", one add", max_classes, 63, W, [with_dups(rng, rows, 3 * n + 5)], True))
            cases.append(Case("claim_wrap", name + ", three adds", max_classes, 63, W,
                              [with_dups(rng, rows[: n // 2], n), rows[rng.permutation(n)], with_dups(rng, rows, 3 * n + 5)], True))
    # 2. the serial pass across the table's end: a shared tag whose home lies in the last window and whose chain is longer than the distance to the end
    for what, max_classes, tag_bits, main_tag, n_chain, through in (("1 tag bit, 128 slots", 64, 1, 1, 56, False), ("1 tag bit, 64 slots", 32, 1, 1, 30, False),
                                                                    ("tag 55 of 6 bits, 256 slots", 128, 6, 55, 12, True)):
        for W in (1, 3):
            owner, chain, others = chain_rows(rng, max_classes, tag_bits, W, main_tag, n_chain, through)
            everything = np.concatenate([owner, chain, others])
            name = "serial wrap, %s, W=%d" % (what, W)
            more = dict(main_tag=main_tag, n_chain=n_chain, through=through, n_others=len(others))
            cases.append(Case("serial_wrap", name + ", owners first", max_classes, tag_bits, W,
                              [np.concatenate([owner, others]), with_dups(rng, everything, 3 * len(everything)), with_dups(rng, everything, 2 * len(everything))],
                              True, **more))
            cases.append(Case("serial_wrap", name + ", one shuffled add", max_classes, tag_bits, W, [with_dups(rng, everything, 3 * len(everything))], False, **more))
    # 3. tables smaller than the serial pass's window: as many distinct rows as the table allows, so that all but the owners go through the serial pass
    for max_classes in (1, 2, 4, 8, 16):
        for tag_bits in (1, 2, 3):
            for W in (1, 3):
                lg = lg_of(max_classes)
                name = "small table, %d slots, %d tag bits, W=%d" % (1 << lg, tag_bits, W)
                if max_classes == 1:
                    row = draw_rows(rng, W, 1, tag_bits, lg)
                    cases.append(Case("small", name, 1, tag_bits, W, [row, np.repeat(row, 257, axis=0)], True))
                    continue
                last = [t for t in range(1, 1 << tag_bits) if ec_home(t, lg) == (1 << lg) - 1] if max_classes <= 4 else []
                while True:
                    rows = draw_rows(rng, W, max_classes, tag_bits, lg)
                    t = tags_of(rows, tag_bits)
                    # a tag is shared; in the smallest tables, where a tag's home is the last slot, that tag: its serial probes start at (slots - 1 + 1) & mask
                    if len(np.unique(t)) < max_classes and (not last or int(np.isin(t, last).sum()) >= 2):
                        break
                alls = [with_dups(rng, rows, 3 * max_classes + 7) for _ in range(3)]
                cases.append(Case("small", name, max_classes, tag_bits, W, [owners_of(rows, tag_bits)] + alls, True))
    # 6. the collision list at its bounds: behind an owner-only add, one add of n distinct rows that share the owner's tag -- the list has n entries, n_rows itself
    for n in (1, 63, 64, 65, 257, 1500):
        for W in (1, 2):
            rows = draw_rows(rng, W, n + 1, 1, lg_of(2048))
            cases.append(Case("list", "collision list of %d, W=%d" % (n, W), 2048, 1, W, [rows[:1], rows[1:]], True, n=n))
    return cases


def limit_cases(rng):
    """4. the serial pass's own limit: under one tag, max_classes distinct rows (the owner first) and one more"""
    out = []
    for max_classes in (1, 4, 100):
        for W in (1, 2):
            rows = draw_rows(rng, W, max_classes + 1, 1, lg_of(max_classes))
            good = with_dups(rng, rows[:max_classes], 2 * max_classes + 3)
            over = np.concatenate([good, rows[max_classes:]])[rng.permutation(len(good) + 1)]
            out.append(dict(name="limit, max_classes %d, W=%d" % (max_classes, W), max_classes=max_classes, W=W, owner=rows[:1], good=good, over=over,
                            extra=rows[max_classes:]))
    return out


_CASES = {}


def all_cases():
    """the cases both files use, made once from one seed"""
    if not _CASES:
        rng = np.random.default_rng(2300)
        _CASES["table"] = table_cases(rng)
        _CASES["limit"] = limit_cases(rng)
    return _CASES["table"], _CASES["limit"]


def cases_of(group):
    return [c for c in all_cases()[0] if c.group == group]


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------------
def test_the_array_mirror_is_the_integer_mirror():
    rng = np.random.default_rng(2301)
    for W in (1, 2, 3, 64):
        rows = rng.integers(0, M64, size=(50, W), dtype=np.uint64, endpoint=True)
        rows[0] = 0; rows[1] = M64
        h = row_hashes(rows)
        assert [int(x) for x in h] == [row_hash(r) for r in rows]
        for tag_bits in (1, 2, 3, 6, 63):
            t = tags_of(rows, tag_bits)
            assert [int(x) for x in t] == [ec_tag(int(x), tag_bits) for x in h] and (t != 0).all() and (t < np.uint64(1 << tag_bits)).all()
            for lg in (1, 3, 7, 11, 19, 27):
                assert [int(x) for x in homes_of(t, lg)] == [ec_home(int(x), lg) for x in t]
    assert ec_tag(0, 5) == 1 and ec_tag(32, 5) == 1 and ec_tag(33, 5) == 1 and ec_tag(2, 5) == 2 and ec_tag(M64, 63) == (1 << 63) - 1
    assert ec_mix(0) == 0 and ec_word_hash(0, 0) == ec_mix(GOLD) and ec_word_hash(M64, 0) == ec_mix(GOLD - 1)


def test_the_home_slots_the_cases_are_built_on():
    """why the older tests never crossed the table's end, and where the new ones do: golden-ratio hashing of the narrowed tag"""
    assert ec_home(1, 11) == 1265
    assert [ec_home(t, 11) for t in range(1, 16)] == [1265, 483, 1749, 966, 184, 1450, 668, 1933, 1151, 369, 1635, 852, 70, 1336, 554]
    assert ec_home(1, 7) == 79 and ec_home(1, 6) == 39 and ec_home(55, 8) >= 253
    assert [lg_of(m) for m in (1, 2, 3, 4, 5, 100, 1000, 1 << 18)] == [1, 2, 3, 3, 4, 8, 11, 19]


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
def test_the_model_by_hand():
    """8 slots, 1 tag bit: every row has tag 1, home 4"""
    assert ec_home(1, 3) == 4
    a, b, c, d, e = (np.array([[v]], dtype=np.uint64) for v in (11, 22, 33, 44, 55))
    m = TableModel(4, 1, 1)
    r = m.add(a)
    assert m.occupied() == {4} and r.serial == 0 and not r.claim_wrapped
    r = m.add(np.concatenate([b, a, c, b]))
    assert m.occupied() == {4, 5, 6} and r.serial == 3 and not r.window_wrapped and m.counts[4:7] == [2, 2, 1]
    r = m.add(np.concatenate([d, e]))          # d takes slot 7; e looks at 5 .. 7, then at the whole table from slot 0: the fifth class
    assert m.occupied() == {4, 5, 6, 7, 0} and r.serial == 2 and r.window_wrapped and r.partial_then_zero and r.limit_serial and not r.limit_claim and not r.full
    # full-width tags: the claim pass alone, across the end
    m = TableModel(4, 63, 1)
    rows = draw_rows(np.random.default_rng(1), 1, 3, 63, 3, lambda t, h: h == 7)
    r = m.add(rows)
    assert m.occupied() == {7, 0, 1} and r.claim_wrapped and r.serial == 0
    # a table that is full: 2 slots, three rows under one tag
    m = TableModel(1, 1, 1)
    assert [m.add(x).full for x in (a, b, c)] == [False, False, True]


def test_the_model_counts_what_numpy_counts():
    for case in all_cases()[0]:
        m, reps = case.run()
        assert not any(r.limit_claim or r.limit_serial for r in reps), case.name
        assert_classes(m.contents(), classes_of_rows(np.concatenate(case.adds), case.n_colors), case.name)


# ---- the guards: every case has the property it is named for -----------------------------------------------------------------------------------
def n_not_owner(case, add):
    """the rows of an add that are not their tag's owner row -- the owners are the first add's rows"""
    owner = {int(t): r.tobytes() for t, r in zip(tags_of(case.adds[0], case.tag_bits), case.adds[0])}
    return sum(1 for t, r in zip(tags_of(add, case.tag_bits), add) if owner[int(t)] != r.tobytes())


def check_owners(case):
    """the first add holds one row per tag and every tag of the case: from then on the serial pass takes exactly the rows that are not owners"""
    first = tags_of(case.adds[0], case.tag_bits)
    assert len(np.unique(first)) == len(first), case.name
    assert set(int(t) for a in case.adds for t in tags_of(a, case.tag_bits)) == set(int(t) for t in first), case.name
    reps = case.run()[1]
    assert reps[0].serial == 0 and [r.serial for r in reps[1:]] == [n_not_owner(case, a) for a in case.adds[1:]], case.name


def guard_claim_wrap(case):
    m, reps = case.run()
    rows = np.concatenate(case.adds)
    assert len(np.unique(tags_of(rows, 63))) == len(np.unique(rows, axis=0)) > case.slots - int(homes_of(tags_of(rows, 63), m.lg).min()), case.name
    assert (homes_of(tags_of(rows, 63), m.lg) >= case.slots - 3).all(), case.name
    assert 0 in m.occupied() and any(r.claim_wrapped for r in reps) and all(r.serial == 0 for r in reps), case.name
    assert len(m.occupied()) <= case.max_classes


def guard_serial_wrap(case):
    m, reps = case.run()
    home = ec_home(case.main_tag, m.lg)
    assert case.slots - home <= min(64, case.slots), case.name + ": the home is not in the last window"
    assert case.n_chain + 1 > case.slots - home, case.name + ": the chain ends before the table does"
    assert 0 in m.occupied() and any(r.window_wrapped for r in reps), case.name
    if case.slots > 64:
        assert any(r.partial_then_zero for r in reps), case.name
    if case.through:
        assert case.n_others >= 1 and any(r.met_foreign for r in reps), case.name + ": the chain meets no other tag"
    if case.owners_fixed:
        check_owners(case)
        assert all(r.serial > 0 for r in reps[1:]), case.name
    else:
        assert len(case.adds) == 1 and reps[0].serial > 0


def guard_small(case):
    m, reps = case.run()
    assert case.slots < 64 and case.slots == 2 * case.max_classes, case.name
    assert len(m.occupied()) == case.max_classes, case.name + ": not as many classes as the table allows"
    check_owners(case)
    if case.max_classes > 1:
        assert all(r.serial > 0 for r in reps[1:]) and len(case.adds) == 4, case.name
    else:
        assert len(case.adds[0]) == 1 and len(case.adds[1]) == 257 and len(np.unique(np.concatenate(case.adds), axis=0)) == 1


def guard_list(case):
    m, reps = case.run()
    n = case.n
    check_owners(case)
    assert len(case.adds[0]) == 1 and len(case.adds[1]) == n == reps[1].serial == len(np.unique(case.adds[1], axis=0)), case.name
    assert len(m.occupied()) == n + 1 <= case.max_classes


GUARDS = {"claim_wrap": guard_claim_wrap, "serial_wrap": guard_serial_wrap, "small": guard_small, "list": guard_list}


def test_every_case_has_its_property():
    table, _ = all_cases()
    for case in table:
        GUARDS[case.group](case)
    names = [c.name for c in table]
    assert len(set(names)) == len(names)
    assert {c.slots for c in cases_of("claim_wrap")} == {8, 64, 128, 256} and {c.W for c in cases_of("claim_wrap")} == {1, 2, 64}
    assert {(c.slots, c.tag_bits) for c in cases_of("serial_wrap")} == {(128, 1), (64, 1), (256, 6)} and {c.W for c in cases_of("serial_wrap")} == {1, 3}
    assert {(c.slots, c.tag_bits) for c in cases_of("small")} == {(s, t) for s in (2, 4, 8, 16, 32) for t in (1, 2, 3)}
    # among the small tables: a second look at the whole table, a start behind the last slot, a chain through another tag's slots
    small = [r for c in cases_of("small") for r in c.run()[1]]
    assert any(r.window_wrapped for r in small) and any(r.start_wrapped for r in small) and any(r.met_foreign for r in small)
    ns = sorted({c.n for c in cases_of("list")})
    assert ns == [1, 63, 64, 65, 257, 1500] and 65 % 64 == 1 and 257 % 64 == 1 and -(-1500 // 256) == 6   # a last wave of one row; six blocks


def test_the_guards_fail_when_a_case_loses_its_property():
    """the same cases with unselected random rows in place of the selected ones"""
    rng = np.random.default_rng(2302)
    swap = lambda c, adds, **kw: Case(c.group, c.name, c.max_classes, c.tag_bits, c.W, adds, c.owners_fixed,
                                      **{k: v for k, v in c.__dict__.items() if k in ("main_tag", "n_chain", "through", "n_others", "n")}, **kw)
    c = [x for x in cases_of("claim_wrap") if x.slots == 256 and x.W == 1][0]
    with pytest.raises(AssertionError):
        guard_claim_wrap(swap(c, [draw_rows(rng, 1, len(a), 63, 8) for a in c.adds]))
    for c in [x for x in cases_of("serial_wrap") if x.W == 1 and x.tag_bits == 6]:
        with pytest.raises(AssertionError):                                             # rows of any tag: no chain at tag 55's home
            guard_serial_wrap(swap(c, [draw_rows(rng, 1, len(a), 6, 8) for a in c.adds]))
    c = [x for x in cases_of("serial_wrap") if x.W == 1 and x.slots == 128 and x.owners_fixed][0]
    with pytest.raises(AssertionError):                                                 # a chain that ends before the table does
        guard_serial_wrap(swap(c, [c.adds[0], c.adds[1][:20], c.adds[2][:20]]))
    with pytest.raises(AssertionError):                                                 # a first add with two rows of one tag: the owners are not fixed
        guard_serial_wrap(swap(c, [np.unique(c.adds[1], axis=0)[:2]] + c.adds[1:]))
    c = [x for x in cases_of("small") if x.slots == 16 and x.tag_bits == 3 and x.W == 1][0]
    with pytest.raises(AssertionError):                                                 # fewer classes than the table allows
        guard_small(swap(c, [c.adds[0], c.adds[0], c.adds[0], c.adds[0]]))
    c = [x for x in cases_of("list") if x.n == 65 and x.W == 1][0]
    with pytest.raises(AssertionError):                                                 # a row twice: the list is longer than the classes
        guard_list(swap(c, [c.adds[0], np.concatenate([c.adds[1][:64], c.adds[1][:1]])]))


def test_the_limit_cases_meet_the_limit_in_the_serial_pass():
    for lc in all_cases()[1]:
        mc, W = lc["max_classes"], lc["W"]
        assert len(np.unique(lc["good"], axis=0)) == mc and len(np.unique(lc["over"], axis=0)) == mc + 1, lc["name"]
        m = TableModel(mc, 1, W)
        reps = [m.add(lc["owner"]), m.add(lc["good"])]
        assert not any(r.limit_claim or r.limit_serial for r in reps) and len(m.occupied()) == mc, lc["name"]
        assert_classes(m.contents(), classes_of_rows(np.concatenate([lc["owner"], lc["good"]]), 64 * W), lc["name"])
        r = m.add(lc["extra"])                                     # in a later add
        assert r.limit_serial and not r.limit_claim and r.serial == 1, lc["name"]
        m = TableModel(mc, 1, W)
        reps = [m.add(lc["owner"]), m.add(lc["over"])]             # in the same add
        assert reps[1].limit_serial and not any(r.limit_claim for r in reps), lc["name"]
