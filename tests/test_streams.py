"""The stream contract of include/finito_amd.h on NON-BLOCKING user streams: every call that takes a stream, and every reader that runs "on that run's stream".

On the NULL stream the legacy default-stream rules order everything against everything, so no other test can see a missing event or wait.  Here every scenario
puts a DELAY (torch.cuda._sleep, calibrated once per module; a chain of torch.mm where that is unusable) on a torch.cuda.Stream(), issues the calls under test
behind it without touching the host, and only then asks for results.  A GUARD -- stream.query() is False right after the last call that must not wait -- proves
both that those calls did not synchronise and that the delay was still running, so the ordering was exercised and nothing passes by luck.

A lost ordering is a wrong answer, never a fault: before each scenario the batch runs read set A on the NULL stream and makes every product the scenario asks
for; then B -- same read lengths, different answers (tests/test_streams_host.py asserts both) -- is loaded.  A call that overtakes the run reads A's data.
Expected values come from the CPU oracle and the numpy definitions of the other test files, never from a NULL-stream run of the library; all comparisons exact.

Measured on an MI355X: the step of the 600-read batch on the NULL stream takes 0.43 ms at k = 31 and 0.53 ms at k = 63; the delay is
max(20 x step, 40 ms) = 40 ms, 75 steps or more (measured with events: 39.9 and 40.6 ms; scenario 4 uses 80 ms on one stream and 40 ms on the other), well
below the 200 ms bound; every guard held."""
import ctypes as C

import numpy as np
import pytest
import torch

import finito_amd as fa
from tests.test_colors_host import assert_pseudo, pack_members, rows_of, unpack
from tests.test_read_class_host import assert_classes
from tests.test_read_summary import assert_screen
from tests.test_read_summary_host import assert_summaries
from tests.test_records import brute_expand
from tests.test_segments_host import assert_segments
from tests.test_streams_host import ADDED_COLOR, KS, N_COLORS, case
from tests.test_unitig_counts import assert_profile
from tests.test_unitig_coverage import assert_cover
from tests.test_unitig_depth import assert_depth

pytestmark = pytest.mark.gpu

MIN_DELAY_MS, MAX_DELAY_MS = 40.0, 95.0   # (scenario 4 doubles it on one stream: below 200 ms)
SCREEN = (20, 300)


class Delay:
    """device work of a known length on a stream: torch.cuda._sleep, calibrated with two events the way torch's own tests do; a chain of 2048^2 torch.mm, sized
    the same way, where _sleep does not give a usable time"""

    def __init__(self):
        self.cycles_per_ms, self.mm, self.mm_ms = 0.0, None, 0.0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1_000_000)
        e0.record(); torch.cuda._sleep(20_000_000); e1.record(); e1.synchronize()
        ms = e0.elapsed_time(e1)
        if 1.0 <= ms <= 2000.0:
            self.cycles_per_ms = 20_000_000 / ms
            return
        self.mm = torch.rand(2048, 2048, device="cuda")
        torch.mm(self.mm, self.mm)
        e0.record()
        for _ in range(20):
            torch.mm(self.mm, self.mm)
        e1.record(); e1.synchronize()
        self.mm_ms = e0.elapsed_time(e1) / 20

    def __call__(self, stream, ms):
        with torch.cuda.stream(stream):
            if self.mm is None:
                torch.cuda._sleep(int(ms * self.cycles_per_ms))
            else:
                for _ in range(int(ms / self.mm_ms) + 1):
                    torch.mm(self.mm, self.mm)


class World:
    """one index of the case on the device, its labelling and colour matrix, the streams and the delay"""

    def __init__(self, k, delay_on):
        self.k, self.c = k, case(k)
        self.p = fa.FinimizerIndex.build(self.c.unitigs, k).to_device(0)
        self.A, self.B, self.bigger = self.c.A, self.c.B, self.c.bigger
        self.S, self.T, self.U = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
        self.delay_on = delay_on
        b = self.p.batch(self.B.reads)   # the batch's own step on the NULL stream
        for _ in range(4):
            b.run()
        torch.cuda.synchronize()
        step, n = b.step_time_ms(skip_first=1)
        b.close()
        assert n == 3 and step["step"] > 0
        self.step_ms = step["step"]
        self.delay_ms = max(20 * self.step_ms, MIN_DELAY_MS)
        assert self.delay_ms <= MAX_DELAY_MS, "a step of %.3f ms wants a delay beyond the bound" % self.step_ms
        print("k=%d: step %.3f ms on the NULL stream, delay %.1f ms" % (k, self.step_ms, self.delay_ms))

    def delay(self, stream, times=1):
        self.delay_on(stream, times * self.delay_ms)

    def labels(self):
        return self.p.labels(self.c.labels)

    def colors(self, bits=True):
        return self.p.colors(N_COLORS, self.c.bits if bits else None)

    def primed(self, mode=0, lab=None, col=None, reads=None):
        """a batch that has run A on the NULL stream in `mode`, has made every product from it -- checked against A's expectation: the stale state is A's --
        and holds B, not yet run"""
        b = self.p.batch(self.A.reads)
        b.text_mode(mode); b.run()
        check_products(self, b, self.A, mode, lab, col, "priming with A")
        torch.cuda.synchronize()
        b.reload(self.B.reads if reads is None else reads)
        return b

    def close(self):
        self.p.close()


@pytest.fixture(scope="module")
def delay_on():
    return Delay()   # calibrated once per module


@pytest.fixture(scope="module", params=KS, ids=lambda k: "k%d" % k)
def w(request, delay_on):
    world = World(request.param, delay_on)
    yield world
    world.close()


def guard(*streams):
    """the calls before this did not wait, and the delay in front of them is still running"""
    for s in streams:
        assert s.query() is False, "a stream is idle where its delay should still run: a call that must not wait has synchronised, or the delay is too short"


def check_products(w, b, E, mode, lab, col, what):
    """everything a batch gives after a run, against the expectation E"""
    k = w.k
    if mode == 2 and b.run_info()["fast_path"]:
        for call in (b.download, lambda: b.download_range(0, 10)):   # text only: the pairs are still refused
            with pytest.raises(fa.FinitoError) as e:
                call()
            assert e.value.code == fa.FIN_EINVAL, what
    else:
        pairs, npos = b.download()
        assert np.array_equal(pairs.astype(np.int64), E.pairs) and npos == E.found, "%s: pairs" % what
        assert np.array_equal(b.download_range(1000, 5000).astype(np.int64), E.pairs[1000:6000]), "%s: range" % what
    assert b.text() == E.text, "%s: text" % what
    recs, stream = b.records()
    assert np.array_equal(brute_expand(recs, stream, k).astype(np.int64), E.pairs), "%s: records" % what
    if mode:
        assert ((recs["meta"] >> 16) == 1).sum() > 50, "%s: the fast path left no records" % what
    assert_segments(b.segments(), E.segments, what)
    assert_summaries(b.read_summaries(), E.summaries, what)
    assert_screen(b.screen(*SCREEN), E.screen, what)
    if lab is not None:
        assert_classes(b.classify(lab), E.classes, what)
    if col is not None:
        for pm in (0, 1000):
            assert_pseudo(b.pseudoalign(col, pm), E.rows[pm], "%s, permille %d" % (what, pm))


def test_the_torch_streams_are_non_blocking(w):
    """hipStreamGetFlags through the HIP runtime the process has loaded: its path is taken from /proc/self/maps, and there is exactly one"""
    fa.lib()
    with open("/proc/self/maps") as f:
        loaded = {line.split()[-1] for line in f if "libamdhip64.so" in line}
    assert len(loaded) == 1, "torch and the library must share one HIP runtime, found %s" % sorted(loaded)
    hip = C.CDLL(loaded.pop())
    hip.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
    for s in (w.S, w.T, w.U):
        flags = C.c_uint(0xFFFF)
        assert s.cuda_stream != 0 and hip.hipStreamGetFlags(C.c_void_p(s.cuda_stream), C.byref(flags)) == 0
        assert flags.value & 1, "not hipStreamNonBlocking"   # hipStreamNonBlocking = 0x01
    assert len({w.S.cuda_stream, w.T.cuda_stream, w.U.cuda_stream}) == 3


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_1_the_step_and_its_readers_on_a_user_stream(w, mode):
    lab, col = w.labels(), w.colors()
    b = w.primed(mode, lab, col)
    w.delay(w.S)
    b.run(stream=w.S.cuda_stream)
    guard(w.S)
    check_products(w, b, w.B, mode, lab, col, "k=%d mode %d on a user stream" % (w.k, mode))
    b.close(); lab.close(); col.close()


@pytest.mark.parametrize("kernel", [3, 2, 0])
def test_1_the_other_kernels_on_a_user_stream(w, kernel):
    w.p.set_option("kernel", kernel)
    try:
        b = w.p.batch(w.A.reads)
        b.run()
        assert np.array_equal(b.download()[0].astype(np.int64), w.A.pairs) and b.run_info()["kernel"] == kernel
        b.reload(w.B.reads)
        w.delay(w.S)
        b.run(stream=w.S.cuda_stream)
        guard(w.S)
        pairs, npos = b.download()
        assert np.array_equal(pairs.astype(np.int64), w.B.pairs) and npos == w.B.found and b.run_info()["kernel"] == kernel
        b.close()
    finally:
        w.p.set_option("kernel", None)


@pytest.mark.parametrize("overlap", [1, 0])
def test_2_the_side_stream_of_the_prefill(w, overlap):
    """kernel 4 with a prefilled output.  overlap_prefill 1: the (-1,-1) fill runs on the batch's side stream beside ingest and pre-pass, and the pipeline's
    first writer waits for it (ev_join).  By itself the fill is over long before the pre-pass, so the join would never decide anything: the test puts a delay
    of twice the launch stream's on the side stream (fin_batch_debug_side_stream), in front of the fill.  A writer that does not wait writes B's pairs at
    one delay and has them wiped by the fill at two; the side stream is synchronised before the download so that the wipe, if there is one, is seen.  What
    this does NOT show is ev_fork: a fill that starts too early lands on A's stale pairs and B's still come out on top.  overlap_prefill 0: the fill is on the
    launch stream, in front of the step"""
    w.p.set_option("write_gaps", 0); w.p.set_option("overlap_prefill", overlap)
    try:
        b = w.p.batch(w.A.reads)
        b.run()
        assert np.array_equal(b.download()[0].astype(np.int64), w.A.pairs)
        b.reload(w.B.reads)
        side = torch.cuda.ExternalStream(b.debug_side_stream()) if overlap else None
        w.delay(w.S)
        if overlap:
            w.delay(side, 2)
        b.run(stream=w.S.cuda_stream)
        guard(w.S)
        if overlap:
            guard(side)
            side.synchronize()
        pairs, npos = b.download()
        info = b.run_info()
        assert info["kernel"] == 4 and not info["no_prefill"], "the run did not prefill"
        bad = np.nonzero((pairs.astype(np.int64) != w.B.pairs).any(axis=1))[0]
        assert len(bad) == 0 and npos == w.B.found, "%d pairs differ, first %d: got %s, oracle %s" % (len(bad), bad[0], pairs[bad[0]], w.B.pairs[bad[0]])
        b.close()
    finally:
        w.p.set_option("write_gaps", None); w.p.set_option("overlap_prefill", None)


@pytest.mark.parametrize("mode", [0, 2])
def test_3_adds_on_another_stream_than_the_run(w, mode):
    """run on S behind the delay, every add on T: the add waits for the run's last event.  Labels.add makes the classes first, which needs the run's overflow
    verdict on the host: it is the one add that waits for the run (include/finito_amd.h), so it comes after the guard and the downloads, when the run is long
    over: for the labels this scenario checks the result of two adds on T (text modes 0 and 2) and NO ordering -- scenario 6 "behind_a_reader" does that"""
    B = w.B
    lab = w.labels()
    b = w.primed(mode, lab)
    hits, cover, depth, col, T = w.p.hits(), w.p.cover(), w.p.depth(), w.colors(bits=False), w.T.cuda_stream
    w.delay(w.S)
    b.run(stream=w.S.cuda_stream)
    hits.add(b, stream=T).add(b, stream=T)
    cover.add(b, stream=T).add(b, stream=T)
    depth.add(b, stream=T).add(b, stream=T)
    col.add(b, ADDED_COLOR, stream=T).add(b, ADDED_COLOR, stream=T)
    guard(w.S)
    counts, total = hits.download()
    assert_profile(counts, total, 2 * B.profile, "hits added twice on T")
    assert_cover(cover.download(), B.cover, "cover added twice on T")
    assert_depth(depth.download(), B.depth.times(2), "depth added twice on T")
    bits, n_set = col.download()
    assert np.array_equal(bits, B.painted) and n_set == int(B.profile.astype(bool).sum()), "colours added on T"
    lab.add(b, stream=T).add(b, stream=T)
    tally, total = lab.download()
    assert np.array_equal(tally, 2 * B.tally) and total == 2 * len(B.reads), "tally added twice on T: got %s, want %s" % (tally, 2 * B.tally)
    if mode == 0:   # the adds read only
        assert np.array_equal(b.download()[0].astype(np.int64), B.pairs)
    assert b.text() == B.text
    for x in (b, hits, cover, depth, col, lab):
        x.close()


@pytest.mark.parametrize("what", ["hits", "cover", "depth", "labels", "colors"])
def test_4_reset_and_add_behind_a_delay_and_the_download_waits_for_every_stream(w, what):
    """the accumulator holds A.  T: a long delay, reset, add(b).  U: a short delay, add(b2).  The add on U is issued after the reset and so counts behind it
    although its own stream is free earlier; the download waits for both streams.  Nothing of A is left, both adds are there"""
    A, B, G = w.A, w.B, w.bigger
    lab = w.labels()
    ba, b, b2 = w.p.batch(A.reads), w.p.batch(B.reads), w.p.batch(G.reads)
    for x in (ba, b, b2):
        x.run(); x.classify(lab)   # runs that have finished; their classes are made (Labels.add would wait to make them)
    torch.cuda.synchronize()
    T, U = w.T.cuda_stream, w.U.cuda_stream
    add = lambda x, s=None, color=None: acc.add(x, stream=s)
    if what == "hits":
        acc = w.p.hits()
        check = lambda want, msg: assert_profile(*acc.download(), want, msg)
        of_a, both = A.profile, B.profile + G.profile
    elif what == "cover":
        acc = w.p.cover()
        check = lambda want, msg: assert_cover(acc.download(), want, msg)
        of_a, both = A.cover, B.cover | G.cover
        assert (A.cover.bits & ~both.bits).any() and (G.cover.bits & ~B.cover.bits).any()
    elif what == "depth":
        acc = w.p.depth()
        check = lambda want, msg: assert_depth(acc.download(), want, msg)
        of_a, both = A.depth, B.depth + G.depth
    elif what == "labels":
        acc = lab
        def check(want, msg):
            tally, total = acc.download()
            assert np.array_equal(tally, want) and total == int(want.sum()), "%s: got %s, want %s" % (msg, tally, want)
        of_a, both = A.tally, B.tally + G.tally
    else:   # (600 reads touch nearly every unitig: each batch paints a colour of its own, so that every one of the three adds shows)
        acc = w.colors(bits=False)
        add = lambda x, s=None, color=None: acc.add(x, color, stream=s)
        check = lambda want, msg: np.testing.assert_array_equal(acc.download()[0], want, msg)
        def painted(E, color):
            m = np.zeros((len(E.painted), N_COLORS), dtype=np.uint8); m[:, color] = unpack(E.painted, N_COLORS)[:, ADDED_COLOR]
            return pack_members(m)
        of_a, both = painted(A, 0), painted(B, ADDED_COLOR) | painted(G, 1)
    add(ba, None, 0)
    check(of_a, "%s filled from A" % what)
    w.delay(w.T, 2)
    acc.reset(stream=T)
    add(b, T, ADDED_COLOR)
    w.delay(w.U, 1)
    add(b2, U, 1)
    guard(w.T, w.U)
    check(both, "%s after reset + add on T and add on U" % what)
    for x in {ba, b, b2, acc, lab}:   # (for the labels, acc is lab)
        x.close()


def test_5_pseudoalignment_behind_pending_colour_adds(w):
    """the matrix gets colour ADDED_COLOR from b1's run, on T behind a delay; b2, whose run was on S, is pseudoaligned at once: its kernel runs on S behind T's add"""
    A, B = w.A, w.B
    col = w.colors()
    b1 = w.p.batch(A.reads); b1.run()
    b2 = w.primed(0, None, col)
    b2.run(stream=w.S.cuda_stream)
    torch.cuda.synchronize()
    final = w.c.bits | A.painted
    w.delay(w.T)
    col.add(b1, ADDED_COLOR, stream=w.T.cuda_stream)
    guard(w.T)
    for pm in (0, 1000):
        assert_pseudo(b2.pseudoalign(col, pm), rows_of(B.pairs, B.nks, final, N_COLORS, pm), "rows behind a pending add, permille %d" % pm)
    assert np.array_equal(col.download()[0], final)
    b1.close(); b2.close(); col.close()


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("verdict_known", [False, True], ids=["first_reader", "behind_a_reader"])
def test_6_classes_made_once_tallied_from_another_stream(w, mode, verdict_known):
    """Labels.add(b, stream=T) makes the classes on the run's stream S and tallies on T behind an event recorded on S; a second add on U finds the classes made
    and waits for them the same way.  Making the classes needs the run's overflow verdict, which is a host decision: as the first reader of a run the add waits
    for it (include/finito_amd.h) -- then the guard sits in front of it.  Behind a reader that has fetched the verdict nothing waits: the classes are made
    behind a second delay on S, and a tally that does not wait for them counts A's classes"""
    B = w.B
    lab = w.labels()
    b = w.primed(mode, lab)
    S, T, U = w.S.cuda_stream, w.T.cuda_stream, w.U.cuda_stream
    w.delay(w.S)
    b.run(stream=S)
    guard(w.S)
    if verdict_known:
        recs, stream = b.records()   # (legal in every text mode)
        assert np.array_equal(brute_expand(recs, stream, w.k).astype(np.int64), B.pairs)
        assert b.device_read_classes_ptr() == 0
        w.delay(w.S)
    lab.add(b, stream=T)
    lab.add(b, stream=U)
    if verdict_known:
        guard(w.S)
    tally, total = lab.download()
    assert np.array_equal(tally, 2 * B.tally) and total == 2 * len(B.reads), "got %s, want %s" % (tally, 2 * B.tally)
    assert_classes(b.classify(lab), B.classes, "the classes after the adds")
    b.close(); lab.close()


def test_7_reload_behind_a_run_still_in_flight(w):
    """a reload waits for the run on the user stream before it overwrites (and, growing, frees) what that run reads"""
    G = w.bigger
    b = w.p.batch(w.B.reads)
    w.delay(w.S)
    b.run(stream=w.S.cuda_stream)
    guard(w.S)
    b.reload(G.reads)
    assert w.S.query() is True, "the reload returned while the run it replaces was still queued"
    b.run()
    pairs, npos = b.download()
    assert np.array_equal(pairs.astype(np.int64), G.pairs) and npos == G.found
    b.close()


def test_8_step_time_on_a_user_stream(w):
    """the events bracket the step, not what was queued in front of it"""
    b = w.p.batch(w.B.reads)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(w.S)
    w.delay(w.S)
    e1.record(w.S)
    for _ in range(3):
        b.run(stream=w.S.cuda_stream)
    guard(w.S)
    w.S.synchronize()
    waited = e0.elapsed_time(e1)
    step, n = b.step_time_ms(skip_first=1)
    print("delay %.2f ms measured, step %.3f ms" % (waited, step["step"]))
    assert n == 2 and 0 < step["step"] < waited and waited >= 0.5 * w.delay_ms
    assert np.array_equal(b.download()[0].astype(np.int64), w.B.pairs)
    b.close()


def test_9_partitioned_batch(w):
    L = fa.lib()
    ps = fa.PartitionedIndex(w.c.unitigs, w.k, device=0, max_part_bases=12000)
    assert int(L.fin_pindex_parts(ps.h)) >= 3
    pb = ps.batch(w.A.reads)
    pb.run()
    assert np.array_equal(pb.download()[0].astype(np.int64), w.A.pairs)
    bases, offsets = fa.flatten(w.B.reads)
    err = C.create_string_buffer(512)
    assert L.fin_pbatch_reload(pb.h, bases.ctypes.data_as(C.c_char_p), offsets.ctypes.data_as(C.POINTER(C.c_uint64)), len(offsets) - 1, err, 512) == 0, err.value
    w.delay(w.S)
    pb.run(stream=w.S.cuda_stream)
    guard(w.S)
    pairs, npos = pb.download()
    assert np.array_equal(pairs.astype(np.int64), w.B.pairs) and npos == w.B.found
    pb.close(); ps.close()


def test_10_the_host_buffer_pipelines_while_user_streams_are_busy(w):
    A, B = w.A, w.B
    col = w.colors()
    b = w.primed(0)
    w.delay(w.S)
    b.run(stream=w.S.cuda_stream)
    guard(w.S)
    got, npos = w.p.search_reads(A.reads)
    assert np.array_equal(got.astype(np.int64), A.pairs) and npos == A.found
    counts, npos = w.p.unitig_counts(A.reads)
    assert np.array_equal(counts, A.profile) and npos == A.found
    rows, heads, npos = w.p.pseudoalign_reads(A.reads, col)
    assert_pseudo((rows, heads), A.rows[1000], "host buffers beside a busy stream")
    pairs, npos = b.download()
    assert np.array_equal(pairs.astype(np.int64), B.pairs) and npos == B.found
    b.close(); col.close()
