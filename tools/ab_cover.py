#!/usr/bin/env python3
"""What the coverage bitmap costs on the device (fin_batch_add_cover, fin_cover.hip) -- `python3 tools/ab_cover.py [workload] [--reads N] [--rounds R]`.

The workload is built the way bench.py builds it (same seeds, same sizes; default chr1); the method is tools/ab_hits.py's: HIP events on one stream, the
variants interleaved in one process.  Every step is followed by four adds, each timed by itself: cover with cover_probe 0 and 1, each into an accumulator of
its own (so both see the same bitmap state), the sibling fin_batch_add_hits behind the same step as the yardstick, and cover_probe 1 once more into the
accumulator it has just filled (what a bitmap that holds this very step costs).

  1. steps 1..4 of FRESH reads (another seed per step) behind a text-mode-2 step and behind a default (mode 0) step: the bitmap is empty at step 1 and
     saturated by step 4; the default of cover_probe is whichever sum over the four steps is smaller
  2. fin_cover_download's count kernel (the download with and without the covered numbers)
  3. from pinned host buffers, k-mers/s: unitig_coverage at the option's default, with cover_probe 0 and with 1 | unitig_counts | search_reads + np.unique on the host
  4. contention: an index of 1 and of 3 unitigs, 200 000 reads each, cover_probe 0 / 1, empty and saturated
  --one-step: three mode-2 steps with their adds and nothing else (for a kernel trace)
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
import finito_amd as fa
from finito_amd import synth


def med(xs):
    return "%.3f ms (%.3f..%.3f, n=%d)" % (statistics.median(xs), min(xs), max(xs), len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="chr1", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-host", action="store_true", help="skip leg 3")
    ap.add_argument("--no-contention", action="store_true", help="skip leg 4")
    ap.add_argument("--one-step", action="store_true")
    a = ap.parse_args()
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    n_reads = a.reads or n_reads
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    sets = [synth.reads(g, n_reads, read_len=read_len, seed=synth.SEED_READS + 1000 * s) for s in range(a.steps)]
    batch = idx.batch(sets[0].as_tuple())
    print("workload %s: %d unitigs, %d bases, %d reads per step, %d k-mers, depth %.1fx per step, set up in %.1f s"
          % (a.workload, idx.n_unitigs, idx.total_len, n_reads, batch.n_kmers, n_reads * read_len / idx.total_len, time.time() - t0), flush=True)
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def timed(f):
        e0, e1 = ev(), ev()
        e0.record(ts); f(); e1.record(ts); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def add_cover(acc, probe, b=batch, ix=idx):
        ix.set_option("cover_probe", probe)
        t = timed(lambda: acc.add(b, stream))
        ix.set_option("cover_probe", None)
        return t

    hits = idx.hits()
    if a.one_step:
        c = idx.cover()
        batch.text_mode(2)
        for _ in range(3):
            batch.run(fa.FIN_MERGED, stream); hits.add(batch, stream); c.add(batch, stream)
        print("three mode-2 steps + adds done; covered %d" % c.download()[2])
        return
    for mode in (2, 0):
        c0, c1 = idx.cover(), idx.cover()
        sums = {"probe 0": 0.0, "probe 1": 0.0, "hits": 0.0}
        for s in range(a.steps):
            if s or mode == 0:
                batch.reload(sets[s].as_tuple())
            batch.text_mode(mode)
            t_step = timed(lambda: batch.run(fa.FIN_MERGED, stream))
            if s == 0:   # (a first launch of each kernel, not timed: into accumulators that are thrown away)
                w = idx.cover(); add_cover(w, 0); add_cover(w, 1); w.close(); hits.add(batch, stream)
            t0_ = add_cover(c0, 0)
            t1_ = add_cover(c1, 1)
            th = timed(lambda: hits.add(batch, stream))
            t1b = add_cover(c1, 1)
            b0, cov0, tot0 = c0.download(); b1, cov1, tot1 = c1.download()
            assert np.array_equal(b0, b1) and np.array_equal(cov0, cov1)
            sums["probe 0"] += t0_; sums["probe 1"] += t1_; sums["hits"] += th
            print("mode %d, step %d: step %.3f ms | add_cover probe 0: %.3f ms, probe 1: %.3f ms | add_hits: %.3f ms | probe 1 again (full): %.3f ms | covered %d of %d k-mers (%.1f %%)"
                  % (mode, s + 1, t_step, t0_, t1_, th, t1b, tot0, idx.n_kmers, 100.0 * tot0 / idx.n_kmers), flush=True)
        print("mode %d, sum over %d steps: probe 0 %.3f ms, probe 1 %.3f ms, add_hits %.3f ms" % (mode, a.steps, sums["probe 0"], sums["probe 1"], sums["hits"]), flush=True)
        if mode == 0:
            td, tb = [], []
            for _ in range(4):
                t = time.perf_counter(); c0.download(); td.append(1e3 * (time.perf_counter() - t))
            L = fa.lib()
            import ctypes as C
            err = C.create_string_buffer(512)
            cov = np.zeros(idx.n_unitigs, dtype=np.uint64)
            for _ in range(4):
                t = time.perf_counter()
                L.fin_cover_download(c0.h, None, cov.ctypes.data_as(C.POINTER(C.c_uint64)), None, err, 512)
                tb.append(1e3 * (time.perf_counter() - t))
            print("fin_cover_download, host wall clock: bits + covered %s | covered only (count kernel + %d bytes back) %s" % (med(td[1:]), 8 * idx.n_unitigs, med(tb[1:])), flush=True)
        c0.close(); c1.close()
    if not a.no_host:
        ns = min(n_reads, 2_000_000)
        sub = sets[0].subset(0, ns)
        pin = fa.PinnedArray((ns * read_len,), np.uint8)
        pin.array[:] = sub.bases
        rd = (pin.array, sub.offsets)
        nk = ns * max(0, read_len - k + 1)
        pout = fa.PinnedArray((max(nk, 1), 2), np.int32)
        ends = idx.export(fa.X_ENDS)
        starts = np.concatenate([[0], ends[:-1]])

        def host_cover():   # (the option's committed default)
            return idx.unitig_coverage(rd)[0]

        def host_cover_probe(v):
            def f():
                idx.set_option("cover_probe", v)
                try:
                    return idx.unitig_coverage(rd)[0]
                finally:
                    idx.set_option("cover_probe", None)
            return f

        def host_counts():
            return idx.unitig_counts(rd)[0]

        def host_pairs():
            pairs, _ = idx.search_reads(rd, fa.FIN_MERGED, out=pout.array)
            uu = pairs[:, 0]
            f = uu >= 0
            gpos = np.unique(starts[uu[f]] + pairs[f, 1])
            return np.bincount(np.searchsorted(ends, gpos, side="right"), minlength=idx.n_unitigs).astype(np.uint64)

        ways = (("unitig_coverage", host_cover), ("unitig_coverage, cover_probe 0", host_cover_probe(0)), ("unitig_coverage, cover_probe 1", host_cover_probe(1)),
                ("unitig_counts", host_counts), ("search_reads + np.unique", host_pairs))
        tw = {n: [] for n, _ in ways}
        outs = {}
        for rnd in range(4):
            for name, f in ways:
                t = time.perf_counter(); outs[name] = f(); dt = time.perf_counter() - t
                if rnd:
                    tw[name].append(dt)
        for name, _ in ways[:3]:
            assert np.array_equal(outs[name], outs["search_reads + np.unique"]), name
        for name, _ in ways:
            print("host buffers, %-34s %.3e k-mers/s (median of %d, %d reads)" % (name + ":", nk / statistics.median(tw[name]), len(tw[name]), ns), flush=True)
        pin.close(); pout.close()
    batch.close()
    if not a.no_contention:
        for nu in (1, 3):
            gg = synth.genome(30000, seed=7 + nu)
            gs = gg.tobytes().decode()
            cuts = [0, len(gs)] if nu == 1 else [0, 9000, 21000, len(gs)]
            small = fa.FinimizerIndex.build([gs[max(0, x - 30) if x else 0:y] for x, y in zip(cuts[:-1], cuts[1:])], 31).to_device(0)
            rd = synth.reads(gg, 200_000, seed=11)
            b = small.batch(rd.as_tuple())
            c = small.cover(); h = small.hits()
            for mode in (2, 0):
                b.text_mode(mode); b.run(fa.FIN_MERGED, stream)
                th = [timed(lambda: h.add(b, stream)) for _ in range(6)][1:]
                for probe in (0, 1):
                    empty, full = [], []
                    for rnd in range(6):
                        c.reset(stream)
                        e = add_cover(c, probe, b, small); f = add_cover(c, probe, b, small)
                        if rnd:
                            empty.append(e); full.append(f)
                    print("contention: %d unitig(s), 200000 reads, mode %d, cover_probe %d: into an empty bitmap %s, into a full one %s | add_hits %s | covered %d"
                          % (nu, mode, probe, med(empty), med(full), med(th), c.download()[2]), flush=True)
            c.close(); h.close(); b.close(); small.close()


if __name__ == "__main__":
    main()
