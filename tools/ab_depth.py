#!/usr/bin/env python3
"""What the per-position depth costs on the device (fin_batch_add_depth, fin_depth_download; fin_depth.hip) -- `python3 tools/ab_depth.py [workload] [--reads N] [--steps S]`.

The workload is built the way bench.py builds it (same seeds, same sizes; default chr1); the method is tools/ab_cover.py's: HIP events on one stream, the
variants interleaved in one process.

  1. steps 1..S of FRESH reads (another seed per step) behind a text-mode-2 step and behind a default (mode 0) step, each followed by three adds, each timed by
     itself: fin_batch_add_depth, and the siblings fin_batch_add_cover and fin_batch_add_hits behind the same step as the yardsticks; medians over the steps
  2. fin_depth_download, host wall clock: the prefix sum + statistics with only the statistics coming back, and with the depths too
  3. from pinned host buffers, k-mers/s: unitig_depth | unitig_coverage | unitig_counts
  --one-step: three mode-2 and three mode-0 steps with their adds, one download, and nothing else (for a kernel trace)
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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip leg 3")
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

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ts); f(); e1.record(ts); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    d, c, h = idx.depth(), idx.cover(), idx.hits()
    if a.one_step:
        for mode in (2, 0):
            batch.text_mode(mode)
            for _ in range(3):
                batch.run(fa.FIN_MERGED, stream); h.add(batch, stream); c.add(batch, stream); d.add(batch, stream)
        print("three mode-2 and three mode-0 steps + adds done; found %d" % d.download(want_positions=False)[2])
        return
    for mode in (2, 0):
        d.reset(stream); c.reset(stream); h.reset(stream)
        td, tc, th = [], [], []
        for s in range(a.steps):
            if s or mode == 0:
                batch.reload(sets[s].as_tuple())
            batch.text_mode(mode)
            t_step = timed(lambda: batch.run(fa.FIN_MERGED, stream))
            if s == 0:   # (a first launch of each kernel, not timed: into accumulators that are thrown away)
                w = (idx.depth(), idx.cover(), idx.hits())
                for x in w:
                    x.add(batch, stream)
                torch.cuda.synchronize()
                for x in w:
                    x.close()
            order = [("depth", d, td), ("cover", c, tc), ("hits", h, th)]
            order = order[s % 3:] + order[:s % 3]   # (interleaved: each goes first, second and third in turn)
            got = {}
            for name, acc, out in order:
                got[name] = timed(lambda: acc.add(batch, stream)); out.append(got[name])
            print("mode %d, step %d: step %.3f ms | add_depth %.3f ms | add_cover %.3f ms | add_hits %.3f ms" % (mode, s + 1, t_step, got["depth"], got["cover"], got["hits"]), flush=True)
        print("mode %d, medians over %d steps: add_depth %s | add_cover %s | add_hits %s" % (mode, a.steps, med(td), med(tc), med(th)), flush=True)
        stats, tot = d.download(want_positions=False)[1:]
        counts, tot_h = h.download()
        cov = c.download()[1]
        assert np.array_equal(stats["sum"], counts) and tot == tot_h and np.array_equal(stats["n_at_least"].astype(np.uint64), cov)
        print("mode %d: found %d, greatest depth %d, positions found at least once %d, at least 5 times %d"
              % (mode, tot, int(stats["max"].max()), int(stats["n_at_least"].sum()), int(d.download(min_depth=5, want_positions=False)[1]["n_at_least"].sum())), flush=True)
    ta, tb = [], []
    for _ in range(6):
        t = time.perf_counter(); d.download(want_positions=False); ta.append(1e3 * (time.perf_counter() - t))
    pin = fa.PinnedArray((idx.total_len,), np.uint32)
    import ctypes as C
    err = C.create_string_buffer(512)
    for _ in range(4):
        t = time.perf_counter()
        rc = fa.lib().fin_depth_download(d.h, 1, pin.array.ctypes.data_as(C.c_void_p), None, None, err, 512)
        tb.append(1e3 * (time.perf_counter() - t))
        assert rc == 0
    print("fin_depth_download over %d positions, host wall clock: prefix sum + statistics, %d bytes back %s | prefix sum + the depths into page-locked memory %s"
          % (idx.total_len, 16 * idx.n_unitigs, med(ta[1:]), med(tb[1:])), flush=True)
    pin.close()
    if not a.no_host:
        ns = min(n_reads, 2_000_000)
        sub = sets[0].subset(0, ns)
        pin = fa.PinnedArray((ns * read_len,), np.uint8)
        pin.array[:] = sub.bases
        rd = (pin.array, sub.offsets)
        nk = ns * max(0, read_len - k + 1)
        ways = (("unitig_depth", lambda: idx.unitig_depth(rd)[0]["n_at_least"].astype(np.uint64)), ("unitig_coverage", lambda: idx.unitig_coverage(rd)[0]),
                ("unitig_counts", lambda: idx.unitig_counts(rd)[0]))
        tw = {n: [] for n, _ in ways}
        outs = {}
        for rnd in range(6):
            for name, f in ways:
                t = time.perf_counter(); outs[name] = f(); dt = time.perf_counter() - t
                if rnd:
                    tw[name].append(dt)
        assert np.array_equal(outs["unitig_depth"], outs["unitig_coverage"])
        for name, _ in ways:
            print("host buffers, %-18s %.3e k-mers/s (median of %d, %d reads)" % (name + ":", nk / statistics.median(tw[name]), len(tw[name]), ns), flush=True)
        pin.close()
    batch.close(); d.close(); c.close(); h.close()


if __name__ == "__main__":
    main()
