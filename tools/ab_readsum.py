#!/usr/bin/env python3
"""What the per-read summaries and the screen cost on the device (fin_batch_read_summaries, fin_batch_screen; fin_readsum.hip), against the cheapest other route
to the same numbers: segments + a reduction on the host -- `python3 tools/ab_readsum.py [workload] [--reads N] [--steps S] [--sets M]`.

The workload is built the way bench.py builds it (same seeds, same sizes; default chr1); the method is tools/ab_depth.py's: HIP events on one stream, the
variants interleaved in one process, text mode 2.

  1. steps 1..S over M sets of FRESH reads (another seed per set, reloaded in turn), each step followed by, each timed by itself with HIP events:
     fin_batch_read_summaries | fin_batch_screen behind it (bits + count + ids; includes its wait for the count) | fin_batch_segments (count + scan + write;
     includes its wait for the count); and, host wall clock: the summaries' download | the segments' download + the numpy reduction to the same four numbers.
     The reduction's result must equal the device's summaries.  Medians over the steps, bytes to the host per read.
  2. from pinned host buffers, k-mers/s: search_reads_summaries | screen_reads | search_reads_segments + the reduction
"""
import argparse
import ctypes as C
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


def reduce_segments(seg_offs, segs, n_reads):
    """the four numbers of a read summary from its segments, in numpy"""
    out = np.zeros(n_reads, dtype=fa.READ_SUMMARY_DTYPE)
    so = seg_offs.astype(np.int64)
    n = np.diff(so)
    out["n_segments"] = n
    has = n > 0
    if len(segs):
        n_abs = np.abs(segs["len"].astype(np.int64))
        first = so[:-1][has]
        out["n_found"][has] = np.add.reduceat(n_abs, first)
        out["longest"][has] = np.maximum.reduceat(n_abs, first)
        last = so[1:][has] - 1
        out["span"][has] = segs["slot"].astype(np.int64)[last] + n_abs[last] - segs["slot"].astype(np.int64)[first]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="chr1", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--no-host", action="store_true", help="skip leg 2")
    a = ap.parse_args()
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    n_reads = a.reads or n_reads
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    sets = [synth.reads(g, n_reads, read_len=read_len, seed=synth.SEED_READS + 1000 * s) for s in range(a.sets)]
    batch = idx.batch(sets[0].as_tuple())
    print("workload %s: %d unitigs, %d bases, %d reads per step, %d k-mers, set up in %.1f s" % (a.workload, idx.n_unitigs, idx.total_len, n_reads, batch.n_kmers, time.time() - t0), flush=True)
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    L = fa.lib()
    err = C.create_string_buffer(512)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ts); rc = f(); e1.record(ts); torch.cuda.synchronize()
        assert rc == 0, err.value
        return e0.elapsed_time(e1)

    n_pass, n_seg = C.c_uint64(0), C.c_uint64(0)
    ways = [("summaries", lambda: L.fin_batch_read_summaries(batch.h, err, 512)),
            ("screen", lambda: L.fin_batch_screen(batch.h, 1, 500, 0, C.byref(n_pass), err, 512)),
            ("segments", lambda: L.fin_batch_segments(batch.h, C.byref(n_seg), err, 512))]
    t = {name: [] for name, _ in ways}
    t_step, t_dl_sum, t_dl_seg, t_reduce = [], [], [], []
    batch.text_mode(2)
    for s in range(a.steps + 1):   # (step 0: a first launch of every kernel, not counted)
        batch.reload(sets[s % a.sets].as_tuple())
        ms = timed(lambda: batch.run(fa.FIN_MERGED, stream) or 0)
        order = ways[s % 3:] + ways[:s % 3]   # (interleaved: each goes first, second and third in turn; the screen finds the summaries made or makes them)
        got = {}
        for name, f in order:
            if name == "screen":   # (timed behind the summaries, not instead of them)
                assert L.fin_batch_read_summaries(batch.h, err, 512) == 0
                torch.cuda.synchronize()
            got[name] = timed(f)
        w0 = time.perf_counter(); summ = batch.read_summaries(); w1 = time.perf_counter()
        seg_offs, segs = batch.segments(); w2 = time.perf_counter()
        red = reduce_segments(seg_offs, segs, n_reads); w3 = time.perf_counter()
        assert np.array_equal(red, summ), "the reduction of the segments differs from the device's summaries"
        if s == 0:
            continue
        t_step.append(ms)
        for name, _ in ways:
            t[name].append(got[name])
        t_dl_sum.append(1e3 * (w1 - w0)); t_dl_seg.append(1e3 * (w2 - w1)); t_reduce.append(1e3 * (w3 - w2))
        print("step %d: step %.3f ms | summaries %.3f ms | screen %.3f ms | segments %.3f ms" % (s, ms, got["summaries"], got["screen"], got["segments"]), flush=True)
    print("medians over %d steps, text mode 2: step %s" % (a.steps, med(t_step)))
    for name, _ in ways:
        print("  fin_batch_%-16s %s" % (name + ":", med(t[name])))
    print("  host wall clock: summaries made + downloaded %s | segments made + downloaded %s | numpy reduction %s" % (med(t_dl_sum), med(t_dl_seg), med(t_reduce)))
    print("  bytes to the host per read: summaries 16 | screen bits %.3f, ids %.3f (%d of %d reads pass min_found 1, min_permille 500) | segments %.1f (%d segments)"
          % (1 / 8, 4 * n_pass.value / n_reads, n_pass.value, n_reads, (16 * n_seg.value + 8 * (n_reads + 1)) / n_reads, n_seg.value), flush=True)
    if not a.no_host:
        ns = min(n_reads, 2_000_000)
        sub = sets[0].subset(0, ns)
        pin = fa.PinnedArray((ns * read_len,), np.uint8)
        pin.array[:] = sub.bases
        rd = (pin.array, sub.offsets)
        nk = ns * max(0, read_len - k + 1)

        def by_segments():
            so, sg, _ = idx.search_reads_segments(rd)
            return reduce_segments(so, sg, ns)
        host = (("search_reads_summaries", lambda: idx.search_reads_summaries(rd)[0]), ("screen_reads", lambda: idx.screen_reads(rd, 1, 500)),
                ("search_reads_segments + reduction", by_segments))
        tw = {n: [] for n, _ in host}
        outs = {}
        for rnd in range(6):
            for name, f in host:
                w = time.perf_counter(); outs[name] = f(); dt = time.perf_counter() - w
                if rnd:
                    tw[name].append(dt)
        assert np.array_equal(outs["search_reads_summaries"], outs["search_reads_segments + reduction"])
        for name, _ in host:
            print("host buffers, %-36s %.3e k-mers/s (median of %d, %d reads)" % (name + ":", nk / statistics.median(tw[name]), len(tw[name]), ns), flush=True)
        pin.close()
    batch.close()


if __name__ == "__main__":
    main()
