#!/usr/bin/env python3
"""What results as segments cost (fin_batch_segments, fin_segments.hip) -- `python3 tools/ab_segments.py [workload] [--reads N] [--modes 2,0] [--no-host]`.

The workload is built the way bench.py builds it (same seeds, same sizes; default chr1); the method is tools/ab_cover.py's: HIP events on one stream, the
variants interleaved in one process.  On a library that has no fin_batch_segments (the parent commit) only the fin_batch_records / search_reads legs run, so the
same script gives the parent's side of the comparison.

  1. behind a step in each text mode: fin_batch_segments and fin_batch_records, each bracketed by events (both wait for their count on the host: the bracket
     holds the kernels and that round trip, not the download)
  2. from pinned host buffers, k-mers/s: search_reads_segments | search_reads_records | search_reads
  3. bytes returned per read: 16 * n_segments + 8 * (n_reads + 1) against 32 * n_reads + 8 * stream_pairs (and 8 per k-mer for the pairs)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="chr1", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--modes", default="2,0")
    ap.add_argument("--no-host", action="store_true", help="skip leg 2")
    a = ap.parse_args()
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    n_reads = a.reads or n_reads
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    reads = synth.reads(g, n_reads, read_len=read_len, seed=synth.SEED_READS)
    batch = idx.batch(reads.as_tuple())
    L = fa.lib()
    have = hasattr(L, "fin_batch_segments")
    L.fin_batch_records.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
    print("workload %s: %d unitigs, %d bases, %d reads, %d k-mers, set up in %.1f s; segments: %s"
          % (a.workload, idx.n_unitigs, idx.total_len, n_reads, batch.n_kmers, time.time() - t0, "yes" if have else "no (records only)"), flush=True)
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    err = C.create_string_buffer(512)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ts); f(); e1.record(ts); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for mode in [int(m) for m in a.modes.split(",")]:
        batch.text_mode(mode)
        t_step, t_seg, t_rec = [], [], []
        n_seg, n_str = C.c_uint64(0), C.c_uint64(0)
        def call(f, out):
            rc = f(batch.h, C.byref(out), err, 512)
            if rc != 0:
                raise fa.FinitoError(rc, err.value.decode(errors="replace"))

        for rnd in range(a.rounds + 1):
            ts_ = timed(lambda: batch.run(fa.FIN_MERGED, stream))
            # (whichever comes second finds records and pairs warmer in the caches: the order alternates; the parent's records leg is the clean one)
            tg = tr = 0.0
            for what in (("seg", "rec") if rnd % 2 else ("rec", "seg")):
                if what == "seg" and have:
                    tg = timed(lambda: call(L.fin_batch_segments, n_seg))
                elif what == "rec":
                    tr = timed(lambda: call(L.fin_batch_records, n_str))
            if rnd:   # (the first launch of each kernel is not counted)
                t_step.append(ts_); t_seg.append(tg); t_rec.append(tr)
        info = batch.run_info()
        print("mode %d (fast path %d): step %s | fin_batch_segments %s | fin_batch_records %s" % (mode, info["fast_path"], med(t_step), med(t_seg), med(t_rec)), flush=True)
        print("mode %d: fin_batch_segments first / second behind the step: %s / %s" % (mode, med(t_seg[1::2]) if have and t_seg[1::2] else "-", med(t_seg[0::2]) if have else "-"), flush=True)
        seg_bytes = 16 * n_seg.value + 8 * (n_reads + 1)
        rec_bytes = 32 * n_reads + 8 * n_str.value
        print("mode %d: %d segments (%.2f per read), %d stream pairs | bytes per read: segments %.1f, records + stream %.1f, pairs %.1f"
              % (mode, n_seg.value, n_seg.value / n_reads, n_str.value, seg_bytes / n_reads, rec_bytes / n_reads, 8.0 * batch.n_kmers / n_reads), flush=True)
    batch.close()
    if not a.no_host:
        ns = min(n_reads, 2_000_000)
        sub = reads.subset(0, ns)
        pin = fa.PinnedArray((ns * read_len,), np.uint8)
        pin.array[:] = sub.bases
        rd = (pin.array, sub.offsets)
        nk = ns * max(0, read_len - k + 1)
        pout = fa.PinnedArray((max(nk, 1), 2), np.int32)
        ways = [("search_reads_records", lambda: idx.search_reads_records(rd)), ("search_reads", lambda: idx.search_reads(rd, fa.FIN_MERGED, out=pout.array))]
        if have:
            ways.insert(0, ("search_reads_segments", lambda: idx.search_reads_segments(rd)))
        tw = {n: [] for n, _ in ways}
        for rnd in range(4):
            for name, f in ways:
                t = time.perf_counter(); f(); dt = time.perf_counter() - t
                if rnd:
                    tw[name].append(dt)
        for name, _ in ways:
            print("host buffers, %-24s %.3e k-mers/s (median of %d, %.3e..%.3e, %d reads)"
                  % (name + ":", nk / statistics.median(tw[name]), len(tw[name]), nk / max(tw[name]), nk / min(tw[name]), ns), flush=True)
        pin.close(); pout.close()
    idx.close()


if __name__ == "__main__":
    main()
