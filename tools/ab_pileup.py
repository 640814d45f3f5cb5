#!/usr/bin/env python3
"""What the base pileup costs on the device (fin_batch_add_pileup, fin_pileup_download, fin_pileup_call; fin_pileup.hip) -- `python3 tools/ab_pileup.py [workload] [--reads N] [--steps S]`.

The workload is built the way bench.py builds it (same seeds, same sizes; default chr1); the method is tools/ab_depth.py's: HIP events on one stream, the
variants interleaved in one process.

  1. steps 1..S of FRESH reads (another seed per step) behind a text-mode-2 step, each followed by two adds, each timed by itself: fin_batch_add_pileup, and
     fin_batch_add_depth behind the same step as the yardstick; the step itself is the text-only step; medians over the steps
  2. fin_pileup_call and fin_pileup_download, host wall clock
  3. the whole add_reads route from pinned host buffers next to the host route it replaces: the records downloaded (search_reads_records), then fin_records_pileup
     on 16 threads
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip leg 3")
    a = ap.parse_args()
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    n_reads = a.reads or n_reads
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    n_sets = min(a.steps, 4)   # (fresh reads, taken in turn: four sets bound the host memory)
    sets = [synth.reads(g, n_reads, read_len=read_len, seed=synth.SEED_READS + 1000 * s) for s in range(n_sets)]
    batch = idx.batch(sets[0].as_tuple())
    print("workload %s: %d unitigs, %d bases, %d reads per step, %d k-mers, depth %.1fx per step, set up in %.1f s"
          % (a.workload, idx.n_unitigs, idx.total_len, n_reads, batch.n_kmers, n_reads * read_len / idx.total_len, time.time() - t0), flush=True)
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ts); f(); e1.record(ts); torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    p, d = idx.pileup(), idx.depth()
    tp, td, tstep = [], [], []
    batch.text_mode(2)
    for s in range(a.steps + 1):   # (step 0: a first launch of each kernel, not counted)
        batch.reload(sets[s % n_sets].as_tuple())
        t_step = timed(lambda: batch.run(fa.FIN_MERGED, stream))
        order = [("pileup", p, tp), ("depth", d, td)]
        order = order[s % 2:] + order[:s % 2]   # (interleaved: each goes first and second in turn)
        got = {}
        for name, acc, out in order:
            got[name] = timed(lambda: acc.add(batch, stream))
            if s:
                out.append(got[name])
        if s:
            tstep.append(t_step)
        print("step %d: text-only step %.3f ms | add_pileup %.3f ms | add_depth %.3f ms" % (s, t_step, got["pileup"], got["depth"]), flush=True)
    print("medians over %d steps: text-only step %s | add_pileup %s | add_depth %s" % (a.steps, med(tstep), med(tp), med(td)), flush=True)
    info = batch.run_info(); fast = batch.pipeline_counts()[41]
    print("last step: fast path %s, %d of %d reads finished by it" % (info["fast_path"], fast, n_reads), flush=True)
    tc, tdl = [], []
    for _ in range(4):
        t = time.perf_counter(); v = p.call(2, 200); tc.append(1e3 * (time.perf_counter() - t))
    cover, alt, counters = None, None, None
    for _ in range(3):
        t = time.perf_counter(); cover, alt, counters = p.download(); tdl.append(1e3 * (time.perf_counter() - t))
    print("counters after %d steps: kept %d, not straight %d, off their unitig %d, too many mismatches %d" % ((a.steps + 1,) + tuple(int(x) for x in counters)), flush=True)
    print("fin_pileup_call(2, 200) over %d positions, host wall clock: %s, %d candidates (%d bytes back) | fin_pileup_download into pageable memory: %s (%d bytes back)"
          % (idx.total_len, med(tc[1:]), len(v), 32 * len(v), med(tdl[1:]), 20 * idx.total_len), flush=True)
    m = alt.max(axis=1)
    assert len(v) == int(((m >= 2) & (1000 * m.astype(np.int64) >= 200 * cover.astype(np.int64))).sum())
    if not a.no_host:
        ns = min(n_reads, 2_000_000)
        sub = sets[0].subset(0, ns)
        pin = fa.PinnedArray((ns * read_len,), np.uint8)
        pin.array[:] = sub.bases
        rd = (pin.array, sub.offsets)
        nk = ns * max(0, read_len - k + 1)
        ends, concat = idx.export(fa.X_ENDS), idx.export(fa.X_CONCAT)
        q = idx.pileup()
        t_dev, t_rec, t_host = [], [], []
        outs = {}
        for rnd in range(4):
            q.reset()
            t = time.perf_counter(); q.add_reads(rd); outs["device"] = q.call(2, 200); dt = time.perf_counter() - t
            t = time.perf_counter(); recs, strm = idx.search_reads_records(rd); dr = time.perf_counter() - t
            t = time.perf_counter(); hc, ha, hn = fa.records_pileup(recs, strm, k, rd, ends, concat, max_mismatch=8, n_threads=16); dh = time.perf_counter() - t
            if rnd:
                t_dev.append(dt); t_rec.append(dr); t_host.append(dh)
        dc, da, dn = q.download()
        assert np.array_equal(dc, hc) and np.array_equal(da, ha) and np.array_equal(dn, hn)
        print("host buffers, %d reads: add_reads + call %.3e k-mers/s | records downloaded %.3e k-mers/s, then fin_records_pileup on 16 threads %.3e k-mers/s, both %.3e k-mers/s (medians of %d)"
              % (ns, nk / statistics.median(t_dev), nk / statistics.median(t_rec), nk / statistics.median(t_host),
                 nk / (statistics.median(t_rec) + statistics.median(t_host)), len(t_dev)), flush=True)
        pin.close(); q.close()
    batch.close(); p.close(); d.close()


if __name__ == "__main__":
    main()
