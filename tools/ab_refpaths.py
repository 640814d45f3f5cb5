#!/usr/bin/env python3
"""What the reference coordinates cost on the device (fin_refpaths_depth, fin_refpaths_lift_variants; fin_refpaths.hip), against the route a user had before --
`python3 tools/ab_refpaths.py [workload] [--reads N] [--steps S] [--records R]`.

The workload is built the way bench.py builds it (same seeds, same sizes; default chr1: 250 Mbp, 10 M reads added to the depth and the pileup).  The references are
the genome itself cut into R records (default 64: about 3.9 Mbp each).  The pileup's reads are drawn without errors from a copy of the genome with one substitution planted every 5 000
bases, so that the candidates are many.  Every call measured here WAITS, so every number is host wall clock around the call, S repetitions (default 20), the routes
interleaved in one process; medians.

  fin_refpaths_depth at windows 1 and 1000                     | Depth.download() + RefPaths.download() + fin_segments_window_depth on 16 threads
  fin_refpaths_depth over ONE record of 1 000 bases            (what the call costs before it lifts anything: the scan, materialised)
  fin_refpaths_lift_variants over Pileup.call's candidates      | RefPaths.download() + fin_segments_lift_variants on 16 threads   (Pileup.call itself: both routes)
The twins' results must equal the device's.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import bench
import finito_amd as fa
from finito_amd import synth


def med(xs):
    return "%.1f ms (%.1f..%.1f, n=%d)" % (statistics.median(xs), min(xs), max(xs), len(xs))


def wall(f):
    t0 = time.perf_counter(); r = f(); return r, 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="chr1", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--records", type=int, default=64)
    a = ap.parse_args()
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    n_reads = a.reads or n_reads
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    ends = idx.export(fa.X_ENDS)
    cuts = np.linspace(0, len(g), a.records + 1).astype(np.uint64)
    rp = idx.ref_paths().add_reads((g, cuts))
    small = idx.ref_paths().add_reads((g[:1000], np.array([0, 1000], dtype=np.uint64)))
    d = idx.depth().add_reads(synth.reads(g, n_reads, read_len=read_len).as_tuple())
    planted = g.copy()
    at = np.arange(2500, len(g), 5000)
    code = np.zeros(256, dtype=np.uint8); code[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.frombuffer(b"CGTA", dtype=np.uint8)
    planted[at] = code[planted[at]]
    pl = idx.pileup().add_reads(synth.reads(planted, n_reads, read_len=read_len, err_rate=0.0, random_frac=0.0, seed=synth.SEED_READS + 7).as_tuple())
    print("workload %s: %d unitigs, %d bases; %d records, %d segments, %d slots; %d reads added; set up in %.1f s"
          % (a.workload, idx.n_unitigs, idx.total_len, rp.n_seqs, rp.n_segments, rp.n_slots, n_reads, time.time() - t0), flush=True)
    t = {}
    add = lambda name, ms: t.setdefault(name, []).append(ms)
    for s in range(a.steps + 1):   # (repetition 0: a first launch of every kernel and the first allocations, not counted)
        got = {}
        for window in (1000, 1) if s % 2 else (1, 1000):
            dev, got["device depth, window %d" % window] = wall(lambda: rp.depth_windows(d, window, 1))
            (depth, _, _), ms_dd = wall(lambda: d.download())
            (nk, so, sg), ms_pd = wall(lambda: rp.download())
            host, ms_tw = wall(lambda: fa.segments_window_depth(nk, so, sg, k, ends, depth, window, 1, n_threads=16))
            got["host depth, window %d: Depth.download" % window] = ms_dd
            got["host depth, window %d: RefPaths.download" % window] = ms_pd
            got["host depth, window %d: twin on 16 threads" % window] = ms_tw
            got["host depth, window %d: sum" % window] = ms_dd + ms_pd + ms_tw
            if s == 0:
                assert host.windows.tobytes() == dev.windows.tobytes() and np.array_equal(host.win_offs, dev.win_offs), "the twin's windows differ from the device's"
            del dev, host, depth
        _, got["device depth, one record of 1000 bases (the materialised scan)"] = wall(lambda: small.depth_windows(d, 1000, 1))
        v, got["Pileup.call (both routes)"] = wall(lambda: pl.call(2, 200))
        dev, got["device lift"] = wall(lambda: rp.lift_variants(v))
        (nk, so, sg), ms_pd = wall(lambda: rp.download())
        host, ms_tw = wall(lambda: fa.segments_lift_variants(nk, so, sg, k, ends, v, n_threads=16))
        got["host lift: RefPaths.download"] = ms_pd; got["host lift: twin on 16 threads"] = ms_tw; got["host lift: sum"] = ms_pd + ms_tw
        if s == 0:
            assert host.tobytes() == dev.tobytes(), "the twin's records differ from the device's"
            print("%d candidates, %d lifted records, %d of them reverse" % (len(v), len(dev), int((dev["flags"] & 1).sum())), flush=True)
            continue
        for name, ms in got.items():
            add(name, ms)
        print("repetition %d: %s" % (s, " | ".join("%s %.1f" % (n.split(":")[0] if n.endswith("sum") else n, ms) for n, ms in got.items() if n.startswith("device") or n.endswith("sum"))), flush=True)
    print("host wall clock, medians over %d repetitions:" % a.steps)
    for name in t:
        print("  %-66s %s" % (name, med(t[name])))
    rp.close(); small.close(); d.close(); pl.close()


if __name__ == "__main__":
    main()
