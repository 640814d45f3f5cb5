#!/usr/bin/env python3
"""What the bootstrap of the abundance estimate costs on the device (fin_eqclasses_bootstrap; fin_bootstrap.hip) -- `python3 tools/ab_bootstrap.py
[--classes 100000,1000000] [--colors 130,4096] [--reads 10000000] [--boot 100] [--iters 20] [--host-boot 3] [--threads 16]`.

Classes: C distinct random rows of 1 to 8 colours each (tools/ab_abundance.py's), every class with --reads / C reads: the dense row list is added that many times,
so the accumulator holds N = --reads rows without an N x W row list ever existing.  Per (C, colours), HIP events, medians of 20:
  resample   fin_launch_ab_resample for one replicate on the dense arrays (counts and the N_b word zeroed in the timed window, as the call does), next to
  iteration  the four launches of fin_launch_ab_iteration at the same size; and the one-off row hashes and slab prefix
  call       EqClasses.bootstrap(--boot, max_iters = --iters, tol = 0), host wall clock, the median of 3 -- a fixed number of iterations, so that every
             estimate of every route does the same work -- against
  repeated   (1 + --boot) x EqClasses.abundance(max_iters = --iters, tol = 0), the median of 5 calls: what keeping the dense list saves (the call is the
             parent's, unchanged by the bootstrap)
  host       download(), then classes_bootstrap on --threads threads with --host-boot replicates, scaled to --boot (its replicates cost the same each)
and from the resample kernel's rate what the 2^38 draws of the limit would take."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import finito_amd as fa
from finito_amd import synth
from tools.ab_abundance import dev, random_classes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", default="100000,1000000")
    ap.add_argument("--colors", default="130,4096")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--boot", type=int, default=100)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-boot", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    L = fa.lib()
    vp, u32, u64, dbl = C.c_void_p, C.c_uint32, C.c_uint64, C.c_double
    L.fin_ab_geometry.argtypes = [u64, u32, u32] + [C.POINTER(u32)] * 4
    L.fin_ab_geometry.restype = None
    L.fin_launch_ab_transpose.argtypes = [vp, u64, u32, vp, vp]
    L.fin_launch_ab_iteration.argtypes = [vp, vp, vp, vp, u64, u32, u32, u32, vp, dbl, dbl, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp]
    L.fin_launch_ab_rowhash.argtypes = [vp, u64, u32, vp, vp]
    L.fin_launch_ab_slabs.argtypes = [vp, u64, vp, vp, vp, vp]
    L.fin_launch_ab_resample.argtypes = [vp, vp, vp, u64, u64, u64, u32, vp, vp, vp]
    g = synth.genome(20000)
    idx = fa.FinimizerIndex.build(synth.unitigs(g, 31).as_tuple(), 31).to_device(0)   # (an accumulator wants an index to live beside)
    stream = torch.cuda.current_stream().cuda_stream

    def timed(f, n, warm):
        out = []
        for i in range(warm + n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(i); e1.record(); e1.synchronize()
            if i >= warm:
                out.append(e0.elapsed_time(e1))
        return out

    def wall(f, n):
        out = []
        for _ in range(n):
            t0 = time.perf_counter(); f(); out.append((time.perf_counter() - t0) * 1e3)
        return out

    med = lambda xs: "%.3f ms (%.3f..%.3f, n=%d)" % (statistics.median(xs), min(xs), max(xs), len(xs))
    for n_colors in [int(x) for x in a.colors.split(",")]:
        for n_classes in [int(x) for x in a.classes.split(",")]:
            rng = np.random.default_rng(2600 + n_colors)
            rows, _ = random_classes(rng, n_classes, n_colors)
            per = max(1, a.reads // n_classes)
            reads = np.full(n_classes, per, dtype=np.uint64)
            lens = rng.uniform(0.5, 2000, n_colors)
            W, N = rows.shape[1], per * n_classes
            print("%d classes, %d colours (W = %d): %d reads each, N = %d" % (n_classes, n_colors, W, per, N), flush=True)
            d_rows, d_reads = dev(rows), dev(reads)
            i64 = lambda k: torch.zeros(k, dtype=torch.int64, device="cuda")
            d_h, d_pref, d_cnt, d_S = i64(n_classes), i64(n_classes), i64(n_classes + 1), i64(1)
            d_slabs = torch.zeros(n_classes, dtype=torch.int32, device="cuda")

            def once(i):
                assert L.fin_launch_ab_rowhash(d_rows.data_ptr(), n_classes, W, d_h.data_ptr(), stream) == 0
                assert L.fin_launch_ab_slabs(d_reads.data_ptr(), n_classes, d_slabs.data_ptr(), d_pref.data_ptr(), d_S.data_ptr(), stream) == 0

            print("  row hashes and slab prefix, once per call  %s" % med(timed(once, 5, 2)))
            S = int(d_S.cpu()[0])

            def resample(i):
                d_cnt.zero_()
                assert L.fin_launch_ab_resample(d_h.data_ptr(), d_reads.data_ptr(), d_pref.data_ptr(), n_classes, S, 7, i & 4095, d_cnt.data_ptr(), d_cnt.data_ptr() + 8 * n_classes,
                                                stream) == 0

            ts = timed(resample, 20, 3)
            rs_ms = statistics.median(ts)
            print("  resample, one replicate (%d slabs)          %s: %.1f G draws/s; 2^38 draws at this rate: %.2f s" % (S, med(ts), N / rs_ms / 1e6, (1 << 38) / (N / rs_ms * 1e3)))
            want = fa.classes_resample(rows[:1000], reads[:1000], n_colors, seed=7, b=22, n_threads=a.threads)
            assert np.array_equal(d_cnt.cpu().numpy()[:1000].view(np.uint64), want), "the device's counts are not the host twin's"
            # one EM iteration at the same size
            geo = [u32() for _ in range(4)]
            L.fin_ab_geometry(n_classes, W, 0, *[C.byref(x) for x in geo])
            cpb, n_ll, chunk, n_chunks = [int(x.value) for x in geo]
            d_rowsT = torch.empty_like(d_rows) if W > 1 else d_rows
            if W > 1:
                assert L.fin_launch_ab_transpose(d_rows.data_ptr(), n_classes, W, d_rowsT.data_ptr(), stream) == 0
            pad = 64 * W
            len_p = np.ones(pad); len_p[:n_colors] = lens
            alpha0 = np.zeros(pad); alpha0[:n_colors] = N / n_colors
            d_len, d_alpha, d_x = dev(len_p), dev(alpha0), dev(alpha0 / len_p)
            f64 = lambda k: torch.empty(k, dtype=torch.float64, device="cuda")
            d_q, d_part, d_ll = f64(n_classes), f64(n_chunks * pad), f64(n_ll)
            d_ok, d_chg = torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(64, dtype=torch.float64, device="cuda")
            d_state, d_trace = torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(32, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()

            def iteration(i):
                assert L.fin_launch_ab_iteration(d_state.data_ptr(), d_rows.data_ptr(), d_rowsT.data_ptr(), d_reads.data_ptr(), n_classes, W, n_colors, 0, d_len.data_ptr(), float(N), 0.0,
                                                 d_alpha.data_ptr(), d_x.data_ptr(), d_q.data_ptr(), d_part.data_ptr(), d_ll.data_ptr(), d_ok.data_ptr(), d_chg.data_ptr(), i,
                                                 d_trace.data_ptr(), stream) == 0

            print("  one EM iteration                            %s" % med(timed(iteration, 20, 3)), flush=True)
            # the whole call on a filled accumulator, and the two routes a caller had before
            col = idx.colors(n_colors)
            eq = col.eqclasses(n_classes)
            for _ in range(per):
                eq.add_rows(d_rows.data_ptr(), n_classes)
            assert eq.stats()[0] == N
            eq.bootstrap(2, seed=7, lengths=lens, max_iters=a.iters, tol=0.0)
            tc = wall(lambda: eq.bootstrap(a.boot, seed=7, lengths=lens, max_iters=a.iters, tol=0.0), 3)
            ta = wall(lambda: eq.abundance(lens, max_iters=a.iters, tol=0.0), 6)[1:]
            print("  the whole call, %d replicates x %d iterations %s" % (a.boot, a.iters, med(tc)))
            print("  one abundance call, %d iterations             %s: x %d = %.1f ms" % (a.iters, med(ta), 1 + a.boot, statistics.median(ta) * (1 + a.boot)))
            t0 = time.perf_counter()
            crows, creads, _ = eq.download()
            t_dl = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            fa.classes_bootstrap(crows, creads, n_colors, a.host_boot, seed=7, lengths=lens, max_iters=a.iters, tol=0.0, n_threads=a.threads)
            t_hb = (time.perf_counter() - t0) * 1e3
            print("  host route: download %.1f ms, classes_bootstrap with %d replicates on %d threads %.1f ms: scaled to %d replicates %.1f ms" %
                  (t_dl, a.host_boot, a.threads, t_hb, a.boot, t_dl + t_hb * (1 + a.boot) / (1 + a.host_boot)), flush=True)
            eq.close(); col.close()
    idx.close()


if __name__ == "__main__":
    main()
