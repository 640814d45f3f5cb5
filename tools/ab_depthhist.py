#!/usr/bin/env python3
"""What the depth histograms cost on the device (fin_depth_histogram, fin_colors_depth_histogram; fin_depthhist.hip), against the route a user had
before them -- `python3 tools/ab_depthhist.py [workload] [--unitigs 10000000] [--colors 5,130,4096] [--bins 64,1024] [--steps S] [--reads N] [--no-index]`.

Part 1, synthetic, tools/ab_colcov.py's matrices: N unitigs x C colours in HBM, rows of 1 to 8 random colours, unitig lengths 31 .. 159 (k = 31), one depth value
per unitig (0 .. 40, every tenth unitig deeper) so that depth is piecewise constant as it is on a real run.  The whole text is one staged array; the library's
loop is repeated here on the launchers: fin_launch_color_classes once, then fin_launch_color_depth_hist per sub-range of what a 64 MB table holds.  HIP events on
one stream, medians of S (default 20).  Against it, host wall clock, once: the depths and the matrix copied to the host | fin_unitig_color_depth_histogram on 16
threads.  Device and host must agree on every byte.

Part 2, the whole waiting call on the workload's index (built the way bench.py builds it), a depth filled by --reads reads (default 10 M): HIP events around the
call on the null stream and wall clock, medians of S:
  Depth.histogram(n_bins)                  | Depth.download() with positions + fin_depth_positions_histogram on 16 threads
  Colors.depth_histogram(depth, n_bins)    | Depth.download() with positions + Colors.download() + fin_unitig_color_depth_histogram on 16 threads
on the index's OWN colouring -- colour c is a window of the genome, searched in (every position lies in two windows) -- and on a synthetic matrix of 1 to 8 colours
per row.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import bench
import finito_amd as fa
from ab_colcov import device_matrix
from finito_amd import synth

K = 31
V_BUDGET = 64 << 20   # the library's


def med(xs):
    return "%.3f ms (%.3f..%.3f, n=%d)" % (statistics.median(xs), min(xs), max(xs), len(xs))


def synthetic(L, a):
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.fin_launch_color_classes.argtypes = [vp, u32, u32, vp, u64, u32, vp, vp, vp]
    L.fin_launch_color_depth_hist.argtypes = [vp, u64, u64, u64, u64, vp, u32, u64, u32, u32, u32, u32, u32, vp, vp, u32, u32, vp, u32, vp, vp, vp]
    rng = np.random.default_rng(39)
    for n in [int(x) for x in a.unitigs.split(",")]:
        lens = rng.integers(K, 160, n).astype(np.int64)
        ends = np.concatenate([[0], np.cumsum(lens)])
        total_len = int(ends[-1])
        assert total_len < 2 ** 32
        per_unitig = rng.integers(0, 41, n).astype(np.int32)
        per_unitig[::10] += rng.integers(0, 2000, len(per_unitig[::10])).astype(np.int32)
        d_depth = torch.repeat_interleave(torch.from_numpy(per_unitig).cuda(), torch.from_numpy(lens).cuda())
        assert d_depth.numel() == total_len and d_depth.data_ptr() % 16 == 0
        d_ends = torch.from_numpy(np.concatenate([ends, [0xFFFFFFFF] * 8]).astype(np.uint32).view(np.int32)).cuda()
        d_cls = torch.zeros(64 + n + 8, dtype=torch.uint8, device="cuda")
        for n_colors in [int(x) for x in a.colors.split(",")]:
            W = (n_colors + 63) // 64
            d_rows = device_matrix(n, n_colors, False, 1000 * n_colors)
            for n_bins in [int(x) for x in a.bins.split(",")]:
                per = min(n, V_BUDGET // (4 * n_bins))
                d_V = torch.zeros(per * n_bins, dtype=torch.int32, device="cuda")
                d_out = torch.zeros((n_colors * 2 + 1) * n_bins, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()

                def launch():
                    d_out.zero_()
                    rc = L.fin_launch_color_classes(d_rows.data_ptr(), n, W, d_ends.data_ptr(), total_len, K, d_cls.data_ptr() + 64, d_cls.data_ptr(), stream)
                    for u_lo in range(0, n, per):
                        u_hi = min(n, u_lo + per)
                        rc = rc or L.fin_launch_color_depth_hist(d_depth.data_ptr(), 0, total_len, int(ends[u_lo]), int(ends[u_hi]), d_ends.data_ptr(), n, total_len, K, n_bins, 1,
                                                                 u_lo, u_hi, d_V.data_ptr(), d_rows.data_ptr(), W, n_colors, d_cls.data_ptr() + 64, 0, d_out.data_ptr(),
                                                                 d_out.data_ptr() + n_colors * 2 * n_bins * 8, stream)
                    return rc

                def timed():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(ts); rc = launch(); e1.record(ts); torch.cuda.synchronize()
                    assert rc == 0, rc
                    return e0.elapsed_time(e1)
                timed()   # (a first run, not counted)
                t = [timed() for _ in range(a.steps)]
                dev = d_out.cpu().numpy().view(np.uint64)
                print("%d unitigs x %d colours (%d words per row) x %d bins, rows of 1 to 8 colours, %d positions, %d sub-ranges of %d unitigs:" % (
                    n, n_colors, W, n_bins, total_len, (n + per - 1) // per, per))
                print("  class kernel + binning + projection, all sub-ranges (HIP events): %s" % med(t))
                w0 = time.perf_counter()
                h_depth = d_depth.cpu().numpy().view(np.uint32)
                h_rows = d_rows.cpu().numpy().view(np.uint64)
                w1 = time.perf_counter()
                host = fa.unitig_color_depth_histogram(h_depth, ends[1:], K, h_rows, n_colors, n_bins, 1, n_threads=16)
                w2 = time.perf_counter()
                assert host.table.tobytes() == dev[: n_colors * 2 * n_bins].tobytes() and host.uncolored.tobytes() == dev[n_colors * 2 * n_bins:].tobytes(), "device and host differ"
                print("  host wall clock (1 run): the copies to the host %.1f ms | fin_unitig_color_depth_histogram on 16 threads %.1f ms" % (1e3 * (w1 - w0), 1e3 * (w2 - w1)))
                sys.stdout.flush()
                del d_V, d_out, h_depth, h_rows
            del d_rows


def own_colouring(idx, g, n_colors):
    """colour c = the window [c, c + 2) / (n_colors + 1) of the genome, searched in as pieces of 5000 bases"""
    col = idx.colors(n_colors)
    step = len(g) // (n_colors + 1)
    for c in range(n_colors):
        piece = np.ascontiguousarray(g[c * step: min(len(g), (c + 2) * step)])
        offs = np.unique(np.append(np.arange(0, len(piece), 5000, dtype=np.uint64), np.uint64(len(piece))))
        col.add_reads((piece, offs), c)
    return col


def whole_call(a):
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    dep = idx.depth()
    left, first = a.reads, 0
    while left > 0:   # (a million reads at a time: the host buffers stay small)
        n = min(left, 1_000_000)
        dep.add_reads(synth.reads(g, n, read_len=read_len, seed=synth.SEED_READS, first=first).as_tuple())
        left -= n; first += n
    ends = idx.export(fa.X_ENDS)
    print("workload %s: %d unitigs, %d bases of text, %d reads added, set up in %.1f s" % (a.workload, idx.n_unitigs, idx.total_len, a.reads, time.time() - t0), flush=True)
    ts = torch.cuda.default_stream()

    def both(call):
        """(HIP event ms, wall clock ms) of one waiting call"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        e0.record(ts); got = call(); e1.record(ts); torch.cuda.synchronize()
        w1 = time.perf_counter()
        return got, e0.elapsed_time(e1), 1e3 * (w1 - w0)

    def compare(title, device_call, host_call, same):
        device_call()   # (the first call: its buffers are made)
        t_ev, t_dev, t_old = [], [], []
        for s in range(a.steps):
            got, ev, wall = both(device_call)
            w1 = time.perf_counter()
            host = host_call()
            w2 = time.perf_counter()
            t_ev.append(ev); t_dev.append(wall); t_old.append(1e3 * (w2 - w1))
            assert same(got, host), "device and host differ"
        print(title)
        print("  the device call, HIP events:                            %s" % med(t_ev))
        print("  the device call, wall clock:                            %s" % med(t_dev))
        print("  the downloads + the host twin on 16 threads, wall clock: %s" % med(t_old), flush=True)

    for n_bins in (256, 1024):
        compare("the spectrum (Depth.histogram), %d bins:" % n_bins, lambda: dep.histogram(n_bins),
                lambda: fa.depth_positions_histogram(dep.download()[0], ends, k, n_bins, n_threads=16), lambda x, y: x.tobytes() == y.tobytes())
    same = lambda x, y: x.table.tobytes() == y.table.tobytes() and x.uncolored.tobytes() == y.uncolored.tobytes()
    for n_colors in [int(x) for x in a.colors.split(",")]:
        for what, col in (("the index's own colouring (windows of the genome)", own_colouring(idx, g, n_colors)),
                          ("a synthetic matrix of 1 to 8 colours per row", idx.colors(n_colors, device_matrix(idx.n_unitigs, n_colors, False, n_colors).cpu().numpy().view(np.uint64)))):
            for n_bins in [int(x) for x in a.bins.split(",")]:
                compare("Colors.depth_histogram, %d colours x %d bins over the index's %d unitigs, %s:" % (n_colors, n_bins, idx.n_unitigs, what),
                        lambda: col.depth_histogram(dep, n_bins),
                        lambda: fa.unitig_color_depth_histogram(dep.download()[0], ends, k, col.download()[0], n_colors, n_bins, n_threads=16), same)
            col.close()
    dep.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="chr1", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--unitigs", default="10000000")
    ap.add_argument("--colors", default="5,130,4096")
    ap.add_argument("--bins", default="64,1024")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--no-index", action="store_true")
    a = ap.parse_args()
    if a.unitigs:
        synthetic(fa.lib(), a)
    if not a.no_index:
        whole_call(a)


if __name__ == "__main__":
    main()
