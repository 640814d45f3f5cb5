#!/usr/bin/env python3
"""What projecting the coverage numbers through the colour matrix costs on the device (fin_colors_coverage; fin_colcov.hip), against the route a
user had before it -- `python3 tools/ab_colcov.py [workload] [--unitigs 1000000,10000000] [--colors 5,130,4096] [--steps S] [--no-index]`.

Part 1, synthetic: N unitigs x C colours in HBM, rows of 1 to 8 random colours ("sparse") and rows of random words ("dense", half the colours each), unitig
lengths 31 .. 159 (k = 31), random covered[] and statistics.  Timed with HIP events on one stream, medians of S (default 20): fin_launch_color_coverage -- the
two memsets, the class kernel and the column kernel -- with the column kernel's two load strategies (0: coalesced slices broadcast through the wave, 1:
wave-uniform loads), interleaved.  Against it, host wall clock, once: the matrix, covered[] and statistics copied to the host | fin_unitig_color_coverage on 16
host threads (skipped where the dense matrix would keep the host busy for minutes).  Both strategies and the host must agree on every byte.

Part 2, the whole waiting call on the workload's index (built the way bench.py builds it): a bitmap and a depth filled by one read set, a synthetic matrix
uploaded; wall clock, medians of S: Colors.coverage(cover, depth) | the route before it: Colors.download + Cover.download + Depth.download(want_positions=False)
+ the host twin on 16 threads.
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

K = 31


def med(xs):
    return "%.3f ms (%.3f..%.3f, n=%d)" % (statistics.median(xs), min(xs), max(xs), len(xs))


def device_matrix(n, n_colors, dense, seed):
    """int64[n, W] on the device; sparse: 1 to 8 colours per row, dense: random words under the colours' mask"""
    W = (n_colors + 63) // 64
    gen = torch.Generator(device="cuda").manual_seed(seed)
    if dense:
        rows = torch.randint(-2 ** 63, 2 ** 63 - 1, (n, W), dtype=torch.int64, device="cuda", generator=gen)
        if n_colors & 63:
            rows[:, W - 1] &= (1 << (n_colors & 63)) - 1
        return rows
    rows = torch.zeros(n * W, dtype=torch.int64, device="cuda")
    sizes = torch.randint(1, min(8, n_colors) + 1, (n,), device="cuda", generator=gen)
    base = torch.arange(n, device="cuda") * W
    one = torch.ones((), dtype=torch.int64, device="cuda")
    for j in range(8):   # (slot j of every row: a row is in the index list once, so the read-modify-write has no conflicts)
        c = torch.randint(0, n_colors, (n,), device="cuda", generator=gen)
        live = sizes > j
        at = (base + (c >> 6))[live]
        rows[at] = rows[at] | (one << (c[live] & 63))
    return rows.view(n, W)


def synthetic(L, a, err):
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    vp = C.c_void_p
    L.fin_launch_color_coverage.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint64, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.fin_colcov_chunk.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
    L.fin_colcov_chunk.restype = C.c_uint32
    rng = np.random.default_rng(34)
    for n in [int(x) for x in a.unitigs.split(",")]:
        lens = rng.integers(K, 160, n).astype(np.int64)
        ends = np.concatenate([[0], np.cumsum(lens)])
        total_len = int(ends[-1])
        assert total_len < 2 ** 32
        nk = (lens - K + 1).astype(np.uint64)
        covered = (nk * rng.random(n)).astype(np.uint64)
        stats = np.zeros(n, dtype=fa.DEPTH_STAT_DTYPE)
        stats["sum"] = covered * rng.integers(1, 2 ** 20, n).astype(np.uint64)
        stats["n_at_least"] = covered // np.uint64(2)
        d_ends = torch.from_numpy(np.concatenate([ends, [0xFFFFFFFF] * 8]).astype(np.uint32).view(np.int32)).cuda()
        d_cov = torch.from_numpy(covered.view(np.int64)).cuda()
        d_stats = torch.from_numpy(stats.view(np.uint8)).cuda()
        d_cls = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
        for n_colors in [int(x) for x in a.colors.split(",")]:
            W = (n_colors + 63) // 64
            for dense in (False, True):
                d_rows = device_matrix(n, n_colors, dense, 1000 * n_colors + dense)
                d_out = [torch.zeros((n_colors + 1) * 8, dtype=torch.int64, device="cuda") for _ in range(2)]
                torch.cuda.synchronize()

                def launch(loads):
                    return L.fin_launch_color_coverage(d_rows.data_ptr(), n, W, n_colors, d_ends.data_ptr(), total_len, K, d_cov.data_ptr(), d_stats.data_ptr(), d_cls.data_ptr(),
                                                       0, loads, d_out[loads].data_ptr(), d_out[loads].data_ptr() + n_colors * 64, stream)

                def timed(loads):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(ts); rc = launch(loads); e1.record(ts); torch.cuda.synchronize()
                    assert rc == 0, rc
                    return e0.elapsed_time(e1)
                timed(0); timed(1)   # (a first launch, not counted)
                t = [[], []]
                for s in range(a.steps):
                    for loads in ((0, 1) if s % 2 == 0 else (1, 0)):   # (interleaved)
                        t[loads].append(timed(loads))
                dev = [o.cpu().numpy().view(np.uint64) for o in d_out]
                assert dev[0].tobytes() == dev[1].tobytes(), "the two load strategies differ"
                print("%d unitigs x %d colours (%d words per row), %s rows, %d bytes of matrix, %d unitigs per chunk:" % (
                    n, n_colors, W, "dense" if dense else "sparse (1 to 8 colours)", n * W * 8, L.fin_colcov_chunk(n, W, 0)))
                print("  projection kernels, coalesced slices + broadcast (loads 0): %s" % med(t[0]))
                print("  projection kernels, wave-uniform loads (loads 1):           %s" % med(t[1]))
                if not dense or n * n_colors <= 5_000_000_000:
                    w0 = time.perf_counter()
                    h_rows = d_rows.cpu().numpy().view(np.uint64)
                    h_cov = d_cov.cpu().numpy().view(np.uint64)
                    h_stats = d_stats.cpu().numpy().view(fa.DEPTH_STAT_DTYPE)
                    w1 = time.perf_counter()
                    host = fa.unitig_color_coverage(h_rows, n_colors, nk, h_cov, h_stats, n_threads=16)
                    w2 = time.perf_counter()
                    assert host.table.tobytes() == dev[0][: n_colors * 8].tobytes(), "device and host differ"
                    print("  host wall clock (1 run): the copies to the host %.1f ms | fin_unitig_color_coverage on 16 threads %.1f ms" % (1e3 * (w1 - w0), 1e3 * (w2 - w1)))
                    del h_rows
                else:
                    print("  host: skipped (%.1e set bits)" % (n * n_colors / 2))
                sys.stdout.flush()
                del d_rows, d_out


def whole_call(a):
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    nu = idx.n_unitigs
    reads = synth.reads(g, min(n_reads, 1_000_000), read_len=read_len, seed=synth.SEED_READS).as_tuple()
    cov, dep = idx.cover().add_reads(reads), idx.depth().add_reads(reads)
    ends = idx.export(fa.X_ENDS)
    nk = (np.diff(np.concatenate([[0], ends])) - k + 1).astype(np.uint64)
    print("workload %s: %d unitigs, %d bases of text, set up in %.1f s" % (a.workload, nu, idx.total_len, time.time() - t0), flush=True)
    for n_colors in [int(x) for x in a.colors.split(",")]:
        col = idx.colors(n_colors, device_matrix(nu, n_colors, False, n_colors).cpu().numpy().view(np.uint64))
        got = col.coverage(cov, dep)   # (the first call: its buffers are made)
        t_dev, t_old = [], []
        for s in range(a.steps):
            w0 = time.perf_counter()
            got = col.coverage(cov, dep)
            w1 = time.perf_counter()
            host = fa.unitig_color_coverage(col.download()[0], n_colors, nk, cov.download()[1], dep.download(1, want_positions=False)[1], n_threads=16)
            w2 = time.perf_counter()
            t_dev.append(1e3 * (w1 - w0)); t_old.append(1e3 * (w2 - w1))
            assert got.table.tobytes() == host.table.tobytes() and got.uncolored == host.uncolored
        print("%d colours over the index's %d unitigs, rows of 1 to 8 colours, wall clock:" % (n_colors, nu))
        print("  Colors.coverage(cover, depth):                          %s" % med(t_dev))
        print("  the three downloads + the host twin on 16 threads:      %s" % med(t_old), flush=True)
        col.close()
    cov.close(); dep.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="chr1", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--unitigs", default="1000000,10000000")
    ap.add_argument("--colors", default="5,130,4096")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-index", action="store_true")
    a = ap.parse_args()
    L = fa.lib()
    err = C.create_string_buffer(512)
    if a.unitigs:
        synthetic(L, a, err)
    if not a.no_index:
        whole_call(a)


if __name__ == "__main__":
    main()
