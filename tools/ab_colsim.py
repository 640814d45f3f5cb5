#!/usr/bin/env python3
"""What the colour matrix times itself costs on the device (fin_colors_shared; fin_colsim.hip), against the route a user had before it --
`python3 tools/ab_colsim.py [workload] [--unitigs 10000000] [--dense-unitigs 1000000] [--colors 5,130,4096] [--steps S] [--no-index]`.

Part 1, synthetic: N unitigs x C colours in HBM, rows of 1 to 8 random colours ("sparse"), and at the largest C one dense shape, rows of 100 to 500 colours,
unitig lengths 31 .. 159 (k = 31).  Timed with HIP events on one stream, medians of S (default 20): fin_launch_color_shared -- the memset, the tile kernel and
the mirror kernel -- with the default weights.  Against it, host wall clock, once: the matrix copied to the host | fin_unitig_color_shared on 16 host threads.
Device and host must agree on every byte.

Part 2, the whole waiting call on the workload's index (built the way bench.py builds it), a synthetic sparse matrix uploaded and a bitmap filled by one read
set; wall clock, medians of S: Colors.shared() and Colors.shared(cover) | the route before it: Colors.download (+ Cover.download) + the host twin on 16 threads.
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


def device_matrix(n, n_colors, lo, hi, seed):
    """int64[n, W] on the device: up to a random lo .. hi colours per row (drawn with replacement)"""
    W = (n_colors + 63) // 64
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rows = torch.zeros(n * W, dtype=torch.int64, device="cuda")
    sizes = torch.randint(lo, min(hi, n_colors) + 1, (n,), device="cuda", generator=gen)
    base = torch.arange(n, device="cuda") * W
    one = torch.ones((), dtype=torch.int64, device="cuda")
    for j in range(min(hi, n_colors)):   # (slot j of every row: a row is in the index list once, so the read-modify-write has no conflicts)
        c = torch.randint(0, n_colors, (n,), device="cuda", generator=gen)
        live = sizes > j
        at = (base + (c >> 6))[live]
        rows[at] = rows[at] | (one << (c[live] & 63))
    return rows.view(n, W)


def synthetic(L, a):
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    vp = C.c_void_p
    L.fin_launch_color_shared.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp, vp]
    L.fin_colsim_chunk.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
    L.fin_colsim_chunk.restype = C.c_uint32
    rng = np.random.default_rng(36)
    colors = [int(x) for x in a.colors.split(",")]
    shapes = [(a.unitigs, c, 1, 8, "sparse (1 to 8 colours)") for c in colors] + [(a.dense_unitigs, max(colors), 100, 500, "dense (100 to 500 colours)")]
    for n, n_colors, lo, hi, name in shapes:
        if n <= 0:
            continue
        lens = rng.integers(K, 160, n).astype(np.int64)
        ends = np.concatenate([[0], np.cumsum(lens)])
        total_len = int(ends[-1])
        assert total_len < 2 ** 32
        nk = (lens - K + 1).astype(np.uint64)
        d_ends = torch.from_numpy(np.concatenate([ends, [0xFFFFFFFF] * 8]).astype(np.uint32).view(np.int32)).cuda()
        W = (n_colors + 63) // 64
        d_rows = device_matrix(n, n_colors, lo, hi, 1000 * n_colors + lo)
        d_out = torch.zeros(n_colors * n_colors, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def timed():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            rc = L.fin_launch_color_shared(d_rows.data_ptr(), n, W, n_colors, d_ends.data_ptr(), total_len, K, None, 0, d_out.data_ptr(), stream)
            e1.record(ts); torch.cuda.synchronize()
            assert rc == 0, rc
            return e0.elapsed_time(e1)
        timed()   # (a first launch, not counted)
        t = [timed() for _ in range(a.steps)]
        dev = d_out.cpu().numpy().view(np.uint64)
        print("%d unitigs x %d colours (%d words per row, %d tiles), %s rows, %d bytes of matrix, %d unitigs per chunk:" % (
            n, n_colors, W, W * (W + 1) // 2, name, n * W * 8, L.fin_colsim_chunk(n, W, 0)))
        print("  product kernels (memset + tiles + mirror): %s" % med(t))
        w0 = time.perf_counter()
        h_rows = d_rows.cpu().numpy().view(np.uint64)
        w1 = time.perf_counter()
        host = fa.unitig_color_shared(h_rows, n_colors, nk, n_threads=16)
        w2 = time.perf_counter()
        assert host.table.tobytes() == dev.tobytes(), "device and host differ"
        print("  host wall clock (1 run): the copy to the host %.1f ms | fin_unitig_color_shared on 16 threads %.1f ms" % (1e3 * (w1 - w0), 1e3 * (w2 - w1)))
        sys.stdout.flush()
        del h_rows, d_rows, d_out, host


def whole_call(a):
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    nu = idx.n_unitigs
    reads = synth.reads(g, min(n_reads, 1_000_000), read_len=read_len, seed=synth.SEED_READS).as_tuple()
    cov = idx.cover().add_reads(reads)
    ends = idx.export(fa.X_ENDS)
    nk = (np.diff(np.concatenate([[0], ends])) - k + 1).astype(np.uint64)
    print("workload %s: %d unitigs, %d bases of text, set up in %.1f s" % (a.workload, nu, idx.total_len, time.time() - t0), flush=True)
    for n_colors in [int(x) for x in a.colors.split(",")]:
        col = idx.colors(n_colors, device_matrix(nu, n_colors, 1, 8, n_colors).cpu().numpy().view(np.uint64))
        col.shared(); col.shared(cover=cov)   # (first calls, not counted)
        for cover in (None, cov):
            t_dev, t_old = [], []
            for s in range(a.steps):
                w0 = time.perf_counter()
                got = col.shared(cover=cover)
                w1 = time.perf_counter()
                host = fa.unitig_color_shared(col.download()[0], n_colors, nk if cover is None else cover.download()[1], n_threads=16)
                w2 = time.perf_counter()
                t_dev.append(1e3 * (w1 - w0)); t_old.append(1e3 * (w2 - w1))
                assert got.table.tobytes() == host.table.tobytes()
            print("%d colours over the index's %d unitigs, rows of 1 to 8 colours, %s, wall clock:" % (n_colors, nu, "the found k-mers" if cover is not None else "the unitigs' k-mers"))
            print("  Colors.shared:                                   %s" % med(t_dev))
            print("  the downloads + the host twin on 16 threads:     %s" % med(t_old), flush=True)
        col.close()
    cov.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="chr1", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--unitigs", type=int, default=10_000_000)
    ap.add_argument("--dense-unitigs", type=int, default=1_000_000)
    ap.add_argument("--colors", default="5,130,4096")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--no-index", action="store_true")
    a = ap.parse_args()
    L = fa.lib()
    synthetic(L, a)
    if not a.no_index:
        whole_call(a)


if __name__ == "__main__":
    main()
