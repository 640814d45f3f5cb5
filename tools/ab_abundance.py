#!/usr/bin/env python3
"""What one EM iteration over equivalence classes costs on the device (fin_eqclasses_abundance; fin_abundance.hip), against what a caller did
before it existed: fin_classes_abundance on the host (16 threads) and the numpy model -- `python3 tools/ab_abundance.py [--classes 100000,1000000]
[--colors 130,4096] [--iters 20] [--threads 16]`.

Classes: C distinct random rows of 1 to 8 colours each, reads 1 to 50, lengths 0.5 to 2000, seeded.  Per (C, colours):
  device   one iteration = the four launches of fin_launch_ab_iteration on dense device arrays, each timed with HIP events on one stream, the median of
           --iters after 3 warm-up iterations; the one-off word-major copy (fin_launch_ab_transpose) timed apart the same way; and the whole waiting call
           EqClasses.abundance(max_iters=1), host wall clock, on an accumulator filled through add_rows -- it holds the table's compaction (occupied, scan,
           gather), the allocations and the copies as well
  host     fin_classes_abundance(max_iters=5) / 5, wall clock, --threads threads
  numpy    the model's iteration over index lists (np.add.reduceat), wall clock, the median of 5
and the column pass's share: it must read C * W * 16 bytes per iteration (a word and a q per class and word); the figure printed is those bytes over the WHOLE
iteration's time, a lower bound of what the column pass achieves.  The device's alpha after the timed iterations must equal the host twin's within 1e-9."""
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


def random_classes(rng, n_classes, n_colors):
    W = (n_colors + 63) // 64
    rows = np.zeros((0, W), dtype=np.uint64)
    while len(rows) < n_classes:
        n = n_classes - len(rows) + 1024
        size = rng.integers(1, 9, n)
        new = np.zeros((n, W), dtype=np.uint64)
        for i in range(8):
            c = rng.integers(0, n_colors, n)
            on = size > i
            np.bitwise_or.at(new, (np.nonzero(on)[0], c[on] >> 6), np.uint64(1) << (c[on] & 63).astype(np.uint64))
        rows = np.unique(np.concatenate([rows, new]), axis=0)
    rows = rows[np.sort(rng.permutation(len(rows))[:n_classes])]
    return rows, rng.integers(1, 51, n_classes).astype(np.uint64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else a.dtype)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", default="100000,1000000")
    ap.add_argument("--colors", default="130,4096")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    L = fa.lib()
    vp, u32, u64, dbl = C.c_void_p, C.c_uint32, C.c_uint64, C.c_double
    L.fin_ab_geometry.argtypes = [u64, u32, u32] + [C.POINTER(u32)] * 4
    L.fin_ab_geometry.restype = None
    L.fin_launch_ab_transpose.argtypes = [vp, u64, u32, vp, vp]
    L.fin_launch_ab_iteration.argtypes = [vp, vp, vp, vp, u64, u32, u32, u32, vp, dbl, dbl, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp]
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

    med = lambda xs: "%.3f ms (%.3f..%.3f, n=%d)" % (statistics.median(xs), min(xs), max(xs), len(xs))
    for n_colors in [int(x) for x in a.colors.split(",")]:
        for n_classes in [int(x) for x in a.classes.split(",")]:
            rng = np.random.default_rng(2400 + n_colors)
            rows, reads = random_classes(rng, n_classes, n_colors)
            lens = rng.uniform(0.5, 2000, n_colors)
            W, N = rows.shape[1], int(reads.sum())
            geo = [u32() for _ in range(4)]
            L.fin_ab_geometry(n_classes, W, 0, *[C.byref(x) for x in geo])
            cpb, n_ll, chunk, n_chunks = [int(x.value) for x in geo]
            print("%d classes, %d colours (W = %d): %d reads, chunks of %d classes (%d), %d blocks in the first pass" % (n_classes, n_colors, W, N, chunk, n_chunks, n_ll), flush=True)
            d_rows, d_reads = dev(rows), dev(reads)
            d_rowsT = torch.empty_like(d_rows) if W > 1 else d_rows
            if W > 1:
                print("  word-major copy        %s" % med(timed(lambda i: L.fin_launch_ab_transpose(d_rows.data_ptr(), n_classes, W, d_rowsT.data_ptr(), stream), 5, 2)))
            pad = 64 * W
            len_p = np.ones(pad); len_p[:n_colors] = lens
            alpha0 = np.zeros(pad); alpha0[:n_colors] = N / n_colors
            d_len, d_alpha, d_x = dev(len_p), dev(alpha0), dev(alpha0 / len_p)
            d_q, d_part, d_ll = torch.empty(n_classes, dtype=torch.float64, device="cuda"), torch.empty(n_chunks * pad, dtype=torch.float64, device="cuda"), torch.empty(n_ll, dtype=torch.float64, device="cuda")
            d_ok, d_chg = torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(64, dtype=torch.float64, device="cuda")
            d_state, d_trace = torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(a.iters + 3, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()

            def iteration(i):
                rc = L.fin_launch_ab_iteration(d_state.data_ptr(), d_rows.data_ptr(), d_rowsT.data_ptr(), d_reads.data_ptr(), n_classes, W, n_colors, 0, d_len.data_ptr(), float(N),
                                               0.0, d_alpha.data_ptr(), d_x.data_ptr(), d_q.data_ptr(), d_part.data_ptr(), d_ll.data_ptr(), d_ok.data_ptr(), d_chg.data_ptr(), i,
                                               d_trace.data_ptr(), stream)
                assert rc == 0, rc

            ts = timed(iteration, a.iters, 3)
            it_ms = statistics.median(ts)
            need = n_classes * W * 16
            print("  one iteration (device) %s; the column pass must read %.1f MB: at least %.1f GB/s" % (med(ts), need / 1e6, need / it_ms / 1e6))
            got = d_alpha.cpu().numpy()[:n_colors]
            t0 = time.perf_counter()
            host = fa.classes_abundance(rows, reads, n_colors, lens, max_iters=5, tol=0.0, n_threads=a.threads)
            print("  one iteration (host, %d threads) %.3f ms" % (a.threads, (time.perf_counter() - t0) * 1e3 / 5))
            want = fa.classes_abundance(rows, reads, n_colors, lens, max_iters=a.iters + 3, tol=0.0, n_threads=a.threads).alpha
            off = float((np.abs(got - want) / np.maximum(np.abs(want), 1)).max())
            assert off <= 1e-9, off
            # numpy: the model's two products over index lists
            jj, cc = [], []
            for b0 in range(0, n_classes, 1 << 16):                          # (in blocks of classes: the dense bits of 10^6 x 4096 would be 4 GB)
                bj, bc = np.nonzero(np.unpackbits(rows[b0: b0 + (1 << 16)].view(np.uint8).reshape(min(1 << 16, n_classes - b0), -1), axis=1, bitorder="little"))
                jj.append(bj + b0); cc.append(bc)
            jj, cc = np.concatenate(jj), np.concatenate(cc)
            row_start = np.searchsorted(jj, np.arange(n_classes))
            o = np.argsort(cc, kind="stable")
            jj_c, cols = jj[o], np.unique(cc)
            col_start = np.searchsorted(cc[o], cols)
            al, nn, tn = np.full(n_colors, N / n_colors), reads.astype(np.float64), []
            for _ in range(5):
                t0 = time.perf_counter()
                x = al / lens
                d = np.add.reduceat(x[cc], row_start)
                ll = (nn * np.log(d / N)).sum()
                S = np.zeros(n_colors); S[cols] = np.add.reduceat((nn / d)[jj_c], col_start)
                al = x * S
                tn.append((time.perf_counter() - t0) * 1e3)
            print("  one iteration (numpy)  %s" % med(tn))
            # the whole waiting call on a filled accumulator
            col = idx.colors(n_colors)
            eq = col.eqclasses(max(n_classes, 1))
            eq.add_rows(d_rows.data_ptr(), n_classes)
            eq.stats()
            tw = []
            for _ in range(4):
                t0 = time.perf_counter()
                r = eq.abundance(lens, max_iters=1, tol=0.0)
                tw.append((time.perf_counter() - t0) * 1e3)
            print("  the whole call, one iteration (compaction, copies, allocations) %s; device differs from the host twin by %.2g" % (med(tw[1:]), off), flush=True)
            eq.close(); col.close()
    idx.close()


if __name__ == "__main__":
    main()
