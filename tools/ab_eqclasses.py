#!/usr/bin/env python3
"""What the equivalence classes of pseudoaligned reads cost on the device (fin_batch_add_eqclasses; fin_eqclasses.hip), against what a caller did before the
accumulator existed: fin_batch_pseudoalign + fin_batch_download_pseudo + np.unique(rows, axis=0, return_counts=True) on the host -- `python3
tools/ab_eqclasses.py [workload] [--reads N] [--steps S] [--sets M] [--colors 5,130,4096] [--permille P]`.

The workload is built the way bench.py builds it (same seeds, same sizes; default chr1); the method is tools/ab_colors.py's: HIP events on one stream, the
variants interleaved in one process, text mode 2.  The matrix is tools/ab_colors.py's: unitig u has colour c when (u * 2654435761 + c * 40503) % 7 < 2, every
16th unitig has none.

  for each number of colours, steps 1..S over M sets of FRESH reads (another seed per set, reloaded in turn), each step followed by, each timed by itself with
  HIP events: fin_batch_pseudoalign alone | fin_batch_add_eqclasses with option ec_combine 1 (a wave's count adds combined over its distinct slots) | the same
  with ec_combine 0 (one atomic per row); and, host wall clock: the accumulator's download | the rows' download + np.unique.  The accumulators are reset before
  every step, untimed, and its classes must equal np.unique's.  Medians over the steps, bytes to the host.
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--colors", default="5,130,4096")
    ap.add_argument("--permille", type=int, default=1000)
    a = ap.parse_args()
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    n_reads = a.reads or n_reads
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    sets = [synth.reads(g, n_reads, read_len=read_len, seed=synth.SEED_READS + 1000 * s) for s in range(a.sets)]
    batch = idx.batch(sets[0].as_tuple())
    nu = idx.n_unitigs
    print("workload %s: %d unitigs, %d bases, %d reads per step, %d k-mers, set up in %.1f s" % (a.workload, nu, idx.total_len, n_reads, batch.n_kmers, time.time() - t0),
          flush=True)
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    L = fa.lib()
    err = C.create_string_buffer(512)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ts); rc = f(); e1.record(ts); torch.cuda.synchronize()
        assert rc == 0, err.value
        return e0.elapsed_time(e1)

    batch.text_mode(2)
    for n_colors in [int(x) for x in a.colors.split(",")]:
        W = (n_colors + 63) // 64
        bits = np.zeros((nu, W), dtype=np.uint64)
        for w in range(W):   # (a word of the matrix at a time: 4096 colours of chr1's unitigs do not fit as one array of flags)
            c = np.arange(64 * w, min(64 * w + 64, n_colors), dtype=np.uint64)
            member = np.zeros((nu, 64), dtype=np.uint8)
            member[:, : len(c)] = (np.arange(nu, dtype=np.uint64)[:, None] * np.uint64(2654435761) + c[None, :] * np.uint64(40503)) % np.uint64(7) < 2
            member[::16] = 0
            bits[:, w] = np.ascontiguousarray(np.packbits(member, axis=1, bitorder="little")).view(np.uint64)[:, 0]
        col = idx.colors(n_colors, bits)
        eq = {1: col.eqclasses(1 << 22), 0: col.eqclasses(1 << 22)}

        def add(combine):
            assert L.fin_index_set_option(idx.h, b"ec_combine", combine) == 0
            return L.fin_batch_add_eqclasses(batch.h, eq[combine].h, a.permille, C.c_void_p(stream), err, 512)

        ways = [("pseudoalign", lambda: L.fin_batch_pseudoalign(batch.h, col.h, a.permille, err, 512)), ("add_eqclasses (combined)", lambda: add(1)),
                ("add_eqclasses (an atomic per row)", lambda: add(0))]
        t = {name: [] for name, _ in ways}
        t_step, t_dl_eq, t_dl_rows, t_unique = [], [], [], []
        n_classes = 0
        try:
            for s in range(a.steps + 1):   # (step 0: a first launch of every kernel, not counted)
                batch.reload(sets[s % a.sets].as_tuple())
                ms = timed(lambda: batch.run(fa.FIN_MERGED, stream) or 0)
                eq[0].reset(stream); eq[1].reset(stream)   # (outside the timed stretches: a reset zeroes the whole table)
                order = ways[s % 3:] + ways[:s % 3]   # (interleaved: each goes first .. third in turn)
                got = {name: timed(f) for name, f in order}
                w0 = time.perf_counter(); rows_e, reads_e, un = eq[1].download(); w1 = time.perf_counter()
                rows, heads = batch.pseudoalign(col, a.permille); w2 = time.perf_counter()
                live = rows[rows.any(axis=1)]
                ur, uc = np.unique(live, axis=0, return_counts=True) if len(live) else (live, np.zeros(0, dtype=np.int64))
                w3 = time.perf_counter()
                assert np.array_equal(rows_e, ur) and np.array_equal(reads_e, uc.astype(np.uint64)) and un == len(rows) - len(live), "the classes differ from np.unique's"
                r0, c0, u0 = eq[0].download()
                assert np.array_equal(r0, ur) and np.array_equal(c0, reads_e) and u0 == un, "the classes of the uncombined count pass differ"
                n_classes = len(ur)
                if s == 0:
                    continue
                t_step.append(ms)
                for name, _ in ways:
                    t[name].append(got[name])
                t_dl_eq.append(1e3 * (w1 - w0)); t_dl_rows.append(1e3 * (w2 - w1)); t_unique.append(1e3 * (w3 - w2))
                print("%d colours, step %d: step %.3f ms | %s" % (n_colors, s, ms, " | ".join("%s %.3f ms" % (name, got[name]) for name, _ in ways)), flush=True)
        finally:
            L.fin_index_clear_option(idx.h, b"ec_combine")
        print("%d colours (%d words per row), %d classes, medians over %d steps, text mode 2: step %s" % (n_colors, W, n_classes, a.steps, med(t_step)))
        for name, _ in ways:
            print("  fin_batch_%-36s %s" % (name + ":", med(t[name])))
        print("  host wall clock: classes compacted + downloaded + sorted %s | rows made + downloaded %s | np.unique %s" % (med(t_dl_eq), med(t_dl_rows), med(t_unique)))
        print("  bytes to the host: classes %d | rows and heads %d; stats %s" % (n_classes * (8 * W + 8), n_reads * (8 * W + 16), eq[1].stats()), flush=True)
        eq[0].close(); eq[1].close(); col.close()
    batch.close()


if __name__ == "__main__":
    main()
