#!/usr/bin/env python3
"""What the compact state of the colour matrix costs and saves on the device (fin_colorsets.hip), each part against its yardstick --
`python3 tools/ab_colorsets.py [workload] [--reads N] [--steps S] [--colors 5,130,4096] [--distinct 1000,1000000]`.

The workload is built the way bench.py builds it (default chr1), as tools/ab_taxa.py does; HIP events on one stream, the variants interleaved in one process,
text mode 2, medians over S steps (default 20).  The matrix is over the workload's own unitigs (their number is printed): D distinct non-empty rows dealt to the
unitigs at random, a twentieth of the unitigs empty.  For every n_colors and D:

  (a) Colors.compact() and Colors.expand(), host wall clock over the whole waiting calls (allocations, kernels, the counters' read-back, frees), against the host
      route to the same state: the matrix's download + fin_unitig_color_sets on 16 threads + upload_sets.  The two (set_of, sets) must expand to the same matrix.
  (b) per step, each timed by itself with HIP events on the batch's stream: fin_batch_pseudoalign and fin_batch_pseudoalign_paired under the DENSE and under the
      COMPACT state of the same colouring, at permille 1000.  The dense kernels are the parent commit's, unchanged (profiles/r38/colorsets.md: equal resource
      remarks before and after): they are the yardstick.  Rows and heads of the two states must be equal.
  (c) bytes of HBM the colouring holds before and after: 8 W n_unitigs + 8 against 4 n_unitigs + 16 + 8 W (n_sets + 1).
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


def wall(f, n):
    out, ts = None, []
    for _ in range(n):
        w = time.perf_counter(); out = f(); ts.append(1e3 * (time.perf_counter() - w))
    return out, ts


def matrix(rng, n_unitigs, n_colors, distinct):
    """uint64[n_unitigs, W]: `distinct` different non-empty rows (1 to 8 colours each, made different by construction) dealt at random; 5 % of the unitigs empty"""
    W = (n_colors + 63) // 64
    pool = np.zeros((distinct, W), dtype=np.uint64)
    for _ in range(8):
        c = rng.integers(0, n_colors, distinct)
        on = rng.random(distinct) < 0.5
        np.bitwise_or.at(pool, (np.flatnonzero(on), (c >> 6)[on]), np.uint64(1) << (c & 63).astype(np.uint64)[on])
    pool[:, 0] |= np.uint64(1)
    pool = np.unique(pool, axis=0)
    which = rng.integers(0, len(pool), n_unitigs)
    bits = pool[which]
    bits[rng.random(n_unitigs) < 0.05] = 0
    return bits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="chr1", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--colors", default="5,130,4096")
    ap.add_argument("--distinct", default="1000,1000000")
    ap.add_argument("--host-steps", type=int, default=3, help="repeats of the host route and of compact / expand")
    a = ap.parse_args()
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    n_reads = (a.reads or n_reads) & ~1
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    reads = synth.reads(g, n_reads, read_len=read_len, seed=synth.SEED_READS)
    batch = idx.batch(reads.as_tuple())
    nu = idx.n_unitigs
    print("workload %s: %d unitigs, %d reads per step, %d k-mers, set up in %.1f s" % (a.workload, nu, n_reads, batch.n_kmers, time.time() - t0), flush=True)
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    L = fa.lib()
    err = C.create_string_buffer(512)
    rng = np.random.default_rng(38)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ts); rc = f(); e1.record(ts); torch.cuda.synchronize()
        assert rc == 0, err.value
        return e0.elapsed_time(e1)

    batch.text_mode(2)
    batch.run(fa.FIN_MERGED, stream)
    torch.cuda.synchronize()
    for n_colors in [int(x) for x in a.colors.split(",")]:
        W = (n_colors + 63) // 64
        for distinct in [int(x) for x in a.distinct.split(",")]:
            if n_colors < 12 and distinct > (1 << n_colors) - 1:
                distinct = (1 << n_colors) // 2       # (5 colours have 31 non-empty sets)
            bits = matrix(rng, nu, n_colors, min(distinct, nu // 2))
            dense, col = idx.colors(n_colors, bits), idx.colors(n_colors, bits)
            # ---- (a) compact / expand against the host route
            col.compact(); n_sets = col.n_sets; st = col.compact_stats(); col.expand()       # (a first launch of every kernel, not counted)
            t_c, t_e = [], []
            for _ in range(a.host_steps):
                torch.cuda.synchronize()
                w = time.perf_counter(); col.compact(); t_c.append(1e3 * (time.perf_counter() - w))
                w = time.perf_counter(); col.expand(); t_e.append(1e3 * (time.perf_counter() - w))
            t_dl, t_tw, t_ul = [], [], []
            host = idx.colors(n_colors, bits)
            for _ in range(a.host_steps):
                w0 = time.perf_counter(); m = host.download()[0]
                w1 = time.perf_counter(); so, se = fa.unitig_color_sets(m, n_colors, 16)
                w2 = time.perf_counter(); host.upload_sets(so, se)
                w3 = time.perf_counter()
                t_dl.append(1e3 * (w1 - w0)); t_tw.append(1e3 * (w2 - w1)); t_ul.append(1e3 * (w3 - w2))
                host.upload(bits)
            col.compact()
            assert len(se) - 1 == n_sets and np.array_equal(col.download()[0], bits)
            host.close()
            b_dense, b_compact = 8 * W * nu + 8, 4 * nu + 16 + 8 * W * (n_sets + 1)
            print("%d colours (W = %d), %d unitigs, %d sets (table of %d slots, longest probe %d, %d rows met a foreign row under their tag)" % (
                n_colors, W, nu, n_sets, st[3], st[2], st[1]))
            print("  (a) compact() %s | expand() %s" % (med(t_c), med(t_e)))
            print("      host route: download %s + fin_unitig_color_sets on 16 threads %s + upload_sets %s" % (med(t_dl), med(t_tw), med(t_ul)))
            print("  (c) HBM: dense %d bytes, compact %d bytes (%.1f %%)" % (b_dense, b_compact, 100.0 * b_compact / b_dense), flush=True)
            # ---- (b) per step
            ways = [("pseudoalign dense", lambda: L.fin_batch_pseudoalign(batch.h, dense.h, 1000, err, 512)),
                    ("pseudoalign compact", lambda: L.fin_batch_pseudoalign(batch.h, col.h, 1000, err, 512)),
                    ("paired dense", lambda: L.fin_batch_pseudoalign_paired(batch.h, dense.h, 1000, 0, err, 512)),
                    ("paired compact", lambda: L.fin_batch_pseudoalign_paired(batch.h, col.h, 1000, 0, err, 512))]
            r_d, r_c = batch.pseudoalign(dense), batch.pseudoalign(col)
            assert np.array_equal(r_d[0], r_c[0]) and np.array_equal(r_d[1], r_c[1]), "rows under the two states differ"
            f_d, f_c = batch.pseudoalign_pairs(dense), batch.pseudoalign_pairs(col)
            assert np.array_equal(f_d[0], f_c[0]) and np.array_equal(f_d[1], f_c[1]), "fragment rows under the two states differ"
            del r_d, r_c, f_d, f_c
            t = {name: [] for name, _ in ways}
            for s in range(a.steps + 1):   # (round 0 not counted; the order rotates)
                for name, f in ways[s % 4:] + ways[:s % 4]:
                    ms = timed(f)
                    if s:
                        t[name].append(ms)
            for name, _ in ways:
                print("  (b) %-22s %s" % (name + ":", med(t[name])))
            for kind_ in ("pseudoalign", "paired"):
                d, c = statistics.median(t[kind_ + " dense"]), statistics.median(t[kind_ + " compact"])
                print("      %s: compact / dense = %.3f%s" % (kind_, c / d, "  ** SLOWER **" if c > 1.02 * d else ""), flush=True)
            dense.close(); col.close()
    batch.close(); idx.close()


if __name__ == "__main__":
    main()
