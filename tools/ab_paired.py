#!/usr/bin/env python3
"""What paired-end pseudoalignment costs on the device (fin_batch_pseudoalign_paired, fin_batch_add_eqclasses_paired; fin_paired.hip), against what the library
offered for the same answer before -- `python3 tools/ab_paired.py [workload] [--reads N] [--steps S] [--sets M] [--colors 5,130,4096]`.

The workload is built the way bench.py builds it (same seeds, same sizes; default chr1); the method is tools/ab_colors.py's: HIP events on one stream, the
variants interleaved in one process, text mode 2, and its matrix.  Reads 2f and 2f + 1 of a set are taken as the mates of fragment f.

  steps 1..S over M sets of FRESH reads, each step followed by, each timed by itself with HIP events:
  fin_batch_pseudoalign_paired (permille 1000) | fin_batch_pseudoalign | fin_batch_add_eqclasses_paired | fin_batch_add_eqclasses; and, host wall clock: the per-read
  rows' download | the numpy AND-or-other over them (the AND of the mates' rows where both have coloured k-mers, else the row of the one that has).  The numpy
  result must equal the device's fragment rows.  Medians over the steps; the second comparison shows half the rows going into the table.
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
    a = ap.parse_args()
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    n_reads = (a.reads or n_reads) & ~1
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    sets = [synth.reads(g, n_reads, read_len=read_len, seed=synth.SEED_READS + 1000 * s) for s in range(a.sets)]
    batch = idx.batch(sets[0].as_tuple())
    nu = idx.n_unitigs
    print("workload %s: %d unitigs, %d bases, %d reads = %d fragments per step, %d k-mers, set up in %.1f s"
          % (a.workload, nu, idx.total_len, n_reads, n_reads // 2, batch.n_kmers, time.time() - t0), flush=True)
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
        member = ((np.arange(nu, dtype=np.uint64)[:, None] * np.uint64(2654435761) + np.arange(n_colors, dtype=np.uint64)[None, :] * np.uint64(40503)) % np.uint64(7) < 2)
        member[::16] = False
        wide = np.zeros((nu, 64 * W), dtype=np.uint8); wide[:, :n_colors] = member
        bits = np.ascontiguousarray(np.packbits(wide, axis=1, bitorder="little")).view(np.uint64).reshape(nu, W)
        del member, wide
        col = idx.colors(n_colors, bits)
        eq_f, eq_r = col.eqclasses(1 << 20), col.eqclasses(1 << 20)
        ways = [("pseudoalign_paired", lambda: L.fin_batch_pseudoalign_paired(batch.h, col.h, 1000, fa.FIN_PAIR_ANY, err, 512)),
                ("pseudoalign", lambda: L.fin_batch_pseudoalign(batch.h, col.h, 1000, err, 512)),
                ("add_eqclasses_paired", lambda: L.fin_batch_add_eqclasses_paired(batch.h, eq_f.h, 1000, fa.FIN_PAIR_ANY, C.c_void_p(stream), err, 512)),
                ("add_eqclasses", lambda: L.fin_batch_add_eqclasses(batch.h, eq_r.h, 1000, C.c_void_p(stream), err, 512))]
        t = {name: [] for name, _ in ways}
        t_step, t_dl, t_np = [], [], []
        for s in range(a.steps + 1):   # (step 0: a first launch of every kernel, not counted)
            batch.reload(sets[s % a.sets].as_tuple())
            ms = timed(lambda: batch.run(fa.FIN_MERGED, stream) or 0)
            order = ways[s % 4:] + ways[:s % 4]   # (interleaved: each goes first .. fourth in turn)
            got = {name: timed(f) for name, f in order}
            frows, fheads = batch.pseudoalign_pairs(col, 1000)
            w0 = time.perf_counter(); rows, heads = batch.pseudoalign(col, 1000); w1 = time.perf_counter()
            ca, cb = heads["n_colored"][0::2] > 0, heads["n_colored"][1::2] > 0
            ra, rb = rows[0::2], rows[1::2]
            host = np.where((ca & cb)[:, None], ra & rb, np.where(ca[:, None], ra, rb)); w2 = time.perf_counter()
            assert np.array_equal(host, frows), "the AND-or-other over the per-read rows differs from the device's fragment rows"
            assert np.array_equal(fheads["n_colored"], heads["n_colored"][0::2] + heads["n_colored"][1::2])
            if s == 0:
                continue
            t_step.append(ms)
            for name, _ in ways:
                t[name].append(got[name])
            t_dl.append(1e3 * (w1 - w0)); t_np.append(1e3 * (w2 - w1))
            print("%d colours, step %d: step %.3f ms | %s" % (n_colors, s, ms, " | ".join("%s %.3f ms" % (name, got[name]) for name, _ in ways)), flush=True)
        print("%d colours (%d words per row), medians over %d steps, text mode 2: step %s" % (n_colors, W, a.steps, med(t_step)))
        for name, _ in ways:
            print("  fin_batch_%-22s %s" % (name + ":", med(t[name])))
        print("  host wall clock: per-read rows made + downloaded %s | numpy AND-or-other %s" % (med(t_dl), med(t_np)))
        print("  bytes to the host per fragment by the old route: %d; classes: %d from fragments, %d from reads" % (2 * (8 * W + 16), eq_f.stats()[2], eq_r.stats()[2]), flush=True)
        eq_f.close(); eq_r.close(); col.close()
    batch.close()


if __name__ == "__main__":
    main()
