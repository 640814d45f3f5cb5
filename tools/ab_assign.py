#!/usr/bin/env python3
"""What assigning reads to references costs on the device (fin_assign_rows, fin_batch_assign; fin_assign.hip), against the route it replaces --
`python3 tools/ab_assign.py [workload] [--rows N] [--steps S] [--colors 5,130,4096] [--no-batch]`.

Part 1, synthetic rows: N rows (default 10 M; 2 M at 4096 colours, as tools/ab_paired.py's matrix bounds it) of 1 to 8 colours each, in HBM.  Timed with HIP
events on one stream, medians of S (default 20): fin_assign_rows with rows and heads written | with the counts alone.  Against it, host wall clock: the rows'
download | fin_rows_assign on 16 host threads.  Device and host results must be equal.

Part 2, behind a search step (the workload is built the way bench.py builds it, text mode 2): fin_batch_pseudoalign alone | fin_batch_assign (which pseudoaligns
first), each behind a fresh step, HIP events.
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


def make_rows(rng, n, n_colors):
    W = (n_colors + 63) // 64
    sizes = rng.integers(1, min(8, n_colors) + 1, n)
    jj = np.repeat(np.arange(n), sizes)
    cc = rng.integers(0, n_colors, len(jj))
    rows = np.zeros((n, W), dtype=np.uint64)
    np.bitwise_or.at(rows, (jj, cc >> 6), np.uint64(1) << (cc & 63).astype(np.uint64))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="chr1", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--colors", default="5,130,4096")
    ap.add_argument("--no-batch", action="store_true")
    a = ap.parse_args()
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    nu = idx.n_unitigs
    print("workload %s: %d unitigs, set up in %.1f s" % (a.workload, nu, time.time() - t0), flush=True)
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    L = fa.lib()
    err = C.create_string_buffer(512)
    rng = np.random.default_rng(32)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ts); rc = f(); e1.record(ts); torch.cuda.synchronize()
        assert rc == 0, err.value
        return e0.elapsed_time(e1)

    batch = None
    if not a.no_batch:
        sets = [synth.reads(g, n_reads, read_len=read_len, seed=synth.SEED_READS + 1000 * s) for s in range(4)]
        batch = idx.batch(sets[0].as_tuple())
        batch.text_mode(2)
    for n_colors in [int(x) for x in a.colors.split(",")]:
        W = (n_colors + 63) // 64
        n = min(a.rows, 2_000_000) if n_colors > 1024 else a.rows
        col = idx.colors(n_colors)
        x = rng.uniform(0.0, 1.0, n_colors) * 10.0 ** rng.integers(-3, 3, n_colors)
        asg = col.assigner(x, 0.5)
        rows = make_rows(rng, n, n_colors)
        d_rows = torch.from_numpy(rows.view(np.int64)).cuda()
        d_out = torch.zeros((n, W), dtype=torch.int64, device="cuda")
        d_heads = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        full = lambda: L.fin_assign_rows(asg.h, C.c_void_p(d_rows.data_ptr()), n, C.c_void_p(d_out.data_ptr()), C.c_void_p(d_heads.data_ptr()), C.c_void_p(stream), err, 512)
        counts = lambda: L.fin_assign_rows(asg.h, C.c_void_p(d_rows.data_ptr()), n, None, None, C.c_void_p(stream), err, 512)
        timed(full); timed(counts)   # (a first launch, not counted)
        t_full, t_counts = [], []
        for s in range(a.steps):
            for name, f in ((("full", full), ("counts", counts)) if s % 2 == 0 else (("counts", counts), ("full", full))):   # (interleaved)
                (t_full if name == "full" else t_counts).append(timed(f))
        asg.reset()
        timed(full)
        dev = (d_out.cpu().numpy().view(np.uint64), np.ascontiguousarray(d_heads.cpu().numpy()).view(fa.READ_ASSIGN_DTYPE).reshape(-1)) + asg.download()
        t_dl, t_host = [], []
        host_rows = np.zeros_like(rows)
        for s in range(3):
            w0 = time.perf_counter()
            host_rows[:] = d_rows.cpu().numpy().view(np.uint64)
            w1 = time.perf_counter()
            host = fa.rows_assign(host_rows, n_colors, x, 0.5, n_threads=16)
            w2 = time.perf_counter()
            t_dl.append(1e3 * (w1 - w0)); t_host.append(1e3 * (w2 - w1))
        for d, h, name in zip(dev, host, ("rows", "heads", "assigned", "sole", "counters")):
            assert d.tobytes() == h.tobytes(), "device and host differ in " + name
        print("%d colours (%d words per row), %d rows of 1 to 8 colours, %d bytes of rows:" % (n_colors, W, n, rows.nbytes))
        print("  fin_assign_rows, rows + heads written: %s" % med(t_full))
        print("  fin_assign_rows, counts alone:         %s" % med(t_counts))
        print("  host wall clock (3 runs): the rows' download %s | fin_rows_assign on 16 threads %s" % (med(t_dl), med(t_host)))
        print("  counters {rows, unaligned, unassigned, multi}: %s" % [int(v) for v in dev[4]], flush=True)
        del d_rows, d_out, d_heads
        if batch is not None:
            member = ((np.arange(nu, dtype=np.uint64)[:, None] * np.uint64(2654435761) + np.arange(n_colors, dtype=np.uint64)[None, :] * np.uint64(40503)) % np.uint64(7) < 2)
            member[::16] = False
            wide = np.zeros((nu, 64 * W), dtype=np.uint8); wide[:, :n_colors] = member
            col.upload(np.ascontiguousarray(np.packbits(wide, axis=1, bitorder="little")).view(np.uint64).reshape(nu, W))
            del member, wide
            asg.reset()
            ways = [("pseudoalign", lambda: L.fin_batch_pseudoalign(batch.h, col.h, 1000, err, 512)),
                    ("assign", lambda: L.fin_batch_assign(batch.h, asg.h, 1000, 0, C.c_void_p(stream), err, 512))]
            t = {name: [] for name, _ in ways}
            t_step = []
            for s in range(a.steps + 1):   # (step 0: a first launch of every kernel, not counted)
                batch.reload(sets[s % 4].as_tuple())
                ms = timed(lambda: batch.run(fa.FIN_MERGED, stream) or 0)
                got = {name: timed(f) for name, f in (ways if s % 2 == 0 else ways[::-1])}
                if s == 0:
                    continue
                t_step.append(ms)
                for name, _ in ways:
                    t[name].append(got[name])
            print("  behind a %s step of %d reads, text mode 2: step %s" % (a.workload, n_reads, med(t_step)))
            print("    fin_batch_pseudoalign alone:                   %s" % med(t["pseudoalign"]))
            print("    fin_batch_assign (pseudoalign, then assign):   %s" % med(t["assign"]), flush=True)
        asg.close(); col.close()
    if batch is not None:
        batch.close()


if __name__ == "__main__":
    main()
