#!/usr/bin/env python3
"""What pseudoalignment against colour sets and colouring by search cost on the device (fin_batch_pseudoalign, fin_batch_add_colors; fin_colors.hip), against the
cheapest other route to the same numbers: segments + a gather of the colour rows and a reduction per read on the host -- `python3 tools/ab_colors.py [workload]
[--reads N] [--steps S] [--sets M] [--colors C] [--permille P]`.

The workload is built the way bench.py builds it (same seeds, same sizes; default chr1); the method is tools/ab_classify.py's: HIP events on one stream, the
variants interleaved in one process, text mode 2.  The matrix: C colours (default 100), unitig u has colour c when (u * 2654435761 + c * 40503) % 7 < 2, every
16th unitig has none.

  steps 1..S over M sets of FRESH reads (another seed per set, reloaded in turn), each step followed by, each timed by itself with HIP events:
  fin_batch_pseudoalign | fin_batch_add_colors | fin_batch_read_summaries (a sibling that reads the same records and pairs) | fin_batch_segments (count + scan +
  write; includes its wait for the count); and, host wall clock: the rows' download | the segments' download + the numpy reduction to the same rows and heads.
  The reduction's result must equal the device's.  Medians over the steps, bytes to the host per read.
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


def reduce_segments(seg_offs, segs, n_reads, member, permille):
    """rows (0/1 [n_reads, n_colors]) and heads from the segments, in numpy: a segment of |len| slots in unitig u is |len| counts for every colour of u"""
    n_colors = member.shape[1]
    heads = np.zeros(n_reads, dtype=fa.READ_PSEUDO_DTYPE)
    cnt = np.zeros((n_reads, n_colors), dtype=np.int64)
    if len(segs):
        read = np.repeat(np.arange(n_reads, dtype=np.int64), np.diff(seg_offs.astype(np.int64)))
        n = np.abs(segs["len"].astype(np.int64))
        m = member[segs["u"]]
        np.add.at(cnt, read, m * n[:, None])
        heads["n_found"] = np.bincount(read, weights=n, minlength=n_reads).astype(np.uint32)
        heads["n_colored"] = np.bincount(read, weights=n * m.any(axis=1), minlength=n_reads).astype(np.uint32)
    inside = (cnt >= 1) & (1000 * cnt >= permille * heads["n_colored"].astype(np.int64)[:, None])
    heads["n_colors"] = inside.sum(axis=1)
    return inside, heads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="chr1", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--colors", type=int, default=100)
    ap.add_argument("--permille", type=int, default=1000)
    a = ap.parse_args()
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    n_reads = a.reads or n_reads
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    sets = [synth.reads(g, n_reads, read_len=read_len, seed=synth.SEED_READS + 1000 * s) for s in range(a.sets)]
    batch = idx.batch(sets[0].as_tuple())
    nu, W = idx.n_unitigs, (a.colors + 63) // 64
    member = ((np.arange(nu, dtype=np.uint64)[:, None] * np.uint64(2654435761) + np.arange(a.colors, dtype=np.uint64)[None, :] * np.uint64(40503)) % np.uint64(7) < 2)
    member[::16] = False
    wide = np.zeros((nu, 64 * W), dtype=np.uint8); wide[:, :a.colors] = member
    bits = np.ascontiguousarray(np.packbits(wide, axis=1, bitorder="little")).view(np.uint64).reshape(nu, W)
    col = idx.colors(a.colors, bits)
    paint = idx.colors(a.colors)
    print("workload %s: %d unitigs, %d bases, %d reads per step, %d k-mers, %d colours (%d words per row), set up in %.1f s"
          % (a.workload, nu, idx.total_len, n_reads, batch.n_kmers, a.colors, W, time.time() - t0), flush=True)
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    L = fa.lib()
    err = C.create_string_buffer(512)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ts); rc = f(); e1.record(ts); torch.cuda.synchronize()
        assert rc == 0, err.value
        return e0.elapsed_time(e1)

    n_seg = C.c_uint64(0)
    ways = [("pseudoalign", lambda: L.fin_batch_pseudoalign(batch.h, col.h, a.permille, err, 512)),
            ("add_colors", lambda: L.fin_batch_add_colors(batch.h, paint.h, 0, C.c_void_p(stream), err, 512)),
            ("read_summaries", lambda: L.fin_batch_read_summaries(batch.h, err, 512)),
            ("segments", lambda: L.fin_batch_segments(batch.h, C.byref(n_seg), err, 512))]
    t = {name: [] for name, _ in ways}
    t_step, t_dl_rows, t_dl_seg, t_reduce = [], [], [], []
    batch.text_mode(2)
    for s in range(a.steps + 1):   # (step 0: a first launch of every kernel, not counted)
        batch.reload(sets[s % a.sets].as_tuple())
        ms = timed(lambda: batch.run(fa.FIN_MERGED, stream) or 0)
        order = ways[s % 4:] + ways[:s % 4]   # (interleaved: each goes first .. fourth in turn)
        got = {name: timed(f) for name, f in order}
        w0 = time.perf_counter(); rows, heads = batch.pseudoalign(col, a.permille); w1 = time.perf_counter()
        seg_offs, segs = batch.segments(); w2 = time.perf_counter()
        inside, rheads = reduce_segments(seg_offs, segs, n_reads, member, a.permille); w3 = time.perf_counter()
        got_inside = np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=1, bitorder="little")[:, :a.colors].astype(bool)
        assert np.array_equal(got_inside, inside) and np.array_equal(heads, rheads), "the reduction of the segments differs from the device's rows"
        if s == 0:
            continue
        t_step.append(ms)
        for name, _ in ways:
            t[name].append(got[name])
        t_dl_rows.append(1e3 * (w1 - w0)); t_dl_seg.append(1e3 * (w2 - w1)); t_reduce.append(1e3 * (w3 - w2))
        print("step %d: step %.3f ms | %s" % (s, ms, " | ".join("%s %.3f ms" % (name, got[name]) for name, _ in ways)), flush=True)
    print("medians over %d steps, text mode 2: step %s" % (a.steps, med(t_step)))
    for name, _ in ways:
        print("  fin_batch_%-16s %s" % (name + ":", med(t[name])))
    print("  host wall clock: rows made + downloaded %s | segments made + downloaded %s | numpy reduction %s" % (med(t_dl_rows), med(t_dl_seg), med(t_reduce)))
    print("  bytes to the host per read: rows %d + heads 16 | segments %.1f (%d segments)" % (8 * W, (16 * n_seg.value + 8 * (n_reads + 1)) / n_reads, n_seg.value), flush=True)
    col.close(); paint.close()
    batch.close()


if __name__ == "__main__":
    main()
