#!/usr/bin/env python3
"""What the fragment geometry costs on the device (fin_batch_add_fragments, fin_batch_fragments; fin_fragments.hip), against the route a user had before and
against a sibling of the same shape -- `python3 tools/ab_fragments.py [workload] [--reads N] [--steps S] [--sets M] [--bins B]`.

The workload is built the way bench.py builds it (same seeds, same sizes; default chr1: 10 M reads = 5 M fragments); the method is tools/ab_paired.py's: HIP events
on one stream, the variants interleaved in one process, text mode 2.  Reads 2f and 2f + 1 of a set are taken as the mates of fragment f (synthetic reads are
drawn one by one: few fragments are inward, which costs the kernel nothing less -- every mate is placed or scanned all the same).

  steps 1..S over M sets of FRESH reads, each step followed by, each timed by itself with HIP events:
  fin_batch_add_fragments (B bins of 1) | fin_batch_fragments | fin_batch_pseudoalign_paired (5 colours, permille 1000: a sibling of the same shape); and, host wall
  clock: fin_batch_records + fin_batch_download_records | fin_records_fragments on 16 threads.  The host twin's fragments and counters must equal the device's.
  Medians over the steps.
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
    ap.add_argument("--bins", type=int, default=1024)
    a = ap.parse_args()
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    n_reads = (a.reads or n_reads) & ~1
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    sets = [synth.reads(g, n_reads, read_len=read_len, seed=synth.SEED_READS + 1000 * s) for s in range(a.sets)]
    batch = idx.batch(sets[0].as_tuple())
    nu = idx.n_unitigs
    ends = idx.export(fa.X_ENDS)
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
    n_colors = 5
    member = ((np.arange(nu, dtype=np.uint64)[:, None] * np.uint64(2654435761) + np.arange(n_colors, dtype=np.uint64)[None, :] * np.uint64(40503)) % np.uint64(7) < 2)
    wide = np.zeros((nu, 64), dtype=np.uint8); wide[:, :n_colors] = member
    col = idx.colors(n_colors, np.ascontiguousarray(np.packbits(wide, axis=1, bitorder="little")).view(np.uint64).reshape(nu, 1))
    del member, wide
    acc = idx.fragments(a.bins, 1)
    ways = [("add_fragments", lambda: L.fin_batch_add_fragments(batch.h, acc.h, C.c_void_p(stream), err, 512)),
            ("fragments", lambda: L.fin_batch_fragments(batch.h, None, err, 512)),
            ("pseudoalign_paired", lambda: L.fin_batch_pseudoalign_paired(batch.h, col.h, 1000, fa.FIN_PAIR_ANY, err, 512))]
    t = {name: [] for name, _ in ways}
    t_step, t_dl, t_host = [], [], []
    for s in range(a.steps + 1):   # (step 0: a first launch of every kernel, not counted)
        batch.reload(sets[s % a.sets].as_tuple())
        ms = timed(lambda: batch.run(fa.FIN_MERGED, stream) or 0)
        acc.reset(stream)
        order = ways[s % 3:] + ways[:s % 3]   # (interleaved: each goes first .. third in turn)
        got = {name: timed(f) for name, f in order}
        frags, st = batch.fragments(), acc.download()
        w0 = time.perf_counter(); recs, pairs = batch.records(); w1 = time.perf_counter()
        hfrags, hhist, hcnt = fa.records_fragments(recs, pairs, k, ends, a.bins, 1, 16); w2 = time.perf_counter()
        assert hfrags.tobytes() == frags.tobytes(), "the host twin's fragments differ from the device's"
        assert np.array_equal(hhist, st.hist) and np.array_equal(hcnt, st.counters), "the host twin's histogram or counters differ from the device's"
        if s == 0:
            print("classes none / one / split / tandem / outward / inward: %s; %d of the reads are kind-1 records" % (st.counters[:6].tolist(), int((recs["meta"] >> 16 == 1).sum())), flush=True)
            continue
        t_step.append(ms)
        for name, _ in ways:
            t[name].append(got[name])
        t_dl.append(1e3 * (w1 - w0)); t_host.append(1e3 * (w2 - w1))
        print("step %d: step %.3f ms | %s | records downloaded %.1f ms | twin %.1f ms" % (s, ms, " | ".join("%s %.3f ms" % (name, got[name]) for name, _ in ways), t_dl[-1], t_host[-1]), flush=True)
    print("%d bins of 1, medians over %d steps, text mode 2: step %s" % (a.bins, a.steps, med(t_step)))
    for name, _ in ways:
        print("  fin_batch_%-22s %s" % (name + ":", med(t[name])))
    print("  host wall clock: fin_batch_records + fin_batch_download_records %s | fin_records_fragments on 16 threads %s" % (med(t_dl), med(t_host)))
    print("  bytes to the host per fragment by the old route: 64 of records plus the searched reads' pairs", flush=True)
    acc.close(); col.close(); batch.close()


if __name__ == "__main__":
    main()
