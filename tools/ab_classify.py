#!/usr/bin/env python3
"""What classifying reads by unitig labels costs on the device (fin_batch_classify, fin_batch_add_classes; fin_classify.hip), against the cheapest other route to
the same numbers: segments + a gather of the labels and a bincount per read on the host -- `python3 tools/ab_classify.py [workload] [--reads N] [--steps S]
[--sets M] [--labels L]`.

The workload is built the way bench.py builds it (same seeds, same sizes; default chr1); the method is tools/ab_readsum.py's: HIP events on one stream, the
variants interleaved in one process, text mode 2.  The labelling: L labels (default 10) over contiguous runs of unitig numbers, every 16th unitig without one.

  1. steps 1..S over M sets of FRESH reads (another seed per set, reloaded in turn), each step followed by, each timed by itself with HIP events:
     fin_batch_classify | fin_batch_add_classes behind it (the tally alone) | fin_batch_read_summaries (the sibling whose cost the classes should be close to) |
     fin_batch_segments (count + scan + write; includes its wait for the count); and, host wall clock: the classes' download | the segments' download + the numpy
     gather / bincount to the same four numbers.  The reduction's result must equal the device's classes.  Medians over the steps, bytes to the host per read.
  2. from pinned host buffers, k-mers/s: classify_reads | Labels.add_reads | search_reads_segments + the reduction
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


def reduce_segments(seg_offs, segs, n_reads, labels, n_labels):
    """the four numbers of a read class from its segments, in numpy: a segment of |len| slots in unitig u is |len| votes for labels[u]"""
    out = np.zeros(n_reads, dtype=fa.READ_CLASS_DTYPE)
    out["label"] = fa.FIN_NO_LABEL
    if not len(segs):
        return out
    read = np.repeat(np.arange(n_reads, dtype=np.int64), np.diff(seg_offs.astype(np.int64)))
    lab = labels[segs["u"]].astype(np.int64)
    named = lab != fa.FIN_NO_LABEL
    votes = np.bincount(read[named] * n_labels + lab[named], weights=np.abs(segs["len"].astype(np.int64))[named], minlength=n_reads * n_labels)
    votes = votes.astype(np.int64).reshape(n_reads, n_labels)
    best = votes.argmax(axis=1)   # (the first maximum: ties go to the smaller label)
    n_best = votes[np.arange(n_reads), best]
    votes[np.arange(n_reads), best] = -1
    has = n_best > 0
    out["label"][has] = best[has]
    out["n_best"] = n_best
    out["n_second"] = np.maximum(votes.max(axis=1), 0) if n_labels > 1 else 0
    out["n_labelled"] = n_best + np.maximum(votes, 0).sum(axis=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="chr1", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--labels", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip leg 2")
    a = ap.parse_args()
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    n_reads = a.reads or n_reads
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    sets = [synth.reads(g, n_reads, read_len=read_len, seed=synth.SEED_READS + 1000 * s) for s in range(a.sets)]
    batch = idx.batch(sets[0].as_tuple())
    labels = (np.arange(idx.n_unitigs, dtype=np.int64) * a.labels // max(idx.n_unitigs, 1)).astype(np.uint32)
    labels[::16] = fa.FIN_NO_LABEL
    lab = idx.labels(labels, a.labels)
    print("workload %s: %d unitigs, %d bases, %d reads per step, %d k-mers, %d labels, set up in %.1f s"
          % (a.workload, idx.n_unitigs, idx.total_len, n_reads, batch.n_kmers, a.labels, time.time() - t0), flush=True)
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
    ways = [("classify", lambda: L.fin_batch_classify(batch.h, lab.h, err, 512)),
            ("add_classes", lambda: L.fin_batch_add_classes(batch.h, lab.h, 1, 0, 0, C.c_void_p(stream), err, 512)),
            ("read_summaries", lambda: L.fin_batch_read_summaries(batch.h, err, 512)),
            ("segments", lambda: L.fin_batch_segments(batch.h, C.byref(n_seg), err, 512))]
    t = {name: [] for name, _ in ways}
    t_step, t_dl_cls, t_dl_seg, t_reduce = [], [], [], []
    batch.text_mode(2)
    for s in range(a.steps + 1):   # (step 0: a first launch of every kernel, not counted)
        batch.reload(sets[s % a.sets].as_tuple())
        ms = timed(lambda: batch.run(fa.FIN_MERGED, stream) or 0)
        order = ways[s % 4:] + ways[:s % 4]   # (interleaved: each goes first .. fourth in turn)
        got = {}
        for name, f in order:
            if name == "add_classes":   # (the tally alone: timed behind the classes, not instead of them)
                assert L.fin_batch_classify(batch.h, lab.h, err, 512) == 0
                torch.cuda.synchronize()
            got[name] = timed(f)
        w0 = time.perf_counter(); cls = batch.classify(lab); w1 = time.perf_counter()
        seg_offs, segs = batch.segments(); w2 = time.perf_counter()
        red = reduce_segments(seg_offs, segs, n_reads, labels, a.labels); w3 = time.perf_counter()
        assert np.array_equal(red, cls), "the reduction of the segments differs from the device's classes"
        if s == 0:
            continue
        t_step.append(ms)
        for name, _ in ways:
            t[name].append(got[name])
        t_dl_cls.append(1e3 * (w1 - w0)); t_dl_seg.append(1e3 * (w2 - w1)); t_reduce.append(1e3 * (w3 - w2))
        print("step %d: step %.3f ms | %s" % (s, ms, " | ".join("%s %.3f ms" % (name, got[name]) for name, _ in ways)), flush=True)
    tally, total = lab.download()
    assert total == (a.steps + 1) * n_reads, "the tally holds %d reads, %d were added" % (total, (a.steps + 1) * n_reads)
    print("medians over %d steps, text mode 2: step %s" % (a.steps, med(t_step)))
    for name, _ in ways:
        print("  fin_batch_%-16s %s" % (name + ":", med(t[name])))
    print("  host wall clock: classes made + downloaded %s | segments made + downloaded %s | numpy gather + bincount %s" % (med(t_dl_cls), med(t_dl_seg), med(t_reduce)))
    print("  bytes to the host per read: classes 16 | tally %.6f (%d bytes per run) | segments %.1f (%d segments)"
          % (8 * (a.labels + 1) / n_reads, 8 * (a.labels + 1), (16 * n_seg.value + 8 * (n_reads + 1)) / n_reads, n_seg.value), flush=True)
    if not a.no_host:
        ns = min(n_reads, 2_000_000)
        sub = sets[0].subset(0, ns)
        pin = fa.PinnedArray((ns * read_len,), np.uint8)
        pin.array[:] = sub.bases
        rd = (pin.array, sub.offsets)
        nk = ns * max(0, read_len - k + 1)

        def by_segments():
            so, sg, _ = idx.search_reads_segments(rd)
            return reduce_segments(so, sg, ns, labels, a.labels)
        host = (("classify_reads", lambda: idx.classify_reads(rd, lab)), ("Labels.add_reads", lambda: lab.add_reads(rd)),
                ("search_reads_segments + reduction", by_segments))
        tw = {n: [] for n, _ in host}
        outs = {}
        for rnd in range(6):
            for name, f in host:
                w = time.perf_counter(); outs[name] = f(); dt = time.perf_counter() - w
                if rnd:
                    tw[name].append(dt)
        assert np.array_equal(outs["classify_reads"], outs["search_reads_segments + reduction"])
        for name, _ in host:
            print("host buffers, %-36s %.3e k-mers/s (median of %d, %d reads)" % (name + ":", nk / statistics.median(tw[name]), len(tw[name]), ns), flush=True)
        pin.close()
    lab.close()
    batch.close()


if __name__ == "__main__":
    main()
