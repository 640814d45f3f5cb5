#!/usr/bin/env python3
"""What the per-unitig profile costs on the device (fin_batch_add_hits, fin_hits.hip) -- `python3 tools/ab_hits.py [workload] [--reads N] [--rounds R]`.

The workload is built the way bench.py builds it (same seeds, same sizes; default chr1).  Everything is timed with HIP events on one stream, the legs
INTERLEAVED round by round in one process (leg A, leg B, ... then again), the first round dropped, median and min..max over the rest:

  1. the step in text mode 2 alone                      -- the comparison base: it exists without this feature (`--base-only` prints only this leg and
                                                           the mode-0 step, for a build of the parent commit)
  2. that step + fin_batch_add_hits                     -- (2) - (1) is the profile's cost; the add kernel alone is timed too, for every `hits_combine`
  3. the default step (mode 0) + fin_batch_add_hits     -- every read through the pair scan; (mode 0) - (mode 2) is what the pair traffic costs
  4. from pinned host buffers, k-mers/s: unitig_counts | search_reads_records + records_unitig_counts on the host | search_reads + np.bincount
  5. contention: an index of 1 and of 3 unitigs, 200 000 reads each, the add kernel's time for every `hits_combine` (recorded, not bounded)
"""
import argparse
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
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--base-only", action="store_true")
    ap.add_argument("--no-host", action="store_true", help="skip leg 4")
    ap.add_argument("--no-contention", action="store_true", help="skip leg 5")
    ap.add_argument("--one-step", action="store_true", help="one mode-2 step + add and nothing else (for a kernel trace)")
    a = ap.parse_args()
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    n_reads = a.reads or n_reads
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    reads = synth.reads(g, n_reads, read_len=read_len, seed=synth.SEED_READS)
    batch = idx.batch(reads.as_tuple())
    print("workload %s: %d unitigs, %d reads, %d k-mers, set up in %.1f s" % (a.workload, idx.n_unitigs, n_reads, batch.n_kmers, time.time() - t0), flush=True)
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    has_hits = hasattr(fa, "Hits") and not a.base_only
    hits = idx.hits() if has_hits else None

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def leg(mode, add):
        batch.text_mode(mode)
        e0, e1, e2 = ev(), ev(), ev()
        e0.record(ts); batch.run(fa.FIN_MERGED, stream); e1.record(ts)
        if add:
            hits.add(batch, stream)
        e2.record(ts)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), e1.elapsed_time(e2)

    if a.one_step:
        for _ in range(3):
            leg(2, True)
        print("three mode-2 steps + add done; found %d" % hits.download()[1])
        return
    legs = [("mode 2 step", 2, False), ("mode 0 step", 0, False)]
    if has_hits:
        legs += [("mode 2 step + add", 2, True), ("mode 0 step + add", 0, True)]
    res = {name: ([], []) for name, _, _ in legs}
    for rnd in range(a.rounds + 1):
        for name, mode, add in legs:
            s, h = leg(mode, add)
            if rnd:
                res[name][0].append(s); res[name][1].append(h)
    for name, _, add in legs:
        print("%-20s step %s%s" % (name, med(res[name][0]), ("   add kernel " + med(res[name][1])) if add else ""), flush=True)
    m2, m0 = statistics.median(res["mode 2 step"][0]), statistics.median(res["mode 0 step"][0])
    print("pair traffic of the fast path's reads (mode 0 - mode 2): %.3f ms" % (m0 - m2))
    if has_hits:
        t2 = statistics.median([s + h for s, h in zip(*res["mode 2 step + add"])])
        t0_ = statistics.median([s + h for s, h in zip(*res["mode 0 step + add"])])
        print("profile's cost, (2) - (1): %.3f ms = %.1f %% of the mode-2 step; mode 0 + add - mode 0: %.3f ms" % (t2 - m2, 100.0 * (t2 - m2) / m2, t0_ - m0))
        _, total = hits.reset().add(batch, stream).download()
        print("found k-mers in the profile: %d of %d" % (total, batch.n_kmers))
        # the add kernel alone, variant by variant, interleaved
        variants = (0, 1, 2, 4, 8, 64)
        for mode in (2, 0):
            batch.text_mode(mode); batch.run(fa.FIN_MERGED, stream)
            tv = {v: [] for v in variants}
            for rnd in range(a.rounds + 1):
                for v in variants:
                    idx.set_option("hits_combine", v)
                    e0, e1 = ev(), ev()
                    e0.record(ts); hits.add(batch, stream); e1.record(ts); torch.cuda.synchronize()
                    if rnd:
                        tv[v].append(e0.elapsed_time(e1))
            idx.set_option("hits_combine", None)
            for v in variants:
                print("add kernel behind a mode-%d step, hits_combine %2d: %s" % (mode, v, med(tv[v])), flush=True)
    if has_hits and not a.no_host:
        ns = min(n_reads, 2_000_000)
        sub = reads.subset(0, ns)
        pin = fa.PinnedArray((ns * read_len,), np.uint8)
        pin.array[:] = sub.bases
        rd = (pin.array, sub.offsets)
        nk = ns * max(0, read_len - k + 1)
        pout = fa.PinnedArray((max(nk, 1), 2), np.int32)

        def host_counts():
            return idx.unitig_counts(rd)[0]

        def host_records():
            recs, stream_pairs = idx.search_reads_records(rd)
            return fa.records_unitig_counts(recs, stream_pairs, k, idx.n_unitigs)

        def host_pairs():
            pairs, _ = idx.search_reads(rd, fa.FIN_MERGED, out=pout.array)
            uu = pairs[:, 0]
            return np.bincount(uu[uu >= 0], minlength=idx.n_unitigs).astype(np.uint64)

        ways = (("unitig_counts", host_counts), ("search_reads_records + records_unitig_counts", host_records), ("search_reads + np.bincount", host_pairs))
        tw = {n: [] for n, _ in ways}
        outs = {}
        for rnd in range(4):
            for name, f in ways:
                t = time.perf_counter(); outs[name] = f(); dt = time.perf_counter() - t
                if rnd:
                    tw[name].append(dt)
        for name, _ in ways:
            assert np.array_equal(outs[name], outs["unitig_counts"]), name
            print("host buffers, %-46s %.3e k-mers/s (median of %d, %d reads)" % (name + ":", nk / statistics.median(tw[name]), len(tw[name]), ns), flush=True)
        pin.close(); pout.close()
    batch.close()
    if has_hits and not a.no_contention:
        for nu in (1, 3):
            gg = synth.genome(30000, seed=7 + nu)
            gs = gg.tobytes().decode()
            cuts = [0, len(gs)] if nu == 1 else [0, 9000, 21000, len(gs)]
            small = fa.FinimizerIndex.build([gs[max(0, x - 30) if x else 0:y] for x, y in zip(cuts[:-1], cuts[1:])], 31).to_device(0)
            rd = synth.reads(gg, 200_000, seed=11)
            b = small.batch(rd.as_tuple())
            h = small.hits()
            for mode in (2, 0):
                b.text_mode(mode); b.run(fa.FIN_MERGED, stream)
                want = None
                for v in (0, 1, 4):
                    small.set_option("hits_combine", v)
                    tt = []
                    for rnd in range(6):
                        h.reset(stream)
                        e0, e1 = ev(), ev()
                        e0.record(ts); h.add(b, stream); e1.record(ts); torch.cuda.synchronize()
                        if rnd:
                            tt.append(e0.elapsed_time(e1))
                    c, tot = h.download()
                    want = c if want is None else want
                    assert np.array_equal(c, want)
                    print("contention: %d unitig(s), 200000 reads, mode %d, hits_combine %d: add kernel %s, found %d" % (nu, mode, v, med(tt), tot), flush=True)
            small.set_option("hits_combine", None)
            h.close(); b.close(); small.close()


if __name__ == "__main__":
    main()
