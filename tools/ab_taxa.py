#!/usr/bin/env python3
"""What the taxonomic classification costs on the device (fin_taxa.hip), each part against its yardstick --
`python3 tools/ab_taxa.py [workload] [--reads N] [--steps S] [--sets M]`.

The workload is built the way bench.py builds it (default chr1), as tools/ab_classify.py does; HIP events on one stream, the variants interleaved in one process,
text mode 2, medians over S steps (default 20).  The tree is synthetic: the colours are the leaves of a tree of fan-out 4, a unitig carries 1 to 8 colours out of
a window of 16 neighbouring ones.  At 5, 130 and 4096 colours:

  1. the labelling: fin_taxonomy_create_from_colors (the whole waiting call: allocations, the tree's upload, the LCA kernel) against the host route, the
     matrix's download + fin_unitig_lca_labels on 16 threads.  The two label arrays must be equal.
  2. per step, each timed by itself: fin_batch_classify under the same labels (the parent's kernel over the same bytes: the yardstick) | fin_batch_taxa at
     confidence 0 | fin_batch_taxa at confidence 100 (lifting) | fin_batch_add_taxa behind it (the tally alone); and, host wall clock, the host route: the
     records' download + fin_records_read_taxa on 16 threads, whose result must equal the device's.
  3. the roll-up at 10^4 and 10^6 taxa, over a tally the run's reads filled: fin_taxonomy_download with the clade counts minus the same call without them
     (the memset, the clade kernel and the second copy) against fin_taxa_clade_reads on the host, for a tree of logarithmic depth and for a deep one.
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


def leaf_tree(n_leaves, fan=4):
    """(parent, leaf taxa): a tree of fan-out `fan` whose last level are the n_leaves colours, numbered level by level from the root"""
    sizes = [n_leaves]
    while sizes[-1] > 1:
        sizes.append((sizes[-1] + fan - 1) // fan)
    sizes = sizes[::-1]                      # 1, ..., n_leaves
    starts = np.concatenate([[0], np.cumsum(sizes)])
    parent = np.zeros(int(starts[-1]), dtype=np.uint32)
    for lv in range(1, len(sizes)):
        parent[starts[lv]:starts[lv + 1]] = starts[lv - 1] + np.arange(sizes[lv]) // fan
    return parent, (starts[-2] + np.arange(n_leaves)).astype(np.uint32)


def matrix(rng, n_unitigs, n_colors):
    W = (n_colors + 63) // 64
    bits = np.zeros((n_unitigs, W), dtype=np.uint64)
    base = rng.integers(0, n_colors, n_unitigs)
    for _ in range(8):
        c = (base + rng.integers(0, 16, n_unitigs)) % n_colors
        on = rng.random(n_unitigs) < 0.45
        np.bitwise_or.at(bits, (np.flatnonzero(on), (c >> 6)[on]), np.uint64(1) << (c & 63).astype(np.uint64)[on])
    first = np.flatnonzero(~bits.any(axis=1))   # every unitig has a colour
    bits[first, base[first] >> 6] |= np.uint64(1) << (base[first] & 63).astype(np.uint64)
    return bits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="chr1", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=2)
    a = ap.parse_args()
    gsize, k, read_len, n_reads, desc, kind = bench.WORKLOADS[a.workload]
    n_reads = a.reads or n_reads
    t0 = time.time()
    g, u, _ = bench.make_inputs(synth, np, kind, gsize, k)
    idx = fa.FinimizerIndex.build_on_device(u.as_tuple(), k, 0).to_device(0)
    sets = [synth.reads(g, n_reads, read_len=read_len, seed=synth.SEED_READS + 1000 * s) for s in range(a.sets)]
    batch = idx.batch(sets[0].as_tuple())
    nu = idx.n_unitigs
    print("workload %s: %d unitigs, %d reads per step, %d k-mers, set up in %.1f s" % (a.workload, nu, n_reads, batch.n_kmers, time.time() - t0), flush=True)
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    L = fa.lib()
    err = C.create_string_buffer(512)
    rng = np.random.default_rng(37)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ts); rc = f(); e1.record(ts); torch.cuda.synchronize()
        assert rc == 0, err.value
        return e0.elapsed_time(e1)

    batch.text_mode(2)
    for n_colors in (5, 130, 4096):
        parent, ct = leaf_tree(n_colors)
        bits = matrix(rng, nu, n_colors)
        col = idx.colors(n_colors, bits)
        # ---- 1. the labelling
        def make():
            t = col.taxonomy(parent, ct); t.close()
        make()
        _, t_dev = wall(make, a.steps)
        host_labels, t_host = wall(lambda: fa.unitig_lca_labels(col.download()[0], n_colors, parent, ct, 16), a.steps)
        tax = col.taxonomy(parent, ct)
        labels = tax.labels()
        assert np.array_equal(labels, host_labels)
        lab = tax.as_labels()
        print("%d colours, %d taxa, %d distinct labels: labelling on the device %s | download + twin on 16 threads %s"
              % (n_colors, len(parent), len(np.unique(labels)), med(t_dev), med(t_host)), flush=True)
        # ---- 2. per step
        ways = [("classify", lambda: L.fin_batch_classify(batch.h, lab.h, err, 512)),
                ("taxa conf 0", lambda: L.fin_batch_taxa(batch.h, tax.h, 1, 0, err, 512)),
                ("taxa conf 100", lambda: L.fin_batch_taxa(batch.h, tax.h, 1, 100, err, 512)),
                ("add_taxa (tally alone)", lambda: L.fin_batch_add_taxa(batch.h, tax.h, 1, 100, C.c_void_p(stream), err, 512))]
        t = {name: [] for name, _ in ways}
        t_step, t_rec, t_twin = [], [], []
        for s in range(a.steps + 1):   # (step 0: a first launch of every kernel, not counted)
            batch.reload(sets[s % a.sets].as_tuple())
            ms = timed(lambda: batch.run(fa.FIN_MERGED, stream) or 0)
            got = {}
            for name, f in ways[s % 3:3] + ways[:s % 3] + ways[3:]:   # (interleaved; the tally last)
                if name.startswith("add_taxa"):   # (the tally alone: timed behind the read taxa of its thresholds, not instead of them)
                    assert L.fin_batch_taxa(batch.h, tax.h, 1, 100, err, 512) == 0
                    torch.cuda.synchronize()
                got[name] = timed(f)
            if s in (0, 1, 2):   # the host route, three times: the records' download, then the twin
                dev = batch.taxa(tax, 1, 100)
                w0 = time.perf_counter(); recs, st = batch.records(); w1 = time.perf_counter()
                host = fa.records_read_taxa(recs, st, k, labels, parent, 1, 100, 16); w2 = time.perf_counter()
                assert np.array_equal(dev, host), "the twin's read taxa differ from the device's"
                t_rec.append(1e3 * (w1 - w0)); t_twin.append(1e3 * (w2 - w1))
            if s == 0:
                continue
            t_step.append(ms)
            for name, _ in ways:
                t[name].append(got[name])
        print("  medians over %d steps: step %s" % (a.steps, med(t_step)))
        for name, _ in ways:
            print("    %-24s %s" % (name + ":", med(t[name])))
        print("    host route: records made + downloaded %s | fin_records_read_taxa on 16 threads %s" % (med(t_rec), med(t_twin)), flush=True)
        called = batch.taxa(tax, 1, 100)
        print("    calls at confidence 100: %.1f %% classified, %.1f %% of those at a leaf" % (
            100.0 * (called["taxon"] != fa.FIN_NO_LABEL).mean(), 100.0 * (called["taxon"][called["taxon"] != fa.FIN_NO_LABEL] >= ct[0]).mean()), flush=True)
        lab.close(); tax.close(); col.close()
    # ---- 3. the roll-up
    for n_taxa in (10 ** 4, 10 ** 6):
        for name, parent in (("logarithmic depth", np.floor(rng.random(n_taxa) * np.arange(n_taxa)).astype(np.uint32)),
                             ("deep (parent among the 64 below)", np.maximum(np.arange(n_taxa) - 1 - rng.integers(0, 64, n_taxa), 0).astype(np.uint32))):
            parent[0] = 0
            labels = rng.integers(0, n_taxa, nu).astype(np.uint32)
            tax = idx.taxonomy(parent, labels)
            tax.add(batch)
            direct = np.zeros(n_taxa + 1, dtype=np.uint64); clade = np.zeros(n_taxa, dtype=np.uint64)
            dp, cp = direct.ctypes.data_as(C.POINTER(C.c_uint64)), clade.ctypes.data_as(C.POINTER(C.c_uint64))
            L.fin_taxonomy_download(tax.h, dp, cp, None, err, 512)
            _, t_without = wall(lambda: L.fin_taxonomy_download(tax.h, dp, None, None, err, 512), a.steps)
            _, t_with = wall(lambda: L.fin_taxonomy_download(tax.h, dp, cp, None, err, 512), a.steps)
            host, t_host = wall(lambda: fa.taxa_clade_reads(direct, parent), a.steps)
            assert np.array_equal(host, clade) and int(clade[0]) + int(direct[n_taxa]) == n_reads
            print("roll-up, %d taxa, %s, %d taxa with reads: download without clades %s | with clades %s | roll-up alone (difference of medians) %.3f ms | "
                  "fin_taxa_clade_reads on the host %s" % (n_taxa, name, int((direct[:n_taxa] != 0).sum()), med(t_without), med(t_with),
                                                              statistics.median(t_with) - statistics.median(t_without), med(t_host)), flush=True)
            tax.close()
    batch.close()


if __name__ == "__main__":
    main()
