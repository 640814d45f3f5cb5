#!/usr/bin/env python3
"""What merging two accumulators of equivalence classes costs (fin_eqclasses_merge; fin_eqclasses.hip), against the route over the host that a
caller had before: download both, fin_classes_merge, reset, fin_eqclasses_add_classes_host -- `python3 tools/ab_eqmerge.py [--classes 100000,1000000]
[--colors 130,4096] [--reps 20] [--out FILE]`.

For each number of colours and classes: two class lists of n random distinct rows each, half of B's rows being rows of A, reads 1 .. 1000; accumulators A and
B hold them (max_classes 2^21), D is the destination.  Per repetition, D is reset and given A (untimed), then
  device: D.merge(B), HIP events on one stream around the call -- the compaction of B, the gather and the three launches of the weighted add;
  host:   wall clock over every step: A.download(), B.download(), classes_merge, D.reset(), D.add_classes(...) (which returns when the add has run).
D's counters must be what the lists say after either.  Medians over the repetitions; repetition 0 (a first launch of every kernel) is not counted.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import finito_amd as fa
from finito_amd import synth


def med(xs):
    return "%.3f ms (%.3f..%.3f, n=%d)" % (statistics.median(xs), min(xs), max(xs), len(xs))


def class_list(rng, n, n_colors):
    W = (n_colors + 63) // 64
    rows = rng.integers(1, 1 << 63, size=(n, W), dtype=np.uint64)
    if n_colors & 63:
        rows[:, W - 1] &= np.uint64((1 << (n_colors & 63)) - 1)
        rows[:, 0] |= np.uint64(1)   # (never empty)
    return rows, rng.integers(1, 1001, n).astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", default="100000,1000000")
    ap.add_argument("--colors", default="130,4096")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n"); out.flush()

    g = synth.genome(200_000)
    idx = fa.FinimizerIndex.build(synth.unitigs(g, 31).as_tuple(), 31).to_device(0)
    ts = torch.cuda.current_stream()
    say("device: %s" % torch.cuda.get_device_name(0))
    for n_colors in [int(x) for x in a.colors.split(",")]:
        W = (n_colors + 63) // 64
        col = idx.colors(n_colors)
        for n in [int(x) for x in a.classes.split(",")]:
            rng = np.random.default_rng(31 + n_colors)
            ra, wa = class_list(rng, n, n_colors)
            rb, wb = class_list(rng, n, n_colors)
            rb[: n // 2] = ra[rng.permutation(n)[: n // 2]]
            A, B, D = (col.eqclasses(1 << 21) for _ in range(3))
            A.add_classes(ra, wa); B.add_classes(rb, wb, 12345)
            n_union = len(np.unique(np.concatenate([ra[:, 0], rb[:, 0]])))   # (word 0 of a random row tells the rows apart)
            want = [int(wa.sum()) + int(wb.sum()) + 12345, 12345, n_union]
            assert A.stats()[2] == n and B.stats()[2] == n
            t_dev, t_host, t_parts = [], [], []
            for rep in range(a.reps + 1):
                D.reset().merge(A); torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ts); D.merge(B, stream=ts.cuda_stream); e1.record(ts); torch.cuda.synchronize()
                assert D.stats()[:3] == want, "the device merge's counters"
                w0 = time.perf_counter()
                da, db = A.download(), B.download(); w1 = time.perf_counter()
                rows, reads = fa.classes_merge(da[0], da[1], db[0], db[1], n_colors); w2 = time.perf_counter()
                D.reset().add_classes(rows, reads, da[2] + db[2]); w3 = time.perf_counter()
                assert D.stats()[:3] == want, "the host route's counters"
                if rep:
                    t_dev.append(e0.elapsed_time(e1)); t_host.append(1e3 * (w3 - w0))
                    t_parts.append((1e3 * (w1 - w0), 1e3 * (w2 - w1), 1e3 * (w3 - w2)))
            parts = [statistics.median(p[i] for p in t_parts) for i in range(3)]
            say("%d colours (%d words per row), %d + %d classes -> %d:" % (n_colors, W, n, n, n_union))
            say("  fin_eqclasses_merge, HIP events:        %s" % med(t_dev))
            say("  host route, wall clock:                 %s" % med(t_host))
            say("    of it, medians: two downloads %.3f ms | fin_classes_merge %.3f ms | reset + add_classes_host %.3f ms" % tuple(parts))
            say("  bytes that cross PCIe on the host route: %d down, %d up; on the device route: none" % (2 * n * (8 * W + 8), n_union * (8 * W + 8)))
            for x in (A, B, D):
                x.close()
        col.close()
    idx.close()


if __name__ == "__main__":
    main()
