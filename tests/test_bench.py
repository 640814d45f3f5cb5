"""bench.py --dump-outputs: what the timed path computed in its last step, as a seeded sample of its pairs -- the same reads whenever the
arguments are the same, read across device batches, and equal to what a caller of the path gets for those reads."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeBatch:
    """download_range of a device batch, over a host array"""

    def __init__(self, pairs):
        self.pairs = pairs

    def download_range(self, first_pair, n_pairs):
        assert 0 <= first_pair and first_pair + n_pairs <= len(self.pairs)
        return self.pairs[first_pair:first_pair + n_pairs]


@pytest.mark.parametrize("n_reads,nk_read,n_batches", [(1000, 120, 1), (100_000, 120, 3), (30_000, 188, 2), (10, 0, 1)])
def test_dump_sample_across_batches(n_reads, nk_read, n_batches):
    import bench
    s = bench.dump_sample(np, n_reads, nk_read)
    assert np.array_equal(s, bench.dump_sample(np, n_reads, nk_read))
    assert len(s) > 0 and np.all(np.diff(s) > 0) and s[0] >= 0 and s[-1] < n_reads
    assert len(s) * nk_read <= bench.DUMP_MAX_PAIRS
    if n_reads * nk_read <= bench.DUMP_MAX_PAIRS:
        assert len(s) == n_reads
    whole = np.arange(2 * n_reads * nk_read, dtype=np.int32).reshape(-1, 2)
    per = -(-n_reads // n_batches)
    batches = [_FakeBatch(whole[b * per * nk_read:min(n_reads, (b + 1) * per) * nk_read]) for b in range(n_batches)]
    got = bench.download_reads(np, batches, per, nk_read, s)
    assert np.array_equal(got, whole.reshape(n_reads, nk_read, 2)[s].reshape(-1, 2))


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_paths_pairs(tmp_path):
    """a plain run (no --full) over three device batches: the dumped pairs are those fin_search_batch gives for the sampled reads,
    and n_found is the whole step's"""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    d = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "chr1x8", "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--genome", "3000000", "--reads", "50000", "--batch-reads", "20000", "--dump-outputs", str(d)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["config"]["batches_per_gpu"] == 3 and "cpu_baseline" not in line
    pairs, sample, n_found = (np.load(d / f) for f in ("pairs.npy", "sample_reads.npy", "n_found.npy"))
    assert pairs.dtype == sample.dtype == n_found.dtype == np.float64
    sample = sample.astype(np.int64)
    assert 0 < len(sample) < 50000 and sample.max() >= 40000   # a sample, with reads of the third batch in it

    import finito_amd as fa
    from finito_amd import synth
    g = synth.genome(3_000_000)
    u = synth.unitigs(g, 31)
    r = synth.reads(g, 50_000, read_len=150)
    idx = fa.FinimizerIndex.build(u.as_tuple(), 31).to_device(0)
    exp, npos = idx.search_reads(r.as_tuple(), fa.FIN_MERGED)
    assert np.array_equal(pairs, exp.reshape(50_000, 120, 2)[sample].reshape(-1, 2).astype(np.float64))
    assert int(n_found[0]) == npos
