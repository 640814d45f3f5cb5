"""tests.util.ref_chunks, the GPU tests' statement of the chunk format, checked base by base against the format's words: every byte value on
both strands, every read length from 0 to 70, every position of a chunk."""
import numpy as np

from tests.util import chunk_offsets, ref_chunks


def _expect(read, strand, p):
    """(code, valid) of position p of a strand, straight from the format's words"""
    n = len(read)
    if p >= n:
        return 0, 0
    b = read[p] if strand == 0 else read[n - 1 - p]
    u = chr(b & 0xDF)   # (upper case; b & ~32)
    if u not in "ACGT":
        return 0, 0
    c = "ACGT".index(u)
    return (c if strand == 0 else 3 - c), 1


def _check(reads):
    ch = ref_chunks(reads)
    off = chunk_offsets(reads)
    assert ch.dtype == np.uint32 and ch.shape == (off[-1], 4)
    for r, read in enumerate(reads):
        nch = (len(read) + 31) // 32
        assert off[r + 1] - off[r] == 2 * nch
        for i in range(2 * nch):
            lo, hi, valid, zero = (int(x) for x in ch[off[r] + i])
            assert zero == 0
            codes = lo | (hi << 32)
            strand, j0 = (0, 32 * i) if i < nch else (1, 32 * (i - nch))
            for j in range(32):
                c, v = _expect(read, strand, j0 + j)
                assert ((codes >> (2 * j)) & 3, (valid >> j) & 1) == (c, v), (r, i, j, read)
    return ch


def test_every_byte_value_at_every_position():
    # bytes(range(256)) rotated by 0..31: every byte value at every position mod 32 of both strands
    whole = bytes(range(256))
    reads = [whole[s:] + whole[:s] for s in range(32)]
    _check(reads)


def test_every_length_up_to_70():
    rng = np.random.default_rng(7)
    alphabet = b"ACGTacgtN"
    reads = []
    for n in range(71):
        reads.append(bytes(alphabet[x] for x in rng.integers(0, len(alphabet), n)))      # mostly bases, both cases
        reads.append(bytes(int(x) for x in rng.integers(0, 256, n)))                      # any byte
    _check(reads)


def test_known_chunks():
    # spelled out by hand: "ACGT" forward = 0b11_10_01_00; its reverse complement is "ACGT" again; "N" and "-" are not bases
    ch = ref_chunks(["ACGT", "", "aN-t"])
    assert ch.tolist() == [[0xE4, 0, 0xF, 0], [0xE4, 0, 0xF, 0],
                           [0x00 | (3 << 6), 0, 0b1001, 0], [0x00 | (3 << 6), 0, 0b1001, 0]]
    # one full chunk and one base: 33 T's -> forward codes all 3 / one 3; reverse all A (0)
    ch = ref_chunks(["T" * 33])
    assert ch.tolist() == [[0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0], [3, 0, 1, 0], [0, 0, 0xFFFFFFFF, 0], [0, 0, 1, 0]]
