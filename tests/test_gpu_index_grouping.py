"""The index build's pair grouping (k_ixsort.hip) at the edges of its layout: one count, two hops into the bins, the bins by id.

Layout constants the cases below come from (k_ixsort.hip): IXS_G = 512 slices; bins of 2^wsh ids, wsh the smallest with at most
IXS_BINS_MAX = 8192 bins (so a bin is ONE id up to NC = 8192, two from 8193, four from 16385 ...); superbins of 2^ssh bins, ssh the
smallest with at most IXS_SB_MAX = 128 superbins (one bin per superbin up to 128 bins, two from 129 ... 64 from 4097); the second hop
takes IXS_K = 16 neighbouring slices per workgroup (SOHIT_IXS_K moves it) and both hops move their pairs in tiles of 4096; a bin of up to
IXS_CAP = 4096 pairs and 16384 ids is ordered in the LDS (SOHIT_IXS_CAP lowers the limit), the others by IXS_W = 16384 counters per LDS pass
(wider bins, NC above 2^27, are split first).  Every case: threshold and index arrays == the oracle's CSR (check_index of test_gpu_parity.py, per chunk).

Run on the GPU box:  python -m pytest tests/test_gpu_index_grouping.py -m gpu -x -q
"""
import numpy as np
import pytest

from test_gpu_parity import check_index, fs, gpu_rows  # noqa: F401  (fs: the module's fixture)

pytestmark = pytest.mark.gpu

SSD = "111111"
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)


class _Chunk:
    """check_index reads chunk 0 of what it is handed: chunk k of a searcher under that name"""

    def __init__(self, s, k):
        self.s, self.k = s, k

    def chunk_index(self, _):
        return self.s.chunk_index(self.k)


def index_vs_oracle(fs, oracle, fa, NC, chk=50000, ssd=SSD):
    """build the index of `fa` (no search) and compare every chunk with the oracle's index of the same sequence range; -> entries per chunk"""
    n = fa.count(b">")
    kw = dict(ssd=ssd, nr=oracle.AA9, ht=NC, chk=chk, step=1, v=500, expect=1e-5, flt="T")
    s = fs.Searcher(**kw)
    s.load_ref_bytes(fa)
    s.build_index()
    sizes = []
    for k, st in enumerate(range(0, n, chk)):
        ix = oracle.Index(fa, ssd, kw["nr"], 1, NC, st, min(st + chk, n))
        assert s.chunk_threshold(k) == ix.threshold, "chunk %d" % k
        check_index(_Chunk(s, k), ix, NC, A=1, S=ssd.count(",") + 1)
        sizes.append(len(ix.locus()))
    s.close()
    return sizes


def random_fasta(lengths, seed):
    rng = np.random.default_rng(seed)
    return "".join(">r%d\n%s\n" % (i, AA[rng.integers(0, 20, n)].tobytes().decode()) for i, n in enumerate(lengths)).encode()


@pytest.fixture(scope="module")
def fa300():
    from swiftortho_amd import synthprot
    return synthprot.synthprot(300, 120, 17)


# one below, at and one above:
#   1 / 2 / 3         a single bin = a single superbin (NC = 1); NC = 2 is the first NC with two superbins, the second holding one bin with one id
#   128 / 129         one bin per superbin -> two (129 bins: 65 superbins, the last one partial: one bin)
#   256 / 257, 4096 / 4097   the superbin width doubles again (3 bins in 2 -> 4; 4097: the widest superbins, 64 bins, the last holds one)
#   8192 / 8193       the bin width doubles (8193: 4097 bins of two ids, the last bin holds one id, the last superbin that one bin)
#   120000000         the default -M: 7325 bins of 16384 ids, 115 superbins, the last one partial (29 bins)
#   9, 16384, 16385, 2^27, 2^27 + 1, 300000007   test_index_grouping_at_every_bucket_count's values: the wide-bin split and the hashed
#                     directory behind the new hops
# (a hop-2 group count that does not divide IXS_G cannot occur: the slices per group are a power of two up to IXS_G / 8 by construction,
#  ixs_k() -- test_second_hop_group_sizes runs the smallest and the largest and a value that is refused)
EDGES = [1, 2, 3, 127, 128, 129, 130, 255, 256, 257, 258, 4095, 4096, 4097, 4098, 8191, 8192, 8193, 8194,
         9, 16384, 16385, 120000000, 134217728, 134217729, 300000007]


@pytest.mark.parametrize("NC", EDGES)
def test_every_width_boundary(fs, oracle, fa300, NC):
    """-M at every value where the bin width, the superbin width or the shape of the last bin / superbin changes (the list above)"""
    assert index_vs_oracle(fs, oracle, fa300, NC)[0] > 30000


@pytest.mark.parametrize("K", ["1", "8", "64", "24"])
@pytest.mark.parametrize("NC", [129, 120000000])
def test_second_hop_group_sizes(fs, oracle, fa300, monkeypatch, NC, K):
    """SOHIT_IXS_K: one slice per hop-2 workgroup, 8, the most (64 = an XCD's eighth of the slices in one group), and 24, which is no
    power of two and falls back to the compiled 16 -- the same index whatever the group size"""
    monkeypatch.setenv("SOHIT_IXS_K", K)
    index_vs_oracle(fs, oracle, fa300, NC)


@pytest.mark.parametrize("NC,K", [(120000000, "-1"), (9, "64")])
def test_several_tiles_per_workgroup(fs, oracle, monkeypatch, NC, K):
    """Both hops take their pairs through the LDS in tiles of 4096 and carry the cursors from tile to tile: 10 000 x 300 residues are
    5 762 pairs per slice (two tiles in the first hop); with NC = 9 and 64 slices per group a second-hop workgroup has ~41 000 (ten tiles,
    every one full of a single digit)"""
    from swiftortho_amd import synthprot
    monkeypatch.setenv("SOHIT_IXS_K", K)
    assert index_vs_oracle(fs, oracle, synthprot.synthprot(10000, 300), NC)[0] > 512 * 4096


@pytest.mark.parametrize("NC", [2, 129, 120000000])
def test_fewer_pairs_than_slices(fs, oracle, NC):
    """two 8-residue sequences = 6 pairs: all but a few slices and nearly every hop-2 workgroup are empty"""
    assert index_vs_oracle(fs, oracle, random_fasta([8, 8], 5), NC) == [6]


def test_no_pair_at_all(fs, oracle):
    """every sequence shorter than the seed (E = 0); then the same for the first of two chunks only"""
    assert index_vs_oracle(fs, oracle, random_fasta([5, 3, 4, 5], 6), 120000000) == [0]
    sizes = index_vs_oracle(fs, oracle, random_fasta([5, 3, 4, 5, 40, 50, 60, 70], 7), 120000000, chk=4)
    assert sizes[0] == 0 and sizes[1] == 35 + 45 + 55 + 65


@pytest.mark.parametrize("NC", [120000000, 9])
def test_skew(fs, oracle, NC):
    """300 copies of one 120-residue sequence: every occupied bucket has 300 members or a multiple and a few superbins receive everything;
    with NC = 9 (bins of one id) five bins hold more than the IXS_CAP = 4096 pairs that k_ixs_bin_lds orders in the LDS and go to
    k_ixs_bin's counters, four hold fewer and stay -- the populations are asserted from the oracle's CSR, the kernels decide by the same
    numbers (test_bin_capacity_boundary moves the limit onto a population)"""
    seq = random_fasta([120], 8).split(b"\n")[1].decode()
    fa = "".join(">c%d\n%s\n" % (i, seq) for i in range(300)).encode()
    if NC == 9:
        pop = bucket_sizes(oracle.Index(fa, SSD, oracle.AA9, 1, NC))
        assert (pop > 4096).sum() == 5 and ((pop > 0) & (pop <= 4096)).sum() == 4
    assert index_vs_oracle(fs, oracle, fa, NC) == [300 * 115]


def bucket_sizes(ix):
    return np.diff(np.append(ix.start().astype(np.int64), len(ix.locus())))


def test_bin_capacity_boundary(fs, oracle, fa300, monkeypatch):
    """SOHIT_IXS_CAP on a bin's population, NC = 9 (nine bins of one id, 3665 .. 3992 pairs): every bin in the LDS; the fullest bin exactly
    at the limit; one below it (that bin alone by the counters); below the emptiest (all by the counters)"""
    pop = bucket_sizes(oracle.Index(fa300, SSD, oracle.AA9, 1, 9))
    assert 64 < pop.min() and pop.max() <= 4096 and (pop == pop.max()).sum() == 1
    for cap in (4096, pop.max(), pop.max() - 1, pop.min() - 1):
        monkeypatch.setenv("SOHIT_IXS_CAP", str(cap))
        index_vs_oracle(fs, oracle, fa300, 9)


@pytest.mark.parametrize("cap", ["0", "64"])
@pytest.mark.parametrize("NC", [1, 129, 8193, 120000000, 134217729])
def test_bins_by_either_kernel(fs, oracle, fa300, monkeypatch, NC, cap):
    """the same index with every bin left to the counters per id (0) and with the limit at 64 pairs, which puts the bins of NC = 129 (~267
    pairs each) on the counters and leaves those of 8193 (~8) and of the default -M (~5) in the LDS; NC = 1 is one bin above any limit, NC
    above 2^27 has bins too wide for the LDS form"""
    monkeypatch.setenv("SOHIT_IXS_CAP", cap)
    index_vs_oracle(fs, oracle, fa300, NC)


def test_two_patterns_through_a_search(fs, oracle, fa300):
    """S = 2 (slot layout (p - p_lo) * AS + tag, invalid windows as holes, the tag field in the entries) through both hops, behind a
    whole search as test_index_grouping_at_every_bucket_count runs one"""
    ssd = "111111,1101011"
    for NC in (2000003, 129):
        kw = dict(ssd=ssd, nr=oracle.AA9, ht=NC, chk=50000, step=1, v=500, expect=1e-5, flt="T")
        s, hits, _ = gpu_rows(fs, fa300, fa300, kw)
        ix = oracle.Index(fa300, ssd, kw["nr"], 1, NC)
        assert s.chunk_threshold(0) == ix.threshold
        check_index(s, ix, NC, A=1, S=2)
        hits.close()
        s.close()


@pytest.mark.parametrize("NC", [120000000, 8193])
def test_three_chunks_of_unequal_size(fs, oracle, fa300, NC):
    """chk = 128 over 300 sequences: chunks of 128, 128 and 44 sequences built one after the other in the same buffers, each against the
    oracle's index of its range"""
    sizes = index_vs_oracle(fs, oracle, fa300, NC, chk=128)
    assert len(sizes) == 3 and sizes[2] < sizes[0]
