"""The chain flow of the sparse seed passes (SOHIT_UQ_CHAINS: what k_ungapq leaves over is sorted per query by k_uqsort_wave /
k_uqsort_wg and chained by k_ungap2 from the list of group heads) on planted multi-hit diagonals: groups of 2, 3, 64, 65 and some 240 hits,
neighbouring diagonals, two groups on one subject, covered and left-bounded seeds, queries of 11 and 512 residues, a subject of several
diagonal bands, leftover counts around every compiled tier limit, the largest tier's cap moved over one query, and the old flow against the
new one.  Every oracle case goes through oracle_vs_gpu (rows, candidates of every query, seed_hits) with SOHIT_UG_COUNT=1 (the number of
BLOSUM lookups too) and SOHIT_BUCKET=0, and the counters say that the flow under test ran.

The sets and the model of their groups come from tests/uqchain_inputs.py (checked against the oracle in tests/test_uqchain_inputs.py).  The
model's figures bound the library's from below: two lone diagonals that share one of k_ungapq's counters are both left over (groups of one
hit in the chain kernel; they occur by chance in these sets).  A leftover count of exactly 1 therefore cannot occur -- a lone diagonal is
k_ungapq's own, a collision leaves two hits over -- and no set is built for it; the smallest planted count is 2."""
import pytest

import uqchain_inputs as ci
from test_gpu_parity import fs, gpu_rows, oracle_vs_gpu  # noqa: F401  (fs is a fixture)

pytestmark = pytest.mark.gpu


def kw_of(oracle, chk=50000):
    # thr: the frequency cap out of reach (as tests/test_gpu_ungapq_edges.py)
    return dict(ssd=ci.SEED, nr=oracle.AA9, ht=ci.HT, chk=chk, step=1, v=500, expect=1e-5, flt="T", thr=100000)


def setenv(monkeypatch, **more):
    monkeypatch.setenv("SOHIT_UG_COUNT", "1")
    monkeypatch.setenv("SOHIT_BUCKET", "0")   # (sets this small would be binned by buckets: every pass on the sorted path)
    for k, v in more.items():
        monkeypatch.setenv(k, str(v))


def tier_limits():
    from swiftortho_amd import _lib
    L = _lib.load()
    return int(L.so_uq_chain_tier(0)), int(L.so_uq_chain_tier(1))


def flow_ran(c, n_groups, left_max, overcap=0):
    assert c["hits_bucketed"] == 0 and c["groups_single"] > 0 and c["groups_chain"] == 0
    assert c["uq_chain_queries"] > 0
    assert c["uq_chain_groups"] >= n_groups, (c["uq_chain_groups"], n_groups)
    assert c["uq_left_max"] >= left_max, (c["uq_left_max"], left_max)
    assert c["uq_chain_overcap"] == overcap


@pytest.fixture(scope="module")
def shape(oracle):
    return ci.shape_set(oracle)


@pytest.fixture(scope="module")
def cap(oracle):
    return ci.cap_set(oracle)


def test_planted_groups(fs, oracle, tmp_path, monkeypatch, shape):
    fasta, m, where = shape
    setenv(monkeypatch)
    c, st = oracle_vs_gpu(fs, oracle, fasta, kw_of(oracle), tmp_path)
    flow_ran(c, m.n_groups(), int(m.left_counts().max()))


def test_planted_groups_two_chunks(fs, oracle, tmp_path, monkeypatch, shape):
    """A group lies on one subject, hence in one chunk: the groups are the model's; a query's leftover hits are split between the chunks, so
    the largest count of a pass is bounded by the largest group only."""
    fasta, m, where = shape
    setenv(monkeypatch)
    c, st = oracle_vs_gpu(fs, oracle, fasta, kw_of(oracle, chk=400), tmp_path)
    assert c["n_chunks"] == 2
    flow_ran(c, m.n_groups(), max(int(m.groups(q)[1].max()) for q in range(len(m.refs)) if len(m.groups(q)[1])))


def test_leftover_counts_at_the_tier_limits(fs, oracle, tmp_path, monkeypatch):
    """Queries whose leftover counts are L - 1, L and L + 1 for both compiled limits.  Above the larger one a query is sorted in place in the
    key array and counted in uq_chain_overcap: at least the family built for L + 1, at most the three families around that limit (a
    collision in k_ungapq can lift a query of L - 1 or L over it)."""
    limits = tier_limits()
    assert 64 < limits[0] < limits[1]
    fasta, m, fam = ci.tier_set(oracle, limits)
    top = limits[1]
    setenv(monkeypatch)
    c, st = oracle_vs_gpu(fs, oracle, fasta, kw_of(oracle), tmp_path)
    over = c["uq_chain_overcap"]
    flow_ran(c, m.n_groups(), top + 1, overcap=over)
    left = m.left_counts()
    assert len(fam[top + 1]) <= over <= int((left >= top - 1).sum())


def test_subject_of_several_bands(fs, oracle, tmp_path, monkeypatch):
    ref, qry, m = ci.band_set(oracle)
    setenv(monkeypatch)
    c, st = oracle_vs_gpu(fs, oracle, ref, kw_of(oracle), tmp_path, qry=qry)
    flow_ran(c, m.n_groups(), int(m.left_counts().max()))


def test_thousands_of_short_queries(fs, oracle, tmp_path, monkeypatch):
    """4000 queries of 30 .. 60 residues: some 25 hits per query, so the pass's hits (about 10^5) are far fewer than the entries the waves of
    k_uqsort_wave reserve in the chain list, a piece of 1024 each -- the list is sized by the waves launched, not by the hits."""
    fasta, m = ci.short_set(oracle)
    setenv(monkeypatch)
    c, st = oracle_vs_gpu(fs, oracle, fasta, kw_of(oracle), tmp_path)
    flow_ran(c, m.n_groups(), int(m.left_counts().max()))
    assert c["uq_chain_queries"] >= 3900 and c["seed_hits"] < 1024 * 1000


def test_cap_moves_over_one_query(fs, oracle, tmp_path, monkeypatch, cap):
    """SOHIT_UQ_CHAINS = ns - 1, ns, ns + 1 for the ns of the one largest query (read back through uq_left_max): that query alone takes the
    in-place instance at ns - 1, none does at ns and ns + 1; the rows are the oracle's all three times."""
    fasta, m, q = cap
    setenv(monkeypatch)
    c, st = oracle_vs_gpu(fs, oracle, fasta, kw_of(oracle), tmp_path)
    ns = c["uq_left_max"]
    left = m.left_counts()
    flow_ran(c, m.n_groups(), int(left[q]))
    assert left[q] <= ns < left[q] + 20   # (the margin to the second largest query of the set: collisions cannot make another one the largest)
    for n, over in ((ns - 1, 1), (ns, 0), (ns + 1, 0)):
        setenv(monkeypatch, SOHIT_UQ_CHAINS=n)
        c, st = oracle_vs_gpu(fs, oracle, fasta, kw_of(oracle), tmp_path)
        flow_ran(c, m.n_groups(), ns, overcap=over)
        assert c["uq_left_max"] == ns


def test_old_flow_gives_the_same_records(fs, oracle, monkeypatch, shape):
    """SOHIT_UQ_CHAINS=0 (library segmented sort + k_ungap + k_first_touch) against the default on the same input: identical hit records and
    BLOSUM lookups; the old flow counts nothing into the new counters."""
    fasta, m, where = shape
    out = {}
    for mode in ("-1", "0"):
        setenv(monkeypatch, SOHIT_UQ_CHAINS=mode)
        s, hits, rows = gpu_rows(fs, fasta, fasta, kw_of(oracle))
        out[mode] = (hits.array().tobytes(), rows, s.counters())
        hits.close()
        s.close()
    (a_rec, a_rows, a), (b_rec, b_rows, b) = out["-1"], out["0"]
    assert a_rec == b_rec and a_rows == b_rows
    assert a["ungap_steps"] == b["ungap_steps"] > 0 and a["groups"] == b["groups"] and a["seed_hits"] == b["seed_hits"]
    assert a["uq_chain_queries"] > 0 and a["uq_chain_groups"] >= m.n_groups()
    assert b["uq_chain_queries"] == 0 and b["uq_chain_groups"] == 0 and b["uq_chain_overcap"] == 0 and b["uq_left_max"] == 0
