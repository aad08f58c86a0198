"""GPU tests of the SEG query mask (k_seg in csrc/k_prep.hip, the host's seg_mask, k_copy_range / k_gather_seqs for -F F).

Expected masks come straight from tests/golden/seg_edges.json, written by the REAL reference's seg() (no oracle in between): mosaics
of low- and high-complexity segments at every length where the kernel changes its path -- the first window below 12 residues, the tail
rule, one / two / three tiles of the 128- and 512-step instances, the instance boundaries 1024 / 4096 / 32768 -- a third of their
residues masked, thousands of mask edges inside the queries.  The same comparison runs under every layout that moves a query to
another kernel instance or batch slot.  The end-to-end cases then put masks inside reported alignments.

Run on the GPU box:  python -m pytest tests/test_gpu_seg.py -m gpu -q
"""
import numpy as np
import pytest

import seg_fixture
from test_gpu_parity import fs, oracle_run, oracle_vs_gpu  # noqa: F401  (fs is a fixture)

pytestmark = pytest.mark.gpu

AA = "ACDEFGHIKLMNPQRSTVWY"
AA9 = "AST,CFILMVY,DN,EQ,G,H,KR,P,W"
KW = dict(ssd="111111", nr=AA9, ht=1000003, chk=50000, step=1, v=500, expect=1e-5)


def reference_record():
    """one unrelated 60-residue subject: the search itself costs nothing"""
    from swiftortho_amd import synthprot
    return synthprot.uniform_proteins(1, 60, 7)


def mosaics():
    """[(name, input, expected)] of the fixture's mosaic cases: 29 distinct upper-cased bytes, so the device masks them"""
    return [(name, s, out) for name, group, s, out in seg_fixture.cases() if not group.startswith("alphabet")]


def ordered(cases, order):
    if order == "long_to_short":
        return sorted(cases, key=lambda c: -len(c[1]))
    if order == "short_to_long":
        return sorted(cases, key=lambda c: len(c[1]))
    assert order == "shuffled"
    return [cases[i] for i in np.random.default_rng(20261018).permutation(len(cases))]


def one_group_for_the_rest(seqs):
    """the reduced alphabet AA9 plus one group of every other byte of `seqs`.  The seed hash packs a residue's code into 5 bits, so a
    search refuses a file with more than 30 distinct codes; under AA9 every byte outside the 20 amino acids is a code of its own, and a
    file of 64 symbols has 53.  With the other bytes in one group it has at most 12: the 9 groups, this one, and ',' and '/', which
    separate groups and alphabets in the option and so stay single.  SEG never sees the reduced alphabet: the masks are the same."""
    rest = set(b"".join(seqs).upper()) - set(AA.encode()) - set(b",/X")
    return AA9 + "," + bytes(sorted(rest)).decode("ascii")


def masks(fs, seqs, opts=None, flt="T", ranges=((-1, -1),), nr=AA9):
    """-> ([per range: masked_query(q) of every query of the file], the searcher's timing map) under the switches `opts`"""
    s = fs.Searcher(flt=flt, **dict(KW, nr=nr))
    try:
        s.set_option("SOHIT_KEEP_MASKED", "1")
        for k, v in (opts or {}).items():
            s.set_option(k, v)
        s.load_ref_bytes(reference_record())
        s.load_queries_bytes(seg_fixture.fasta(seqs))
        assert s.num_queries == len(seqs)
        out = []
        for lo, hi in ranges:
            # (an upper end below 0 means the number of REFERENCE sequences, as in the reference: the whole file is asked for by its count)
            s.search(0 if lo < 0 else lo, len(seqs) if hi < 0 else hi).close()
            out.append([s.masked_query(q) for q in range(len(seqs))])
        return out, s.timing()
    finally:
        s.close()


def check(got, cases, lo=0, hi=None, what=""):
    hi = len(cases) if hi is None else hi
    bad = []
    for q, (name, s, want) in enumerate(cases):
        if lo <= q < hi:
            d = seg_fixture.first_difference(got[q], want)
            if d:
                bad.append("%s query %d (%s, %d residues): %s" % (what, q, name, len(s), d))
        else:
            assert got[q] is None, (what, q)
    assert not bad, "%d of %d masks differ from the reference's:\n%s" % (len(bad), hi - lo, "\n".join(bad[:12]))


LAYOUTS = [("long_to_short", {}), ("short_to_long", {}), ("shuffled", {}),
           ("long_to_short", {"SOHIT_BATCH": "7"}), ("shuffled", {"SOHIT_BATCH": "7"}),
           ("short_to_long", {"SOHIT_QCLASS": "0"}), ("shuffled", {"SOHIT_QCLASS": "0"}),
           ("shuffled", {"SOHIT_QCLASS": "0", "SOHIT_BATCH": "7"})]


@pytest.mark.parametrize("order,opts", LAYOUTS, ids=["%s%s" % (o, "".join("-%s=%s" % (k[6:].lower(), v) for k, v in e.items())) for o, e in LAYOUTS])
def test_masks_equal_the_real_reference(fs, order, opts):
    """every mosaic of the fixture, byte for byte, whatever slot and batch the file order, the batch size and the class order give it
    (SOHIT_QCLASS=0: every instance is launched over all slots)"""
    cases = ordered(mosaics(), order)
    (got,), tm = masks(fs, [c[1] for c in cases], opts)
    assert tm["load.seg_on_device"] == 1
    check(got, cases, what=order)


@pytest.mark.parametrize("opts", [{}, {"SOHIT_QCLASS": "0"}, {"SOHIT_BATCH": "7"}], ids=["default", "qclass=0", "batch=7"])
def test_masks_of_a_query_subrange(fs, opts):
    """search(st, ed) with st > 0: the launch offsets q_lo / q_mid / q_long of a range that holds a 4097- and a 33 293-residue query"""
    cases = ordered(mosaics(), "shuffled")
    names = [c[0] for c in cases]
    st, ed = 5, len(cases) - 4
    assert st <= names.index("plain_4097") < ed and st <= names.index("plain_33293") < ed
    (got,), _ = masks(fs, [c[1] for c in cases], opts, ranges=((st, ed),))
    check(got, cases, st, ed, what="range %d..%d" % (st, ed))


def test_second_search_reuses_the_batch_layout(fs):
    """two searches on one Searcher (the second finds the slot layout made), then another range and the first again: the same masks"""
    cases = ordered(mosaics(), "shuffled")
    n = len(cases)
    got, _ = masks(fs, [c[1] for c in cases], ranges=((-1, -1), (-1, -1), (9, n - 9), (9, n - 9), (-1, -1)))
    for k, (lo, hi) in enumerate(((0, n), (0, n), (9, n - 9), (9, n - 9), (0, n))):
        check(got[k], cases, lo, hi, what="search %d" % k)
    assert got[0] == got[1] == got[4] and got[2] == got[3]


@pytest.mark.parametrize("poison", ["0xFF", "0x5A"])
def test_masks_do_not_depend_on_stale_memory(fs, poison):
    """every fresh device allocation filled with a byte pattern: the mask buffer is written only up to n - 12, the walk must not read
    past it; the staged instances keep their mask in LDS"""
    cases = ordered(mosaics(), "shuffled")
    (got,), _ = masks(fs, [c[1] for c in cases], {"SOHIT_POISON": poison})
    check(got, cases, what="poison " + poison)
    (got,), _ = masks(fs, [c[1] for c in cases], {"SOHIT_POISON": poison, "SOHIT_QCLASS": "0", "SOHIT_BATCH": "7"})
    check(got, cases, what="poison " + poison + ", unordered batches of 7")


@pytest.mark.parametrize("nsym,on_device", [(64, 1), (65, 0)])
def test_symbol_count_boundary_picks_the_implementation(fs, nsym, on_device):
    """64 distinct upper-cased bytes: the device kernel folds them to its 64 symbols; 65: the host's seg_mask.  Both give the reference's
    masks, and load.seg_on_device says which one ran."""
    cases = [(name, s, out) for name, group, s, out in seg_fixture.cases() if group == "alphabet%d" % nsym]
    assert len(cases) == 5 and len(set(b"".join(c[1] for c in cases).upper())) == nsym
    seqs = [c[1] for c in cases]
    (got,), tm = masks(fs, seqs, nr=one_group_for_the_rest(seqs))
    assert tm["load.seg_on_device"] == on_device
    check(got, cases, what="alphabet%d" % nsym)


@pytest.mark.parametrize("opts", [{}, {"SOHIT_BATCH": "7"}], ids=["default", "batch=7"])
def test_host_mask_at_every_length(fs, opts):
    """the mosaics in one file with the 65-symbol group: the whole file is masked by the host's seg_mask -- its first window, tail rule and
    walk at every length of the fixture"""
    cases = ordered(mosaics(), "shuffled") + [(name, s, out) for name, group, s, out in seg_fixture.cases() if group == "alphabet65"]
    seqs = [c[1] for c in cases]
    (got,), tm = masks(fs, seqs, opts, nr=one_group_for_the_rest(seqs))
    assert tm["load.seg_on_device"] == 0
    check(got, cases, what="host")


@pytest.mark.parametrize("opts", [{}, {"SOHIT_QCLASS": "0"}], ids=["class_order_gathers", "file_order_copies"])
def test_no_filter_leaves_the_raw_bytes(fs, opts):
    """-F F: the batch holds the raw bytes, lower case and odd bytes untouched -- gathered slot by slot in a class-ordered batch
    (k_gather_seqs), copied as one range in file order (k_copy_range), for the whole file and for a range with st > 0"""
    cases = ordered(mosaics(), "shuffled")
    raw = [(name, s, s) for name, s, _ in cases]
    assert any(s != s.upper() for _, s, _ in raw)
    n = len(raw)
    got, tm = masks(fs, [c[1] for c in raw], opts, flt="F", ranges=((-1, -1), (5, n - 4)))
    assert tm["load.seg_on_device"] == 0
    check(got[0], raw, what="-F F")
    check(got[1], raw, 5, n - 4, what="-F F range")


# ---- end to end: rows and candidates where the mask sits inside alignments -----------------------------------------------------------

def island(rng):
    """a low-complexity stretch of 8-35 residues: iid over 2-7 letters, a homopolymer, or a tandem repeat of period 2-6"""
    n, kind = int(rng.integers(8, 36)), int(rng.integers(0, 3))
    if kind == 0:
        sub = rng.choice(20, int(rng.integers(2, 8)), replace=False)
        return [AA[sub[i]] for i in rng.integers(0, len(sub), n)]
    if kind == 1:
        return [AA[int(rng.integers(0, 20))]] * n
    unit = [AA[i] for i in rng.integers(0, 20, int(rng.integers(2, 7)))]
    return (unit * (n // len(unit) + 1))[:n]


def island_families(ancestor_lengths, members, seed):
    """families of 10 % point-mutated copies of ancestors that carry 1-3 low-complexity islands -> FASTA bytes"""
    rng = np.random.default_rng(seed)
    recs = []
    for f, n in enumerate(ancestor_lengths):
        anc = [AA[i] for i in rng.integers(0, 20, n)]
        for _ in range(int(rng.integers(1, 4))):
            isl = island(rng)
            p = int(rng.integers(0, n - len(isl)))
            anc[p:p + len(isl)] = isl
        for m in range(members):
            seq = list(anc)
            for p in np.nonzero(rng.random(n) < 0.10)[0]:
                seq[int(p)] = AA[int(rng.integers(0, 20))]
            recs.append(">f%d_m%d\n%s\n" % (f, m, "".join(seq)))
    return "".join(recs).encode()


def family_sets():
    rng = np.random.default_rng(5)
    small = island_families([int(x) for x in rng.integers(180, 341, 20)], 6, 11)
    long_ = island_families([int(x) for x in rng.integers(1100, 1401, 4)] + [int(x) for x in rng.integers(4200, 4501, 4)], 6, 12)
    return {"20_families_of_6": small, "mid_and_giant_instances": long_}


@pytest.mark.parametrize("name", ["20_families_of_6", "mid_and_giant_instances"])
def test_masks_inside_alignments_vs_oracle(fs, oracle, tmp_path, name):
    """families whose members share low-complexity islands: rows and candidate lists with and without the filter equal the oracle's --
    after checking that the filter matters here (the oracle's -F T and -F F outputs differ in more than 100 rows, oracle.seg changes
    more than a third of the queries), so the case cannot silently stop exercising masks"""
    fa = family_sets()[name]
    seqs = fa.split(b"\n")[1::2]
    assert len(seqs) == (120 if name == "20_families_of_6" else 48)
    changed = sum(oracle.seg(s) != s for s in seqs)
    assert 3 * changed > len(seqs), changed
    rows = {}
    for flt in ("T", "F"):
        (tmp_path / flt).mkdir()
        rows[flt] = set(oracle_run(oracle, fa, dict(KW, flt=flt), -1, -1, tmp_path / flt)[1].split(b"\n"))
    assert len(rows["T"] ^ rows["F"]) > 100, len(rows["T"] ^ rows["F"])
    for flt in ("T", "F"):
        c, _ = oracle_vs_gpu(fs, oracle, fa, dict(KW, flt=flt), tmp_path / flt)
        assert c["rows"] >= len(seqs)
