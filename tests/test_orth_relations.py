"""The relations stage of find_orth on the host (find_orth.relation_tables + lines_from_tables): the split returns the lines
relations_from_candidates() always returned, the numpy tables equal a plain-Python restatement value for value, and the clique inputs of
tests/orth_rel_inputs.py reach what the inputs of tests/orth_inputs.py do not -- surviving and dropped repeats, pairs that occur three times and
more in a block, taxa with more than 64 forward in-paralog pairs, taxon codes that do not ascend with the names, a zero normaliser, the
mean-over-all branch, and scores whose sums depend on the order of the additions."""
import functools

import numpy as np
import pytest

import orth_inputs as oi
import orth_rel_inputs as ri
from conftest import orth_golden_cases
from test_orth_candidates import _golden, generated

CPU_KS = (2, 3, 12, 16, 17, 33)


@functools.lru_cache(maxsize=None)
def clique_stage(k, flags):
    """-> (cols, Candidates, RelationTables, plain-Python reference) of clique(k)"""
    from swiftortho_amd import find_orth as fo
    cols = ri.clique(k)
    cand = fo.candidates(cols, *ri.FLAGS[flags])
    return cols, cand, fo.relation_tables(cols.names, cand.tax, cand.taxa, cand), ri.reference(cols.names, cand.tax, cand)


def _both_ways(fo, cols, flags):
    cand = fo.candidates(cols, *flags)
    tax, taxa = fo._taxa(cols.names, flags[3] if len(flags) > 3 else "|")
    tables = fo.relation_tables(cols.names, tax, taxa, cand)
    return tables, fo.lines_from_tables(cols.names, tables), fo.relations_from_candidates(cols.names, tax, taxa, cand)


@pytest.mark.parametrize("name,variant", orth_golden_cases())
def test_tables_then_lines_reproduce_the_goldens(name, variant):
    from swiftortho_amd import find_orth as fo
    cols, flags, want = _golden(name, variant)
    tables, lines, old = _both_ways(fo, cols, flags)
    assert lines == old == want
    assert len(tables.ip_a) + len(tables.ot_a) + len(tables.co_a) == len(want)
    for k in fo.RelationTables.FIELDS:
        assert getattr(tables, k).dtype == (np.float64 if k.endswith("_v") else np.int64), k


@pytest.mark.parametrize("flags", sorted(oi.FLAG_SETS))
def test_tables_then_lines_on_generated_inputs(flags):
    from swiftortho_amd import find_orth as fo
    tables, lines, old = _both_ways(fo, generated(0), oi.FLAG_SETS[flags])
    assert lines == old and len(lines) > 1000
    assert np.all(tables.ip_a < tables.ip_b)


@pytest.mark.parametrize("flags", sorted(ri.FLAGS))
@pytest.mark.parametrize("k", CPU_KS)
def test_clique_tables_equal_plain_python(k, flags):
    from swiftortho_amd import find_orth as fo
    cols, cand, tables, ref = clique_stage(k, flags)
    got = ri.as_lists(tables)
    for sec in ("ip", "ot", "co"):
        assert got[sec] == ref[sec], sec
    assert fo.lines_from_tables(cols.names, tables) == fo.relations_from_candidates(cols.names, cand.tax, cand.taxa, cand)
    assert (tables.n_rows, tables.n_runs, tables.n_groups) == (cand.n_rows, cand.n_runs, cand.n_groups)


@pytest.mark.parametrize("flags", ("no", "bsr"))
def test_kept_edges_input_holds_what_it_promises(flags):
    """oi.kept_edges(): more than 32768 rows survive the filter, a dropped row stands directly before and after kept rows 256, 8192 and
    32768, and every section of the numpy answer is there"""
    cols = oi.kept_edges()
    coverage, identity, _ = oi.FLAG_SETS[flags]
    keep = ~(((1. + np.abs(cols.qed - cols.qst)) / cols.qlen < coverage) | (cols.idy < identity))
    kept = np.flatnonzero(keep)
    assert len(kept) > 32768
    for k in (256, 8192, 32768):
        assert not keep[kept[k] - 1] and not keep[kept[k] + 1]
    t = ri.numpy_tables(cols, *oi.FLAG_SETS[flags])
    assert t.n_rows == len(kept) and len(t.ot_a) > 0 and len(t.ip_a) > 0 and len(t.co_a) > 0
    assert ri.same_tables(t, ri.numpy_tables(generated(0), *oi.FLAG_SETS[flags])) == ""      # the dropped rows change nothing


@pytest.mark.parametrize("k", CPU_KS)
def test_clique_guarantees(k):
    cols, cand, tables, ref = clique_stage(k, "no")
    tax = cand.tax
    assert [t.decode() for t in cand.taxa] == ["ab", "ab-c", "ac", "y", "z"]
    assert tax[:3 * k].tolist() == [1] * k + [0] * k + [2] * k                     # taxon codes do not ascend with the names
    fwd = cand.ip_a < cand.ip_b
    per_taxon = np.bincount(tax[cand.ip_a[fwd]], minlength=5).tolist()
    assert per_taxon == [k * (k - 1) // 2] * 3 + [3, 1]
    assert set(ref["products"]) == {k * k} and len(ref["products"]) == 3 * k == len(cand.ot_a)
    assert ref["blocks"] == {"ot": 2, "co": 2}
    assert ref["kept"] == 2 and ref["dropped"] > 0 and ref["max_occ"] == k          # a repeat of each block's first pair survives, the others go
    assert ref["avg"][4] == 0. and not np.any(tax[tables.ip_a] == 4)               # z: normaliser 0, no IP row
    has_ot = set(cand.ot_a.tolist()) | set(cand.ot_b.tolist())
    y = [c for c in range(len(tax)) if tax[c] == 3]
    assert not has_ot & set(y) and np.sum(tax[tables.ip_a] == 3) == 3              # y: no ortholog -- the mean over all pairs
    # every output row is there: k(k-1)/2 forward pairs per clique taxon + 3, 3k orthologs, every lower cross pair once + the 2 survivors
    assert (len(tables.ip_a), len(tables.ot_a), len(tables.co_a)) == (3 * k * (k - 1) // 2 + 3, 3 * k, 3 * k * (k - 1) + 2)


def test_clique_sizes_the_issue_names():
    assert [clique_stage(k, "no")[3]["max_occ"] for k in (2, 3)] == [2, 3]          # k = 3: a third occurrence
    assert [len(clique_stage(k, "no")[0].q) for k in (33,)] == [9710]
    assert oi.ORTH_WAVE_ROWS < 12 * 11 // 2 and 16 * 16 == 256 and 17 * 17 == 289


@pytest.mark.parametrize("flags", sorted(ri.FLAGS))
def test_sums_depend_on_their_order(flags):
    """with the additions reversed at least one in-paralog normaliser and one (block, taxon) mean change: a kernel that adds in another order
    than the table's cannot pass on these inputs"""
    cols, cand, tables, ref = clique_stage(16, flags)
    rev = ri.reference(cols.names, cand.tax, cand, reverse=True)
    assert any(ref["avg"][t] != rev["avg"][t] for t in ref["avg"])
    assert any(ref["means"][g] != rev["means"][g] for g in ref["means"])
    assert set(ref["means"]) == set(rev["means"]) and ref["co"] != rev["co"]


def _edge_cases():
    both = dict(oi.edge_inputs())
    both.update(ri.edge_inputs())
    return both


@pytest.mark.parametrize("case", sorted(_edge_cases()))
def test_edge_inputs_equal_plain_python(case):
    from swiftortho_amd import find_orth as fo
    cols = _edge_cases()[case]
    for flags in oi.FLAG_SETS.values():
        cand = fo.candidates(cols, *flags)
        if np.isnan(cand.ip_s).any() or np.isnan(cand.ot_s).any() or np.isnan(cand.co_best).any():
            continue                                                                # (0 / 0 under bsr: outside what the stage defines)
        tables = fo.relation_tables(cols.names, cand.tax, cand.taxa, cand)
        ref = ri.reference(cols.names, cand.tax, cand)
        got = ri.as_lists(tables)
        for sec in ("ip", "ot", "co"):
            assert got[sec] == ref[sec], (flags, sec)
        assert fo.lines_from_tables(cols.names, tables) == fo.relations_from_candidates(cols.names, cand.tax, cand.taxa, cand)


def test_edge_inputs_of_the_products():
    """the three hand-made inputs: only the first gene of an ortholog pair has in-paralogs, only the second, neither"""
    from swiftortho_amd import find_orth as fo
    seen = {}
    for case, cols in ri.edge_inputs().items():
        cand = fo.candidates(cols, .5, 0., "no")
        assert len(cand.ip_a) and len(cand.ot_a) and len(cand.co_key), case
        nq = np.searchsorted(cand.ip_a, cand.ot_a, "right") - np.searchsorted(cand.ip_a, cand.ot_a, "left")
        ns = np.searchsorted(cand.ip_a, cand.ot_b, "right") - np.searchsorted(cand.ip_a, cand.ot_b, "left")
        seen[case] = (bool(np.any((nq > 0) & (ns == 0))), bool(np.any((nq == 0) & (ns > 0))), bool(np.all((nq == 0) & (ns == 0))))
        tables = ri.numpy_tables(cols)
        assert len(tables.co_a) == (0 if case == "both_zero" else 1), case
    assert seen == {"nq_only": (True, False, False), "ns_only": (False, True, False), "both_zero": (False, False, True)}
