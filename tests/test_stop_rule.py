"""CPU: the designed candidate lists of tests/stop_rule_inputs.py have the shape their labels name -- decided by the oracle's walk alone
(oracle.Result.walk) -- and the Python restatement of the device's round policy and stop walk (tests/stop_rule_model.py) reproduces the
oracle on every one of them.  CAUGHT_BY names, for each single deviation of the restatement, cases on which the deviated restatement
differs from the undeviated one in what tests/test_gpu_stop_rule.py compares the device with: the per-query state, the tasks and cells
aligned, the reported selection (for some entries only the tasks or cells differ, not the rows)."""
import math

import numpy as np
import pytest

import stop_rule_inputs as inputs
import stop_rule_model as model
from stop_rule_model import model_query, model_rounds, model_stop  # noqa: F401  (the names the GPU modules use)

SHADOW = 300   # ranks aligned behind each query's stop: more than any round of these cases reaches past it
_RUNS = {}


def oracle_walk(oracle, tmp_path_factory, name):
    """(Result with walks and shadow, rows text, Result without walks, rows text) of one case, computed once per session"""
    if name not in _RUNS:
        _, ref, qry, kw, _ = inputs.case(name)
        d = tmp_path_factory.mktemp("sr_" + name)
        (d / "r.fsa").write_bytes(ref)
        (d / "q.fsa").write_bytes(qry)
        rw = oracle.blastp(str(d / "q.fsa"), str(d / "r.fsa"), str(d / "w.sc"), walk=True, shadow=SHADOW, **kw)
        r0 = oracle.blastp(str(d / "q.fsa"), str(d / "r.fsa"), str(d / "o.sc"), **kw)
        _RUNS[name] = (rw, (d / "w.sc").read_bytes(), r0, (d / "o.sc").read_bytes())
    return _RUNS[name]


def mixed_shapes(walks, v):
    out = []
    for w in walks:
        m = model_query(w, v)
        out.append(None if not w["ranks"] else (w["walked"], m["stop"], [u for _, _, u in m["rounds"]][:-1], m["state"][3]))
    return out


def test_the_static_list_of_names_is_the_builder_s():
    assert inputs.case_names() == [c[0] for c in inputs.all_cases()] and len(set(inputs.case_names())) == len(inputs.case_names())


def seen(walk):
    """the walk as a string: H a hit, M a miss, T a rank of several (or no) tiles, ? a rank without a verdict"""
    return "".join("?" if k["passed"] is None else ("T" if k["tasks"] != 1 else ("H" if k["passed"] else "M")) for k in walk["ranks"])


@pytest.mark.parametrize("name", inputs.case_names())
def test_case_has_the_shape_its_label_names(oracle, tmp_path_factory, name):
    _, ref, qry, kw, lab = inputs.case(name)
    rw, rows_w, r0, rows_0 = oracle_walk(oracle, tmp_path_factory, name)
    # the walk changes nothing: same rows, same counters
    assert rows_w == rows_0 and np.array_equal(rw.ints, r0.ints)
    assert rw.stats["alignments"] == r0.stats["alignments"] and rw.stats["cells"] == r0.stats["cells"]
    walks = [rw.walk(q) for q in range(rw.nqueries)]
    # ... and adds up to them
    assert sum(k["tasks"] for w in walks for k in w["ranks"][:w["walked"]]) == rw.stats["alignments"]
    assert sum(sum(k["cells"]) for w in walks for k in w["ranks"][:w["walked"]]) == rw.stats["cells"]
    v = kw["v"]
    for q, w in enumerate(walks):
        assert w["mmiss"] == inputs.mmiss(w["ncand"], kw["max_miss"])
        assert len(w["ranks"]) == min(w["ncand"], inputs.vmax(v))
        m = model_query(w, v, qsort=oracle.qsort_perm)
        # the restatement against the oracle: it stops where the reference's loop stops, selects what it emits, reports its rows
        assert not m["blind"]
        assert m["state"][0] == w["walked"], (q, m["state"], w["walked"])
        assert m["state"][3] == sum(k["passed"] for k in w["ranks"][:w["walked"]])
        assert m["cells"] is not None, "query %d: a round reaches more than SHADOW ranks past the stop" % q
        got = [(w["ranks"][r]["subj"], w["ranks"][r]["bits"][t]) for r, t in m["selection"]]
        rows = r0.ints[r0.ints[:, 0] == q]
        assert got == [(int(x[1]), int(x[9])) for x in rows], "query %d: reported rows" % q
    if lab.get("mixed"):
        assert walks[lab["no_candidate"]]["ncand"] == 0 and walks[lab["single_candidate"]]["ncand"] == 1
        finished = {len(model_query(w, v)["rounds"]) for w in walks}
        assert len(finished - {0}) >= lab["min_distinct_rounds"] and 0 in finished, finished
        # the shape every query has in this batch: ranks walked, (round, bit) of the stop, unmch behind the rounds before the last, nsel
        got = mixed_shapes(walks, v)
        assert len(got) == len(lab["shapes"]) == rw.nqueries
        for q, (a, b) in enumerate(zip(got, lab["shapes"])):
            assert a == b, "query %d: %s, labelled %s" % (q, a, b)
        return
    w = walks[0]
    m = model_query(w, v, qsort=oracle.qsort_perm)
    for q, pat in enumerate(lab.get("patterns", [])):
        assert seen(walks[q]).replace("?", "M") == pat.replace("C", "H")[:len(walks[q]["ranks"])], "query %d" % q
    for q, n in enumerate(lab.get("n", [])):
        assert walks[q]["ncand"] == n
    if "cm_is" in lab:
        assert math.ceil(w["mmiss"]) == lab["cm_is"] == lab["cm"][0]
    if "mmiss_is" in lab:
        assert w["mmiss"] == lab["mmiss_is"]
    if lab.get("regime") == "n*m+1":
        assert w["mmiss"] == w["ncand"] * kw["max_miss"] + 1
    if lab.get("regime") == "100/m":
        assert w["mmiss"] == 100. / (w["ncand"] * kw["max_miss"] + 1) > w["ncand"] * kw["max_miss"] + 1
    if lab.get("regime") == "fraction":
        assert w["mmiss"] != math.floor(w["mmiss"]) and 10 < w["mmiss"] < 11
    if lab.get("regime") == "-m 0":
        assert kw["max_miss"] == 0 and w["mmiss"] == 100. / (w["ncand"] * 1e-3 + 1)
    for q, n in enumerate(lab.get("walked", [])):
        assert walks[q]["walked"] == n, (q, walks[q]["walked"])
    for q, n in enumerate(lab.get("nsel", [])):
        assert sum(k["passed"] for k in walks[q]["ranks"][:walks[q]["walked"]]) == n
    for q, n in enumerate(lab.get("ranks_listed", [])):
        assert len(walks[q]["ranks"]) == n < walks[q]["ncand"]
    stop = lab.get("stop")
    if stop == "miss":
        last = w["ranks"][:w["walked"]]
        run = 0
        for k in reversed(last):
            if k["passed"]:
                break
            run += 1
        assert run == math.ceil(w["mmiss"]) and m["stop"] is not None
    if stop == "quota":
        assert m["state"][2] >= v + w["mmiss"] > m["state"][2] - 1 and m["state"][1] < w["mmiss"] and m["stop"] is not None
    if stop == "end":
        assert w["walked"] == w["ncand"] and m["stop"] is None and m["state"][4] == 1
    if stop == "vmax":
        assert w["walked"] == inputs.vmax(v) < w["ncand"] and m["stop"] is None
        assert seen(rw.walk(0))[-1] == "H", "the last walked rank is a hit"
    if "round_of_stop" in lab:
        assert m["stop"] == (lab["round_of_stop"], lab["bit_of_stop"]), m["stop"]
    if "unmch_round_end" in lab:
        want = lab["unmch_round_end"][0]
        assert [u for _, _, u in m["rounds"]][:len(want)] == want, m["rounds"]
    if lab.get("list_ends_at_round_end"):
        first, count, _ = m["rounds"][-1]
        need = max(math.ceil(w["mmiss"]) - (m["rounds"][-2][2] if len(m["rounds"]) > 1 else 0), 8 << (len(m["rounds"]) - 1))
        assert first + count == w["ncand"] and count == need
    if lab.get("behind"):
        first, count, _ = m["rounds"][-1]
        behind = seen(w)[w["walked"]:first + count]
        assert behind.count("H") == lab["behind"] and m["state"][3] == lab["nsel"][0]
    if "rows" in lab:
        assert len(r0.ints) == lab["rows"]
    if "equal_bits" in lab:
        assert len(set(r0.ints[:, 9])) == 1 and sum(k["passed"] for k in w["ranks"][:w["walked"]]) == lab["equal_bits"] > v
    if "nsel_over" in lab:
        assert m["state"][3] > lab["nsel_over"] and len(set(r0.ints[:, 9])) < 10
    if lab.get("tiled"):
        assert any(k["tasks"] > 1 for k in w["ranks"][:w["walked"]])
    if lab.get("two_passing_tiles"):
        assert any(k["passed"] >= 2 for k in w["ranks"][:w["walked"]])
    if lab.get("long_subject"):
        assert max(len(s) for s in ref.decode().split("\n")) >= 4096
    if lab.get("one_task_per_rank"):
        assert all(k["tasks"] == 1 for k in w["ranks"])   # (the ballot walk, not the serial one)


# which designed case tells which single deviation of the restatement from the oracle (at least these: the test prints all of them)
CAUGHT_BY = {
    "gt_for_ge": ["clamp_floor_10", "hit_after_cm", "clamp_ceiling_120"],
    "floor_for_ceil": ["clamp_10_3", "clamp_maxmiss_0", "quota_stop"],
    "unmch_not_carried": ["hit_after_cm_plus_1", "rounds_carry_1_6_5_stop_in_round_4", "ballot_bit63"],
    "mask_at_used_64": ["ballot_bit63", "ballot_late_bit63_hits_behind", "clamp_ceiling_120"],
    "bv_per_rank": ["tiles_long_query"],
    "vmax_plus_1": ["vmax_cut"],
    "nout_without_v": ["select_more_than_v_equal_bits", "quota_stop", "v_zero"],
}


def test_every_deviation_is_caught_by_a_named_case(oracle, tmp_path_factory):
    assert sorted(CAUGHT_BY) == sorted(model.DEVIATIONS)
    table = {d: [] for d in model.DEVIATIONS}
    for name in inputs.case_names():
        kw = inputs.case(name)[3]
        rw = oracle_walk(oracle, tmp_path_factory, name)[0]
        for q in range(rw.nqueries):
            w = rw.walk(q)
            base = model.observable(model_query(w, kw["v"], qsort=oracle.qsort_perm))
            for d in model.DEVIATIONS:
                if model.observable(model_query(w, kw["v"], dev=d, qsort=oracle.qsort_perm)) != base and name not in table[d]:
                    table[d].append(name)
    for d in sorted(table):
        print("%-18s %s\n    caught by: %s" % (d, model.DEVIATIONS[d], ", ".join(table[d])))
    for d, names in CAUGHT_BY.items():
        for name in names:
            assert name in table[d], "%s is not caught by %s (caught by: %s)" % (d, name, table[d])
