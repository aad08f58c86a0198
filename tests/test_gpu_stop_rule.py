"""GPU: the chain between "candidates" and "rows" (csrc/k_phase2.hip) on the designed candidate lists of tests/stop_rule_inputs.py.

Every case: rows byte for byte and candidates equal to the oracle's (oracle_vs_gpu), then per query the device's own phase-2 state
(Searcher.query_phase2) against the restatement of the round policy and of the stop walk run on the oracle's walk
(tests/stop_rule_model.py), and the work counters against the same models.  A failure names the case, the query and the field."""
import pytest

import stop_rule_inputs as inputs
from stop_rule_model import model_query
from test_gpu_parity import fs, oracle_vs_gpu  # noqa: F401  (fs: fixture)
from test_stop_rule import SHADOW

pytestmark = pytest.mark.gpu


def check_case(fs, oracle, tmp_path, name):
    _, ref, qry, kw, _ = inputs.case(name)

    def phase2_state(s, r):
        tasks = cells = 0
        for q in range(r.nqueries):
            m = model_query(r.walk(q), kw["v"])
            got = s.query_phase2(q)
            assert got is not None, "%s: no phase-2 state kept for query %d" % (name, q)
            assert m["cells"] is not None
            want = dict(zip(("next", "unmch", "bv", "nsel", "done"), m["state"]), ntask=m["ntask"], ntile=m["ntile"], qcells=m["cells"])
            for f in fs.Searcher.P2_FIELDS:
                assert got[f] == want[f], "%s: query %d, %s: device %d, model %d (device %s, model %s)" % (name, q, f, got[f], want[f], got, want)
            tasks += m["tasks"]
            cells += m["cells"]
        c = s.counters()
        assert c["alignments"] == tasks, "%s: alignments: device %d, model %d" % (name, c["alignments"], tasks)
        assert c["cells"] == cells, "%s: cells: device %d, model %d" % (name, c["cells"], cells)
        assert c["alignments"] >= r.stats["alignments"] and c["cells"] >= r.stats["cells"]

    # candidates, then the state and the counters, then rows and records byte for byte
    oracle_vs_gpu(fs, oracle, ref, kw, tmp_path, qry=qry, shadow=SHADOW, stage=phase2_state)


@pytest.mark.parametrize("spec", ["0", "1"], ids=["spec_off", "spec_on"])
@pytest.mark.parametrize("name", inputs.case_names())
def test_designed_case(fs, oracle, tmp_path, monkeypatch, name, spec):
    monkeypatch.setenv("SOHIT_SPEC", spec)
    check_case(fs, oracle, tmp_path, name)


@pytest.mark.parametrize("env", [{"SOHIT_ALIGN_LANE_MIN": "0"}, {"SOHIT_ALIGN_PK": "0"}, {"SOHIT_POISON": "0xFF"}, {"SOHIT_POISON": "0xFF", "SOHIT_SPEC": "1"}],
                         ids=["lane_forced", "packed_off", "poison", "poison_spec"])
def test_mixed_batch_under_switches(fs, oracle, tmp_path, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    check_case(fs, oracle, tmp_path, "mixed_batch")
