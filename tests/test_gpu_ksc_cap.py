"""The frequency cap -- k_cap_all, k_cap, k_ksc_order_lds<512|1024|4096>, k_ksc_order_g and the choice among them in chunk_qhits /
chunk_qhits_deferred -- against the oracle on DESIGNED queries: every sort size at which wave_ref_qsort takes another path (1, 2, 6, 7, 8,
31 .. 33, 63 .. 65, 128, 129 windows, every LDS instance at its last and the next at its first window count, the global kernel at 4097 and
with a leaf list that fills), seven key shapes at every size from 33 up, the cut on and around the 64-rank step of k_cap, at the first and
at the last rank and on a total that equals the limit, the flows of the lazy orders (half / one more than half of the batch open, two lists
in three chunks, a long open query deferred to the side stream, in class and in file order), two seed spans and two alphabets.

Per set, on poisoned allocations, twice in one process, with the orders on demand and with the batch: Searcher.query_work() IS the
oracle's number of visited index entries QUERY BY QUERY (before the search's own batch exists and behind it), oracle_vs_gpu passes (the
candidates of every query, rows, seed_hits), and the profile keys say which chunks asked for orders -- as the model of the host's choice
predicts them.  Integers throughout.  The sets, the models and the proof that a per-query sum tells a wrong order or a wrong cut apart on
them are in tests/ksc_cap_inputs.py / tests/test_ksc_cap_inputs.py."""
import pytest

import ksc_cap_inputs as kc
from test_gpu_parity import fs, oracle_vs_gpu  # noqa: F401  (fs is a fixture)

pytestmark = pytest.mark.gpu


def asked(fs, S, kw):
    """(seed.kmer_orders_open_chunks, seed.kmer_orders_all_at_chunk) of one profiled search of the whole set"""
    s = fs.Searcher(profile=True, **kw)
    s.load_ref_bytes(S.ref)
    s.load_queries_bytes(S.qry)
    s.search(0, len(S.qrys)).close()
    t = s.timing()
    s.close()
    return int(t.get("seed.kmer_orders_open_chunks", 0)), int(t.get("seed.kmer_orders_all_at_chunk", 0))


def same_work(S, got, want, when):
    bad = [(q, S.tag.get(q, "query %d" % q), g, w) for q, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not bad, "%s, %s: (query, case, query_work, oracle) %r" % (S.name, when, bad[:8])


def check(fs, oracle, tmp_path, monkeypatch, name, lazy, env=None):
    monkeypatch.setenv("SOHIT_POISON", "165")
    monkeypatch.setenv("SOHIT_KSC_LAZY", lazy)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    S = kc.get_set(oracle, name)
    kw = S.kw(oracle)
    want, _ = kc.reference_work(oracle, name)
    nq = len(S.qrys)
    for turn in ("first", "second"):
        s = fs.Searcher(**kw)   # the pre-pass alone: no search has laid the batch out
        s.load_ref_bytes(S.ref)
        s.load_queries_bytes(S.qry)
        same_work(S, s.query_work().tolist(), want, turn + " searcher, before a search")
        same_work(S, s.query_work(1, nq).tolist(), want[1:], turn + " searcher, a sub-range")
        s.close()

        def stage(s, r):
            same_work(S, s.query_work().tolist(), want, turn + " searcher, behind the search")

        c, st = oracle_vs_gpu(fs, oracle, S.ref, kw, tmp_path, sub=(0, nq), qry=S.qry, stage=stage)
        assert c["seed_hits"] == sum(want)
    flow = asked(fs, S, kw)
    print(name, "lazy", lazy, "flow", flow, "work", want)
    assert flow == kc.model_flow(S, kc.model_of(oracle, S), lazy == "1")[0]
    return flow


LAZY = pytest.mark.parametrize("lazy", ["1", "0"], ids=["orders_on_demand", "orders_with_the_batch"])


@LAZY
@pytest.mark.parametrize("shape", kc.SHAPES)
def test_key_shapes_at_every_tier_edge(fs, oracle, tmp_path, monkeypatch, shape, lazy):
    """33, 63, 64, 65, 128, 129, 512, 513, 1024, 1025, 4096 and 4097 windows of one key shape in one batch: all tied, two values
    interleaved, ascending, descending, a sawtooth, random residues, a SEG-masked stretch (-F T)"""
    check(fs, oracle, tmp_path, monkeypatch, shape, lazy)


@LAZY
def test_sequential_leaf_sizes(fs, oracle, tmp_path, monkeypatch, lazy):
    """1, 2, 6, 7, 8, 31 and 32 windows: the insertion sort, the pivot of exactly 7 elements, the first partition, the last sizes below
    WQS_PAR"""
    check(fs, oracle, tmp_path, monkeypatch, "small", lazy)


@LAZY
@pytest.mark.parametrize("place", kc.PLACES)
def test_cut_places(fs, oracle, tmp_path, monkeypatch, place, lazy):
    """the total in front of rank 62 / 63 / 64 / 65 IS the limit (the <= of the cut on both sides of k_cap's 64-rank step), the first
    window alone exceeds it, only the last window does (k_cap_all opens the query, k_cap keeps it whole): tied and two-valued queries
    of 129 and 1025 windows"""
    check(fs, oracle, tmp_path, monkeypatch, "cut_" + place, lazy)


@LAZY
def test_total_on_the_limit_stays_closed(fs, oracle, tmp_path, monkeypatch, lazy):
    """the windows' total EQUALS the limit: k_cap_all keeps the query whole and asks for no order"""
    assert check(fs, oracle, tmp_path, monkeypatch, "closed", lazy) == (0, 0)


@LAZY
@pytest.mark.parametrize("name", ["half", "half1", "chunks3"])
def test_lazy_order_flows(fs, oracle, tmp_path, monkeypatch, name, lazy):
    """four of eight queries reach their cap (the open ones are ordered), five of eight (everybody is); three chunks with nothing open,
    then queries 1 and 3, then 2 and 3 (a second list, have[] keeps query 3's order)"""
    flow = check(fs, oracle, tmp_path, monkeypatch, name, lazy)
    assert lazy == "0" or flow == {"half": (1, 0), "half1": (0, 1), "chunks3": (6, 0)}[name]


@LAZY
def test_leaf_list_flush(fs, oracle, tmp_path, monkeypatch, lazy):
    """one tied query of FLUSH_NK windows: k_ksc_order_g's leaf list fills and is flushed"""
    check(fs, oracle, tmp_path, monkeypatch, "flush", lazy)


@LAZY
@pytest.mark.parametrize("qclass", ["1", "0"], ids=["class_order", "file_order"])
def test_long_open_query_deferred(fs, oracle, tmp_path, monkeypatch, qclass, lazy):
    """an open query above 4096 windows behind seven light ones: in a class-ordered batch its order is computed on the side stream and
    its class's cap deferred (chunk_qhits_deferred); SOHIT_QCLASS=0: the same queries in one class"""
    flow = check(fs, oracle, tmp_path, monkeypatch, "deferred", lazy, {"SOHIT_QCLASS": qclass})
    assert lazy == "0" or flow == (1, 0)


@LAZY
@pytest.mark.parametrize("name", ["spans", "alphabets"])
def test_several_patterns(fs, oracle, tmp_path, monkeypatch, name, lazy):
    """seeds 111111,11111011111 and two alphabets: a window's count sums over patterns and alphabets, mink is the shorter span"""
    check(fs, oracle, tmp_path, monkeypatch, name, lazy)
