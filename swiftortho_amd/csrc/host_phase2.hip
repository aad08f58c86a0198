// host_phase2.hip -- libsohit.so host side: phase 2 -- candidates in the reference's order, banded alignments in rounds, stop rule, traces, row emission (see host.h).
#include "host.h"


void aln_decode(const u32* w, int AL, const u8* qp, const u8* sp, char* sq, char* ss) {
    for (int f = 0; f < AL; ++f) {
        const int cc = AL - 1 - f;
        const u32 code = (w[cc >> 4] >> ((cc & 15) << 1)) & 3u;
        sq[f] = code != 2 ? (char)*qp++ : '-';
        ss[f] = code != 3 ? (char)*sp++ : '-';
    }
}

// wait for the row-emission job of the previous batch (if any) and apply its rare post-filter
void emit_join(so_ctx* c, HitBuf& out) {
    if (!c->emit.active) return;
    c->emit.th.join();
    c->emit.active = false;
    if (c->emit.err) {
        std::exception_ptr e = c->emit.err;
        c->emit.err = nullptr;
        std::rethrow_exception(e);
    }
    if (c->emit.dropped.load()) {
        // entry_point re-checks e <= expect (3234).  k_stop_round_w applied the same test to the same
        // doubles, so this never fires; kept as the reference has it.
        const double expect = c->expect;
        if (c->emit.cig) {   // (CIGARs) the batch's runs are the last of out.cig, found through the rows' offsets: compacted first, while the rows still lie where their offsets say
            CigarBuf& g = out.cig;
            size_t w = c->emit.base;
            int64_t rp = g.off[c->emit.base], ap = rp;
            for (size_t k = c->emit.base; k < c->emit.base + c->emit.n; ++k) {
                const int64_t re = g.off[k + 1], nr = re - rp;
                if (out.p[k].evalue <= expect) {
                    if (nr && ap != rp) memmove(g.ops + ap, g.ops + rp, (size_t)nr * sizeof(uint32_t));
                    ap += nr;
                    g.off[++w] = ap;
                }
                rp = re;
            }
            g.n = (size_t)ap;
        }
        size_t wpos = c->emit.base;
        // (alignments) the batch's strings are the last bytes of out.aln, row after row: they are moved along with their rows
        size_t bytes = 0;
        if (c->emit.aln)
            for (size_t k = c->emit.base; k < c->emit.base + c->emit.n; ++k) bytes += 2 * (size_t)std::max(0, out.p[k].aln);
        size_t rpos = out.aln.n - std::min(bytes, out.aln.n), apos = rpos;
        for (size_t k = c->emit.base; k < c->emit.base + c->emit.n; ++k) {
            const size_t nb = c->emit.aln ? 2 * (size_t)std::max(0, out.p[k].aln) : 0;
            if (out.p[k].evalue <= expect) {
                if (nb && apos != rpos) memmove(out.aln.p + apos, out.aln.p + rpos, nb);
                apos += nb;
                out.p[wpos++] = out.p[k];
            }
            rpos += nb;
        }
        out.n = wpos;
        if (c->emit.aln) out.aln.n = apos;
    }
}

// pow(2, -bit) (bit2e, fsearch.py:1086) for bit < P2TAB_N, tabulated once with libm: exact powers of two, 0 past the subnormals
enum { P2TAB_N = 1200 };
static const double* pow2_table() {
    static const std::vector<double> t = [] {
        std::vector<double> v(P2TAB_N);
        for (int k = 0; k < P2TAB_N; ++k) v[k] = p_pow(2, (double)(-k));
        return v;
    }();
    return t.data();
}

// The reported rows' alignment strings, one chain for the search and so_align_pairs_aln.  Slots for the columns of the walks of `list`
// (k_aln_units, scan, k_aln_scatter): the emitting walks write to a.code at a.aofs[task] (ntasks of them).
static void aln_slots(so_ctx* c, AlnChain& a, const AlnTask* tasks, const u32* list, u32 n, u32 ntasks, const AlnSeqs& s) {
    a.units.ensure((size_t)n + 4), a.rofs.ensure((size_t)n + 4), a.aofs.ensure((size_t)ntasks + 4);
    c->d_scan_tmp.ensure(scan_u32_temp_elems((size_t)n + 1) + 8);
    // (a row takes at most 129 units: the 32-bit offsets -- and the word offsets of the compacted columns -- hold 8 M rows per batch)
    if ((u64)n * 129u >= (1ull << 30)) throw SoError("alignments: more than 8 M reported rows in one batch; search a smaller query range per call");
    launch_aln_units(tasks, list, n, s, a.units.p, c->st);
    const size_t units = d2h_u32(c, scan_u32(a.units.p, a.rofs.p, (size_t)n + 1, false, c->d_scan_tmp.p, c->st));
    a.slot_words = units * aln_unit_words();
    a.code.ensure(a.slot_words + 64);
    launch_aln_scatter(list, n, a.rofs.p, a.aofs.p, c->st);
}
// the walks' columns compacted in list order into a.comp (k_aln_words, scan, k_aln_compact) -> their words
static size_t aln_compact(so_ctx* c, AlnChain& a, const u32* list, u32 n, const AlnRes* res) {
    a.words.ensure((size_t)n + 4), a.cofs.ensure((size_t)n + 4);
    launch_aln_words(list, n, res, a.words.p, c->st);
    const size_t words = d2h_u32(c, scan_u32(a.words.p, a.cofs.p, (size_t)n + 1, false, c->d_scan_tmp.p, c->st));
    a.comp.ensure(words + 64);
    launch_aln_compact(list, n, a.aofs.p, a.code.p, a.cofs.p, a.comp.p, c->st);
    return words;
}
// the walks' columns run-length coded in list order (k_cigar_count, scan, k_cigar_emit): a.oofs (n + 1 offsets) and a.ops -> the runs
static size_t cigar_code(so_ctx* c, AlnChain& a, const u32* list, u32 n, const AlnRes* res) {
    // (a run is at least one column and a slot word holds sixteen: the 32-bit scan of the runs holds as long as the slots' words stay below 2^28)
    if (a.slot_words * 16ull >= (1ull << 32)) throw SoError("CIGARs: the reported rows of one batch hold 2^32 columns or more; search a smaller query range per call");
    a.runs.ensure((size_t)n + 4), a.oofs.ensure((size_t)n + 4);
    launch_cigar_count(list, n, a.aofs.p, a.code.p, res, a.runs.p, c->st);
    const size_t n_ops = d2h_u32(c, scan_u32(a.runs.p, a.oofs.p, (size_t)n + 1, false, c->d_scan_tmp.p, c->st));
    a.ops.ensure(n_ops + 64);
    launch_cigar_emit(list, n, a.aofs.p, a.code.p, res, a.oofs.p, a.ops.p, c->st);
    return n_ops;
}
// where list position i's compacted columns start: the running sum of ceil(aln_at(i) / 16) words, which must come to the compacted total
template <class F>
static std::vector<size_t> aln_word_offsets(size_t n, F aln_at, size_t words, const char* who) {
    std::vector<size_t> w(n + 1, 0);
    for (size_t i = 0; i < n; ++i) w[i + 1] = w[i] + (size_t)(std::max(0, (int)aln_at(i)) + 15) / 16;
    if (w[n] != words) throw SoError(std::string(who) + ": column words do not add up");
    return w;
}

// what the stages of one phase2() call hand on to each other
struct P2 {
    P2(so_ctx* c, const Batch& b) : sc(c), nq(b.nq) {}
    const double t0 = wall();
    StageClock sc;
    u32 nq, Ntot = 0, NT = 0, nspec = 0, NO = 0;
    AlnSeqs seqs{};
    bool align_sort = false, pk_on = false, pk_mixed = false, lane_on = false, traced_pk = false, aln_on = false, cig_on = false;
    u32 stride = 0, slab = 0, TU = 0;   // batch-wide trace stride, tasks per trace slab, trace unit
    size_t var_budget_words = 0, aln_words = 0, cig_ops = 0;
    int parts = 1; u32 qstep = 0;       // emission ranges, queries per range
    std::array<u32, EMIT_PARTS_MAX + 1> part_row{};   // first row of emission range q, NO behind the last
    std::vector<u32> h_ooff;   // (permuted batch, host rows: the slots' first rows, for the file-order placement -- fetched with the totals)
};

// the chunks' candidates of every query, gathered per query (b.fin_rec at b.qcoff); false: there are none
static bool gather_candidates(so_ctx* c, Batch& b, P2& p) {
    const int nchunks = (int)c->chunks.size();
    const u32 nq = p.nq;
    const u32 Ntot = p.Ntot = b.chunk_base.empty() ? 0u : b.chunk_base.back();
    b.qtot.ensure((size_t)nq + 4), b.qcoff.ensure((size_t)nq + 4), b.prior.ensure((size_t)nq + 4), b.cqoff.ensure((size_t)nq + 4);
    HIP_CHECK(hipMemsetAsync(b.qtot.p, 0, ((size_t)nq + 4) * sizeof(u32), c->st));
    for (int ci = 0; ci < nchunks; ++ci) launch_add_u32(b.qtot.p, b.ccnt.p + (size_t)ci * nq, nq, c->st);
    c->d_scan_tmp.ensure(scan_u32_temp_elems((size_t)nq + 1) + 8);
    scan_u32(b.qtot.p, b.qcoff.p, (size_t)nq + 1, false, c->d_scan_tmp.p, c->st);
    b.fin_rec.ensure(4 * (size_t)Ntot + 16);
    HIP_CHECK(hipMemsetAsync(b.prior.p, 0, ((size_t)nq + 4) * sizeof(u32), c->st));
    for (int ci = 0; ci < nchunks; ++ci) {
        const u32 lo = ci == 0 ? 0u : b.chunk_base[ci - 1], hi = b.chunk_base[ci];
        const u32* cc = b.ccnt.p + (size_t)ci * nq;
        if (hi > lo) {
            scan_u32(cc, b.cqoff.p, nq, false, c->d_scan_tmp.p, c->st);
            launch_gather_cands(b.cand_q.p + lo, b.cand_rec.p + 4 * (size_t)lo, hi - lo, b.cqoff.p, b.prior.p, b.qcoff.p, b.fin_rec.p,
                                c->st);
        }
        launch_add_u32(b.prior.p, cc, nq, c->st);
    }
    p.sc.lap("phase2.gather");
    // candidate dump for so_query_candidates (tests only)
    if (tune().keep_cands) {
        std::vector<u32> qcoff((size_t)nq + 1), rec(4 * (size_t)Ntot + 4);
        HIP_CHECK(hipMemcpyAsync(qcoff.data(), b.qcoff.p, ((size_t)nq + 1) * sizeof(u32), hipMemcpyDeviceToHost, c->st));
        if (Ntot) HIP_CHECK(hipMemcpyAsync(rec.data(), b.fin_rec.p, 4 * (size_t)Ntot * sizeof(u32), hipMemcpyDeviceToHost, c->st));
        HIP_CHECK(hipStreamSynchronize(c->st));
        for (u32 q = 0; q < nq; ++q) {
            auto& dst = c->last_cands[(size_t)(b.q_lo - c->last_q_lo) + b.qid[q]];
            dst.assign(rec.begin() + 4 * (size_t)qcoff[q], rec.begin() + 4 * (size_t)qcoff[q + 1]);
        }
    }
    return Ntot != 0;
}

// csort: the candidates each query considers, in order; mktasks: their alignment tasks; and the aligners' settings for the batch
static void make_tasks(so_ctx* c, Batch& b, P2& p) {
    const u32 nq = p.nq, Ntot = p.Ntot;
    const u32 vmax = (u32)std::max<i64>(100, std::max<i64>(c->v + 100, (i64)((double)c->v * 1.1)));  // fsearch.py:3059
    // ranks = candidates considered (top vmax); tasks = alignments (1 per rank, or one per 4096-tile
    // of a long candidate, kswat_st_long)
    b.perm.ensure((size_t)Ntot + 4), b.ntask.ensure((size_t)nq + 4), b.ntile.ensure((size_t)nq + 4);
    b.toff.ensure((size_t)nq + 4), b.roffc.ensure((size_t)nq + 4);
    HIP_CHECK(hipMemsetAsync(b.ntask.p, 0, ((size_t)nq + 4) * sizeof(u32), c->st));
    HIP_CHECK(hipMemsetAsync(b.ntile.p, 0, ((size_t)nq + 4) * sizeof(u32), c->st));
    // queries with more candidates than the LDS sort holds need global scratch for the wave sort
    // (through the pinned per-query buffer of the seed stage: a pageable read of nq words costs more than the kernels around it)
    if (c->h_qhits_cap < nq) {
        if (c->h_qhits) (void)hipHostFree(c->h_qhits);
        c->h_qhits_cap = (size_t)nq + 1024;
        HIP_CHECK(hipHostMalloc((void**)&c->h_qhits, c->h_qhits_cap * sizeof(unsigned long long), hipHostMallocDefault));
    }
    const u32* qt = reinterpret_cast<const u32*>(c->h_qhits);
    HIP_CHECK(hipMemcpyAsync(c->h_qhits, b.qtot.p, (size_t)nq * sizeof(u32), hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    u32 mx = 0;
    for (u32 i = 0; i < nq; ++i) mx = std::max(mx, qt[i]);
    u64* gx = nullptr;
    u32 *gL = nullptr, *gR = nullptr;
    if ((int)mx > csort_lds_max()) {
        b.gx.ensure((size_t)Ntot + 4), b.gL.ensure((size_t)Ntot + 4), b.gR.ensure((size_t)Ntot + 4);
        gx = b.gx.p, gL = b.gL.p, gR = b.gR.p;
    }
    // (the lists too long for the LDS instances are sorted in global scratch, a wave each: beside the LDS instances, on the side stream)
    const bool cs_aside = gx != nullptr;
    if (cs_aside) {
        HIP_CHECK(hipEventRecord(c->ev_ug_go, c->st));
        HIP_CHECK(hipStreamWaitEvent(c->st_side, c->ev_ug_go, 0));
    }
    launch_csort(b.fin_rec.p, b.qcoff.p, nq, vmax, b.dev.d_off.p, c->ref.d_off.p, b.perm.p, b.ntask.p, b.ntile.p, gx, gL, gR, c->st,
                 cs_aside ? c->st_side : c->st);
    if (cs_aside) {
        HIP_CHECK(hipEventRecord(c->ev_ug_done, c->st_side));
        HIP_CHECK(hipStreamWaitEvent(c->st, c->ev_ug_done, 0));
    }
    const u32* dNRk = scan_u32(b.ntask.p, b.roffc.p, (size_t)nq + 1, false, c->d_scan_tmp.p, c->st);
    stash_u32(c, dNRk, SM_STASH0);
    const u32* dNT = scan_u32(b.ntile.p, b.toff.p, (size_t)nq + 1, false, c->d_scan_tmp.p, c->st);
    u32 NRK;
    d2h_pair(c, dNT, NRK, p.NT);
    const u32 NT = p.NT;
    p.sc.lap("phase2.csort");
    b.tasks.ensure((size_t)NT + 4), b.ares.ensure((size_t)NT + 4), b.bits.ensure((size_t)NT + 4), b.sel.ensure((size_t)NT + 4);
    b.rk_slot.ensure((size_t)NRK + 4);
    b.qcells.ensure((size_t)nq + 2);
    HIP_CHECK(hipMemsetAsync(b.qcells.p, 0, ((size_t)nq + 2) * sizeof(unsigned long long), c->st));   // cells per query, added up by the stop rule
    launch_mktasks(b.fin_rec.p, b.qcoff.p, b.perm.p, b.ntask.p, b.roffc.p, b.toff.p, nq, b.dev.d_off.p, c->ref.d_off.p, b.tasks.p,
                   b.rk_slot.p, c->st);
    // k_align runs four alignments per wave and a wave lasts as long as its longest one: every launch list is ordered by band rows,
    // longest first (one 13-bit radix sort; config 3: align rounds 33.6 -> 28.4 ms, sort included).  SOHIT_ALIGN_SORT=0: as listed.
    p.align_sort = tune().align_sort;
    // The packed 16-bit aligner takes a task whose scores fit its cells: 11 * min(rows, columns), or the smaller of the two sequences'
    // score bounds (k_seq_bound), within range.  That is a property of the TASK: a launch list is split into the tasks it cannot take
    // (k_task_rows clears bit 13 of their sort key, so they lead the sorted list, and counts them) and the rest.  Only batches that hold
    // a query AND a reference sequence above the length limit can contain such tasks at all.
    const u32 maxwin_q = std::min<u32>(b.maxqlen, LONG_SEQ), maxwin_s = std::min<u32>(c->ref.maxlen, LONG_SEQ);
    p.pk_on = tune().align_pk && align_pk_supported(c->st);
    p.pk_mixed = p.pk_on && (int)std::min(maxwin_q, maxwin_s) > align_pk_max_len();
    p.seqs = AlnSeqs{aln_side(b.dev), aln_side(c->ref), c->d_b62c.p};
    // score-only rounds by k_align_lane (a lane per alignment pair) when every task's windows end where its sequences end: no tiles
    p.lane_on = p.pk_on && tune().align_lane && b.maxqlen < LONG_SEQ && c->ref.maxlen < LONG_SEQ;
    p.traced_pk = p.pk_on;   // traced alignments by the packed kernel too (k_align<true> keeps the tasks whose scores need 32-bit cells)
    p.stride = align_trace_stride((int)std::min<u32>(std::max(maxwin_q, maxwin_s), std::min(maxwin_q, maxwin_s) + 16) + 1);   // (longest band + 1)
    // (SOHIT_TRACE_VAR_MAX, tests: both budgets lowered to its value, so that small sets take the slab route and the kept traces' fallback)
    const long long trace_var_max = tune().trace_var_max;
    const size_t budget_words = trace_var_max >= 0 ? (size_t)trace_var_max : (size_t)1 << 30;  // 4 GiB of trace scratch for the fixed-stride slabs
    p.slab = (u32)std::max<size_t>(16, std::min<size_t>(std::max<u32>(NT, 1), budget_words / std::max<u32>(p.stride, 1)));
    // Traces take what each task's own band needs: room per task (k_trace_units), scanned into b.tr_ofs; up to 8 GiB per launch list,
    // beyond that the list falls back to slabs of the batch-wide stride.  (`stride` follows the longest window of the batch: one
    // 4096-residue pair and every 300-row alignment owned 33 KB of trace, which its traceback then strode over.)
    p.var_budget_words = trace_var_max >= 0 ? (size_t)trace_var_max : (size_t)1 << 31;
    p.TU = align_trace_unit();
    b.st_state.ensure(5 * (size_t)nq + 8), b.rcnt.ensure((size_t)nq + 4), b.tcnt.ensure((size_t)nq + 4), b.roff.ensure((size_t)nq + 4);
    b.order_tmp.ensure((size_t)nq + 4);
    b.ridx.ensure((size_t)NT + 4);
    HIP_CHECK(hipMemsetAsync(b.st_state.p, 0, (5 * (size_t)nq + 8) * sizeof(u32), c->st));
    p.sc.lap("phase2.mktasks");
}

// Positions [0, n) of launch list `in` to `out`, longest band first: k_task_rows' keys, one radix sort.  n_wide (non-null, zeroed): the tasks
// the packed kernel cannot take lead the list and are counted there; cells (non-null): += their band cells.
// (ordering inside blocks of 2^k queries instead of globally -- key = query block << 13 | rows -- was measured: 24.9-25.2 ms of align rounds
// for k = 7 ... 13 against 24.8-25.2)
static void order_by_rows(so_ctx* c, Batch& b, const AlnSeqs& s, const u32* in, u32 n, u32* out, u32* n_wide, unsigned long long* cells) {
    if (!n) return;
    b.tmp64.ensure((size_t)n + 2), b.c_ft2.ensure((size_t)n + 2);
    ensure_sort_tmp(c, sort_pairs_u64_u32_temp_bytes(n, 64));
    launch_task_rows(b.tasks.p, in, n, s, n_wide, cells, b.tmp64.p, c->st);
    sort_pairs_u64_u32(c->d_sort_tmp.p, c->d_sort_tmp.cap, b.tmp64.p, b.c_ft2.p, in, out, n, n_wide ? 14 : 13, c->st);
}

// an align round's launch list, ordered by band rows into b.ridx2 unless it is short or SOHIT_ALIGN_SORT=0 asks for none; n_wide (non-null):
// the tasks at its head that need the 32-bit cells (all of them when the packed kernels are off)
static const u32* round_list(so_ctx* c, Batch& b, const P2& p, const u32* list, u32 n, u32* n_wide) {
    const bool split = n_wide && p.pk_mixed;
    if (n_wide) *n_wide = p.pk_on ? 0u : n;
    if (!split && (!p.align_sort || n < 4096)) return list;
    b.ridx2.ensure((size_t)n + 2);
    c->d_small.ensure(SM_WORDS);
    if (split) HIP_CHECK(hipMemsetAsync(c->d_small.p + SM_WIDE_ROUND, 0, sizeof(u32), c->st));
    order_by_rows(c, b, p.seqs, list, n, b.ridx2.p, split ? c->d_small.p + SM_WIDE_ROUND : nullptr, b.ucount.p + 2);
    if (split) *n_wide = d2h_u32(c, c->d_small.p + SM_WIDE_ROUND);
    return b.ridx2.p;
}

// trace room of every position of a launch list (b.tr_ofs, units of p.TU words) -> words the list's traces need
static size_t trace_offsets(so_ctx* c, Batch& b, const P2& p, const u32* list, u32 n) {
    // the offsets are a 32-bit scan of units: a list whose total could wrap (no task needs more units than the batch-wide stride holds)
    // takes the slab path -- "does not fit" for both callers
    if ((u64)n * ((u64)(p.stride + p.TU - 1) / p.TU + 1) >= (1ull << 32)) return ~(size_t)0;
    b.tr_units.ensure((size_t)n + 4), b.tr_ofs.ensure((size_t)n + 4);
    c->d_scan_tmp.ensure(scan_u32_temp_elems((size_t)n + 1) + 8);
    launch_trace_units(b.tasks.p, list, n, p.seqs, b.tr_units.p, c->st);
    return (size_t)d2h_u32(c, scan_u32(b.tr_units.p, b.tr_ofs.p, (size_t)n + 1, false, c->d_scan_tmp.p, c->st)) * p.TU;
}

// banded alignments in rounds (see k_round_counts / k_stop_round_w), score-only but for the speculative traces of the first round
static void align_rounds(so_ctx* c, Batch& b, P2& p) {
    const u32 nq = p.nq, NT = p.NT;
    const AlnSeqs& s = p.seqs;
    u32 aligned_total = 0;
    // Speculative traces (k_round_counts_spec): in the FIRST round, the leading tasks of every query whose ungapped score alone would pass
    // the e-value test are aligned with traces at once; reported rows that have one skip the second alignment.  SOHIT_SPEC=0: off.
    // SOHIT_SPEC=0 / 1: off / on whatever the size (default: on from 2^21 tasks; below that the extra launches cost more than they save:
    // config 2, 0.55 M tasks, 16.7 -> 17.1 ms).  SOHIT_SPEC_SLACK: the guess tests the ungapped score against expect x this (default 1e6 since the end of
    // round 6 -- with the cheaper walk and the one-launch alignment of the rows left over, config 3 interleaved: 1e2 47.70 ms, 1e3 47.56, 1e4 47.51, 1e5 47.38,
    // 1e6 47.21, 1e7 47.17, 1e8 47.28, 1e10 53.2 (the first round's traces no longer fit); the weight-6 and mixed-length sets do not care.  Round 5, 1e3:
    // config 3 keeps 1.44 M traces, all of them of reported rows, 175 k rows are left for the second pass; 1: 1.30 M / 315 k; 1e6: 1.56 M /
    // 57 k with 1.3 k traces unused -- a wrong guess costs about as much as a right one saves).
    const bool spec_on = tune().spec >= 0 ? tune().spec != 0 : NT >= (1u << 21);
    const double spec_slack = tune().spec_slack;
    u32 spec_cap = NT;   // (8 GiB of kept traces at most: checked on the list's actual trace sizes below)
    if (tune().spec_cap >= 0) spec_cap = (u32)tune().spec_cap;   // (tests: the round that does not fit)
    if (spec_on) {
        b.tpos.ensure((size_t)NT + 4);
        HIP_CHECK(hipMemsetAsync(b.tpos.p, 0xFF, ((size_t)NT + 4) * sizeof(u32), c->st));   // 0xFFFFFFFF = no trace kept
    }
    bool first_round = true;
    for (u32 minr = 8;; minr = minr < 256 ? minr * 2 : minr) {
        u32 NR = 0, RR = 0, NS = 0;
        bool spec_round = spec_on && first_round;
        first_round = false;
        if (spec_round) {
            b.spcnt.ensure((size_t)nq + 4), b.spoff.ensure((size_t)nq + 4), b.sidx.ensure((size_t)NT + 4);
            c->d_small.ensure(SM_WORDS);
            HIP_CHECK(hipMemsetAsync(c->d_small.p + SM_ANY_RANK, 0, sizeof(u32), c->st));
            launch_round_counts_spec(b.ntask.p, b.ntile.p, b.roffc.p, b.rk_slot.p, b.qcoff.p, b.st_state.p, nq, c->max_miss, minr, b.tasks.p, b.toff.p,
                                     b.dev.d_off.p, c->ref.d_off.p, c->d_bittab.p, so_ctx::BITTAB_N, c->ref.N, c->expect * spec_slack, b.rcnt.p, b.tcnt.p, b.spcnt.p,
                                     c->d_small.p + SM_ANY_RANK, c->st);
            stash_u32(c, scan_u32(b.tcnt.p, b.roff.p, (size_t)nq + 1, false, c->d_scan_tmp.p, c->st), SM_STASH0);
            stash_u32(c, scan_u32(b.spcnt.p, b.spoff.p, (size_t)nq + 1, false, c->d_scan_tmp.p, c->st), SM_STASH1);
            u32* v = (u32*)small_host(c);
            HIP_CHECK(hipMemcpyAsync(v, c->d_small.p, (SM_ANY_RANK + 1) * sizeof(u32), hipMemcpyDeviceToHost, c->st));
            HIP_CHECK(hipStreamSynchronize(c->st));
            NR = v[SM_STASH0], NS = v[SM_STASH1], RR = v[SM_ANY_RANK];
            if (NS > spec_cap) spec_round = false;   // the traces would not fit: this round again, without them
        }
        if (!spec_round) {
            NS = 0;
            launch_round_counts(b.ntask.p, b.ntile.p, b.roffc.p, b.rk_slot.p, b.qcoff.p, b.st_state.p, nq, c->max_miss, minr, b.rcnt.p,
                                b.tcnt.p, c->st);
            const u32* dNR = scan_u32(b.tcnt.p, b.roff.p, (size_t)nq + 1, false, c->d_scan_tmp.p, c->st);
            stash_u32(c, dNR, SM_STASH0);
            // ranks left this round (a round may hold ranks with zero tiles only)
            const u32* dRR = scan_u32(b.rcnt.p, b.order_tmp.p, (size_t)nq + 1, false, c->d_scan_tmp.p, c->st);
            d2h_pair(c, dRR, NR, RR);
        }
        if (RR == 0) break;
        if (spec_round) {
            launch_round_idx_spec(b.tcnt.p, b.spcnt.p, b.roff.p, b.spoff.p, b.toff.p, b.ntask.p, b.ntile.p, b.roffc.p, b.rk_slot.p, b.st_state.p, nq,
                                  b.ridx.p, b.sidx.p, c->st);
            if (NS) {
                u32 nw_s = 0;   // (leading tasks of the ordered list whose scores need 32-bit cells)
                const u32* slist = round_list(c, b, p, b.sidx.p, NS, p.traced_pk ? &nw_s : nullptr);
                if (!p.traced_pk) nw_s = NS;
                const size_t tw = trace_offsets(c, b, p, slist, NS);
                ProfTimer pt(c, &c->cnt.align_ms, &c->cnt.align_launches);
                if (tw <= p.var_budget_words) {
                    b.spec_trace.ensure(tw + 64);
                    launch_align_traced(b.tasks.p, slist, NS, s, b.spec_trace.p, p.TU, b.tr_ofs.p, b.ares.p, b.tpos.p, 0u, c->st, nw_s);
                    p.nspec = NS;
                } else {   // the traces would not fit after all: these tasks score-only, like the rest of the round
                    if (tune().debug) fprintf(stderr, "[sohit] kept traces do not fit: %u tasks scored only\n", NS);
                    launch_align(b.tasks.p, slist, NS, s, b.ares.p, c->st);
                }
                pt.stop();
            }
        } else if (NR) {
            launch_round_idx(b.tcnt.p, b.roff.p, b.toff.p, b.ntask.p, b.ntile.p, b.roffc.p, b.rk_slot.p, b.st_state.p, nq, b.ridx.p, c->st);
        }
        if (NR) {
            // score-only: the stop rule needs the maximum alone; the reported rows are traced in a second pass (trace_pass)
            u32 n_wide = 0;
            const u32* rlist = round_list(c, b, p, b.ridx.p, NR, &n_wide);
            ProfTimer pt(c, &c->cnt.align_ms, &c->cnt.align_launches);
            // score-only: the packed 16-bit kernel (two alignments per register) for every task whose scores fit it, the 32-bit one for the
            // n_wide tasks at the head of the list that do not
            // (the few wide tasks of a mixed batch are its longest: a launch of their own lasts as long as one 4096-row band, ~0.5 ms per
            // round with the GPU nearly idle -- so they run beside the packed kernel, on st_side, which is idle in phase 2; st_ug would
            // not do: it shares its hardware queue with the batch's stream on this runtime -- four queues, dealt round-robin)
            const bool wide_aside = n_wide && NR > n_wide;
            hipStream_t wst = wide_aside ? c->st_side : c->st;
            if (wide_aside) {
                HIP_CHECK(hipEventRecord(c->ev_ug_go, c->st));
                HIP_CHECK(hipStreamWaitEvent(c->st_side, c->ev_ug_go, 0));
            }
            if (n_wide) launch_align(b.tasks.p, rlist, n_wide, s, b.ares.p, wst);
            if (wide_aside) HIP_CHECK(hipEventRecord(c->ev_ug_done, c->st_side));
            if (NR > n_wide) {
                // (a lane walks a whole alignment alone: a launch lasts at least one alignment's ~0.4 ms however few tasks it holds -- the last
                // rounds of config 3, 6.6 k and 64 tasks, took 0.63 and 0.40 ms; sixteen lanes per pair finish those in 0.1; SOHIT_ALIGN_LANE_MIN, default 2^18)
                if (p.lane_on && (long long)(NR - n_wide) >= tune().align_lane_min) {
                    c->d_small.ensure(SM_WORDS);
                    launch_align_lane(b.tasks.p, rlist + n_wide, NR - n_wide, s, b.ares.p, c->d_small.p + SM_LANE_CTR, c->ncu, c->st);
                } else {
                    launch_align_pk(b.tasks.p, rlist + n_wide, NR - n_wide, s, b.ares.p, c->st);
                }
            }
            if (wide_aside) HIP_CHECK(hipStreamWaitEvent(c->st, c->ev_ug_done, 0));
            pt.stop();
            c->cnt.align_wide += n_wide;
        }
        launch_stop_round_w(b.tasks.p, b.ares.p, b.qcoff.p, b.ntask.p, b.ntile.p, b.roffc.p, b.rk_slot.p, b.toff.p, b.rcnt.p, nq,
                            b.dev.d_off.p, c->ref.d_off.p, c->d_bittab.p, so_ctx::BITTAB_N, c->ref.N, c->expect, c->max_miss, c->v, b.sel.p,
                            b.st_state.p, b.bits.p, b.qcells.p, c->st);
        aligned_total += NR + NS;
    }
    launch_sum_u64(b.qcells.p, nq, b.ucount.p + 1, c->st);
    // state dump for so_query_phase2 (tests only)
    if (tune().keep_cands) {
        std::vector<u32> state(5 * (size_t)nq), ntask(nq), ntile(nq);
        std::vector<unsigned long long> qcells(nq);
        HIP_CHECK(hipMemcpyAsync(state.data(), b.st_state.p, 5 * (size_t)nq * sizeof(u32), hipMemcpyDeviceToHost, c->st));
        HIP_CHECK(hipMemcpyAsync(ntask.data(), b.ntask.p, (size_t)nq * sizeof(u32), hipMemcpyDeviceToHost, c->st));
        HIP_CHECK(hipMemcpyAsync(ntile.data(), b.ntile.p, (size_t)nq * sizeof(u32), hipMemcpyDeviceToHost, c->st));
        HIP_CHECK(hipMemcpyAsync(qcells.data(), b.qcells.p, (size_t)nq * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->st));
        HIP_CHECK(hipStreamSynchronize(c->st));
        for (u32 q = 0; q < nq; ++q) {
            auto& dst = c->last_p2[(size_t)(b.q_lo - c->last_q_lo) + b.qid[q]];
            for (int k = 0; k < 5; ++k) dst[k] = (int64_t)state[5 * (size_t)q + k];
            dst[5] = (int64_t)ntask[q], dst[6] = (int64_t)ntile[q], dst[7] = (int64_t)qcells[q];
        }
    }
    p.sc.lap("phase2.align_rounds");
    c->cnt.alignments += aligned_total;
}

// final selection: the reported rows, their total and the first rows of the emission ranges
static void select_rows(so_ctx* c, Batch& b, P2& p) {
    const u32 nq = p.nq;
    b.nout.ensure((size_t)nq + 4), b.ooff.ensure((size_t)nq + 4);
    HIP_CHECK(hipMemsetAsync(b.nout.p, 0xFF, (size_t)nq * sizeof(u32), c->st));  // 0xFFFFFFFF = not selected yet
    HIP_CHECK(hipMemsetAsync(b.nout.p + nq, 0, 4 * sizeof(u32), c->st));
    launch_final_select(b.toff.p, nq, c->v, b.sel.p, b.st_state.p, b.bits.p, b.nout.p, c->st);
    const u32* dNO = scan_u32(b.nout.p, b.ooff.p, (size_t)nq + 1, false, c->d_scan_tmp.p, c->st);
    // The reported rows leave in up to EMIT_PARTS_MAX query ranges: a range's rows are traced, written and sent to the host while the next
    // range is being traced (one batch per search leaves nothing else to hide the download behind).  The ranges' first rows come
    // back with the row total: ooff at every (nq / parts)-th query.
    // SOHIT_EMIT_PARTS (1-8, default 4) / SOHIT_EMIT_MIN_ROWS (default 2^18: smaller results leave in one piece): tuning and test switches
    // (with kept traces -- nspec -- on a batch of mixed lengths the last stage orders and launches per range: two ranges, 66.0 against 66.9 ms with
    // four on the log-normal set; a uniform batch takes four since its left-over rows are aligned in one launch: config 3 1 range 48.26 ms, 2 47.19, 3 46.98,
    // 4 46.91, 5 47.06, 6 47.16, 8 47.47)
    const int emit_parts = std::min<int>(EMIT_PARTS_MAX, std::max(1, (p.nspec && (b.permuted || p.pk_mixed)) ? 2 : (int)tune().emit_parts));
    const u32 emit_min_rows = (u32)std::max(1ll, tune().emit_min_rows);
    // (config 3, one batch: 1 part 57.0 ms per step, 4 parts 56.0)
    const u32 qstep = p.qstep = (nq + emit_parts - 1) / emit_parts;
    c->d_small.ensure(SM_WORDS);
    launch_stride_gather(b.ooff.p, qstep, (nq + qstep - 1) / qstep, c->d_small.p + SM_PART_ROW, c->st);
    stash_u32(c, dNO, SM_STASH0);
    u32* v = (u32*)small_host(c);
    HIP_CHECK(hipMemcpyAsync(v, c->d_small.p, (SM_PART_ROW + EMIT_PARTS_MAX) * sizeof(u32), hipMemcpyDeviceToHost, c->st));
    if (b.permuted && !c->dev_out) {
        p.h_ooff.resize((size_t)nq + 1);
        HIP_CHECK(hipMemcpyAsync(p.h_ooff.data(), b.ooff.p, ((size_t)nq + 1) * sizeof(u32), hipMemcpyDeviceToHost, c->st));
    }
    HIP_CHECK(hipStreamSynchronize(c->st));
    const u32 NO = p.NO = v[SM_STASH0];
    for (int q = 0; q <= emit_parts; ++q) p.part_row[q] = (u64)q * qstep < nq ? v[SM_PART_ROW + q] : NO;
    p.parts = (c->dev_out || NO < emit_min_rows) ? 1 : emit_parts;
    if (p.parts == 1) p.part_row[1] = NO;
    p.aln_on = c->want_aln && !c->dev_out;
    p.cig_on = c->want_cigar && !c->dev_out;
    p.sc.lap("phase2.stop");
}

// Kept traces: rows that have one only need the walk, the others are aligned with traces now.  The row list is split stably
// (flags, scan, scatter) into b.sel_b (no trace) and b.sel_a; range q's rows without a trace are b.sel_b's [pb[q], pb[q + 1]), the others
// b.sel_a's [first row - pb[q], ...): the scan values at the ranges' first rows come back in one small copy.  (pb[0] = 0 on entry)
static void split_kept_traces(so_ctx* c, Batch& b, const P2& p, u32* pb /*parts + 1*/) {
    const u32 NO = p.NO;
    const int parts = p.parts;
    const u32* slist = b.sel_idx.p;
    b.flags.ensure((size_t)NO + 4), b.gidx.ensure((size_t)NO + 4), b.sel_b.ensure((size_t)NO + 4), b.sel_a.ensure((size_t)NO + 4);
    c->d_scan_tmp.ensure(scan_u32_temp_elems((size_t)NO + 1) + 8);
    launch_trace_flags(slist, NO, b.tpos.p, b.flags.p, c->st);
    const u32* dNB = scan_u32(b.flags.p, b.gidx.p, NO, false, c->d_scan_tmp.p, c->st);
    launch_trace_split(slist, NO, b.flags.p, b.gidx.p, b.sel_b.p, b.sel_a.p, c->st);
    u32* v = (u32*)small_host(c);
    HIP_CHECK(hipMemcpyAsync(v + parts, dNB, sizeof(u32), hipMemcpyDeviceToHost, c->st));
    for (int q = 1; q < parts; ++q)
        if (p.part_row[q] < NO) HIP_CHECK(hipMemcpyAsync(v + q, b.gidx.p + p.part_row[q], sizeof(u32), hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    pb[parts] = v[parts];
    for (int q = 1; q < parts; ++q) pb[q] = p.part_row[q] < NO ? v[q] : pb[parts];
    if (tune().debug) fprintf(stderr, "[sohit] kept traces %u, reported rows %u, of them without a trace %u\n", p.nspec, NO, pb[parts]);
}

// The trace pass's lists ordered by band rows inside each emission range (b.tl_sorted; with kept traces also the walk-only list, b.al_sorted).
// nwide[q]: the tasks at the head of range q's traced list that need the 32-bit cells, when the packed kernel takes the rest of a mixed batch.
static void order_trace_lists(so_ctx* c, Batch& b, const P2& p, const u32* tlist, u32 tn, const u32* alist, const u32* pb, u32* nwide) {
    // (the ranges' counts come back in ONE copy behind the loop: a synchronisation per range stalled the range-by-range overlap)
    c->d_small.ensure(SM_WORDS);
    const bool split = p.traced_pk && p.pk_mixed;
    if (split) HIP_CHECK(hipMemsetAsync(c->d_small.p + SM_WIDE_PART, 0, EMIT_PARTS_MAX * sizeof(u32), c->st));
    b.tl_sorted.ensure((size_t)tn + 4);
    if (p.nspec) b.al_sorted.ensure((size_t)(p.NO - tn) + 4);
    for (int q = 0; q < p.parts; ++q) {
        const u32 a0 = p.part_row[q] - pb[q], a1 = p.part_row[q + 1] - pb[q + 1];
        order_by_rows(c, b, p.seqs, tlist + pb[q], pb[q + 1] - pb[q], b.tl_sorted.p + pb[q], split ? c->d_small.p + SM_WIDE_PART + q : nullptr, nullptr);
        if (p.nspec) order_by_rows(c, b, p.seqs, alist + a0, a1 - a0, b.al_sorted.p + a0, nullptr, nullptr);
    }
    if (split) {
        u32* v = (u32*)small_host(c);
        HIP_CHECK(hipMemcpyAsync(v, c->d_small.p + SM_WIDE_PART, EMIT_PARTS_MAX * sizeof(u32), hipMemcpyDeviceToHost, c->st));
        HIP_CHECK(hipStreamSynchronize(c->st));
        for (int q = 0; q < p.parts; ++q) nwide[q] = v[q];
    }
}

// second aligner pass, with traces + traceback, over the rows that are reported (a few percent of the alignments); the rows of emission
// range q are written (k_emit_hits) and sent to the host while range q + 1 is traced
static void trace_pass(so_ctx* c, Batch& b, P2& p, HitBuf& out) {
    const u32 nq = p.nq, NO = p.NO, nspec = p.nspec;
    const int parts = p.parts;
    b.sel_idx.ensure((size_t)NO + 4);
    launch_selected_idx(b.toff.p, b.sel.p, b.nout.p, b.ooff.p, nq, b.sel_idx.p, c->st);
    u32 maxpart = 0;
    for (int q = 0; q < parts; ++q) maxpart = std::max(maxpart, p.part_row[q + 1] - p.part_row[q]);
    b.outrec.ensure(12 * (size_t)NO + 16);
    if (c->rows_in_flight) {  // the previous batch's rows may still be on their way out of b.outrec
        HIP_CHECK(hipStreamWaitEvent(c->st, c->ev_rows_done, 0));
        c->rows_in_flight = false;
    }
    if (!c->dev_out) {
        emit_join(c, out);  // the previous batch's job reads the staging buffer and writes into `out`
        // pinned staging buffer: pageable D2H runs at ~1 GB/s, pinned at PCIe speed
        if (c->pinned_cap < (size_t)NO * sizeof(HostRow)) {
            if (c->pinned) (void)hipHostFree(c->pinned);
            c->pinned_cap = (size_t)NO * sizeof(HostRow) * 5 / 4 + 4096;
            HIP_CHECK(hipHostMalloc(&c->pinned, c->pinned_cap, hipHostMallocDefault));
        }
    }
    const u32* slist = b.sel_idx.p;  // (ordering this pass by rows too costs more than it saves: 9.1 -> 9.9 ms on config 3)
    // Alignments asked for (so_search_loaded_aln): every reported row gets a slot for the columns its walk can take, in row order, and
    // the walks of this pass write them there (k_traceback<true>); the slots' offsets go to the walks per task, whatever list walks it.
    // CIGARs asked for (so_search_loaded_cigar): the same slots and walks; the runs are coded from the slots behind the last range.
    const bool emit_cols = p.aln_on || p.cig_on;
    if (emit_cols) aln_slots(c, b.aln, b.tasks.p, slist, NO, p.NT, p.seqs);
    u32* acode = emit_cols ? b.aln.code.p : nullptr;
    const u32* aofs = emit_cols ? b.aln.aofs.p : nullptr;
    // the list aligned with traces now: the rows without a kept trace (nspec), or all rows -- range q's are its [pb[q], pb[q + 1]); its
    // traces take their own sizes (b.tr_ofs) when the whole list fits the budget, else slabs of the batch-wide stride
    std::array<u32, EMIT_PARTS_MAX + 1> pb = p.part_row;
    if (nspec) split_kept_traces(c, b, p, pb.data());
    const u32* tlist = nspec ? b.sel_b.p : slist;
    const u32 tn = pb[parts];
    const u32* alist = b.sel_a.p;   // (nspec) rows that only need the walk
    // On a batch of mixed lengths the lists are ordered by band rows inside each emission range: k_align runs four alignments per
    // wave and k_traceback sixty-four walks, and either lasts as long as its longest (on uniform lengths the sort costs more than
    // it saves -- config 3: 9.1 -> 9.9 ms -- hence the test).  The traces' offsets follow the ordered list.
    const bool order_rows = b.permuted || (u64)b.maxqlen * b.nq > 3ull * b.h_off[b.nq] / 2;
    // tasks of emission range q's traced list that need the 32-bit cells (they lead the ordered range); a mixed batch whose lists are
    // not ordered keeps the 32-bit kernel for all of them
    u32 nwide_part[EMIT_PARTS_MAX] = {0};
    if (order_rows) {
        order_trace_lists(c, b, p, tlist, tn, alist, pb.data(), nwide_part);
        tlist = b.tl_sorted.p;
        if (nspec) alist = b.al_sorted.p;
    }
    const size_t tw = tn ? trace_offsets(c, b, p, tlist, tn) : 0;
    const bool tvar = tw <= p.var_budget_words;
    if (!tvar && tune().debug) fprintf(stderr, "[sohit] trace slabs: %u rows of %u per range at most, %u tasks per slab\n", tn, maxpart, p.slab);
    b.trace.ensure(tvar ? tw + 64 : (size_t)std::min(p.slab, std::max<u32>(maxpart, 1)) * p.stride + 64);
    // The rows without a kept trace are aligned in ONE launch in front of the ranges when none of them needs the 32-bit kernel (uniform
    // sets): a range's share (config 3: 87 k tasks = 1.3 fillings of the chip) left half a filling idle -- 0.35 + 1.0 ms in two launches,
    // 0.7 in one; the ranges then only walk their kept traces (config 3, interleaved runs: 47.49 against 47.61 ms -- the second range's
    // kept-trace walk now runs beside the first range's row download and pays for it).
    // (only behind kept traces: without them this list is every reported row, and its ranges' downloads overlap the later ranges' alignments)
    const bool hoist = nspec && tvar && p.traced_pk && !p.pk_mixed && parts > 1 && tn > 0;
    if (hoist) {
        // ... and walked at once, while their traces are in the L2 (walked range by range, the second range's came back from the Infinity
        // Cache behind the first range's 0.9 GB of kept traces: 0.94 instead of 0.27 ms)
        ProfTimer pt(c, &c->cnt.align_ms, &c->cnt.align_launches);
        launch_align_walk(b.tasks.p, tlist, tn, p.seqs, b.trace.p, p.TU, b.tr_ofs.p, b.ares.p, c->st, 0u, acode, aofs);
        pt.stop();
    }
    for (int q = 0; q < parts; ++q) {
        const u32 r0 = p.part_row[q], r1 = p.part_row[q + 1];
        const u32 qa = parts > 1 ? std::min<u32>(nq, (u32)q * p.qstep) : 0u, qb = parts > 1 ? std::min<u32>(nq, (u32)(q + 1) * p.qstep) : nq;
        if (r1 > r0) {
            // the range's traced positions [t0, t1) and, with kept traces, its walk-only positions [a0, a1)
            const u32 t0 = pb[q], t1 = pb[q + 1], a0 = r0 - t0, a1 = r1 - t1;
            // the range's leading tasks that take the 32-bit kernel
            const u32 nw = !p.traced_pk ? t1 - t0 : (order_rows ? std::min(nwide_part[q], t1 - t0) : (p.pk_mixed ? t1 - t0 : 0u));
            ProfTimer pt(c, &c->cnt.align_ms, &c->cnt.align_launches);
            if (!hoist && tvar)
                launch_align_walk(b.tasks.p, tlist + t0, t1 - t0, p.seqs, b.trace.p, p.TU, b.tr_ofs.p + t0, b.ares.p, c->st, nw, acode, aofs);
            else if (!hoist)   // (slabs of the batch-wide stride)
                for (u32 t = t0; t < t1; t += p.slab) {
                    const u32 n = std::min(p.slab, t1 - t);
                    launch_align_walk(b.tasks.p, tlist + t, n, p.seqs, b.trace.p, p.stride, nullptr, b.ares.p, c->st, std::min(n, nw > t - t0 ? nw - (t - t0) : 0u),
                                      acode, aofs);
                }
            if (nspec) launch_traceback(b.tasks.p, alist + a0, a1 - a0, p.seqs, b.spec_trace.p, p.TU, b.tpos.p, nullptr, b.ares.p, c->st, acode, aofs);
            pt.stop();
        }
        launch_emit_hits(b.tasks.p, b.ares.p, b.toff.p, b.sel.p, b.nout.p, b.ooff.p, b.bits.p, qa, qb, b.outrec.p, c->st);
        if (!c->dev_out && r1 > r0) {
            // the range's rows are downloaded on a second stream, behind the kernel that wrote them
            HIP_CHECK(hipEventRecord(c->ev_rows, c->st));
            HIP_CHECK(hipStreamWaitEvent(c->st_rows, c->ev_rows, 0));
            HIP_CHECK(hipMemcpyAsync((char*)c->pinned + (size_t)r0 * sizeof(HostRow), b.outrec.p + 12 * (size_t)r0, (size_t)(r1 - r0) * sizeof(HostRow),
                                     hipMemcpyDeviceToHost, c->st_rows));
            HIP_CHECK(hipEventRecord(c->ev_part[q], c->st_rows));
        }
    }
    // the rows' columns compacted in row order and sent to the host with the batch's query residues (as the walks read them: masked)
    if (p.aln_on) {
        const size_t aln_words = p.aln_words = aln_compact(c, b.aln, slist, NO, b.ares.p);
        const size_t qbytes = b.h_off[nq], need = aln_words * 4 + qbytes + 64;
        if (c->pinned_aln_cap < need) {   // (the previous batch's worker, which reads it, was joined above)
            if (c->pinned_aln) (void)hipHostFree(c->pinned_aln);
            c->pinned_aln = nullptr, c->pinned_aln_cap = 0;
            HIP_CHECK(hipHostMalloc(&c->pinned_aln, need * 5 / 4 + 4096, hipHostMallocDefault));
            c->pinned_aln_cap = need * 5 / 4 + 4096;
        }
        if (aln_words) HIP_CHECK(hipMemcpyAsync(c->pinned_aln, b.aln.comp.p, aln_words * 4, hipMemcpyDeviceToHost, c->st));
        if (qbytes) HIP_CHECK(hipMemcpyAsync((char*)c->pinned_aln + aln_words * 4, b.dev.d_res.p, qbytes, hipMemcpyDeviceToHost, c->st));
        HIP_CHECK(hipEventRecord(c->ev_aln, c->st));
    }
    // (CIGARs) runs per row from the slots, scanned, every run written once in row order: the offsets and the runs leave in one piece each
    if (p.cig_on) {
        const size_t n_ops = p.cig_ops = cigar_code(c, b.aln, slist, NO, b.ares.p);
        const size_t need = ((size_t)NO + 1 + n_ops) * sizeof(u32) + 64;
        if (c->pinned_aln_cap < need) {   // (the previous batch's worker, which reads it, was joined above)
            if (c->pinned_aln) (void)hipHostFree(c->pinned_aln);
            c->pinned_aln = nullptr, c->pinned_aln_cap = 0;
            HIP_CHECK(hipHostMalloc(&c->pinned_aln, need * 5 / 4 + 4096, hipHostMallocDefault));
            c->pinned_aln_cap = need * 5 / 4 + 4096;
        }
        HIP_CHECK(hipMemcpyAsync(c->pinned_aln, b.aln.oofs.p, ((size_t)NO + 1) * sizeof(u32), hipMemcpyDeviceToHost, c->st));
        if (n_ops) HIP_CHECK(hipMemcpyAsync((u32*)c->pinned_aln + NO + 1, b.aln.ops.p, n_ops * sizeof(u32), hipMemcpyDeviceToHost, c->st));
        HIP_CHECK(hipEventRecord(c->ev_aln, c->st));
    }
    p.sc.lap("phase2.trace_pass");
    {   // SOHIT_TEST_OOM_PHASE2=1 (tests): the first multi-query batch of the process fails here, as a device allocation of the
        // emission stage would -- search_loaded() reruns it as two halves
        static bool fired = false;
        if (!fired && nq > 1 && tune().test_oom_phase2) {
            fired = true;
            throw DevOom(0);
        }
    }
}

// device-resident results: the so_hit records are built in HBM and appended to the ctx's result buffer
static void emit_device(so_ctx* c, Batch& b, P2& p) {
    const u32 nq = p.nq, NO = p.NO;
    if (!c->d_p2tab.p) {
        c->d_p2tab.ensure(P2TAB_N);
        HIP_CHECK(hipMemcpy(c->d_p2tab.p, pow2_table(), P2TAB_N * sizeof(double), hipMemcpyHostToDevice));
    }
    c->d_hits.ensure((c->d_hits_n + NO) * sizeof(so_hit) + 256, true, c->st);
    const u32 *d_qid = nullptr, *d_ostart = nullptr;
    if (b.permuted) {   // records in file order: row counts scattered to file order, scanned
        b.d_ocnt.ensure((size_t)nq + 4), b.d_ostart.ensure((size_t)nq + 4);
        launch_scatter_u32(b.nout.p, b.d_qid.p, nq, b.d_ocnt.p, c->st);
        HIP_CHECK(hipMemsetAsync(b.d_ocnt.p + nq, 0, sizeof(u32), c->st));
        scan_u32(b.d_ocnt.p, b.d_ostart.p, (size_t)nq + 1, false, c->d_scan_tmp.p, c->st);
        d_qid = b.d_qid.p, d_ostart = b.d_ostart.p;
    }
    launch_make_hits(b.outrec.p, NO, b.q_lo, d_qid, b.ooff.p, d_ostart, c->qry.d_off.p, c->ref.d_off.p, c->ref.N, c->d_p2tab.p, P2TAB_N,
                     c->d_hits.p + c->d_hits_n * sizeof(so_hit), c->st);
    c->d_hits_n += NO;
    p.sc.lap("phase2.emit_device");
}

// host rows: a worker thread converts the downloaded rows into `out` (and rebuilds their strings) while the next batch runs
static void emit_host(so_ctx* c, Batch& b, P2& p, HitBuf& out) {
    const u32 nq = p.nq, NO = p.NO;
    const HostRow* rows = (const HostRow*)c->pinned;
    // the worker below waits for the last range's copy, the main thread goes on to the next batch (whose row kernel in turn waits
    // for that copy before it overwrites the device rows)
    HIP_CHECK(hipEventRecord(c->ev_rows_done, c->st_rows));
    c->rows_in_flight = true;
    if (c->profile) HIP_CHECK(hipEventSynchronize(c->ev_rows_done));
    p.sc.lap("phase2.emit_d2h");
    const size_t base = out.n;
    out.grow(NO);
    so_hit* dst = out.p + base;
    out.n = base + NO;
    // A batch that holds its queries in length-class order hands the rows over in that order; they are written in FILE order:
    // slot s's rows, [ooff[s], ooff[s + 1]) of the download, start at row ostart[qid[s]] -- place[s] = {query, destination - source}.
    std::shared_ptr<std::vector<std::pair<u32, i64>>> place;
    if (b.permuted) {
        const std::vector<u32>& ooff = p.h_ooff;
        std::vector<u32> ocnt((size_t)nq + 1, 0);
        for (u32 s = 0; s < nq; ++s) ocnt[b.qid[s]] = ooff[s + 1] - ooff[s];
        u32 run = 0;
        for (u32 o = 0; o < nq; ++o) {
            const u32 n = ocnt[o];
            ocnt[o] = run;
            run += n;
        }
        place = std::make_shared<std::vector<std::pair<u32, i64>>>(nq);
        for (u32 s = 0; s < nq; ++s) (*place)[s] = {b.qid[s], (i64)ocnt[b.qid[s]] - (i64)ooff[s]};
    }
    c->emit.base = base, c->emit.n = NO, c->emit.aln = p.aln_on, c->emit.cig = p.cig_on;
    if (p.cig_on) out.cig.rows(base + NO);   // (the worker fills the batch's offsets and appends its runs)
    c->emit.dropped.store(0);
    c->emit.active = true;
    // The worker converts range q's rows as soon as they have arrived, while the GPU traces range q + 1: behind the last copy only
    // the last range is left (it used to wait for ALL rows: ~1.3 ms of a config-3 step with the GPU idle).  Its threads are started
    // once and walk the ranges together.
    // (alignments) the strings are rebuilt behind the rows: the batch's query offsets travel with the job (the next batch overwrites b.h_off)
    std::shared_ptr<std::vector<u32>> aln_qoff;
    if (p.aln_on) aln_qoff = std::make_shared<std::vector<u32>>(b.h_off.begin(), b.h_off.begin() + nq + 1);
    c->emit.th = std::thread([c, rows, dst, NO, D = c->ref.N, expect = c->expect, q_lo = b.q_lo, p2p = pow2_table(), place, part_row = p.part_row, parts = p.parts, aln_qoff,
                              abuf = &out.aln, aln_words = p.aln_words, cbuf = p.cig_on ? &out.cig : nullptr, cig_ops = p.cig_ops, base] {
        try {
            HIP_CHECK(hipSetDevice(c->device));
            auto convert = [&](i64 i) {
                const int* v = rows[i].v;
                so_hit h;
                i64 di = i;
                if (place) {
                    const auto& pl = (*place)[(size_t)v[0]];
                    h.qidx = q_lo + pl.first;
                    di = i + pl.second;
                } else {
                    h.qidx = q_lo + v[0];
                }
                h.sidx = v[1];
                h.aln = v[2], h.mis = v[3], h.gap = v[4], h.qst = v[5], h.qed = v[6], h.sst = v[7], h.sed = v[8], h.bit = v[9];
                h.ungapped = v[10], h.matches = v[11];
                h.qlen = (int32_t)c->qry.len(h.qidx);
                h.slen = (int32_t)c->ref.len(h.sidx);
                // idy: one += 1. per identical column, then idy *= (100. / AL) (fsearch.py:1458-1459, 1471)
                h.identity = (double)h.matches * (100. / (double)h.aln);
                // bit2e (1086): D * len(sqi) * len(sqj) * pow(2, -bit)
                const double pw = (h.bit >= 0 && h.bit < P2TAB_N) ? p2p[h.bit] : p_pow(2, (double)(-h.bit));
                h.evalue = (double)(D * (i64)h.qlen * (i64)h.slen) * pw;
                if (!(h.evalue <= expect)) c->emit.dropped.fetch_add(1);
                dst[di] = h;
            };
            const unsigned nt = NO < 200000 ? 1u : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
            std::array<std::atomic<i64>, EMIT_PARTS_MAX> next;
            for (auto& n : next) n.store(0);
            std::exception_ptr werr;
            std::mutex wmu;
            auto worker = [&] {
                try {
                    HIP_CHECK(hipSetDevice(c->device));
                    for (int q = 0; q < parts; ++q) {
                        const i64 lo = part_row[(size_t)q], n = (i64)part_row[(size_t)q + 1] - lo;
                        if (n <= 0) continue;
                        HIP_CHECK(hipEventSynchronize(c->ev_part[q]));   // the range's rows have arrived in the pinned buffer
                        for (;;) {
                            const i64 b0 = next[(size_t)q].fetch_add(4096);
                            if (b0 >= n) break;
                            for (i64 i = b0; i < std::min(n, b0 + 4096); ++i) convert(lo + i);
                        }
                    }
                } catch (...) {
                    std::lock_guard<std::mutex> g(wmu);
                    werr = std::current_exception();
                }
            };
            std::vector<std::thread> th;
            for (unsigned t = 1; t < nt; ++t) th.emplace_back(worker);
            worker();
            for (auto& t : th) t.join();
            if (werr) std::rethrow_exception(werr);
            if (aln_qoff) {
                // row k of the result (file order) takes 2 aln_k bytes at the running sum; row i of the download has its columns at the
                // running sum of ceil(aln / 16) words in download order, in walk order (last column first)
                HIP_CHECK(hipEventSynchronize(c->ev_aln));
                const u32* codes = (const u32*)c->pinned_aln;
                const u8* qres = (const u8*)c->pinned_aln + aln_words * 4;
                const std::vector<size_t> woff = aln_word_offsets((size_t)NO, [&](size_t i) { return rows[i].v[2]; }, aln_words, "alignments");
                std::vector<i64> boff((size_t)NO + 1, 0);
                for (i64 k = 0; k < (i64)NO; ++k) boff[k + 1] = boff[k] + 2 * (i64)std::max(0, dst[k].aln);
                const size_t a0 = abuf->n;
                abuf->grow((size_t)boff[NO]);
                char* ab = abuf->p + a0;
                const u8* rres = c->ref.res.data();
                const std::vector<u32>& roff = c->ref.off;
                const std::vector<u32>& qoff = *aln_qoff;
                parallel_for((i64)NO, [&](i64 i) {
                    const int* v = rows[i].v;
                    const i64 di = place ? i + (*place)[(size_t)v[0]].second : i;
                    const int AL = std::max(0, v[2]);
                    if (!AL) return;
                    char* sq = ab + boff[di];
                    aln_decode(codes + woff[i], AL, qres + qoff[(size_t)v[0]] + (v[5] - 1), rres + roff[(size_t)v[1]] + (v[7] - 1), sq, sq + AL);
                });
                abuf->n = a0 + (size_t)boff[NO];
            }
            if (cbuf) {
                // row i of the download has its runs at [roff[i], roff[i + 1]) of the downloaded runs; row k of the result (file order) takes
                // them at the running sum of the rows' run counts
                HIP_CHECK(hipEventSynchronize(c->ev_aln));
                const u32* roff = (const u32*)c->pinned_aln;
                const u32* rops = roff + NO + 1;
                if (roff[NO] != cig_ops) throw SoError("CIGARs: the runs do not add up");
                const size_t g0 = cbuf->n;
                cbuf->grow(cig_ops);
                int64_t* goff = cbuf->off + base;
                goff[0] = (int64_t)g0;
                if (!place) {
                    parallel_for((i64)NO, [&](i64 i) { goff[i + 1] = (int64_t)g0 + roff[i + 1]; });
                } else {
                    for (i64 i = 0; i < (i64)NO; ++i) goff[i + (*place)[(size_t)rows[i].v[0]].second + 1] = roff[i + 1] - roff[i];
                    for (i64 k = 0; k < (i64)NO; ++k) goff[k + 1] += goff[k];
                }
                // (row by row on all threads: a config-3 result is 118 MB of runs)
                parallel_for((i64)NO, [&](i64 i) {
                    const i64 di = place ? i + (*place)[(size_t)rows[i].v[0]].second : i;
                    if (roff[i + 1] > roff[i]) memcpy(cbuf->ops + goff[di], rops + roff[i], (size_t)(roff[i + 1] - roff[i]) * sizeof(u32));
                });
                cbuf->n = g0 + cig_ops;
            }
        } catch (...) {
            c->emit.err = std::current_exception();
        }
    });
}

void phase2(so_ctx* c, Batch& b, HitBuf& out) {
    P2 p(c, b);
    if (p.nq == 0) return;
    if (gather_candidates(c, b, p)) {
        make_tasks(c, b, p);
        align_rounds(c, b, p);
        select_rows(c, b, p);
        if (p.NO) trace_pass(c, b, p, out);
        if (p.NO && c->dev_out) {
            emit_device(c, b, p);
        } else {
            if (p.NO) emit_host(c, b, p, out);
            p.sc.lap("phase2.emit_host");
        }
    }
    c->cnt.phase2_ms += (wall() - p.t0) * 1e3;
}

// so_align_pairs (tests): explicit windows through ONE aligner of phase 2, by the product's own launch functions on the product's device arrays.
// The raw loaded queries are the batch (upload_set, as for a batch masked on the host): a task's q is its query ordinal.  Every task the
// search would never hand the chosen kernel is refused before anything runs, so a refused call writes nothing.
// aln (so_align_pairs_aln): kernels 3 and 4 only; the walks write their columns through the search's own chain -- aln_slots, the emitting
// walk, aln_compact -- and the compacted columns are found by aln_word_offsets and decoded by aln_decode, as the emission worker does;
// task t's strings land at 2 * sum_{m<t} aln_m of *aln.
// cig (so_align_pairs_cigar): the same slots and walks, then the search's cigar_code; task t's runs land at cig->off[t] .. cig->off[t + 1].
void align_pairs(so_ctx* c, int kernel, i64 n, const int64_t* task6, const uint32_t* order, int32_t* out, AlnBytes* aln, CigarBuf* cig) {
    if (!c->ref_loaded || !c->qry_loaded) throw SoError("so_align_pairs: load a reference and queries first");
    if (kernel < 0 || kernel > 4) throw SoError("so_align_pairs: kernel must be 0 ... 4");
    if (aln && kernel < 3) throw SoError("so_align_pairs_aln: only the traced kernels (3, 4) give alignments");
    if (cig && kernel < 3) throw SoError("so_align_pairs_cigar: only the traced kernels (3, 4) give alignments");
    if (cig) cig->rows((size_t)std::max<i64>(n, 0)), std::fill(cig->off, cig->off + std::max<i64>(n, 0) + 1, (int64_t)0);
    if (n < 0 || n > (1ll << 24)) throw SoError("so_align_pairs: n must be 0 ... 2^24");
    if (n == 0) return;
    if (!task6 || !out) throw SoError("so_align_pairs: task6 or out is NULL");
    const SeqSet& Q = c->qry;
    const SeqSet& R = c->ref;
    const bool packed = kernel == 1 || kernel == 2 || kernel == 4, traced = kernel >= 3;
    std::vector<AlnTask> tk((size_t)n);
    for (i64 t = 0; t < n; ++t) {
        const int64_t* v = task6 + 6 * t;
        auto refuse = [&](const std::string& why) { throw SoError("so_align_pairs: task " + std::to_string(t) + ": " + why); };
        if (v[0] < 0 || v[0] >= Q.N) refuse("query index out of range");
        if (v[1] < 0 || v[1] >= R.N) refuse("subject index out of range");
        const i64 lq = Q.len(v[0]), ls = R.len(v[1]);
        const i64 qe = v[4] == -1 ? lq : v[4], se = v[5] == -1 ? ls : v[5];
        if (v[2] < 0 || v[2] > qe || qe > lq) refuse("query window out of range");
        if (v[3] < 0 || v[3] > se || se > ls) refuse("subject window out of range");
        // (a pair with a sequence of 4096+ residues is aligned in kswat_st_long tiles of at most 4096 x 4096)
        if (qe - v[2] > LONG_SEQ || se - v[3] > LONG_SEQ) refuse("window longer than 4096 residues");
        if (kernel == 2 && (qe != lq || se != ls)) refuse("k_align_lane takes no tile: both windows must end where their sequences end");
        if (kernel == 2 && (lq >= LONG_SEQ || ls >= LONG_SEQ)) refuse("k_align_lane takes no sequence of 4096 residues or more");
        tk[(size_t)t] = AlnTask{(u32)v[0], (u32)v[1], (u32)v[2], (u32)v[3], 0u, 0u, (u32)qe, (u32)se};
    }
    std::vector<u32> list((size_t)n);
    std::vector<char> listed((size_t)n, 0);
    for (i64 p = 0; p < n; ++p) {
        const u32 s = order ? order[p] : (u32)p;
        if ((i64)s >= n) throw SoError("so_align_pairs: order[" + std::to_string(p) + "] out of range");
        // (k_traceback reads the maximum's cell the aligner parked in the task's result: a task walked twice would read the other walk's result)
        if (traced && listed[s]) throw SoError("so_align_pairs: a traced launch list holds every task once");
        listed[s] = 1, list[(size_t)p] = s;
    }
    if (packed && !(tune().align_pk && align_pk_supported(c->st))) throw SoError("so_align_pairs: the packed aligners are switched off or not supported here");
    SeqSet qs;
    upload_set(c, qs, Q.res.data(), Q.off, (u32)Q.N);
    const AlnSeqs seqs{aln_side(qs), aln_side(R), c->d_b62c.p};
    DevBuf<AlnTask> d_tasks;
    DevBuf<u32> d_list, d_cnt;
    DevBuf<u64> d_keys;
    DevBuf<AlnRes> d_res;
    d_tasks.ensure((size_t)n + 4), d_list.ensure((size_t)n + 4), d_cnt.ensure(4), d_keys.ensure((size_t)n + 4), d_res.ensure((size_t)n + 4);
    HIP_CHECK(hipMemcpyAsync(d_tasks.p, tk.data(), (size_t)n * sizeof(AlnTask), hipMemcpyHostToDevice, c->st));
    HIP_CHECK(hipMemcpyAsync(d_list.p, list.data(), (size_t)n * sizeof(u32), hipMemcpyHostToDevice, c->st));
    HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, 4 * sizeof(u32), c->st));
    // the split of a score-only round: bit 13 of the key clear = the task needs the 32-bit cells
    launch_task_rows(d_tasks.p, d_list.p, (u32)n, seqs, d_cnt.p, nullptr, d_keys.p, c->st);
    std::vector<u64> keys((size_t)n);
    HIP_CHECK(hipMemcpyAsync(keys.data(), d_keys.p, (size_t)n * sizeof(u64), hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    std::vector<char> wide((size_t)n, 0);
    for (i64 p = 0; p < n; ++p) wide[list[(size_t)p]] = (keys[(size_t)p] & 8192u) ? 0 : 1;
    if (packed)
        for (i64 t = 0; t < n; ++t)
            if (listed[(size_t)t] && wide[(size_t)t])
                throw SoError("so_align_pairs: task " + std::to_string(t) + ": its scores need 32-bit cells, the packed aligners do not take it");
    DevBuf<u32> d_units, d_tofs, d_trace;
    AlnChain chain;   // (aln)
    std::vector<u32> h_acomp, h_oofs, h_ops;
    size_t aln_words = 0;
    switch (kernel) {
    case 0:
        launch_align(d_tasks.p, d_list.p, (u32)n, seqs, d_res.p, c->st);
        break;
    case 1:
        launch_align_pk(d_tasks.p, d_list.p, (u32)n, seqs, d_res.p, c->st);
        break;
    case 2:
        launch_align_lane(d_tasks.p, d_list.p, (u32)n, seqs, d_res.p, d_cnt.p + 1, c->ncu, c->st);
        break;
    default: {
        // variable trace offsets, as the final emission lays them out: trace room per task (k_trace_units), scanned
        const u32 TU = align_trace_unit();
        d_units.ensure((size_t)n + 4), d_tofs.ensure((size_t)n + 4);
        c->d_scan_tmp.ensure(scan_u32_temp_elems((size_t)n + 1) + 8);
        launch_trace_units(d_tasks.p, d_list.p, (u32)n, seqs, d_units.p, c->st);
        const size_t tw = (size_t)d2h_u32(c, scan_u32(d_units.p, d_tofs.p, (size_t)n + 1, false, c->d_scan_tmp.p, c->st)) * TU;
        d_trace.ensure(tw + 64);
        if (aln || cig) aln_slots(c, chain, d_tasks.p, d_list.p, (u32)n, (u32)n, seqs);
        // kernel 3: every task by the 32-bit kernel; 4: every task by the packed one
        launch_align_walk(d_tasks.p, d_list.p, (u32)n, seqs, d_trace.p, TU, d_tofs.p, d_res.p, c->st, kernel == 3 ? (u32)n : 0u, aln || cig ? chain.code.p : nullptr,
                          aln || cig ? chain.aofs.p : nullptr);
        if (cig) {   // the runs coded in list order and downloaded with their offsets
            const size_t n_ops = cigar_code(c, chain, d_list.p, (u32)n, d_res.p);
            h_oofs.resize((size_t)n + 1), h_ops.resize(n_ops + 1);
            HIP_CHECK(hipMemcpyAsync(h_oofs.data(), chain.oofs.p, ((size_t)n + 1) * sizeof(u32), hipMemcpyDeviceToHost, c->st));
            if (n_ops) HIP_CHECK(hipMemcpyAsync(h_ops.data(), chain.ops.p, n_ops * sizeof(u32), hipMemcpyDeviceToHost, c->st));
        }
        if (aln) {   // the columns compacted in list order and downloaded
            aln_words = aln_compact(c, chain, d_list.p, (u32)n, d_res.p);
            h_acomp.resize(aln_words + 1);
            if (aln_words) HIP_CHECK(hipMemcpyAsync(h_acomp.data(), chain.comp.p, aln_words * sizeof(u32), hipMemcpyDeviceToHost, c->st));
        }
        break;
    }
    }
    std::vector<AlnRes> res((size_t)n);
    HIP_CHECK(hipMemcpyAsync(res.data(), d_res.p, (size_t)n * sizeof(AlnRes), hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    if (aln) {
        // list position p's columns at the running sum of ceil(aln / 16) words in list order; task t's strings at the running sum of 2 aln in task order
        const std::vector<size_t> woff = aln_word_offsets((size_t)n, [&](size_t p) { return res[list[p]].aln; }, aln_words, "so_align_pairs_aln");
        std::vector<size_t> boff((size_t)n + 1, 0);
        for (i64 t = 0; t < n; ++t) boff[(size_t)t + 1] = boff[(size_t)t] + 2 * (size_t)std::max(0, res[(size_t)t].aln);
        const size_t a0 = aln->n;
        aln->grow(boff[(size_t)n]);
        for (i64 p = 0; p < n; ++p) {
            const u32 t = list[(size_t)p];
            const AlnRes& r = res[t];
            if (r.aln <= 0) continue;
            const u32* w = h_acomp.data() + woff[(size_t)p];
            int nq_adv = 0, ns_adv = 0;   // (the columns must cover the coordinates before anything is read through them)
            for (int cc = 0; cc < r.aln; ++cc) {
                const u32 code = (w[cc >> 4] >> ((cc & 15) << 1)) & 3u;
                nq_adv += code != 2, ns_adv += code != 3;
            }
            if (r.qst < 0 || r.sst < 0 || nq_adv != r.qed - r.qst || ns_adv != r.sed - r.sst || r.qed > (int)Q.len(tk[t].q) || r.sed > (int)R.len(tk[t].subj))
                throw SoError("so_align_pairs_aln: task " + std::to_string(t) + ": the columns do not cover its coordinates");
            char* sq = aln->p + a0 + boff[t];
            aln_decode(w, r.aln, Q.res.data() + Q.off[tk[t].q] + r.qst, R.res.data() + R.off[tk[t].subj] + r.sst, sq, sq + r.aln);
        }
        aln->n = a0 + boff[(size_t)n];
    }
    if (cig) {
        // list position p's runs at h_oofs[p]; task t's at the running sum of the tasks' run counts
        for (i64 p = 0; p < n; ++p) cig->off[list[(size_t)p] + 1] = (int64_t)h_oofs[(size_t)p + 1] - (int64_t)h_oofs[(size_t)p];
        for (i64 t = 0; t < n; ++t) cig->off[t + 1] += cig->off[t];
        cig->grow((size_t)cig->off[n]);
        for (i64 p = 0; p < n; ++p) {
            const u32 t = list[(size_t)p];
            const AlnRes& r = res[t];
            const u32* w = h_ops.data() + h_oofs[(size_t)p];
            const i64 nr = cig->off[t + 1] - cig->off[t];
            i64 cols = 0, nq_adv = 0, ns_adv = 0;   // (the runs must cover the coordinates)
            for (i64 k = 0; k < nr; ++k) cols += w[k] >> 4, nq_adv += (w[k] & 15u) != 2u ? w[k] >> 4 : 0u, ns_adv += (w[k] & 15u) != 1u ? w[k] >> 4 : 0u;
            if (cols != std::max(0, r.aln) || (nr && (nq_adv != r.qed - r.qst || ns_adv != r.sed - r.sst)))
                throw SoError("so_align_pairs_cigar: task " + std::to_string(t) + ": the runs do not cover its coordinates");
            if (nr) memcpy(cig->ops + cig->off[t], w, (size_t)nr * sizeof(u32));
        }
        cig->n = (size_t)cig->off[n];
    }
    for (i64 t = 0; t < n; ++t) {
        int32_t* o = out + 10 * t;
        const AlnRes& r = res[(size_t)t];
        if (!listed[(size_t)t]) {   // (not in the launch list)
            for (int k = 0; k < 10; ++k) o[k] = -1;
            continue;
        }
        o[0] = r.maxscore, o[1] = r.aln, o[2] = r.matches, o[3] = r.gap, o[4] = r.qst, o[5] = r.qed, o[6] = r.sst, o[7] = r.sed, o[8] = r.cells;
        o[9] = wide[(size_t)t];
    }
}
