// hit_table.h -- what the stages that work on hit tables (orth.hip, rbh.hip) share: rows of name codes (q, s) that come as host columns or
// as the so_hit records of a search, a taxon per name, and the error word the row kernels report through.
#pragma once
#include "device_call.h"
#include "../../include/sohit.h"

#include <string>

// the error word of a stage: bits 1 / 2 by hit_codes, 4 by the stage's row check (a name code outside [0, n_names)); higher bits are the stage's own
inline void hit_table_errors(const char* who, u32 err) {
    if (err & 1u) throw SoError(std::string(who) + ": a record's qidx lies outside the query map");
    if (err & 2u) throw SoError(std::string(who) + ": a record's sidx lies outside the subject map");
    if (err & 4u) throw SoError(std::string(who) + ": a name code lies outside 0 .. n_names - 1");
}

// What every entry point checks of the table's extents before anything touches the device; stage_limits() throws for what the stage
// itself cannot hold -- before the taxon of every name is read, so an n_names it refuses is never walked.
template <class Limits>
void hit_table_check(const char* who, i64 n, i64 n_names, const int32_t* tax, i64 n_taxa, Limits stage_limits) {
    if (n < 0 || n_names < 0 || n_taxa < 0 || (n_names > 0 && !tax)) throw SoError(std::string(who) + ": bad arguments");
    if (n >= (1ll << 31)) throw SoError(std::string(who) + ": 2^31 rows and more are not supported (32-bit row numbers)");
    stage_limits();
    for (i64 i = 0; i < n_names; ++i)
        if (tax[i] < 0 || tax[i] >= n_taxa) throw SoError(std::string(who) + ": name " + std::to_string(i) + " has a taxon outside 0 .. n_taxa - 1");
}

#ifdef __HIPCC__
// record -> the name codes of its query and subject through the maps; err |= 1 / 2: a qidx / sidx outside its map (the code is 0 then)
__device__ __forceinline__ void hit_codes(const so_hit& r, const int* __restrict__ qmap, i64 nq, const int* __restrict__ smap, i64 ns, int& qc, int& sc,
                                          u32* __restrict__ err) {
    qc = 0, sc = 0;
    if (r.qidx < 0 || r.qidx >= nq) atomicOr(err, 1u);
    else qc = qmap[r.qidx];
    if (r.sidx < 0 || r.sidx >= ns) atomicOr(err, 2u);
    else sc = smap[r.sidx];
}
#endif
