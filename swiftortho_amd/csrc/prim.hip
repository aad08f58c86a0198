// prim.hip -- a direct door to the shared device primitives (so_prim_*, include/sohit.h): the scans and the run / numbering helpers of
// k_util.hip and the library sorts of k_sort.hip / k_sortseg.hip, each reached through the very wrapper the stages call (kernels.h).
// For tests/test_gpu_prim.py: host arrays in, the wrapper on a stream of the call, everything it wrote out -- with the words around an
// output range, and the bytes behind a sort's scratch, set to a sentinel first and handed back, so that a write outside shows.
// No kernel lives here.
#include "device_call.h"
#include "sohit.h"

#include <cstring>

namespace {

std::string g_prim_err;

constexpr u32 PRIM_SENTINEL = 0xA5C3F00Du;   // the guard words (so_prim_scan, so_prim_effscan) and the unwritten words of `start`
constexpr int PRIM_GUARD = 4;                // guard words on each side of an output range
constexpr int PRIM_SORT_FILL = 0xD6;         // byte the sorts' outputs are filled with before the call
constexpr int PRIM_TEMP_FILL = 0x5A;         // ... and the PRIM_TEMP_GUARD bytes behind their scratch
constexpr size_t PRIM_TEMP_GUARD = 256;

template <class F>
int prim_call(F body) {
    return guarded_call(g_prim_err, (int*)nullptr, [](int*) {}, body);
}

void check_skew(const char* who, int skew) {
    if (skew < 0 || skew > 3) throw SoError(std::string(who) + ": a skew is 0 .. 3");
}

// n elements from the device into a host array of the caller (arrived after the call's next wait)
template <class T>
void download(DeviceCall& call, T* h, const T* d, size_t n) {
    if (n) call.fetch(h, d, n);
}

template <class T>
void to_device(T* d, const T* h, size_t n, hipStream_t st) {
    if (n) HIP_CHECK(hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, st));
}

// an output range of n words `skew` words off 16-byte alignment inside buf, PRIM_GUARD words free on either side
u32* skewed(DevBuf<u32>& buf, size_t n, int skew) {
    buf.ensure(n + 2 * PRIM_GUARD + 8);
    return buf.p + PRIM_GUARD + skew;   // (hipMalloc aligns to 256 bytes, PRIM_GUARD words are 16)
}

void fetch_guards(DeviceCall& call, u32* guards, const u32* range, size_t n) {
    download(call, guards, range - PRIM_GUARD, PRIM_GUARD);
    download(call, guards + PRIM_GUARD, range + n, PRIM_GUARD);
}

}  // namespace

extern "C" {

const char* so_prim_last_error(void) { return g_prim_err.c_str(); }

int32_t so_prim_scan_path(int64_t n, int64_t* tiles) {
    size_t nb = 0;
    const int path = scan_u32_path(n < 0 ? 0 : (size_t)n, &nb);
    if (tiles) *tiles = (int64_t)nb;
    return path;
}

int32_t so_prim_seg_variant(int32_t kind, int64_t n, int64_t nseg, int32_t width) {
    if (n < 0 || nseg < 0 || nseg > 0xFFFFFFFFll) return -1;
    if (kind == 3 || kind == 4) return seg_variant((size_t)n, (u32)nseg, width);
    if (kind == 5) return cand_keys_cfg((size_t)n, (u32)nseg);
    return kind == 6 ? 0 : -1;
}

int32_t so_prim_sort_tier(int32_t kind, int64_t n, int64_t* single_block, int64_t* merge_limit) {
    if (kind < 0 || kind > 2 || n < 0) return -1;
    size_t s = 0, m = 0;
    const int tier = sort_u64_tier((size_t)n, kind == 0 ? 0 : kind == 1 ? 4 : 8, &s, &m);
    if (single_block) *single_block = (int64_t)s;
    if (merge_limit) *merge_limit = (int64_t)m;
    return tier;
}

int so_prim_scan(int device, int64_t n, const uint32_t* in, int32_t in_skew, int32_t out_skew, int32_t inclusive, int32_t in_place, uint32_t* out,
                 uint32_t* guards, uint32_t* total, int32_t* path, int64_t* tiles) {
    return prim_call([&] {
        if (n < 0 || n >= (1ll << 31)) throw SoError("so_prim_scan: n is 0 .. 2^31 - 1");
        if (!guards || !total || !path || !tiles || (n > 0 && (!in || !out))) throw SoError("so_prim_scan: a null array");
        check_skew("so_prim_scan", in_skew), check_skew("so_prim_scan", out_skew);
        if (in_place && in_skew != out_skew) throw SoError("so_prim_scan: in place, the two skews are one");
        check_device("so_prim_scan", device);
        DeviceCall call(device);
        const size_t N = (size_t)n;
        DevBuf<u32> a, b, tmp;
        u32* d_in = skewed(a, N, in_skew);
        u32* d_out = in_place ? d_in : skewed(b, N, out_skew);
        DevBuf<u32>& ob = in_place ? a : b;
        fill_u32(ob.p, N + 2 * PRIM_GUARD + 8, PRIM_SENTINEL, call.st);
        to_device(d_in, in, N, call.st);
        tmp.ensure(scan_u32_temp_elems(N));
        size_t nb = 0;
        *path = scan_u32_path(N, &nb), *tiles = (int64_t)nb;
        const u32* d_total = scan_u32(d_in, d_out, N, inclusive != 0, tmp.p, call.st);
        HIP_CHECK(hipGetLastError());
        download(call, out, d_out, N);
        fetch_guards(call, guards, d_out, N);
        call.fetch(total, d_total);
        call.wait();
    });
}

int so_prim_effscan(int device, int64_t n, const uint8_t* mark, int32_t mark_skew, const uint32_t* scnt, int32_t scnt_skew, uint32_t* hoff, uint32_t* cidx,
                    uint32_t* guards, uint32_t* totals, int64_t* tiles) {
    return prim_call([&] {
        if (n < 0 || n >= (1ll << 31)) throw SoError("so_prim_effscan: n is 0 .. 2^31 - 1");
        if (!guards || !totals || !tiles || (n > 0 && (!mark || !scnt || !hoff || !cidx))) throw SoError("so_prim_effscan: a null array");
        check_skew("so_prim_effscan", mark_skew), check_skew("so_prim_effscan", scnt_skew);
        check_device("so_prim_effscan", device);
        DeviceCall call(device);
        const size_t N = (size_t)n;
        DevBuf<u8> m;
        DevBuf<u32> s, h, c, tmp;
        m.ensure(N + 32);
        u8* d_mark = m.p + 16 + mark_skew;
        u32 *d_scnt = skewed(s, N, scnt_skew), *d_hoff = skewed(h, N, scnt_skew), *d_cidx = skewed(c, N, scnt_skew);
        fill_u32(h.p, N + 2 * PRIM_GUARD + 8, PRIM_SENTINEL, call.st);
        fill_u32(c.p, N + 2 * PRIM_GUARD + 8, PRIM_SENTINEL, call.st);
        to_device(d_mark, mark, N, call.st);
        to_device(d_scnt, scnt, N, call.st);
        tmp.ensure(effscan_temp_elems(N));   // (hipMalloc: 8-byte aligned)
        size_t nb = 0;
        (void)scan_u32_path(N, &nb);
        *tiles = (int64_t)nb;
        const u32* d_totals = effscan(d_mark, d_scnt, N, d_hoff, d_cidx, tmp.p, call.st);
        HIP_CHECK(hipGetLastError());
        download(call, hoff, d_hoff, N), download(call, cidx, d_cidx, N);
        fetch_guards(call, guards, d_hoff, N), fetch_guards(call, guards + 2 * PRIM_GUARD, d_cidx, N);
        call.fetch(totals, d_totals, 2);
        call.wait();
    });
}

int so_prim_runs(int device, int64_t n, int32_t key_bytes, const void* key, uint32_t* head, uint32_t* rid, uint32_t* start, int64_t* n_runs) {
    return prim_call([&] {
        if (n < 1 || n >= (1ll << 31)) throw SoError("so_prim_runs: n is 1 .. 2^31 - 1");
        if (key_bytes != 4 && key_bytes != 8) throw SoError("so_prim_runs: keys of 4 (int) or 8 (u64) bytes");
        if (!key || !head || !rid || !start || !n_runs) throw SoError("so_prim_runs: a null array");
        check_device("so_prim_runs", device);
        DeviceCall call(device);
        const u32 N = (u32)n;
        DevBuf<u8> k;
        DevBuf<u32> h, r, s, tmp;
        k.ensure((size_t)N * key_bytes), h.ensure(N), r.ensure(N), s.ensure((size_t)N + 2), tmp.ensure(scan_u32_temp_elems(N));
        to_device(k.p, (const u8*)key, (size_t)N * key_bytes, call.st);
        fill_u32(s.p, (size_t)N + 2, PRIM_SENTINEL, call.st);
        const u32* d_nruns = key_bytes == 4 ? key_runs(reinterpret_cast<const int*>(k.p), N, h.p, r.p, tmp.p, call.st)
                                            : key_runs(reinterpret_cast<const u64*>(k.p), N, h.p, r.p, tmp.p, call.st);
        run_starts(h.p, r.p, N, d_nruns, s.p, call.st);
        HIP_CHECK(hipGetLastError());
        u32 nruns = 0;
        call.fetch(&nruns, d_nruns);
        download(call, head, h.p, (size_t)N), download(call, rid, r.p, (size_t)N), download(call, start, s.p, (size_t)N + 2);
        call.wait();
        *n_runs = nruns;
    });
}

int so_prim_number(int device, int64_t nr, int64_t n_codes, const int32_t* cx, const int32_t* cy, int32_t* X, int32_t* Y, int32_t* gene_code, uint32_t* first,
                   uint32_t* flag, int64_t* n_genes) {
    return prim_call([&] {
        if (nr < 1 || nr >= (1ll << 30)) throw SoError("so_prim_number: nr is 1 .. 2^30 - 1");
        if (n_codes < 1 || n_codes >= (1ll << 31)) throw SoError("so_prim_number: n_codes is 1 .. 2^31 - 1");
        if (!cx || !cy || !X || !Y || !gene_code || !first || !flag || !n_genes) throw SoError("so_prim_number: a null array");
        for (int64_t i = 0; i < nr; ++i)
            if (cx[i] < 0 || cx[i] >= n_codes || cy[i] < 0 || cy[i] >= n_codes) throw SoError("so_prim_number: a code outside 0 .. n_codes - 1");
        check_device("so_prim_number", device);
        DeviceCall call(device);
        const size_t N = (size_t)nr, NC = (size_t)n_codes, G = std::min(NC, 2 * N);
        DevBuf<int> dx, dy, X_, Y_, gc;
        DevBuf<u32> fi, fl, rk, tmp;
        dx.ensure(N), dy.ensure(N), X_.ensure(N), Y_.ensure(N), gc.ensure(G), fi.ensure(NC), fl.ensure(2 * N), rk.ensure(2 * N), tmp.ensure(scan_u32_temp_elems(2 * N));
        to_device(dx.p, cx, N, call.st), to_device(dy.p, cy, N, call.st);
        HIP_CHECK(hipMemsetAsync(gc.p, 0xFF, G * sizeof(int), call.st));   // genes beyond the count: -1
        const u32* d_ng = number_by_first_appearance(dx.p, dy.p, (u32)N, (u32)NC, fi.p, fl.p, rk.p, tmp.p, X_.p, Y_.p, gc.p, call.st);
        HIP_CHECK(hipGetLastError());
        u32 ng = 0;
        call.fetch(&ng, d_ng);
        download(call, X, X_.p, N), download(call, Y, Y_.p, N), download(call, gene_code, gc.p, G);
        download(call, first, fi.p, NC), download(call, flag, fl.p, 2 * N);
        call.wait();
        *n_genes = ng;
    });
}

int so_prim_sort(int device, int32_t kind, int64_t n, const uint64_t* kin, const void* vin, int64_t nseg, const uint32_t* seg_begin, const uint32_t* seg_end,
                 int32_t begin_bit, int32_t end_bit, uint64_t* kout, void* vout, int64_t* info) {
    return prim_call([&] {
        const bool wrapper_only = (kind & 0x100) != 0;   // n >= 2^31 straight to the sort, which must refuse it as its *_temp_bytes does
        kind &= ~0x100;
        const bool seg = kind >= 3 && kind <= 6, pairs = kind == 1 || kind == 2;
        if (kind < 0 || kind > 6) throw SoError("so_prim_sort: kind is 0 .. 6");
        if (n < 0 || nseg < 0 || nseg >= (1ll << 31)) throw SoError("so_prim_sort: a count is negative, or 2^31 segments and more");
        if (begin_bit < 0 || end_bit > 64 || begin_bit >= end_bit) throw SoError("so_prim_sort: 0 <= begin_bit < end_bit <= 64");
        if (pairs && begin_bit != 0) throw SoError("so_prim_sort: the pair sorts take bits from 0");
        if (seg && nseg < 1) throw SoError("so_prim_sort: a segmented sort has a segment");
        if (!info) throw SoError("so_prim_sort: a null array");
        check_device("so_prim_sort", device);
        // the scratch size first: by the matching *_temp_bytes alone, before any array is read (it refuses what the sort refuses)
        const size_t N = (size_t)n;
        const u32 S = (u32)nseg;
        size_t tb = 0;
        if (wrapper_only) {
            if (n < (1ll << 31)) throw SoError("so_prim_sort: the wrapper alone is asked with 2^31 keys and more");
            // (no scratch, no arrays: a sort that did not refuse would only report a size)
            switch (kind) {
                case 0: sort_keys_u64(nullptr, tb, nullptr, nullptr, N, begin_bit, end_bit, nullptr); break;
                case 1: sort_pairs_u64_u32(nullptr, tb, nullptr, nullptr, nullptr, nullptr, N, end_bit, nullptr); break;
                case 2: sort_pairs_u64_u64(nullptr, tb, nullptr, nullptr, nullptr, nullptr, N, end_bit, nullptr); break;
                case 3: sort_keys_u64_seg(nullptr, tb, nullptr, nullptr, N, S, nullptr, begin_bit, end_bit, nullptr); break;
                case 4: sort_keys_u64_seg2(nullptr, tb, nullptr, nullptr, N, S, nullptr, nullptr, begin_bit, end_bit, nullptr); break;
                case 5: sort_cand_keys_seg(nullptr, tb, nullptr, nullptr, N, S, nullptr, begin_bit, end_bit, nullptr); break;
                default: sort_keys_u64_seg_desc(nullptr, tb, nullptr, nullptr, N, S, nullptr, begin_bit, end_bit, nullptr); break;
            }
            throw SoError("so_prim_sort: the sort did not refuse 2^31 keys and more");
        }
        switch (kind) {
            case 0: tb = sort_keys_u64_temp_bytes(N, end_bit); break;
            case 1: tb = sort_pairs_u64_u32_temp_bytes(N, end_bit); break;
            case 2: tb = sort_pairs_u64_u64_temp_bytes(N, end_bit); break;
            case 3: case 4: tb = sort_keys_u64_seg_temp_bytes(N, S, begin_bit, end_bit); break;
            case 5: tb = sort_cand_keys_seg_temp_bytes(N, S, begin_bit, end_bit); break;
            default: tb = sort_keys_u64_seg_desc_temp_bytes(N, S, begin_bit, end_bit); break;
        }
        info[0] = seg ? so_prim_seg_variant(kind, n, nseg, end_bit - begin_bit) : -1;
        info[1] = seg ? -1 : so_prim_sort_tier(kind, n, nullptr, nullptr);
        if (kind == 0 && info[1] == 1 && sort_keys_skips_merge(begin_bit, end_bit)) info[1] = 2;
        info[2] = (int64_t)tb, info[3] = 0;
        if (N && (!kin || !kout || (pairs && (!vin || !vout)))) throw SoError("so_prim_sort: a null array");
        const size_t nb = seg ? (kind == 4 ? S : (size_t)S + 1) : 0;   // words at seg_begin
        if (seg) {
            if (!seg_begin || (kind == 4 && !seg_end)) throw SoError("so_prim_sort: a null segment array");
            u64 prev = 0;
            for (size_t k = 0; k < nb; ++k) {
                if (seg_begin[k] < prev) throw SoError("so_prim_sort: the segments overlap or fall");
                prev = seg_begin[k];
                if (kind == 4) {
                    if (seg_end[k] < prev) throw SoError("so_prim_sort: a segment ends before it begins");
                    prev = seg_end[k];
                }
            }
            if (prev > N) throw SoError("so_prim_sort: a segment ends behind the keys");
        }
        DeviceCall call(device);
        const size_t vb = kind == 1 ? 4 : 8;
        DevBuf<u64> ki, ko;
        DevBuf<u8> vi, vo, tmp;
        DevBuf<u32> sb, se;
        ki.ensure(N + 2), ko.ensure(N + 2), tmp.ensure(tb + PRIM_TEMP_GUARD);
        to_device(ki.p, kin, N, call.st);
        HIP_CHECK(hipMemsetAsync(ko.p, PRIM_SORT_FILL, (N + 2) * sizeof(u64), call.st));
        HIP_CHECK(hipMemsetAsync(tmp.p + tb, PRIM_TEMP_FILL, PRIM_TEMP_GUARD, call.st));
        if (pairs) {
            vi.ensure(N * vb + 16), vo.ensure(N * vb + 16);
            to_device(vi.p, (const u8*)vin, N * vb, call.st);
            HIP_CHECK(hipMemsetAsync(vo.p, PRIM_SORT_FILL, N * vb + 16, call.st));
        }
        if (seg) {
            sb.ensure(nb + 2), to_device(sb.p, seg_begin, nb, call.st);
            if (kind == 4) se.ensure(nb + 2), to_device(se.p, seg_end, nb, call.st);
        }
        switch (kind) {
            case 0: sort_keys_u64(tmp.p, tb, ki.p, ko.p, N, begin_bit, end_bit, call.st); break;
            case 1: sort_pairs_u64_u32(tmp.p, tb, ki.p, ko.p, reinterpret_cast<const u32*>(vi.p), reinterpret_cast<u32*>(vo.p), N, end_bit, call.st); break;
            case 2: sort_pairs_u64_u64(tmp.p, tb, ki.p, ko.p, reinterpret_cast<const u64*>(vi.p), reinterpret_cast<u64*>(vo.p), N, end_bit, call.st); break;
            case 3: sort_keys_u64_seg(tmp.p, tb, ki.p, ko.p, N, S, sb.p, begin_bit, end_bit, call.st); break;
            case 4: sort_keys_u64_seg2(tmp.p, tb, ki.p, ko.p, N, S, sb.p, se.p, begin_bit, end_bit, call.st); break;
            case 5: sort_cand_keys_seg(tmp.p, tb, ki.p, ko.p, N, S, sb.p, begin_bit, end_bit, call.st); break;
            default: sort_keys_u64_seg_desc(tmp.p, tb, ki.p, ko.p, N, S, sb.p, begin_bit, end_bit, call.st); break;
        }
        HIP_CHECK(hipGetLastError());
        u8 guard[PRIM_TEMP_GUARD];
        download(call, kout, ko.p, N);
        if (pairs) download(call, (u8*)vout, vo.p, N * vb);
        download(call, guard, tmp.p + tb, PRIM_TEMP_GUARD);
        call.wait();
        for (size_t k = 0; k < PRIM_TEMP_GUARD; ++k) info[3] += guard[k] != PRIM_TEMP_FILL;
    });
}

}  // extern "C"
