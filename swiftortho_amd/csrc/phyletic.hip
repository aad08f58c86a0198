// phyletic.hip -- phyletic profiles on the device: the pairs of gene families that are gained and lost together across the genomes, what
// swiftortho_amd/phyletic.py `linked_pairs()` defines.  From the (family row, taxon) pairs of the kept members (pan.py member_table):
//   * present[r] = the distinct taxa of row r; a row is ELIGIBLE iff r < n_file_rows and n_min <= present[r] <= n_max;
//   * two eligible rows a < b with taxon sets A, B: k = |A & B|, u = present[a] + present[b] - k; LINKED iff k >= k_min and
//     k * den >= num * u (num / den is the Jaccard threshold, equality passes);
//   * the linked pairs as (a, b, k), ordered by (a, b), a and b the rows' own numbers.
// The product is P P^T over the families, the transpose of so_pan_shared's: too large to store (4 * 10^10 cells at 200 000 families), so
// it is thresholded in the tile and only the sparse list leaves it.  Integers only: nothing depends on scheduling but the order inside
// the emit pass, which the sort on the (unique) keys removes.
//
// Kernels.  k_pan_rowbits (pan_bits.h): the row-major presence words, a pair outside the table flagged and written nowhere.  k_pp_present:
// a row per lane, present[] by popcount and the eligibility flag; scan_u32 over the flags.  k_pp_gather: the eligible profiles WORD-major,
// prof[w * Epad + e] (Epad = E rounded up to 64, the pad rows zero) -- the 64 rows of a tile side for one taxon word are 512 consecutive
// bytes --, with n_e[e] = present and el[e] = the row's own number, in row order.  k_pp_tile<EMIT>: a workgroup of 256 lanes per pair
// I <= J of tiles of 64 eligible rows, the lane layout and the LDS image of k_pan_shared (4 x 4 sums per lane, both sides staged as
// [word][row] in chunks of PP_CHUNK words).  The K dimension is short (at most 64 taxon words): a workgroup walks ALL words of its tile
// and holds the finished k of its 16 cells in registers -- no range split, no atomics into a matrix, no E x E array anywhere -- and
// applies the integer test per cell (a diagonal tile keeps x < y; a cell with x >= E or y >= E is never tested).  It runs twice: the
// count pass adds every workgroup's passing cells to one 64-bit total, from which the host sizes the output exactly; the emit pass
// reserves each workgroup's slots with one add to a global cursor (the lanes' places inside them from an LDS cursor) and writes
// (el[x] << 32 | el[y], k).  One sort_pairs_u64_u32 orders them; k_pp_unpack splits the keys.
// Tile index.  E is known on the device only until the count has come back, so neither pass is launched tile for tile: a fixed grid of
// workgroups (as many as the device holds at a time: the runtime's occupancy figure for the kernel, times the CUs) strides over the nt (nt + 1) / 2 tile pairs in row-major order, workgroup g
// taking pairs g, g + G, g + 2 G, ...  It keeps (I, J - I) and steps over the rows of tiles as they end: nt steps at most in a workgroup's
// WHOLE walk of tiles / G pairs, not per pair as k_pan_shared's walk from blockIdx.x would be (nt is 3125 at 200 000 families).  No block
// is launched for a pair below the diagonal or beyond the eligible rows, and both passes run the same grid.
// The test in 32 bits: k <= 4096 and u <= 4096 (rows hold no bit beyond taxon 4095), num <= den < 2^20, so k * den and num * u stay
// below 4096 * 2^20 = 2^32, and both factors of either product fit 24 bits (one v_mul_u32_u24 each).
// Two host waits (DeviceCall, device_call.h): the count, then the result.
#include "pan_bits.h"
#include "../../include/sohit.h"

#include <cstring>
#include <string>

namespace {

const u32 PP_TILE = 64u;
const u32 PP_MAX_TILES = 65535u;   // tiles a side: their pairs I <= J number below 2^31

// a row per lane: its distinct taxa and whether it takes part
__global__ __launch_bounds__(256) void k_pp_present(u32 R, u32 n_file, u32 TW, const ull* __restrict__ rowbits, int n_min, int n_max, int* __restrict__ present,
                                                    u32* __restrict__ flag) {
    const size_t r = tid256();
    if (r >= R) return;
    const ull* b = rowbits + r * TW;
    int n = 0;
    for (u32 w = 0; w < TW; ++w) n += __popcll(b[w]);
    present[r] = n;
    flag[r] = (r < n_file && n >= n_min && n <= n_max) ? 1u : 0u;
}

// eligible row r -> slot e = pos[r] of the compacted arrays (pos: the exclusive scan of flag, so the slots are in row order)
__global__ __launch_bounds__(256) void k_pp_gather(u32 R, u32 TW, const ull* __restrict__ rowbits, const int* __restrict__ present, const u32* __restrict__ flag,
                                                   const u32* __restrict__ pos, const u32* __restrict__ d_E, ull* __restrict__ prof, u32* __restrict__ n_e,
                                                   u32* __restrict__ el) {
    const size_t r = tid256();
    if (r >= R || !flag[r]) return;
    const u32 e = pos[r];   // < E
    const size_t Epad = ((size_t)*d_E + PP_TILE - 1u) / PP_TILE * PP_TILE;
    for (u32 w = 0; w < TW; ++w) prof[w * Epad + e] = rowbits[r * TW + w];
    n_e[e] = (u32)present[r], el[e] = (u32)r;
}

// Lane (ty, tx) of the 16 x 16 holds eligible rows x = I * 64 + ty * 4 + r against y = J * 64 + tx * 4 + c.  The LDS image is
// k_pan_shared's: a lane's four rows are 32 consecutive bytes, the 16 lanes of one ty read one address (a broadcast).  Every read of
// prof and n_e lies below Epad (I, J < nt), every read of el below E.  total[0]: the count pass's sum; total[1]: the emit pass's cursor;
// cap: the slots of key / val (the count pass's sum: no store lands beyond it).  Every lane of a workgroup walks the same pairs, so all
// of them meet every barrier.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_pp_tile(const ull* __restrict__ prof, const u32* __restrict__ n_e, const u32* __restrict__ el, const u32* __restrict__ d_E, u32 TW,
                                                 u32 k_min, u32 num, u32 den, ull* __restrict__ total, u64* __restrict__ key, u32* __restrict__ val, u32 cap) {
    __shared__ __attribute__((aligned(16))) ull sA[PP_CHUNK][PP_TILE];
    __shared__ __attribute__((aligned(16))) ull sB[PP_CHUNK][PP_TILE];
    __shared__ u32 s_n, s_base;
    const u32 E = *d_E;
    if (E < 2u || E > PP_TILE * PP_MAX_TILES) return;   // (the whole grid: no pair of rows, or more rows than a call serves -- the host refuses them)
    const u32 nt = (E + PP_TILE - 1u) / PP_TILE;
    const size_t Epad = (size_t)nt * PP_TILE;
    const u32 tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const u32 lcol = threadIdx.x & 63u, lpart = threadIdx.x >> 6;
    u32 I = 0, o = blockIdx.x;   // o = J - I; row I of tiles holds the pairs o = 0 .. nt - I - 1
    for (;; o += gridDim.x) {
        while (I < nt && o >= nt - I) o -= nt - I, ++I;
        if (I >= nt) break;
        const u32 J = I + o;
        if (threadIdx.x == 0) s_n = 0u;   // (the last pair's sum has been read; the chunk loop's barriers stand between this and the lanes' adds)
        u32 acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = 0u;
        for (u32 w0 = 0; w0 < TW; w0 += PP_CHUNK) {
            const u32 nw = min((u32)PP_CHUNK, TW - w0);
            __syncthreads();   // the last chunk's readers are done
            for (u32 k = lpart; k < nw; k += 4u) {
                const ull* src = prof + (size_t)(w0 + k) * Epad;
                sA[k][lcol] = src[I * PP_TILE + lcol];
                sB[k][lcol] = src[J * PP_TILE + lcol];
            }
            __syncthreads();
            for (u32 k = 0; k < nw; ++k) {
                const ulonglong2 a0 = *reinterpret_cast<const ulonglong2*>(&sA[k][ty * 4u]), a1 = *reinterpret_cast<const ulonglong2*>(&sA[k][ty * 4u + 2u]);
                const ulonglong2 b0 = *reinterpret_cast<const ulonglong2*>(&sB[k][tx * 4u]), b1 = *reinterpret_cast<const ulonglong2*>(&sB[k][tx * 4u + 2u]);
                const ull av[4] = {a0.x, a0.y, a1.x, a1.y}, bv[4] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[r][c] += (u32)__popcll(av[r] & bv[c]);
            }
        }
        const u32 x0 = I * PP_TILE + ty * 4u, y0 = J * PP_TILE + tx * 4u;
        const uint4 na4 = *reinterpret_cast<const uint4*>(n_e + x0), nb4 = *reinterpret_cast<const uint4*>(n_e + y0);
        const u32 na[4] = {na4.x, na4.y, na4.z, na4.w}, nb[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
        u32 pass = 0u;   // bit r * 4 + c: the cell is a linked pair
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const u32 x = x0 + (u32)r, y = y0 + (u32)c, k = acc[r][c];
                const bool ok = x < E && y < E && (I != J || x < y) && k >= k_min && (u32)__umul24(k, den) >= (u32)__umul24(num, na[r] + nb[c] - k);   // (__umul24 returns int: both reach 2^31)
                pass |= (ok ? 1u : 0u) << (r * 4 + c);
            }
        const u32 cnt = (u32)__popc(pass);
        const u32 off = cnt ? atomicAdd(&s_n, cnt) : 0u;
        __syncthreads();
        if (threadIdx.x == 0 && s_n) {
            const ull before = atomicAdd(total + (EMIT ? 1 : 0), (ull)s_n);
            if (EMIT) s_base = (u32)before;
        }
        if (!EMIT) continue;
        __syncthreads();
        u32 p = s_base + off;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (!((pass >> (r * 4 + c)) & 1u)) continue;
                if (p < cap) key[p] = ((u64)el[x0 + (u32)r] << 32) | (u64)el[y0 + (u32)c], val[p] = acc[r][c];
                ++p;
            }
    }
}

__global__ __launch_bounds__(256) void k_pp_unpack(u32 n, const u64* __restrict__ key, const u32* __restrict__ val, int* __restrict__ a, int* __restrict__ b,
                                                   int* __restrict__ shared) {
    const size_t i = tid256();
    if (i < n) a[i] = (int)(key[i] >> 32), b[i] = (int)(u32)key[i], shared[i] = (int)val[i];
}

thread_local std::string g_phyletic_err;

auto slots(so_phyletic_result* r) { return result_slots(&r->present, &r->a, &r->b, &r->shared); }

}  // namespace

extern "C" {

const char* so_phyletic_last_error(void) { return g_phyletic_err.c_str(); }

void so_phyletic_free(so_phyletic_result* r) {
    if (r) release_slots(r, slots(r));
}

int so_phyletic_pairs(int device, int64_t m, const int32_t* row, const int32_t* taxon, int64_t n_rows, int64_t n_file_rows, int64_t n_taxa, int32_t n_min, int32_t n_max,
                      int32_t k_min, int32_t num, int32_t den, int32_t flags, so_phyletic_result* out) {
    const std::string who = "so_phyletic_pairs";
    return guarded_call(g_phyletic_err, out, so_phyletic_free, [&] {
        if (!out) throw SoError(who + ": result pointer is NULL");
        memset(out, 0, sizeof *out);
        if (flags & ~3) throw SoError(who + ": unknown flag bits (bit 0: no pair arrays in the result, bit 1: count, emit and sort timed by events)");
        if (m < 0 || n_rows < 0) throw SoError(who + ": bad arguments");
        if (n_taxa < 1 || n_taxa > PAN_MAX_TAXA) throw SoError(who + ": the taxa number 1 .. " + std::to_string(PAN_MAX_TAXA) + " (n_taxa is " + std::to_string(n_taxa) + ")");
        if (n_rows >= (1ll << 31)) throw SoError(who + ": 2^31 rows and more are not supported");
        if (m >= (1ll << 31)) throw SoError(who + ": 2^31 members and more are not supported");
        if (n_file_rows < 0 || n_file_rows > n_rows) throw SoError(who + ": n_file_rows lies in 0 .. n_rows (it is " + std::to_string(n_file_rows) + ")");
        if (n_min < 1) throw SoError(who + ": n_min is at least 1 (it is " + std::to_string(n_min) + ")");
        if (k_min < 1) throw SoError(who + ": k_min is at least 1 (it is " + std::to_string(k_min) + ")");
        if (num < 1 || num > den || den >= (1 << 20))
            throw SoError(who + ": the threshold num / den needs 0 < num <= den < 2^20 (they are " + std::to_string(num) + " and " + std::to_string(den) + ")");
        if (m > 0 && (!row || !taxon)) throw SoError(who + ": a member column is NULL");
        if (m > 0 && n_rows == 0) throw SoError(who + ": a row outside 0 .. n_rows - 1");
        const bool want = !(flags & 1), timed = flags & 2;
        out->n_rows = n_rows;
        check_device(who.c_str(), device);
        if (n_rows == 0) {   // nothing to launch
            fill_empty_slots(slots(out));
            return;
        }
        DeviceCall call(device);
        hipStream_t st = call.st;
        const char* w = who.c_str();
        const u32 M = (u32)m, R = (u32)n_rows, F = (u32)n_file_rows, T = (u32)n_taxa, TW = (T + 63u) / 64u;
        // E, the eligible rows, is known after the first wait only: until then the file rows bound it
        const size_t EP = ((size_t)F + PP_TILE - 1u) / PP_TILE * PP_TILE;
        // the grid of k_pp_tile: as many workgroups as the device holds at a time, fewer where the tile pairs of `rows` rows are fewer.  The
        // kernel takes 71 registers, seven workgroups a CU; held to 64 by a second launch bound (eight a CU, nothing spilled) both passes
        // were 5 % slower in alternating runs (profiles/phyletic_cost.txt), so it is left as it compiles and the runtime says how many fit
        int cus = 0, per_cu = 0;
        HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pp_tile<true>, 256, 0));
        const auto tile_grid = [&](u64 rows) {
            const u64 nt = (rows + PP_TILE - 1u) / PP_TILE;
            return dim3((u32)std::min<u64>(nt * (nt + 1u) / 2, (u64)std::max(cus, 1) * (u64)std::max(per_cu, 1)));
        };
        DevBuf<int> d_row, d_tax, present;
        DevBuf<ull> rowbits, prof, total;
        DevBuf<u32> err, flag, pos, tmp, n_e, el;
        upload(d_row, row, (size_t)m, st), upload(d_tax, taxon, (size_t)m, st);
        rowbits.ensure((size_t)R * TW + 2), present.ensure((size_t)R + 2), flag.ensure((size_t)R + 2), pos.ensure((size_t)R + 2), tmp.ensure(scan_u32_temp_elems(R) + 2);
        prof.ensure((size_t)TW * EP + 2), n_e.ensure(EP + 4), el.ensure(EP + 4), err.ensure(4), total.ensure(4);
        HIP_CHECK(hipMemsetAsync(rowbits.p, 0, (size_t)R * TW * sizeof(ull), st));
        HIP_CHECK(hipMemsetAsync(err.p, 0, sizeof(u32), st));
        HIP_CHECK(hipMemsetAsync(total.p, 0, 2 * sizeof(ull), st));
        if (EP) {   // the pad rows of the last tile hold no taxon
            HIP_CHECK(hipMemsetAsync(prof.p, 0, (size_t)TW * EP * sizeof(ull), st));
            HIP_CHECK(hipMemsetAsync(n_e.p, 0, EP * sizeof(u32), st));
        }
        if (M) hipLaunchKernelGGL(k_pan_rowbits, grid256(M), dim3(256), 0, st, M, d_row.p, d_tax.p, R, T, TW, rowbits.p, err.p);
        hipLaunchKernelGGL(k_pp_present, grid256(R), dim3(256), 0, st, R, F, TW, rowbits.p, (int)n_min, (int)n_max, present.p, flag.p);
        const u32* d_E = scan_u32(flag.p, pos.p, R, false, tmp.p, st);   // (tmp is not scanned with again: the word stays)
        StageEvents ev(timed);   // marks 0, 1 around the count pass; 2, 3, 4 around the emit pass and the sort
        if (F >= 2u) {   // (fewer file rows: no pair, and no grid of 0 blocks)
            hipLaunchKernelGGL(k_pp_gather, grid256(R), dim3(256), 0, st, R, TW, rowbits.p, present.p, flag.p, pos.p, d_E, prof.p, n_e.p, el.p);
            ev.mark(0, st);
            hipLaunchKernelGGL(k_pp_tile<false>, tile_grid(F), dim3(256), 0, st, prof.p, n_e.p, el.p, d_E, TW, (u32)k_min, (u32)num, (u32)den, total.p,
                               (u64*)nullptr, (u32*)nullptr, 0u);
            ev.mark(1, st);
        }
        HIP_CHECK(hipGetLastError());
        u32 e = 0, E = 0;
        ull tot[2] = {0, 0};
        call.fetch(&e, err.p), call.fetch(&E, d_E), call.fetch(tot, total.p);
        static_assert(sizeof(int) == sizeof(int32_t), "the counts are copied out as int32");
        out->present = host_copy(w, present.p, (size_t)R, st);
        call.wait();   // the count that sizes the output
        out->waits = call.waits;
        if (e & 1u) throw SoError(who + ": a row outside 0 .. n_rows - 1");
        if (e & 2u) throw SoError(who + ": a taxon outside 0 .. n_taxa - 1");
        if (E > PP_TILE * PP_MAX_TILES)
            throw SoError(who + ": " + std::to_string(E) + " eligible rows are more than one call serves (" + std::to_string(PP_TILE * PP_MAX_TILES) +
                          ": " + std::to_string(PP_MAX_TILES) + " tiles of " + std::to_string(PP_TILE) + ")");
        const u32 nt = (E + PP_TILE - 1u) / PP_TILE;
        out->n_eligible = E, out->n_pairs = (i64)tot[0], out->tiles = E >= 2u ? (i64)nt * (nt + 1u) / 2 : 0;
        if (F >= 2u) out->count_ms = ev.ms(0);
        if (tot[0] >= (1ull << 31)) throw SoError(who + ": " + std::to_string(tot[0]) + " linked pairs: 2^31 and more are not supported (raise the thresholds)");
        if (tot[0] == 0) {   // no pair: nothing more to launch
            fill_empty_slots(slots(out));
            return;
        }
        const u32 N = (u32)tot[0];
        const int bits = 32 + ceil_log2(R);
        const size_t sort_bytes = sort_pairs_u64_u32_temp_bytes(N, bits);
        {   // keys and counts before and after the sort, the three result columns, the sort's scratch
            const size_t bytes = (size_t)N * (2 * (sizeof(u64) + sizeof(u32)) + 3 * sizeof(int)) + sort_bytes;
            size_t free_b = 0, total_b = 0;
            HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            if (bytes + bytes / 8 > free_b / 2)
                throw SoError(who + ": the " + std::to_string(N) + " linked pairs and their sort would take " + std::to_string(bytes) +
                              " bytes, more than half of the free device memory (" + std::to_string(free_b) + " bytes free): raise the thresholds");
        }
        DevBuf<u64> key, skey;
        DevBuf<u32> val, sval;
        DevBuf<u8> sort_tmp;
        DevBuf<int> d_a, d_b, d_s;
        key.ensure((size_t)N + 2), val.ensure((size_t)N + 2), skey.ensure((size_t)N + 2), sval.ensure((size_t)N + 2), sort_tmp.ensure(sort_bytes + 16);
        d_a.ensure((size_t)N + 2), d_b.ensure((size_t)N + 2), d_s.ensure((size_t)N + 2);
        ev.mark(2, st);
        hipLaunchKernelGGL(k_pp_tile<true>, tile_grid(E), dim3(256), 0, st, prof.p, n_e.p, el.p, d_E, TW, (u32)k_min, (u32)num, (u32)den, total.p, key.p, val.p, N);
        ev.mark(3, st);
        sort_pairs_u64_u32(sort_tmp.p, sort_bytes, key.p, skey.p, val.p, sval.p, N, bits, st);
        ev.mark(4, st);
        hipLaunchKernelGGL(k_pp_unpack, grid256(N), dim3(256), 0, st, N, skey.p, sval.p, d_a.p, d_b.p, d_s.p);
        HIP_CHECK(hipGetLastError());
        call.fetch(tot, total.p, 2);
        if (want) out->a = host_copy(w, d_a.p, (size_t)N, st), out->b = host_copy(w, d_b.p, (size_t)N, st), out->shared = host_copy(w, d_s.p, (size_t)N, st);
        call.wait();   // the result
        out->waits = call.waits;
        if (tot[1] != tot[0]) throw SoError(who + ": the emit pass wrote " + std::to_string(tot[1]) + " pairs where the count pass found " + std::to_string(tot[0]));
        out->emit_ms = ev.ms(2), out->sort_ms = ev.ms(3);
        fill_empty_slots(slots(out));
    });
}

}  // extern "C"
