// itx_tablebuild.h — the rules of the repeat table's build, each stated once: the host build (itx_tablehost.h), the device build
// (itx_table_device.hip) and their tests (tests/tablebuild_main.cpp) all call these and keep no copy. Plain C++ on the host,
// __host__ __device__ under hipcc; nothing here touches memory but its arguments.
//   ItxIv, TbPair, TbQuad  the table's records as plain structs
//   tb_bin_of_range   level and bin of a row as binKeeperAdd files it (cuskent/binRange.c:20-21,119-138)
//   tb_row_ok         when a row is valid: binKeeperAdd's conditions, the id ranges, "fits a bin level"
//   tb_rank_key       the sort key whose ascending, stable order from file order is binKeeperFind's return order inside a
//                     chromosome: level coarse (5) -> fine (0), bin descending, file order ascending (binRange.c:209-225)
//   tb_key_passes     8-bit passes a radix sort needs for keys up to `max_key`
//   tb_row_unit       a row's unit among its name's units
//   tb_row_record     a row's ItxIv, all but pbelow
//   TbRun, tb_run_*   the running maximum of the ends of a chromosome's rows below a row (ItxIv.pbelow), as a summary of a
//                     stretch of start-sorted rows that can be joined with the stretch before it
//   tb_first          the one bisection; tb_chrom_of_bin, tb_bin_bound, tb_starts_before, tb_ends_by, tb_first_start,
//                     tb_first_reach: a bin's entry of the binned index; tb_n_windows, tb_window_unit: a window's first unit
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/iteres_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TB_HD __host__ __device__ __forceinline__
#else
#define TB_HD static inline
#endif

#define ITX_LOGW 13         // slots per partition / LDS window of the partition path (W = 8192)

// One interval of the device table, 32 bytes (two dwordx4 loads). Intervals of a chromosome are
// contiguous and sorted by (start, file order).
struct __attribute__((aligned(16))) ItxIv {
    // first 16 bytes: all the overlap scan reads
    int32_t  s, e;        // genomic [s, e)
    int32_t  pbelow;      // max e over this chromosome's intervals BELOW this one (INT32_MIN for the first): a scan that
                          // walks down from here goes on only while pbelow > query start
    uint32_t rank;        // position in binKeeperFind's list order within the chromosome (binRange.c:209-225)
    // second 16 bytes: read once, for the chosen row
    uint32_t cs;          // consensus_start as the reference parses it (generic.c:1596-1600)
    uint32_t jcap;        // min(consensus_end, repeat length): first consensus index NOT incremented
    uint32_t covslot;     // first slot of the interval's unit inside the slot space (rep_len+1 slots per unit)
    uint32_t zslot;       // covslot + rep_len: the unit's extra slot (never part of the coverage output)
};
static_assert(sizeof(ItxIv) == 32, "ItxIv must be 32 bytes");
// What the device code holds as uint2 (a bin's entry of ItxDevTable.bl) and uint4 (a unit's ids: rep, fam, cla, solo).
struct __attribute__((aligned(8))) TbPair {
    uint32_t x, y;
};
struct __attribute__((aligned(16))) TbQuad {
    uint32_t x, y, z, w;
};
static_assert(sizeof(TbPair) == 8 && sizeof(TbQuad) == 16, "TbPair and TbQuad stand for uint2 and uint4");

// level 0 = finest (128 kb); false: the range fits no level (an empty range at 0, cuskent's errAbort)
TB_HD bool tb_bin_of_range(int start, int end, int *level, int *bin)
{
    const int offsets[6] = {4096 + 512 + 64 + 8 + 1, 512 + 64 + 8 + 1, 64 + 8 + 1, 8 + 1, 1, 0};
    int sb = start >> 17, eb = (end - 1) >> 17;
    for (int i = 0; i < 6; ++i) {
        if (sb == eb) {
            *level = i;
            *bin = offsets[i] + sb;
            return true;
        }
        sb >>= 3;
        eb >>= 3;
    }
    return false;
}

// A row is valid when its chromosome exists and is not empty, its ids are in range, binKeeperAdd would take it
// (cuskent/binRange.c:176-178) and it fits a bin level; then *level and *bin are where it is filed.
TB_HD bool tb_row_ok(const itx_row &r, const int64_t *chrom_size, int n_chrom, uint32_t n_rep, uint32_t n_fam, uint32_t n_cla, int *level, int *bin)
{
    if (!(r.chrom >= 0 && r.chrom < n_chrom && (int)chrom_size[r.chrom] != 0 && r.rep < n_rep && r.fam < n_fam && r.cla < n_cla)) return false;
    const int s = (int)r.start, e = (int)r.end, maxPos = (int)chrom_size[r.chrom];
    return !(s < 0 || e > maxPos || s > e) && tb_bin_of_range(s, e, level, bin);
}

// a bin is below 4681 + 2^14 (positions are ints): 16 bits hold it, the level goes above them
#define TB_RANK_KEY_BITS 19u
TB_HD uint32_t tb_rank_key(int level, int bin) { return ((uint32_t)(5 - level) << 16) | (0xffffu - (uint32_t)bin); }

TB_HD uint32_t tb_key_passes(uint64_t max_key)
{
    uint32_t p = 1;
    while (p < 8 && (max_key >> (8 * p)) != 0) p++;
    return p;
}

// The units of a name are neighbours in (rep, fam, cla) order: a row's unit is its name's first unit or one of the handful
// behind it (the row's triple is among the units; the guard keeps the scan inside them whatever the ids hold).
TB_HD uint32_t tb_row_unit(const itx_row &r, const uint32_t *first_unit, const TbQuad *unit_ids, uint32_t n_units)
{
    uint32_t u = first_unit[r.rep];
    while (u + 1 < n_units && (unit_ids[u].y != r.fam || unit_ids[u].z != r.cla)) u++;
    return u;
}

#define TB_NO_END INT32_MIN        // pbelow of a chromosome's first row
// The record of a row whose name is `len` long, whose unit's slots begin at `slot` and whose place in binKeeperFind's return
// order is `rank`; pbelow is left at TB_NO_END.
TB_HD ItxIv tb_row_record(const itx_row &r, uint32_t len, uint32_t slot, uint32_t rank)
{
    ItxIv d;
    d.s = (int32_t)r.start;
    d.e = (int32_t)r.end;
    d.pbelow = TB_NO_END;
    d.rank = rank;
    d.cs = r.cons_start;
    d.jcap = r.cons_end < len ? r.cons_end : len;
    d.covslot = slot;
    d.zslot = slot + len;
    return d;
}

// A stretch of start-sorted rows: its last chromosome, the maximum end over its rows of that chromosome, and whether the
// whole stretch lies in it. An empty stretch has last_chrom -1.
struct TbRun {
    int32_t last_chrom, last_max;
    int32_t one_chrom;
};
TB_HD TbRun tb_run_empty(void)
{
    TbRun r = {-1, TB_NO_END, 1};
    return r;
}
// the stretch with one more row behind it
TB_HD TbRun tb_run_push(TbRun r, int32_t chrom, int32_t end)
{
    if (r.last_chrom == chrom) {
        r.last_max = end > r.last_max ? end : r.last_max;
    } else {
        r.one_chrom = r.last_chrom < 0;
        r.last_chrom = chrom;
        r.last_max = end;
    }
    return r;
}
// stretch a followed by stretch b
TB_HD TbRun tb_run_join(TbRun a, TbRun b)
{
    if (b.last_chrom < 0) return a;
    if (a.last_chrom < 0) return b;
    if (b.one_chrom && a.last_chrom == b.last_chrom) {
        a.last_max = b.last_max > a.last_max ? b.last_max : a.last_max;
        return a;
    }
    b.one_chrom = 0;
    return b;
}
// pbelow of a row of `chrom` that follows the stretch
TB_HD int32_t tb_run_below(TbRun before, int32_t chrom) { return before.last_chrom == chrom ? before.last_max : TB_NO_END; }

// The first k of [lo, hi) for which before(k) no longer holds, hi if it holds throughout; before() holds on a prefix.
template <class Before>
TB_HD uint32_t tb_first(uint32_t lo, uint32_t hi, Before before)
{
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (before(mid)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The binned index (ItxDevTable.bl). Bin g of all bins belongs to the last chromosome whose bins start at or before g, and begins
// at `bound` inside it. Its entry: .x the chromosome's first row that does not start before the bound, .y its first row whose
// prefix-maximum end max(pbelow, e) passes the bound. Starts and prefix-maximum ends both rise along a chromosome.
TB_HD uint32_t tb_chrom_of_bin(const uint32_t *bin_off, uint32_t n_chrom, uint32_t g)
{
    return tb_first(0, n_chrom + 1, [=](uint32_t c) { return bin_off[c] <= g; }) - 1;
}
TB_HD int64_t tb_bin_bound(uint32_t g, uint32_t first_bin, int shift) { return (int64_t)(g - first_bin) << shift; }
TB_HD bool tb_starts_before(const ItxIv &v, int64_t bound) { return (int64_t)v.s < bound; }
TB_HD bool tb_ends_by(const ItxIv &v, int64_t bound) { return (int64_t)(v.pbelow > v.e ? v.pbelow : v.e) <= bound; }
TB_HD uint32_t tb_first_start(const ItxIv *iv, uint32_t lo, uint32_t hi, int64_t bound)
{
    return tb_first(lo, hi, [=](uint32_t k) { return tb_starts_before(iv[k], bound); });
}
TB_HD uint32_t tb_first_reach(const ItxIv *iv, uint32_t lo, uint32_t hi, int64_t bound)
{
    return tb_first(lo, hi, [=](uint32_t k) { return tb_ends_by(iv[k], bound); });
}

// The slot space in windows of 2^ITX_LOGW slots (k_hist sums the starts of a window per unit), two to spare; the first unit
// that reaches into window w (ItxDevTable.part_unit): the first whose slots end behind the window's first slot, n_units if none.
TB_HD size_t tb_n_windows(uint64_t slots) { return ((size_t)slots >> ITX_LOGW) + 2; }
TB_HD uint32_t tb_window_unit(const uint32_t *unit_slot, uint32_t n_units, uint32_t w)
{
    const uint64_t bound = (uint64_t)w << ITX_LOGW;
    return tb_first(0, n_units, [=](uint32_t u) { return (uint64_t)unit_slot[u + 1] <= bound; });
}
