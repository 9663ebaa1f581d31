// itx_tablebuild.h — the rules of the repeat table's build that the host build, the device build (both csrc/itx_table.hip) and
// their tests share. Plain C++ on the host, __host__ __device__ under hipcc; nothing here touches memory but its arguments.
//   tb_bin_of_range   level and bin of a row as binKeeperAdd files it (cuskent/binRange.c:20-21,119-138)
//   tb_rank_key       the sort key whose ascending, stable order from file order is binKeeperFind's return order inside a
//                     chromosome: level coarse (5) -> fine (0), bin descending, file order ascending (binRange.c:209-225)
//   tb_key_passes     8-bit passes a radix sort needs for keys up to `max_key`
//   TbRun, tb_run_*   the running maximum of the ends of a chromosome's rows below a row (ItxIv.pbelow), as a summary of a
//                     stretch of start-sorted rows that can be joined with the stretch before it
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TB_HD __host__ __device__ __forceinline__
#else
#define TB_HD static inline
#endif

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

// a bin is below 4681 + 2^14 (positions are ints): 16 bits hold it, the level goes above them
#define TB_RANK_KEY_BITS 19u
TB_HD uint32_t tb_rank_key(int level, int bin) { return ((uint32_t)(5 - level) << 16) | (0xffffu - (uint32_t)bin); }

TB_HD uint32_t tb_key_passes(uint64_t max_key)
{
    uint32_t p = 1;
    while (p < 8 && (max_key >> (8 * p)) != 0) p++;
    return p;
}

// A stretch of start-sorted rows: its last chromosome, the maximum end over its rows of that chromosome, and whether the
// whole stretch lies in it. An empty stretch has last_chrom -1.
struct TbRun {
    int32_t last_chrom, last_max;
    int32_t one_chrom;
};
#define TB_NO_END INT32_MIN        // pbelow of a chromosome's first row
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
