// itx_bwzoomrule.h — which zoom levels a bigWig gets (cuskent/bwgCreate.c:826-885), stated once for the three places that decide it:
// the dense plan (host/bw_dense.c, counts in closed form), the sparse host writer (host/bw_sparse.c, counts by reducing) and the
// device builder of filter -W (csrc/itx_gcovbw.hip, counts from its chain kernels). Plain C, valid as C11 and as C++17, host only.
// The rule decides from COUNTS — how many summaries a reduction gives — and the caller supplies them (tests/bwzoomrule_main.c):
//   first level    the first try is 10 times the mean resolution. A try is counted; when twice its 32-byte summaries are at least
//                  half the data's size (and not the size of the try before), the next try is
//                  max((int)(1.1 * reduction * size / half), 2 * reduction); otherwise the level is fixed.
//   further ones   up to nine, each 4 times the reduction before (the dropped ones included), none above 10^9, each counted from the
//                  last level KEPT. A level is dropped when its 32-byte summaries are exactly the last size the first-level loop
//                  refused, and the levels end with the first count that is no more than the number of chromosomes.
// long long throughout, with the reference's (int) cast. A reduction outside 1 .. ITX_BWZ_MAX_RED (its BIGNUM), or a product the
// cast cannot hold, is REPORTED, never computed with: the reference overflows an int there. Further levels are in range.
#ifndef ITX_BWZOOMRULE_H
#define ITX_BWZOOMRULE_H
#include <stdint.h>
#include <string.h>

#define ITX_BWZ_MAX_LEVELS 10
#define ITX_BWZ_MAX_RED 0x3fffffffll

enum { ITX_BWZ_FIXED = 0, ITX_BWZ_COUNT = 1, ITX_BWZ_RANGE = 2 };

typedef struct itx_bwzoom {
    long long red;                                  /* the reduction to count, or (ITX_BWZ_RANGE) the one that was refused */
    unsigned long long max_reduced, last_size, n_chrom;
    unsigned reduce_rounds;                         /* tries of the first reduction that were counted */
    int n_levels, further;                          /* levels kept; further levels tried */
    uint32_t reduction[ITX_BWZ_MAX_LEVELS];
} itx_bwzoom;

static inline int itx_bwzoom_try(itx_bwzoom *Z, long long red)
{
    Z->red = red;
    return red < 1 || red > ITX_BWZ_MAX_RED ? ITX_BWZ_RANGE : ITX_BWZ_COUNT;
}

/* full_size: the bytes of all sections' payloads; min_res: the mean of the sections' smallest item lengths (bwgCreate.c:629-686) */
static inline int itx_bwzoom_init(itx_bwzoom *Z, unsigned long long full_size, int min_res, unsigned long long n_chrom)
{
    memset(Z, 0, sizeof *Z);
    Z->max_reduced = full_size / 2;
    Z->n_chrom = n_chrom;
    return itx_bwzoom_try(Z, (long long)min_res * 10);
}

/* n: the summaries of reduction Z->red over the data. ITX_BWZ_COUNT: count Z->red next; ITX_BWZ_FIXED: Z->red is level 0 */
static inline int itx_bwzoom_first(itx_bwzoom *Z, unsigned long long n)
{
    const unsigned long long size = 2ull * 32ull * n;          /* "summary not compressing as well as primary data" */
    Z->reduce_rounds++;
    if (size >= Z->max_reduced && size != Z->last_size) {
        const double t = 1.1 * (double)Z->red * (double)size / (double)Z->max_reduced;
        long long next = 2 * Z->red;
        if (!(t < 2147483648.0)) return itx_bwzoom_try(Z, ITX_BWZ_MAX_RED + 1);    /* no int holds it */
        if ((long long)(int)t > next) next = (long long)(int)t;
        Z->last_size = size;
        return itx_bwzoom_try(Z, next);
    }
    Z->reduction[0] = (uint32_t)Z->red;
    Z->n_levels = 1;
    return ITX_BWZ_FIXED;
}

/* 1: count reduction Z->red over the last level kept, then itx_bwzoom_keep; 0: the levels are complete */
static inline int itx_bwzoom_next(itx_bwzoom *Z)
{
    if (Z->further < 0 || Z->further == ITX_BWZ_MAX_LEVELS - 1) return 0;
    Z->further++;
    Z->red *= 4;
    return Z->red <= 1000000000ll;
}

/* n: the summaries of reduction Z->red. 1: it is level Z->n_levels - 1 now; 0: dropped */
static inline int itx_bwzoom_keep(itx_bwzoom *Z, unsigned long long n)
{
    const int keep = 32ull * n != Z->last_size;
    if (keep) Z->reduction[Z->n_levels++] = (uint32_t)Z->red;
    if (n <= Z->n_chrom) Z->further = -1;
    return keep;
}

#endif
