// itx_lociline.h — one line of the per-locus table of `iteres filter` (writeFilterOut, generic.c:1709-1746) or `iteres cpgfilter`
// (writeFilterOutMRE, generic.c:1748-1772), and where the line stands in its file:
//
//   filter     "%s\t%d\t%d\t%d\t%s\t%s\t%s\t%d\t%.3f\t%.3f\n"   chr start end length repName repClass repFamily count RPKM RPM
//   cpgfilter  "%s\t%d\t%d\t%d\t%s\t%s\t%s\t%d\t%.3f\n"         chr start end length repName repClass repFamily count total
//
// stated once for the device (csrc/itx_loci.hip), for the host writers (host/writers.c) and for the host build the tests hold
// against Python's own `%` (tests/lociline_host.cpp). Plain C over bytes and integers, valid as C and as C++:
//   itx_loci_bin / itx_loci_key   binFromRange (cuskent/binRange.c:119-138) and the sort key of a row: the file walks hashRmsk's
//                   chromosomes in hash order and a chromosome's rows by bin ascending, newest insertion first
//                   (cuskent/binRange.c:365-392), so rows sorted by (chromosome rank, bin), stable, from DESCENDING row order are
//                   in file order
//   itx_loci_rpkm / itx_loci_rpm  the two doubles of a filter line, the expressions of generic.c:35-41
//   itx_loci_f3     "%.3f" of a double without printf: v = m * 2^e with m < 2^53, so for e < 0 the thousandths m * 1000 fit 63
//                   bits and the rounding is one shift, one compare of the remainder against the half, ties to even — what a
//                   correctly rounding printf does (glibc's); for e >= 0 the value is an integer and ".000" follows
//   itx_loci_hard   the line holds a double this rule does not model (not finite: "inf" / "-nan"; magnitude >= 2^63): the host
//                   has to look
//   itx_loci_len / itx_loci_write  the length of a line and its bytes [lo, hi), so that a line may be laid down piece by piece
// Numbers are printed digit by digit, every digit from its own division by a constant power of ten (itx_bedline.h says why).
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef ITX_LOCI_FN
#ifdef __HIPCC__
#define ITX_LOCI_FN static __host__ __device__ inline
#else
#define ITX_LOCI_FN static inline
#endif
#endif

#define ITX_LOCI_FILTER 0
#define ITX_LOCI_CPG 1
#define ITX_LOCI_BIN_BITS 13         /* the key holds bins 0 .. 8191: coordinates below 3511 * 2^17 (460 M) */

/* cuskent/binRange.c:119-138 with the offsets of binOffsetsExtended; -1: no level holds the range */
ITX_LOCI_FN int itx_loci_bin(int start, int end)
{
    int sb = start >> 17, eb = (end - 1) >> 17;
    if (sb == eb) return 4096 + 512 + 64 + 8 + 1 + sb;
    sb >>= 3, eb >>= 3;
    if (sb == eb) return 512 + 64 + 8 + 1 + sb;
    sb >>= 3, eb >>= 3;
    if (sb == eb) return 64 + 8 + 1 + sb;
    sb >>= 3, eb >>= 3;
    if (sb == eb) return 8 + 1 + sb;
    sb >>= 3, eb >>= 3;
    if (sb == eb) return 1 + sb;
    sb >>= 3, eb >>= 3;
    if (sb == eb) return sb;
    return -1;
}
ITX_LOCI_FN int itx_loci_bin_fits(int bin) { return bin >= 0 && bin < (1 << ITX_LOCI_BIN_BITS); }
/* chrom_rank: the chromosome's place in hashRmsk's iteration order; bin: one that fits */
ITX_LOCI_FN uint32_t itx_loci_key(uint32_t chrom_rank, int bin) { return chrom_rank << ITX_LOCI_BIN_BITS | (uint32_t)bin; }

/* generic.c:35-41 (cal_rpkm, cal_rpm): the conversions and the order of the operations are the reference's */
ITX_LOCI_FN double itx_loci_rpkm(unsigned long long reads_count, unsigned long long total_length, unsigned long long mapped_reads_num)
{
    return reads_count / (mapped_reads_num * 1e-9 * total_length);
}
ITX_LOCI_FN double itx_loci_rpm(unsigned long long reads_count, unsigned long long mapped_reads_num)
{
    return reads_count / (mapped_reads_num * 1e-6);
}

/* ---- "%.3f": sign, integer part, thousandths */
typedef struct ItxLociNum {
    uint64_t ip;
    uint32_t fp, neg;
} ItxLociNum;

ITX_LOCI_FN uint64_t itx_loci_bits(double v)
{
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}
/* not finite, or a magnitude of 2^63 and above (0x43e0... is 2^63; inf and nan compare above it as integers) */
ITX_LOCI_FN int itx_loci_f3_hard(double v) { return (itx_loci_bits(v) & 0x7fffffffffffffffull) >= 0x43e0000000000000ull; }

ITX_LOCI_FN ItxLociNum itx_loci_f3(double v)
{
    const uint64_t b = itx_loci_bits(v);
    ItxLociNum r;
    uint64_t m = b & 0xfffffffffffffull;
    int ex = (int)(b >> 52 & 0x7ffu);
    if (ex) m |= 1ull << 52;
    else ex = 1;                                                   /* subnormal: no hidden bit, the exponent of the smallest normal */
    const int e = ex - 1075;                                       /* v = m * 2^e */
    r.neg = (uint32_t)(b >> 63);
    if (e >= 0) {
        r.ip = m << (e > 10 ? 10 : e);                             /* (e > 10 is 2^63 and above: hard, never printed) */
        r.fp = 0;
    } else {
        const uint32_t s = (uint32_t)-e;
        const uint64_t M = m * 1000ull;                            /* < 2^63 */
        uint64_t q = 0;
        if (s < 64u) {                                             /* (s >= 64: M < 2^63 <= the half, the value rounds to 0) */
            const uint64_t rem = M & ((1ull << s) - 1ull), half = 1ull << (s - 1u);
            q = M >> s;
            q += (uint64_t)((rem > half) | ((rem == half) & (q & 1ull)));
        }
        r.ip = q / 1000ull;
        r.fp = (uint32_t)(q % 1000ull);
    }
    return r;
}

ITX_LOCI_FN uint32_t itx_loci_declen(uint32_t v)
{
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
           (v >= 1000000000u);
}
ITX_LOCI_FN uint32_t itx_loci_declen64(uint64_t v)
{
    if (v < 1000000000ull) return itx_loci_declen((uint32_t)v);
    return 10u + (v >= 10000000000ull) + (v >= 100000000000ull) + (v >= 1000000000000ull) + (v >= 10000000000000ull) + (v >= 100000000000000ull) +
           (v >= 1000000000000000ull) + (v >= 10000000000000000ull) + (v >= 100000000000000000ull) + (v >= 1000000000000000000ull);
}
ITX_LOCI_FN uint32_t itx_loci_ilen(int32_t v) { return v < 0 ? 1u + itx_loci_declen(0u - (uint32_t)v) : itx_loci_declen((uint32_t)v); }
ITX_LOCI_FN uint32_t itx_loci_f3len(double v)
{
    const ItxLociNum n = itx_loci_f3(v);
    return n.neg + itx_loci_declen64(n.ip) + 4u;
}

/* ---- the bytes [lo, hi) of a piece of text into dst[0 .. hi - lo); `pos` runs over the line */
#define ITX_LOCI_PUT(b)                                                 \
    do {                                                                \
        if (pos >= lo && pos < hi) dst[pos - lo] = (uint8_t)(b);        \
        pos++;                                                          \
    } while (0)

ITX_LOCI_FN uint32_t itx_loci_put_str(uint8_t *dst, uint32_t lo, uint32_t hi, uint32_t pos, const uint8_t *s, uint32_t n)
{
    const uint32_t a = pos > lo ? pos : lo, b = pos + n < hi ? pos + n : hi;
    for (uint32_t k = a; k < b; k++) dst[k - lo] = s[k - pos];
    return pos + n;
}

/* the last nd decimal digits of v (nd <= 10), leading zeros included */
ITX_LOCI_FN uint32_t itx_loci_put_digits(uint8_t *dst, uint32_t lo, uint32_t hi, uint32_t pos, uint32_t v, uint32_t nd)
{
    if (pos + nd <= lo || pos >= hi) return pos + nd;
#define ITX_LOCI_DIGIT(k, p10) \
    if (nd > k) ITX_LOCI_PUT('0' + (v / p10) % 10u);
    ITX_LOCI_DIGIT(9, 1000000000u)
    ITX_LOCI_DIGIT(8, 100000000u)
    ITX_LOCI_DIGIT(7, 10000000u)
    ITX_LOCI_DIGIT(6, 1000000u)
    ITX_LOCI_DIGIT(5, 100000u)
    ITX_LOCI_DIGIT(4, 10000u)
    ITX_LOCI_DIGIT(3, 1000u)
    ITX_LOCI_DIGIT(2, 100u)
    ITX_LOCI_DIGIT(1, 10u)
    ITX_LOCI_DIGIT(0, 1u)
#undef ITX_LOCI_DIGIT
    return pos;
}

/* "%d" */
ITX_LOCI_FN uint32_t itx_loci_put_i32(uint8_t *dst, uint32_t lo, uint32_t hi, uint32_t pos, int32_t v)
{
    const uint32_t mag = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    if (v < 0) ITX_LOCI_PUT('-');
    return itx_loci_put_digits(dst, lo, hi, pos, mag, itx_loci_declen(mag));
}

/* "%.3f" of a double that is not hard: up to 19 digits before the point, as one digit and two groups of nine */
ITX_LOCI_FN uint32_t itx_loci_put_f3(uint8_t *dst, uint32_t lo, uint32_t hi, uint32_t pos, double v)
{
    const ItxLociNum n = itx_loci_f3(v);
    const uint32_t nd = itx_loci_declen64(n.ip);
    if (pos + n.neg + nd + 4u <= lo || pos >= hi) return pos + n.neg + nd + 4u;
    if (n.neg) ITX_LOCI_PUT('-');
    const uint64_t low18 = n.ip % 1000000000000000000ull;
    if (nd > 18u) ITX_LOCI_PUT('0' + (uint32_t)(n.ip / 1000000000000000000ull));
    if (nd > 9u) pos = itx_loci_put_digits(dst, lo, hi, pos, (uint32_t)(low18 / 1000000000ull), nd > 18u ? 9u : nd - 9u);
    pos = itx_loci_put_digits(dst, lo, hi, pos, (uint32_t)(low18 % 1000000000ull), nd > 9u ? 9u : nd);
    ITX_LOCI_PUT('.');
    return itx_loci_put_digits(dst, lo, hi, pos, n.fp, 3u);
}

/* ---- the line */
typedef struct ItxLociLine {
    const uint8_t *chr, *rep, *cla, *fam;
    uint32_t chr_len, rep_len, cla_len, fam_len;
    int32_t start, end, length, count;
    double a, b;                       /* filter: RPKM, RPM; cpgfilter: the total score (b unused) */
    int kind;                          /* ITX_LOCI_FILTER / ITX_LOCI_CPG */
} ItxLociLine;

/* the numbers of a filter line from a row and its count, with the casts of writeFilterOut (generic.c:1724-1728); the names are
 * the caller's. The line is printed iff L->count >= the -t threshold. */
ITX_LOCI_FN void itx_loci_filter_numbers(ItxLociLine *L, uint32_t start, uint32_t end, uint32_t locus_cnt, unsigned long long reads_num)
{
    const int count = (int)locus_cnt;
    const unsigned length = end - start;
    L->kind = ITX_LOCI_FILTER;
    L->start = (int32_t)start;
    L->end = (int32_t)end;
    L->length = (int32_t)length;
    L->count = count;
    L->a = itx_loci_rpkm((unsigned long long)count, (unsigned long long)length, reads_num);
    L->b = itx_loci_rpm((unsigned long long)count, reads_num);
}
/* the same for cpgfilter (generic.c:1762-1766); the line is printed iff total > the -t threshold */
ITX_LOCI_FN void itx_loci_cpg_numbers(ItxLociLine *L, uint32_t start, uint32_t end, int cpg_count, double total)
{
    L->kind = ITX_LOCI_CPG;
    L->start = (int32_t)start;
    L->end = (int32_t)end;
    L->length = (int32_t)(end - start);
    L->count = cpg_count;
    L->a = total;
    L->b = 0.0;
}

ITX_LOCI_FN int itx_loci_hard(const ItxLociLine *L) { return itx_loci_f3_hard(L->a) || (L->kind == ITX_LOCI_FILTER && itx_loci_f3_hard(L->b)); }

/* of a line that is not hard */
ITX_LOCI_FN uint32_t itx_loci_len(const ItxLociLine *L)
{
    uint32_t n = L->chr_len + 1u + itx_loci_ilen(L->start) + 1u + itx_loci_ilen(L->end) + 1u + itx_loci_ilen(L->length) + 1u + L->rep_len + 1u + L->cla_len + 1u +
                 L->fam_len + 1u + itx_loci_ilen(L->count) + 1u + itx_loci_f3len(L->a) + 1u;
    if (L->kind == ITX_LOCI_FILTER) n += itx_loci_f3len(L->b) + 1u;
    return n;
}

ITX_LOCI_FN void itx_loci_write(const ItxLociLine *L, uint8_t *dst, uint32_t lo, uint32_t hi)
{
    uint32_t pos = 0;
    pos = itx_loci_put_str(dst, lo, hi, pos, L->chr, L->chr_len);
    ITX_LOCI_PUT('\t');
    pos = itx_loci_put_i32(dst, lo, hi, pos, L->start);
    ITX_LOCI_PUT('\t');
    pos = itx_loci_put_i32(dst, lo, hi, pos, L->end);
    ITX_LOCI_PUT('\t');
    pos = itx_loci_put_i32(dst, lo, hi, pos, L->length);
    ITX_LOCI_PUT('\t');
    pos = itx_loci_put_str(dst, lo, hi, pos, L->rep, L->rep_len);
    ITX_LOCI_PUT('\t');
    pos = itx_loci_put_str(dst, lo, hi, pos, L->cla, L->cla_len);
    ITX_LOCI_PUT('\t');
    pos = itx_loci_put_str(dst, lo, hi, pos, L->fam, L->fam_len);
    ITX_LOCI_PUT('\t');
    pos = itx_loci_put_i32(dst, lo, hi, pos, L->count);
    ITX_LOCI_PUT('\t');
    pos = itx_loci_put_f3(dst, lo, hi, pos, L->a);
    if (L->kind == ITX_LOCI_FILTER) {
        ITX_LOCI_PUT('\t');
        pos = itx_loci_put_f3(dst, lo, hi, pos, L->b);
    }
    ITX_LOCI_PUT('\n');
}
