// Host build of the .loci line rule (csrc/itx_lociline.h) for tests/test_lociline.py.
#include "../iteres_amd/csrc/itx_lociline.h"

extern "C" int itxl_bin(int start, int end) { return itx_loci_bin(start, end); }
extern "C" uint32_t itxl_key(uint32_t rank, int bin) { return itx_loci_key(rank, bin); }
extern "C" int itxl_f3_hard(double v) { return itx_loci_f3_hard(v); }

// "%.3f" of v[i] into out + 32 i (0xAA behind it), its length into len[i]; -1 for a value the rule does not model
extern "C" void itxl_f3_many(const double *v, size_t n, uint8_t *out, int32_t *len)
{
    for (size_t i = 0; i < n; i++) {
        uint8_t *o = out + 32 * i;
        for (int k = 0; k < 32; k++) o[k] = 0xAA;
        if (itx_loci_f3_hard(v[i])) {
            len[i] = -1;
            continue;
        }
        const uint32_t l = itx_loci_f3len(v[i]);
        len[i] = (int32_t)l;
        if (l <= 32u && itx_loci_put_f3(o, 0, l, 0, v[i]) != l) len[i] = -2;
    }
}

// the two doubles of a filter line from its integers
extern "C" void itxl_filter_doubles(const uint32_t *count, const uint32_t *length, const uint64_t *reads_num, size_t n, double *rpkm, double *rpm)
{
    for (size_t i = 0; i < n; i++) {
        ItxLociLine L;
        itx_loci_filter_numbers(&L, 0u, length[i], count[i], reads_num[i]);
        rpkm[i] = L.a;
        rpm[i] = L.b;
    }
}

// One line. Returns its length, -1 when the host has to look, -2 when it does not fit `cap`. The line is laid down in pieces of
// `piece` bytes, each by a call of its own, the way the device lays it down window by window; 0xAA fills what no call should touch.
extern "C" long long itxl_line(int kind, const uint8_t *chr, uint32_t chr_len, const uint8_t *rep, uint32_t rep_len, const uint8_t *cla, uint32_t cla_len,
                               const uint8_t *fam, uint32_t fam_len, uint32_t start, uint32_t end, uint32_t count, uint64_t reads_num, double total, uint8_t *out,
                               uint32_t cap, uint32_t piece)
{
    ItxLociLine L;
    if (kind == ITX_LOCI_FILTER) itx_loci_filter_numbers(&L, start, end, count, reads_num);
    else itx_loci_cpg_numbers(&L, start, end, (int)count, total);
    L.chr = chr;
    L.chr_len = chr_len;
    L.rep = rep;
    L.rep_len = rep_len;
    L.cla = cla;
    L.cla_len = cla_len;
    L.fam = fam;
    L.fam_len = fam_len;
    if (itx_loci_hard(&L)) return -1;
    const uint32_t len = itx_loci_len(&L);
    if (len > cap) return -2;
    for (uint32_t k = 0; k < cap; k++) out[k] = 0xAA;
    if (piece == 0) piece = len;
    for (uint32_t lo = 0; lo < len; lo += piece) {
        const uint32_t hi = lo + piece < len ? lo + piece : len;
        itx_loci_write(&L, out + lo, lo, hi);
    }
    return (long long)len;
}
