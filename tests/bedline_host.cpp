// Host build of the bed line rule (csrc/itx_bedline.h) for tests/test_bedline.py: one record as raw BAM bytes in, its line out.
#include "../iteres_amd/csrc/itx_bedline.h"

// Returns the line's length (what itx_bed_len says), -1 when the scan calls the record one the host has to look at, -2 when the
// line does not fit `cap`. The line is laid down in pieces of `piece` bytes, each by a call of its own, the way the device lays
// it down window by window; 0xAA fills what no call should touch.
extern "C" long long itxb_line_host(const uint8_t *rec, const uint8_t *chr, uint32_t chr_len, uint32_t start, uint32_t end, uint32_t mapq, uint32_t strand, int with_xa,
                                    uint8_t *out, uint32_t cap, uint32_t piece)
{
    const ItxBedScan sc = itx_bed_scan(rec, with_xa != 0);
    if (sc.hard) return -1;
    ItxBedLine L;
    L.chr = chr;
    L.chr_len = chr_len;
    L.start = start;
    L.end = end;
    L.mapq = mapq;
    L.strand = strand;
    L.qname = rec + 36;
    L.qname_len = sc.qname_len;
    L.has_xa = with_xa && sc.xa_off != ITX_BED_NO_XA;
    L.xa = rec + (L.has_xa ? sc.xa_off : 0u);
    L.xa_len = sc.xa_len;
    L.nm = sc.nm;
    const uint32_t len = itx_bed_len(&L, with_xa != 0);
    if (len > cap) return -2;
    for (uint32_t k = 0; k < cap; k++) out[k] = 0xAA;
    if (piece == 0) piece = len ? len : 1;
    for (uint32_t lo = 0; lo < len; lo += piece) {
        const uint32_t hi = lo + piece < len ? lo + piece : len;
        itx_bed_write(&L, with_xa != 0, out + lo, lo, hi);
    }
    return (long long)len;
}
