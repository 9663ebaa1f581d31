// Host build of the coordinate-sort rule (csrc/itx_bamsortrule.h) for tests/test_bamsort_rule.py. With ITX_BAMSORT_MAIN it is a
// stand-alone program for a sanitizer build: it reads cases from a file (see main) and runs the pieces that take untrusted bytes
// over them, every input in a heap block of its exact size so that a byte read or written outside it is seen.
#include "../iteres_amd/csrc/itx_bamsortrule.h"

#include <stdio.h>
#include <stdlib.h>

// the key of the record at rec (len = 4 + block_size bytes): out = {tid, pos, reverse, low key, high key}; returns 1 when it cannot be sorted
extern "C" int itxs_key(const uint8_t *rec, uint32_t len, int64_t *out)
{
    ItxBamSortKey k;
    const int bad = itx_bamsort_key(rec, len, &k);
    out[0] = k.tid;
    out[1] = k.pos;
    out[2] = k.reverse;
    out[3] = itx_bamsort_low(&k);
    out[4] = itx_bamsort_high(&k);
    return bad;
}

extern "C" uint32_t itxs_high_passes(uint32_t n_ref) { return itx_bamsort_high_passes(n_ref); }
extern "C" uint32_t itxs_header_growth(void) { return ITX_BAMSORT_HEADER_GROWTH; }

// the header text under -s: out has room for len + itxs_header_growth() bytes (NULL: the length only)
extern "C" size_t itxs_header_text(const char *text, size_t len, char *out) { return itx_bamsort_header_text(text, len, out); }

// what itx_bamout_append_host does with the caller's bytes in sort mode, restated over the rule: walk whole records (the walk and
// its refusals are append_host's), a key per record. Returns the number of records, -1 when the bytes are not whole records.
extern "C" long itxs_walk(const uint8_t *bytes, size_t len, uint64_t *key_sum)
{
    size_t at = 0;
    long n = 0;
    while (at < len) {
        uint32_t bs = 0;
        if (len - at >= 4) memcpy(&bs, bytes + at, 4);
        if (len - at < 4 || bs >= 0x40000000u || (size_t)bs > len - at - 4) return -1;
        ItxBamSortKey k;
        (void)itx_bamsort_key(bytes + at, 4u + bs, &k);
        *key_sum += itx_bamsort_low(&k) + ((uint64_t)itx_bamsort_high(&k) << 32);
        at += 4 + (size_t)bs;
        n++;
    }
    return n;
}

#ifdef ITX_BAMSORT_MAIN
// cases file: repeated { 1 byte kind ('H' header text, 'R' record bytes), 4 bytes little-endian length, the bytes }
int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    unsigned n_cases = 0;
    for (;;) {
        uint8_t head[5];
        if (fread(head, 1, 5, f) != 5) break;
        const uint32_t len = itx_bamsort_u32(head + 1);
        char *in = (char *)malloc(len ? len : 1);                            // exactly the input: nothing behind it may be read
        if (len && fread(in, 1, len, f) != len) return 3;
        if (head[0] == 'H') {
            const size_t want = itx_bamsort_header_text(in, len, NULL);
            if (want > (size_t)len + ITX_BAMSORT_HEADER_GROWTH) return 4;
            char *out = (char *)malloc(want ? want : 1);                    // exactly the output: nothing behind it may be written
            if (itx_bamsort_header_text(in, len, out) != want) return 5;
            fwrite(out, 1, want, stdout);
            free(out);
        } else {
            uint64_t sum = 0;
            const long n = itxs_walk((const uint8_t *)in, len, &sum);
            printf("%ld %llu\n", n, (unsigned long long)sum);
        }
        free(in);
        n_cases++;
    }
    fclose(f);
    fprintf(stderr, "%u cases\n", n_cases);
    return 0;
}
#endif
