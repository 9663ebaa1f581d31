// Host build of the tag walk (iteres_amd/csrc/itx_auxwalk.h) for tests/test_auxwalk.py, a program of its own so that it can be
// built with -fsanitize=address,undefined and run as it is:
//
//   auxwalk_host IN OUT
//
// IN: records, each a u32 length and that many bytes (a BAM record from its block_len on). Every record is copied into a heap
// block of exactly its size before it is read, so a read past the record's end is one past the block's. OUT, per record:
// u8 has_xa, i32 nm, u32 xa_len, the string's bytes. The walk is asked three ways — XA and NM in one pass, XA alone, NM alone —
// and the program fails when they disagree.
#include "../iteres_amd/csrc/itx_auxwalk.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t len;
    size_t n = 0;
    while (fread(&len, 4, 1, in) == 1) {
        uint8_t *rec = (uint8_t *)malloc(len ? len : 1);
        if (len && fread(rec, 1, len, in) != len) return 3;
        const uint8_t *s, *end, *xa = NULL, *nm = NULL, *xa1 = NULL, *nm1 = NULL;
        if (itx_aux_bounds(rec, &s, &end)) {
            itx_aux_find(s, end, ITX_AUX_TAG('X', 'A'), &xa, ITX_AUX_TAG('N', 'M'), &nm);
            itx_aux_find(s, end, ITX_AUX_TAG('X', 'A'), &xa1, 0, NULL);
            itx_aux_find(s, end, ITX_AUX_TAG('N', 'M'), &nm1, 0, NULL);
            if (xa != xa1 || nm != nm1) {
                fprintf(stderr, "record %zu: the one-pass walk and the single walks disagree\n", n);
                return 4;
            }
        }
        if (end != rec + len || s > end) {
            fprintf(stderr, "record %zu: bounds outside the record\n", n);
            return 5;
        }
        const uint8_t has = xa != NULL;
        const int32_t v = has ? itx_aux_int(nm, end) : 0;
        uint32_t xl = 0;
        const uint8_t *z = itx_aux_str(xa, end, &xl);
        if (!has) xl = 0;
        fwrite(&has, 1, 1, out);
        fwrite(&v, 4, 1, out);
        fwrite(&xl, 4, 1, out);
        if (xl) fwrite(z, 1, xl, out);
        free(rec);
        n++;
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
