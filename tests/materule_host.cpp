// Host build of the mates rule (csrc/itx_materule.h) for tests/test_materule.py. With ITX_MATERULE_MAIN it is a stand-alone program
// for a sanitizer build: it reads cases from a file (see main) and runs the rule over them, every input in a heap block of its exact
// size so that a byte read outside it is seen.
#include "../iteres_amd/csrc/itx_materule.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// everything the rule says about `len` bytes at rec: out = {fixed, whole, wanted, candidate, h32, candidate key tid, pos, wanted key
// tid, pos}; the hash and the keys only for a whole record (else 0)
extern "C" void itxm_eval(const uint8_t *rec, uint32_t len, int64_t *out)
{
    memset(out, 0, 9 * sizeof(int64_t));
    out[0] = itx_mate_fixed(rec, len);
    out[1] = itx_mate_whole(rec, len);
    out[2] = itx_mate_wanted(rec, len);
    out[3] = itx_mate_candidate(rec, len);
    if (out[1]) {
        const ItxMateKey c = itx_mate_key_candidate(rec), w = itx_mate_key_wanted(rec);
        out[4] = c.h32;
        out[5] = c.tid;
        out[6] = c.pos;
        out[7] = w.tid;
        out[8] = w.pos;
        if (w.h32 != c.h32) out[4] = -1;
    }
}

extern "C" int itxm_match(const uint8_t *r, uint32_t r_len, const uint8_t *c, uint32_t c_len) { return itx_mate_match(r, r_len, c, c_len); }
extern "C" uint32_t itxm_h32(const uint8_t *name, uint32_t n) { return itx_mate_h32(name, n); }

extern "C" int itxm_key_cmp(const uint32_t *a, const uint32_t *b)
{
    const ItxMateKey ka = {a[0], a[1], a[2]}, kb = {b[0], b[1], b[2]};
    return itx_mate_key_cmp(&ka, &kb);
}

// what itx_bamout_mates_append_host does with the caller's bytes: the walk over whole records and the candidate check of each.
// Returns the number of records, -1 when the bytes are not whole records; *n_cand candidates, *key_sum a sum over their keys.
extern "C" long itxm_walk(const uint8_t *bytes, size_t len, uint64_t *n_cand, uint64_t *key_sum)
{
    long n = 0;
    *n_cand = 0;
    *key_sum = 0;
    for (size_t at = 0, next = 0; at < len; at = next) {
        if (itx_mate_next(bytes, len, at, &next)) return -1;
        if (itx_mate_candidate(bytes + at, (uint32_t)(next - at))) {
            const ItxMateKey k = itx_mate_key_candidate(bytes + at);
            *n_cand += 1;
            *key_sum += (uint64_t)k.tid * 1000003u + (uint64_t)k.pos * 7u + k.h32;
        }
        n++;
    }
    return n;
}

#ifdef ITX_MATERULE_MAIN
static uint8_t *block(FILE *f, uint32_t len)
{
    uint8_t *p = (uint8_t *)malloc(len ? len : 1);                          // exactly the input: nothing behind it may be read
    if (len && fread(p, 1, len, f) != len) exit(3);
    return p;
}

// cases file: repeated { 1 byte kind, 4 bytes little-endian length, the bytes }. 'E': one record (possibly cut short) -> itxm_eval;
// 'M': 4 bytes length of r, then r, then c -> itxm_match; 'W': the bytes of a host-route window -> itxm_walk
int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    unsigned n_cases = 0;
    for (;;) {
        uint8_t head[5];
        if (fread(head, 1, 5, f) != 5) break;
        const uint32_t len = itx_mate_u32(head + 1);
        if (head[0] == 'E') {
            uint8_t *in = block(f, len);
            int64_t o[9];
            itxm_eval(in, len, o);
            printf("E %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)o[0], (long long)o[1], (long long)o[2], (long long)o[3], (long long)o[4], (long long)o[5],
                   (long long)o[6], (long long)o[7], (long long)o[8]);
            free(in);
        } else if (head[0] == 'M') {
            uint8_t l4[4];
            if (len < 4 || fread(l4, 1, 4, f) != 4) return 3;
            const uint32_t rl = itx_mate_u32(l4);
            if (rl > len - 4) return 3;
            uint8_t *r = block(f, rl), *c = block(f, len - 4 - rl);          // each record in a block of its own
            printf("M %d\n", itxm_match(r, rl, c, len - 4 - rl));
            free(r);
            free(c);
        } else {
            uint8_t *in = block(f, len);
            uint64_t nc = 0, sum = 0;
            const long n = itxm_walk(in, len, &nc, &sum);
            printf("W %ld %llu %llu\n", n, (unsigned long long)nc, (unsigned long long)sum);
            free(in);
        }
        n_cases++;
    }
    fclose(f);
    fprintf(stderr, "%u cases\n", n_cases);
    return 0;
}
#endif
