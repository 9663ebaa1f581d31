// Host build of the tag rule of filter -b -a (csrc/itx_reptag.h) for tests/test_reptag.py, which loads it as a library and holds it
// against the Python restatement (tests/reptagcase.py). Built as a program (it has a main) it runs the rule over the same families
// of cases by itself, whole records against pieces with guard bytes around every piece: the form in which it is built with
// -fsanitize=address,undefined (DESIGN.md records that run).
#include "../iteres_amd/csrc/itx_reptag.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static ItxRepTag make_tag(const uint8_t *rep, uint32_t nl, const uint8_t *cla, uint32_t cl, const uint8_t *fam, uint32_t fl, uint32_t start, uint32_t end)
{
    ItxRepTag t;
    t.rep = rep, t.cla = cla, t.fam = fam;
    t.rep_len = nl, t.cla_len = cl, t.fam_len = fl;
    t.start = start, t.end = end;
    return t;
}

extern "C" uint32_t itxr_len(uint32_t nl, uint32_t cl, uint32_t fl)
{
    const ItxRepTag t = make_tag(nullptr, nl, nullptr, cl, nullptr, fl, 0, 0);
    return itx_reptag_len(&t);
}

// bytes [from, to) of the annotated record into dst
extern "C" void itxr_piece(const uint8_t *rec, uint32_t rec_len, const uint8_t *rep, uint32_t nl, const uint8_t *cla, uint32_t cl, const uint8_t *fam, uint32_t fl,
                           uint32_t start, uint32_t end, uint32_t from, uint32_t to, uint8_t *dst)
{
    const ItxRepTag t = make_tag(rep, nl, cla, cl, fam, fl, start, end);
    itx_reptag_write(rec, rec_len, &t, from, to, dst);
}

#define GUARD 32u
// every pair cuts[a] <= cuts[b] as a piece, written between guard bytes and held against want[from, to); returns the number of pairs
// checked, or -(1 + the index of the first pair that failed)
static long check_pairs(const uint8_t *rec, uint32_t rec_len, const ItxRepTag *t, const uint32_t *cuts, uint32_t n_cuts, const uint8_t *want)
{
    const uint32_t whole = rec_len + itx_reptag_len(t);
    std::vector<uint8_t> buf((size_t)whole + 2 * GUARD);
    long done = 0;
    for (uint32_t a = 0; a < n_cuts; a++)
        for (uint32_t b = 0; b < n_cuts; b++) {
            const uint32_t from = cuts[a], to = cuts[b];
            if (from > to || to > whole) continue;
            const uint8_t fill = (uint8_t)(0xA5u ^ (done & 1 ? 0xffu : 0u));       // both values: a byte that equals the guard is still seen
            memset(buf.data(), fill, buf.size());
            itx_reptag_write(rec, rec_len, t, from, to, buf.data() + GUARD);
            if (memcmp(buf.data() + GUARD, want + from, to - from) != 0) return -(1 + done);
            for (uint32_t k = 0; k < GUARD; k++)
                if (buf[k] != fill || buf[GUARD + (to - from) + k] != fill) return -(1 + done);
            for (size_t k = GUARD + (to - from) + GUARD; k < buf.size(); k++)
                if (buf[k] != fill) return -(1 + done);
            done++;
        }
    return done;
}

extern "C" long itxr_check_pairs(const uint8_t *rec, uint32_t rec_len, const uint8_t *rep, uint32_t nl, const uint8_t *cla, uint32_t cl, const uint8_t *fam, uint32_t fl,
                                 uint32_t start, uint32_t end, const uint32_t *cuts, uint32_t n_cuts, const uint8_t *want)
{
    const ItxRepTag t = make_tag(rep, nl, cla, cl, fam, fl, start, end);
    return check_pairs(rec, rec_len, &t, cuts, n_cuts, want);
}

// ---- the program: the same families of cases, the whole record (one piece) as the expectation of every other piece
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n)
{
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 24) % n);
}

static std::vector<uint8_t> bytes_of(uint32_t n, uint8_t first)
{
    std::vector<uint8_t> v(n);
    for (uint32_t i = 0; i < n; i++) v[i] = (uint8_t)(first + i % 23u);
    return v;
}

// a record of rec_len >= 36 bytes whose block_size says so
static std::vector<uint8_t> record_of(uint32_t rec_len)
{
    std::vector<uint8_t> r = bytes_of(rec_len, 0x30);
    const uint32_t bs = rec_len - 4u;
    for (int k = 0; k < 4; k++) r[k] = (uint8_t)(bs >> (8 * k));
    return r;
}

static long g_pairs = 0;
static int one_case(uint32_t rec_len, uint32_t nl, uint32_t cl, uint32_t fl, uint32_t start, uint32_t end, int every_pair)
{
    const std::vector<uint8_t> rec = record_of(rec_len), rep = bytes_of(nl, 'A'), cla = bytes_of(cl, 'a'), fam = bytes_of(fl, 'K');
    const ItxRepTag t = make_tag(rep.data(), nl, cla.data(), cl, fam.data(), fl, start, end);
    const uint32_t whole = rec_len + itx_reptag_len(&t);
    if (itx_reptag_len(&t) != 26u + nl + cl + fl) return 1;
    std::vector<uint8_t> want((size_t)whole + 1);
    itx_reptag_write(rec.data(), rec_len, &t, 0, whole, want.data());
    // what must hold whatever the pieces are: block_size, the original bytes, the keys, the NULs and the integers
    uint32_t bs = 0, v = 0;
    memcpy(&bs, want.data(), 4);
    if (bs != whole - 4u || memcmp(want.data() + 4, rec.data() + 4, rec_len - 4u) != 0) return 2;
    uint32_t at = rec_len;
    const uint32_t lens[3] = {nl, cl, fl};
    const std::vector<uint8_t> *names[3] = {&rep, &cla, &fam};
    for (int k = 0; k < 3; k++) {
        if (want[at] != 'Z' || want[at + 1] != "NCF"[k] || want[at + 2] != 'Z' || (lens[k] && memcmp(want.data() + at + 3, names[k]->data(), lens[k]) != 0) ||
            want[at + 3 + lens[k]] != 0)
            return 3;
        at += 4u + lens[k];
    }
    memcpy(&v, want.data() + at + 3, 4);
    if (memcmp(want.data() + at, "ZSI", 3) != 0 || v != start) return 4;
    memcpy(&v, want.data() + at + 10, 4);
    if (memcmp(want.data() + at + 7, "ZEI", 3) != 0 || v != end || at + 14 != whole) return 5;
    // the cuts: every byte (every_pair 1: short records), a few anywhere (2), or every byte within 8 of a field boundary (0)
    std::vector<uint32_t> cuts;
    if (every_pair == 1) {
        for (uint32_t c = 0; c <= whole; c++) cuts.push_back(c);
    } else if (every_pair == 2) {                                          // (the seeded pairs: a few cuts anywhere)
        cuts.push_back(0u), cuts.push_back(whole);
        for (int k = 0; k < 14; k++) cuts.push_back(rnd(whole + 1u));
    } else {
        std::vector<uint32_t> edge = {0u, 4u, rec_len};
        uint32_t e = rec_len;
        for (int k = 0; k < 3; k++) {
            edge.push_back(e + 3u);
            edge.push_back(e + 3u + lens[k]);
            e += 4u + lens[k];
            edge.push_back(e);
        }
        edge.push_back(e + 3u), edge.push_back(e + 7u), edge.push_back(e + 10u), edge.push_back(e + 14u);
        for (uint32_t b : edge)
            for (int d = -8; d <= 8; d++)
                if ((long)b + d >= 0 && (uint32_t)(b + d) <= whole) cuts.push_back((uint32_t)(b + d));
    }
    const long n = check_pairs(rec.data(), rec_len, &t, cuts.data(), (uint32_t)cuts.size(), want.data());
    if (n < 0) return 6;
    g_pairs += n;
    return 0;
}

int main(void)
{
    static const uint32_t name_lens[] = {0, 1, 2, 254, 65535}, coords[] = {0, 1, 0x80000000u, 0xffffffffu}, rec_lens[] = {36, 37, 100, 8191, 8192, 32768, 70000};
    long cases = 0;
    int why = 0;
#define CASE(...)                                                                          \
    do {                                                                                   \
        if ((why = one_case(__VA_ARGS__)) != 0) {                                          \
            fprintf(stderr, "reptag_host: case %ld failed (check %d): %s\n", cases, why, #__VA_ARGS__); \
            return 1;                                                                      \
        }                                                                                  \
        cases++;                                                                           \
    } while (0)
    for (uint32_t a : name_lens)
        for (int pos = 0; pos < 3; pos++) CASE(120, pos == 0 ? a : 3, pos == 1 ? a : 4, pos == 2 ? a : 5, 1000, 2000, 0);
    for (uint32_t s : coords)
        for (uint32_t e : coords) CASE(77, 5, 3, 7, s, e, 0);
    for (uint32_t L : rec_lens) CASE(L, 6, 4, 9, 123456, 234567, 0);
    CASE(36, 0, 0, 0, 0, 0, 1);
    CASE(61, 7, 3, 5, 0x01020304u, 0xa1b2c3d4u, 1);
    CASE(70000, 254, 1, 2, 0x01020304u, 0xa1b2c3d4u, 0);
    for (int k = 0; k < 2000; k++) CASE(36 + rnd(k % 50 == 0 ? 69000 : 400), rnd(40), rnd(12), rnd(20), rnd(0xffffffffu), rnd(0xffffffffu), 2);
    printf("reptag_host: %ld cases, %ld pieces, all as the whole record says\n", cases, g_pairs);
    return 0;
}
