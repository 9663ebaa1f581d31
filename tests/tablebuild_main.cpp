// Stand-alone check of iteres_amd/csrc/itx_tablebuild.h (tests/test_tablebuild.py builds and runs it, plain and with the address
// and undefined-behaviour sanitizers): the rules the device build of the repeat table shares with the host build, each against
// the loop the host build runs (csrc/itx_table.hip, table_create_host), on random and boundary rows.
//   tb_bin_of_range  against binFromRangeBinKeeperExtended's loop written out here
//   tb_rank_key      a stable sort by the key from file order == std::sort by (level desc, bin desc, file order asc)
//   tb_key_passes    the 8-bit passes of a key
//   TbRun            pbelow from stretches of any length joined in any grouping == the serial running maximum per chromosome,
//                    and the very decomposition k_tb_runs uses (threads of R rows, a doubling scan over the workgroup, a carry)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <random>
#include <vector>

#include "../iteres_amd/csrc/itx_tablebuild.h"

#define FAIL(...)                                                        \
    do {                                                                 \
        fprintf(stderr, __VA_ARGS__);                                    \
        fprintf(stderr, "\n");                                           \
        return false;                                                    \
    } while (0)

// cuskent/binRange.c:20-21,119-138, as the host build had it
static const int kOffsets[6] = {4096 + 512 + 64 + 8 + 1, 512 + 64 + 8 + 1, 64 + 8 + 1, 8 + 1, 1, 0};
static bool ref_bin_of_range(int start, int end, int *level, int *bin)
{
    int sb = start >> 17, eb = (end - 1) >> 17;
    for (int i = 0; i < 6; ++i) {
        if (sb == eb) {
            *level = i;
            *bin = kOffsets[i] + sb;
            return true;
        }
        sb >>= 3;
        eb >>= 3;
    }
    return false;
}

struct Row {
    int chrom, start, end;
};

static bool check_bins(std::mt19937_64 &rng, unsigned long *n_checked)
{
    std::vector<std::pair<int, int>> cases;
    // every boundary of every level, one base either side, and the ends of the int range
    for (int lv = 0; lv < 6; lv++) {
        const int64_t w = (int64_t)1 << (17 + 3 * lv);
        for (int64_t m = 1; m <= 5; m++) {
            const int64_t b = w * m;
            if (b > 0x7fffffffLL) break;
            for (int ds = -2; ds <= 2; ds++)
                for (int de = -2; de <= 2; de++) {
                    const int64_t s = b + ds, e = b + de;
                    if (s >= 0 && e >= s && e <= 0x7fffffffLL) cases.emplace_back((int)s, (int)e);
                    if (b - w + ds >= 0 && e >= b - w + ds && e <= 0x7fffffffLL) cases.emplace_back((int)(b - w + ds), (int)e);
                }
        }
    }
    cases.emplace_back(0, 0);                      // empty at 0: fits no level
    cases.emplace_back(0, 1);
    cases.emplace_back(5, 5);
    cases.emplace_back(0, 0x7fffffff);
    cases.emplace_back(0x7fffffff, 0x7fffffff);
    cases.emplace_back(0x7ffffffe, 0x7fffffff);
    for (int k = 0; k < 200000; k++) {
        const int s = (int)(rng() % 0x7fffffffULL);
        const int len = (int)(rng() % ((uint64_t)1 << (rng() % 31)));
        const int64_t e = std::min<int64_t>((int64_t)s + len, 0x7fffffffLL);
        cases.emplace_back(s, (int)e);
    }
    int seen_levels = 0;
    for (auto &c : cases) {
        int l0 = -1, b0 = -1, l1 = -1, b1 = -1;
        const bool r0 = ref_bin_of_range(c.first, c.second, &l0, &b0), r1 = tb_bin_of_range(c.first, c.second, &l1, &b1);
        if (r0 != r1 || (r0 && (l0 != l1 || b0 != b1))) FAIL("bin_of_range(%d, %d): %d level %d bin %d, expected %d level %d bin %d", c.first, c.second, r1, l1, b1, r0, l0, b0);
        if (r1) {
            seen_levels |= 1 << l1;
            const uint32_t key = tb_rank_key(l1, b1);
            if (key >> TB_RANK_KEY_BITS) FAIL("rank key %u of level %d bin %d exceeds %u bits", key, l1, b1, TB_RANK_KEY_BITS);
            if ((int)(5 - (key >> 16)) != l1 || (int)(0xffffu - (key & 0xffffu)) != b1) FAIL("rank key %u does not hold level %d bin %d", key, l1, b1);
        }
        ++*n_checked;
    }
    if (seen_levels != 63) FAIL("levels seen: %d", seen_levels);
    return true;
}

static bool check_rank_order(std::mt19937_64 &rng, unsigned long *n_checked)
{
    for (int round = 0; round < 40; round++) {
        const size_t n = 1 + rng() % 3000;
        std::vector<int> lvl(n), bin(n);
        std::vector<uint32_t> key(n);
        for (size_t i = 0; i < n; i++) {
            // few distinct places: many ties in (level, bin)
            const int lv = (int)(rng() % 6);
            const int64_t w = (int64_t)1 << (17 + 3 * lv);
            const int64_t s = ((int64_t)(rng() % 6) * w) % 0x7fff0000LL;
            const int64_t e = std::min<int64_t>(s + 1 + (int64_t)(rng() % (uint64_t)w), 0x7fffffffLL);
            if (!tb_bin_of_range((int)s, (int)e, &lvl[i], &bin[i])) FAIL("no bin for %lld-%lld", (long long)s, (long long)e);
            key[i] = tb_rank_key(lvl[i], bin[i]);
        }
        std::vector<uint32_t> canon(n), by_key(n);
        for (size_t i = 0; i < n; i++) canon[i] = by_key[i] = (uint32_t)i;
        std::sort(canon.begin(), canon.end(), [&](uint32_t a, uint32_t b) {           // the host build's comparison
            if (lvl[a] != lvl[b]) return lvl[a] > lvl[b];
            if (bin[a] != bin[b]) return bin[a] > bin[b];
            return a < b;
        });
        std::stable_sort(by_key.begin(), by_key.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
        if (canon != by_key) FAIL("round %d: the stable order by rank key differs from (level desc, bin desc, file order)", round);
        *n_checked += n;
    }
    return true;
}

static bool check_passes(void)
{
    const struct {
        uint64_t k;
        uint32_t p;
    } c[] = {{0, 1}, {1, 1}, {255, 1}, {256, 2}, {65535, 2}, {65536, 3}, {(1u << TB_RANK_KEY_BITS) - 1, 3}, {0xffffff, 3}, {0x1000000, 4},
             {0x7fffffff, 4}, {0xffffffffULL, 4}, {0x100000000ULL, 5}, {~0ULL, 8}};
    for (auto &x : c)
        if (tb_key_passes(x.k) != x.p) FAIL("tb_key_passes(%llu) = %u, expected %u", (unsigned long long)x.k, tb_key_passes(x.k), x.p);
    return true;
}

// the host build's loop over start-sorted rows
static std::vector<int32_t> serial_pbelow(const std::vector<Row> &r)
{
    std::vector<int32_t> pb(r.size());
    int32_t pm = INT32_MIN, cur = r.empty() ? -1 : r[0].chrom;
    for (size_t k = 0; k < r.size(); k++) {
        if (r[k].chrom != cur) {
            cur = r[k].chrom;
            pm = INT32_MIN;
        }
        pb[k] = pm;
        pm = std::max(pm, r[k].end);
    }
    return pb;
}

// k_tb_runs on paper: workgroups of wg threads with rpt rows each, a doubling scan with tb_run_join, a serial carry over workgroups
static std::vector<int32_t> blocked_pbelow(const std::vector<Row> &r, size_t wg, size_t rpt)
{
    const size_t n = r.size(), per = wg * rpt, nb = (n + per - 1) / per;
    std::vector<int32_t> pb(n, 12345);
    std::vector<TbRun> totals(nb), carry(nb);
    std::vector<std::vector<TbRun>> scans(nb);
    for (size_t b = 0; b < nb; b++) {
        std::vector<TbRun> s(wg);
        for (size_t t = 0; t < wg; t++) {
            TbRun mine = tb_run_empty();
            for (size_t k = std::min(n, b * per + t * rpt); k < std::min(n, b * per + (t + 1) * rpt); k++) mine = tb_run_push(mine, r[k].chrom, r[k].end);
            s[t] = mine;
        }
        for (size_t d = 1; d < wg; d <<= 1) {
            std::vector<TbRun> nx = s;
            for (size_t t = d; t < wg; t++) nx[t] = tb_run_join(s[t - d], s[t]);
            s = nx;
        }
        totals[b] = s[wg - 1];
        scans[b] = s;
    }
    TbRun acc = tb_run_empty();
    for (size_t b = 0; b < nb; b++) {
        carry[b] = acc;
        acc = tb_run_join(acc, totals[b]);
    }
    for (size_t b = 0; b < nb; b++)
        for (size_t t = 0; t < wg; t++) {
            TbRun before = carry[b];
            if (t > 0) before = tb_run_join(before, scans[b][t - 1]);
            for (size_t k = std::min(n, b * per + t * rpt); k < std::min(n, b * per + (t + 1) * rpt); k++) {
                pb[k] = tb_run_below(before, r[k].chrom);
                before = tb_run_push(before, r[k].chrom, r[k].end);
            }
        }
    return pb;
}

static bool check_runs(std::mt19937_64 &rng, unsigned long *n_checked)
{
    for (int round = 0; round < 300; round++) {
        // chromosomes with 0, 1 or many rows; now and then an early long row whose end dominates for a long while
        const int n_chrom = 1 + (int)(rng() % 12);
        std::vector<Row> r;
        for (int c = 0; c < n_chrom; c++) {
            const size_t m = rng() % 4 == 0 ? rng() % 2 : rng() % 400;
            std::vector<Row> rc;
            for (size_t i = 0; i < m; i++) {
                const int s = (int)(rng() % 1000000);
                const int len = (i == 0 && rng() % 3 == 0) ? 2000000 : (int)(rng() % 3000);
                rc.push_back(Row{c, s, s + len});
            }
            if (m && rng() % 8 == 0) rc[0].end = 0x7fffffff;
            std::stable_sort(rc.begin(), rc.end(), [](const Row &a, const Row &b) { return a.start < b.start; });
            r.insert(r.end(), rc.begin(), rc.end());
        }
        const std::vector<int32_t> want = serial_pbelow(r);
        const size_t shapes[][2] = {{1, 1}, {2, 1}, {4, 3}, {8, 32}, {256, 32}, {4, 1 + (size_t)(rng() % 7)}};
        for (auto &sh : shapes) {
            const std::vector<int32_t> got = blocked_pbelow(r, sh[0], sh[1]);
            for (size_t k = 0; k < r.size(); k++)
                if (got[k] != want[k]) FAIL("round %d, %zu threads x %zu rows: pbelow[%zu] = %d, expected %d (chrom %d)", round, sh[0], sh[1], k, got[k], want[k], r[k].chrom);
        }
        *n_checked += r.size();
    }
    // joins in any grouping give the same summary: (a b) c == a (b c)
    for (int round = 0; round < 20000; round++) {
        TbRun x[3];
        for (auto &v : x) {
            v = tb_run_empty();
            const int m = (int)(rng() % 4);
            int c = (int)(rng() % 3);
            for (int i = 0; i < m; i++) {
                c += (int)(rng() % 2);
                v = tb_run_push(v, c, (int32_t)(rng() % 100) - 50);
            }
        }
        const TbRun l = tb_run_join(tb_run_join(x[0], x[1]), x[2]), q = tb_run_join(x[0], tb_run_join(x[1], x[2]));
        if (l.last_chrom != q.last_chrom || l.last_max != q.last_max || (l.last_chrom >= 0 && !l.one_chrom != !q.one_chrom)) FAIL("tb_run_join is not associative (round %d)", round);
    }
    return true;
}

int main(void)
{
    std::mt19937_64 rng(20240607);
    unsigned long bins = 0, ranks = 0, rows = 0;
    if (!check_bins(rng, &bins) || !check_rank_order(rng, &ranks) || !check_passes() || !check_runs(rng, &rows)) return 1;
    printf("ok %lu ranges, %lu ranked rows, %lu scanned rows\n", bins, ranks, rows);
    return 0;
}
