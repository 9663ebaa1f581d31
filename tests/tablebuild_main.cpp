// Stand-alone check of the repeat table's build without a GPU (tests/test_tablebuild.py builds and runs it, plain and with the
// address and undefined-behaviour sanitizers). First the rules of iteres_amd/csrc/itx_tablebuild.h that both builds call, each
// against a loop written out here, on random and boundary rows:
//   tb_bin_of_range  against binFromRangeBinKeeperExtended's loop written out here
//   tb_rank_key      a stable sort by the key from file order == std::sort by (level desc, bin desc, file order asc)
//   tb_key_passes    the 8-bit passes of a key
//   TbRun            pbelow from stretches of any length joined in any grouping == the serial running maximum per chromosome,
//                    and the very decomposition k_tb_runs uses (threads of R rows, a doubling scan over the workgroup, a carry)
// Then the HOST build as a whole — tb_host_arrays of iteres_amd/csrc/itx_tablehost.h, the arrays ITX_TABLE_HOST=1 uploads and the
// oracle of the device build in tests/test_gpu_table_device.py — against a model of the table in the plainest form (model_table
// below: per chromosome a stable sort by start, an explicit sort for the ranks, a serial running maximum, a std::map of the
// triples, linear searches for the binned index and the windows' units), which shares nothing with the build but
// tb_bin_of_range. Every array and scalar is compared element by element on the shapes of that GPU test, on a table of more
// than 2 x 65 536 rows that the build cuts into several slices, and on its bad rows.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "../iteres_amd/csrc/itx_tablehost.h"

// the library's error message, as csrc/itx_basics.hip keeps it
static char g_err[512];
void itx_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

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

// ------------------------------------------------------------------------------------------------ the host build as a whole
struct Case {
    const char *name;
    std::vector<itx_row> rows;
    std::vector<int64_t> sizes;
    std::vector<uint32_t> rep_len;
    uint32_t n_fam, n_cla;
    size_t sampled_bins;               // 0: every bin of the binned index is checked; else that many, and those around every chromosome's first
};

// the table written out: what include/iteres_amd.h and the comments of ItxIv / ItxDevTable say it holds
struct Model {
    std::vector<ItxIv> iv;
    std::vector<int32_t> orig;
    std::vector<uint32_t> row_unit, part_unit, unit_first, unit_slot, chrom_off, bin_off;
    std::vector<TbQuad> unit_ids;
    std::vector<uint64_t> unit_covoff;
    uint64_t slots = 0, cov = 0;
    int shift = 0;
    long bad = -1;                     // the first row binKeeperAdd would refuse, or with ids out of range
    // bin b of chromosome c: the first row at or after the bin's first base, the first row whose prefix-maximum end passes it
    TbPair bin_entry(int c, uint32_t b) const
    {
        const int64_t bound = (int64_t)b << shift;
        TbPair p = {chrom_off[c + 1], chrom_off[c + 1]};
        for (uint32_t k = chrom_off[c]; k < chrom_off[c + 1]; k++)
            if ((int64_t)iv[k].s >= bound) {
                p.x = k;
                break;
            }
        int64_t reach = INT64_MIN;
        for (uint32_t k = chrom_off[c]; k < chrom_off[c + 1]; k++) {
            reach = std::max(reach, (int64_t)iv[k].e);
            if (reach > bound) {
                p.y = k;
                break;
            }
        }
        return p;
    }
};

static Model model_table(const Case &cs)
{
    Model M;
    const size_t n = cs.rows.size();
    const int n_chrom = (int)cs.sizes.size();
    const uint32_t n_rep = (uint32_t)cs.rep_len.size();
    std::vector<int> level(n), bin(n);
    for (size_t i = 0; i < n && M.bad < 0; i++) {
        const itx_row &r = cs.rows[i];
        bool ok = r.chrom >= 0 && r.chrom < n_chrom && r.rep < n_rep && r.fam < cs.n_fam && r.cla < cs.n_cla;
        if (ok) {
            const int64_t size = cs.sizes[r.chrom];
            ok = size != 0 && r.start <= 0x7fffffffu && r.start <= r.end && (int64_t)r.end <= size && ref_bin_of_range((int)r.start, (int)r.end, &level[i], &bin[i]);
        }
        if (!ok) M.bad = (long)i;
    }
    if (M.bad >= 0) return M;
    // units: the distinct triples in order; a name's units are neighbours
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, uint32_t> units;
    for (const itx_row &r : cs.rows) units[std::make_tuple(r.rep, r.fam, r.cla)] = 0;
    std::vector<uint64_t> name_cov(n_rep + 1, 0);
    for (uint32_t r = 0; r < n_rep; r++) name_cov[r + 1] = name_cov[r] + cs.rep_len[r];
    M.cov = name_cov[n_rep];
    std::vector<uint32_t> units_of_name(n_rep, 0);
    for (auto &u : units) units_of_name[std::get<0>(u.first)]++;
    M.unit_first.assign(n_rep + 1, 0);
    for (auto &u : units) {
        const uint32_t rep = std::get<0>(u.first), k = (uint32_t)M.unit_ids.size();
        u.second = k;
        if (k == 0 || M.unit_ids[k - 1].x != rep) M.unit_first[rep] = k;
        M.unit_ids.push_back(TbQuad{rep, std::get<1>(u.first), std::get<2>(u.first), units_of_name[rep] == 1 ? 1u : 0u});
        M.unit_slot.push_back((uint32_t)M.slots);
        M.unit_covoff.push_back(name_cov[rep]);
        M.slots += (uint64_t)cs.rep_len[rep] + 1;
    }
    M.unit_slot.push_back((uint32_t)M.slots);
    // bins of 128 bp .. 128 kb: the narrowest with which the genome, two spare bins per chromosome, fits 1.5 bins per row (65 536 at least)
    uint64_t genome = 0;
    for (int64_t s : cs.sizes) genome += (uint64_t)s;
    const uint64_t budget = std::max<uint64_t>(n + n / 2, 65536);
    for (M.shift = 7; M.shift < 17; M.shift++)
        if ((genome >> M.shift) + 2 * (uint64_t)n_chrom <= budget) break;
    M.bin_off.assign(1, 0);
    for (int64_t s : cs.sizes) M.bin_off.push_back(M.bin_off.back() + (uint32_t)((uint64_t)s >> M.shift) + 2);
    // rows, chromosome by chromosome
    M.chrom_off.assign(1, 0);
    for (int c = 0; c < n_chrom; c++) {
        std::vector<uint32_t> by_start, by_rank;
        for (size_t i = 0; i < n; i++)
            if (cs.rows[i].chrom == c) by_start.push_back((uint32_t)i);
        by_rank = by_start;
        std::stable_sort(by_start.begin(), by_start.end(), [&](uint32_t a, uint32_t b) { return cs.rows[a].start < cs.rows[b].start; });
        std::sort(by_rank.begin(), by_rank.end(), [&](uint32_t a, uint32_t b) {
            return std::make_tuple(-level[a], -bin[a], a) < std::make_tuple(-level[b], -bin[b], b);
        });
        std::map<uint32_t, uint32_t> rank;
        for (size_t k = 0; k < by_rank.size(); k++) rank[by_rank[k]] = (uint32_t)k;
        int32_t below = INT32_MIN;
        for (uint32_t i : by_start) {
            const itx_row &r = cs.rows[i];
            const uint32_t u = units[std::make_tuple(r.rep, r.fam, r.cla)], len = cs.rep_len[r.rep];
            ItxIv d;
            d.s = (int32_t)r.start;
            d.e = (int32_t)r.end;
            d.pbelow = below;
            d.rank = rank[i];
            d.cs = r.cons_start;
            d.jcap = std::min(r.cons_end, len);
            d.covslot = M.unit_slot[u];
            d.zslot = M.unit_slot[u] + len;
            below = std::max(below, d.e);
            M.iv.push_back(d);
            M.orig.push_back((int32_t)i);
            M.row_unit.push_back(u);
        }
        M.chrom_off.push_back((uint32_t)M.iv.size());
    }
    // the first unit that reaches into every window of 8192 slots, two windows to spare
    for (uint64_t w = 0; w < (M.slots >> 13) + 2; w++) {
        uint32_t u = 0;
        while (u < M.unit_ids.size() && (uint64_t)M.unit_slot[u + 1] <= w * 8192) u++;
        M.part_unit.push_back(u);
    }
    return M;
}

static std::string show(uint32_t v) { return std::to_string(v); }
static std::string show(int32_t v) { return std::to_string(v); }
static std::string show(uint64_t v) { return std::to_string(v); }
static std::string show(const TbPair &v) { return "(" + std::to_string(v.x) + ", " + std::to_string(v.y) + ")"; }
static std::string show(const TbQuad &v) { return "(" + std::to_string(v.x) + ", " + std::to_string(v.y) + ", " + std::to_string(v.z) + ", " + std::to_string(v.w) + ")"; }
static std::string show(const ItxIv &v)
{
    return "{s " + std::to_string(v.s) + " e " + std::to_string(v.e) + " pbelow " + std::to_string(v.pbelow) + " rank " + std::to_string(v.rank) + " cs " + std::to_string(v.cs) +
           " jcap " + std::to_string(v.jcap) + " covslot " + std::to_string(v.covslot) + " zslot " + std::to_string(v.zslot) + "}";
}
template <class T>
static bool same_array(const char *cs, const char *what, const std::vector<T> &got, const std::vector<T> &want)
{
    if (got.size() != want.size()) FAIL("%s: %s has %zu elements, the model %zu", cs, what, got.size(), want.size());
    for (size_t k = 0; k < got.size(); k++)
        if (memcmp(&got[k], &want[k], sizeof(T)) != 0) FAIL("%s: %s[%zu] = %s, the model has %s", cs, what, k, show(got[k]).c_str(), show(want[k]).c_str());
    return true;
}

static bool check_case(const Case &cs, std::mt19937_64 &rng, unsigned long *n_rows, unsigned long *n_bins)
{
    const Model M = model_table(cs);
    const int n_chrom = (int)cs.sizes.size();
    TbHostArrays A;
    size_t bad = 77;
    g_err[0] = 0;
    int rc = tb_check_args(cs.rows.data(), cs.rows.size(), cs.sizes.data(), n_chrom, cs.rep_len.data(), (uint32_t)cs.rep_len.size(), &A);
    if (rc != ITX_OK) FAIL("%s: tb_check_args %d (%s)", cs.name, rc, g_err);
    rc = tb_host_arrays(cs.rows.data(), cs.rows.size(), cs.sizes.data(), n_chrom, cs.rep_len.data(), (uint32_t)cs.rep_len.size(), cs.n_fam, cs.n_cla, A, &bad);
    if (M.bad >= 0) {
        const itx_row &r = cs.rows[M.bad];
        char want[512];
        snprintf(want, sizeof want, "itx_table_create: row %ld (chrom %d, %u-%u) is outside its chromosome or has bad ids", M.bad, r.chrom, r.start, r.end);
        if (rc != ITX_E_RANGE || bad != (size_t)M.bad || strcmp(g_err, want) != 0)
            FAIL("%s: code %d, bad row %zu, \"%s\"; expected code %d, bad row %ld, \"%s\"", cs.name, rc, bad, g_err, ITX_E_RANGE, M.bad, want);
        return true;
    }
    if (rc != ITX_OK || bad != 77) FAIL("%s: code %d (%s), bad row %zu", cs.name, rc, g_err, bad);
    if (A.shift != M.shift) FAIL("%s: shift %d, the model has %d", cs.name, A.shift, M.shift);
    if (A.U.n != M.unit_ids.size() || A.U.slots != M.slots || A.U.cov != M.cov)
        FAIL("%s: %u units, %llu slots, coverage %llu; the model has %zu, %llu, %llu", cs.name, A.U.n, (unsigned long long)A.U.slots, (unsigned long long)A.U.cov, M.unit_ids.size(),
             (unsigned long long)M.slots, (unsigned long long)M.cov);
    if (!same_array(cs.name, "chrom_off", A.chrom_off, M.chrom_off) || !same_array(cs.name, "bin_off", A.bin_off, M.bin_off) ||
        !same_array(cs.name, "unit_ids", A.U.ids, M.unit_ids) || !same_array(cs.name, "unit_first", A.U.first, M.unit_first) ||
        !same_array(cs.name, "unit_slot", A.U.slot, M.unit_slot) || !same_array(cs.name, "unit_covoff", A.U.covoff, M.unit_covoff) ||
        !same_array(cs.name, "iv", A.iv, M.iv) || !same_array(cs.name, "orig", A.orig, M.orig) || !same_array(cs.name, "row_unit", A.row_unit, M.row_unit) ||
        !same_array(cs.name, "part_unit", A.part_unit, M.part_unit))
        return false;
    if (A.bl.size() != M.bin_off[n_chrom]) FAIL("%s: bl has %zu bins, the model %u", cs.name, A.bl.size(), M.bin_off[n_chrom]);
    for (int c = 0; c < n_chrom; c++) {
        const uint32_t nb = M.bin_off[c + 1] - M.bin_off[c];
        std::vector<uint32_t> which;
        if (cs.sampled_bins == 0) {
            for (uint32_t b = 0; b < nb; b++) which.push_back(b);
        } else {
            for (uint32_t b = 0; b < nb && b < 3; b++) which.push_back(b), which.push_back(nb - 1 - b);      // next to the chromosome's ends
            for (size_t k = 0; k < cs.sampled_bins * nb / M.bin_off[n_chrom]; k++) which.push_back((uint32_t)(rng() % nb));
        }
        for (uint32_t b : which) {
            const TbPair got = A.bl[M.bin_off[c] + b], want = M.bin_entry(c, b);
            if (got.x != want.x || got.y != want.y)
                FAIL("%s: bl[%u] (chromosome %d, bin %u) = %s, the model has %s", cs.name, M.bin_off[c] + b, c, b, show(got).c_str(), show(want).c_str());
        }
        *n_bins += which.size();
    }
    *n_rows += cs.rows.size();
    return true;
}

static itx_row row_of(int chrom, int64_t start, int64_t end, uint32_t cons_start, uint32_t cons_end, uint32_t rep, uint32_t fam, uint32_t cla)
{
    itx_row r = {chrom, (uint32_t)start, (uint32_t)end, cons_start, cons_end, rep, fam, cla};
    return r;
}
// n valid rows over the chromosomes in random file order, as random_rows of tests/test_gpu_table_device.py makes them;
// n_starts: that few distinct starts per chromosome (ties)
static Case random_case(const char *name, std::mt19937_64 &rng, size_t n, const std::vector<int64_t> &sizes, uint32_t n_rep = 37, int64_t max_len = 3000, int64_t n_starts = 0)
{
    Case cs = {name, {}, sizes, {}, 5, 3, 0};
    std::vector<int> ok;
    for (size_t c = 0; c < sizes.size(); c++)
        if (sizes[c] > 1) ok.push_back((int)c);
    for (size_t i = 0; i < n; i++) {
        const int c = ok[rng() % ok.size()];
        int64_t start = (int64_t)(rng() % (uint64_t)(sizes[c] - 1));
        if (n_starts) start -= start % std::max<int64_t>(sizes[c] / n_starts, 1);
        const int64_t end = std::min<int64_t>(start + 1 + (int64_t)(rng() % (uint64_t)max_len), sizes[c]);
        const uint32_t rep = (uint32_t)(rng() % n_rep);
        cs.rows.push_back(row_of(c, start, end, (uint32_t)(rng() % 50), (uint32_t)(rng() % 400), rep, rep % 5, rep % 3));
    }
    for (uint32_t r = 0; r < n_rep; r++) cs.rep_len.push_back(1 + (uint32_t)(rng() % 299));
    return cs;
}

static bool check_host_build(std::mt19937_64 &rng, unsigned long *n_rows, unsigned long *n_bins, unsigned long *n_bad)
{
    std::vector<Case> cases;
    {   // a name with two pairs first seen out of order, a name of length 0, an unused name
        Case cs = {"units", {}, {100000}, {50, 0, 9, 20}, 3, 2, 0};
        const uint32_t rep[8] = {0, 3, 0, 1, 0, 3, 1, 0}, fam[8] = {1, 2, 0, 0, 1, 2, 0, 0}, cla[8] = {0, 1, 0, 1, 0, 1, 1, 0};
        for (int i = 0; i < 8; i++) cs.rows.push_back(row_of(0, i * 100, i * 100 + 250, 0, 60, rep[i], fam[i], cla[i]));
        cases.push_back(cs);
    }
    cases.push_back(Case{"no rows", {}, {1000, 70000}, {5, 6}, 1, 1, 0});
    {   // about 300 chromosomes: some without rows, some with one, one of size 0
        std::vector<int64_t> sizes;
        for (int c = 0; c < 300; c++) sizes.push_back(2000 + (int64_t)(rng() % 58000));
        sizes[7] = 0;
        Case cs = random_case("300 chromosomes", rng, 9000, sizes);
        std::vector<itx_row> kept;
        bool seen[300] = {false};
        for (const itx_row &r : cs.rows) {
            const int c = r.chrom;
            if (c == 0 || c == 11 || c == 255 || c == 256 || c == 299) continue;
            if ((c == 1 || c == 257 || c == 298) && seen[c]) continue;
            seen[c] = true;
            kept.push_back(r);
        }
        cs.rows = kept;
        cases.push_back(cs);
    }
    // ties in both orders: a few dozen distinct starts and bins over a few thousand rows
    cases.push_back(random_case("ties", rng, 6000, {3000000, 700000}, 37, 200000, 40));
    {   // a slot space of many windows of 2^13 slots; the first unit ends exactly where the second window begins
        Case cs = random_case("windows", rng, 3000, {2000000}, 600);
        for (uint32_t &len : cs.rep_len) len *= 40;
        cs.rep_len[0] = 8191;
        cs.rows[0].rep = cs.rows[0].fam = cs.rows[0].cla = 0;
        cases.push_back(cs);
    }
    {   // all six bin levels on chromosomes of 2^31 - 1 (the widest bins, shift 17)
        const int64_t size = 0x7fffffff;
        Case cs = {"six levels", {}, {size, size, size}, {120, 0, 40, 7}, 4, 4, 0};
        std::vector<std::pair<int64_t, int64_t>> se;
        for (int lv = 1; lv <= 5; lv++)
            for (int64_t m = 1; m <= 3; m += 2) {
                const int64_t b = ((int64_t)1 << (14 + 3 * lv)) * m;
                if (b >= size) continue;
                se.insert(se.end(), {{b - 10, b + 10}, {b - 1, b + 1}, {b, b + 7}, {b - 5000, b}});
            }
        se.insert(se.end(), {{0, 1}, {5, 100}, {size - 1, size}, {0, size}, {(int64_t)1 << 30, ((int64_t)1 << 30) + 50}});
        std::shuffle(se.begin(), se.end(), rng);
        for (auto &x : se) {
            const uint32_t rep = (uint32_t)(rng() % 4);
            cs.rows.push_back(row_of((int)(rng() % 3), x.first, x.second, 0, 100, rep, rep, rep));
        }
        int levels = 0, lv, bn;
        for (const itx_row &r : cs.rows)
            if (ref_bin_of_range((int)r.start, (int)r.end, &lv, &bn)) levels |= 1 << lv;
        if (levels != 63) FAIL("six levels: levels seen %d", levels);
        cases.push_back(cs);
    }
    {   // more than 2 x 65 536 rows: the build cuts them into slices. Chromosome 0 ends inside a slice; chromosome 1 begins with a row
        // that reaches its end, so that row's end is pbelow of every later row of the chromosome, across the following slices
        const size_t n0 = 70017, n1 = 80000, n2 = 100;
        Case cs = {"slices", {}, {4000000, 9000000, 50000}, std::vector<uint32_t>(9, 77), 2, 1, 3000};
        for (size_t i = 0; i < n0 + n1 + n2; i++) {
            const int c = i < n0 ? 0 : i < n0 + n1 ? 1 : 2;
            const int64_t start = 200 + (int64_t)(rng() % (uint64_t)(cs.sizes[c] - 400));
            const uint32_t rep = (uint32_t)(rng() % 9);
            cs.rows.push_back(row_of(c, start, start + 1 + (int64_t)(rng() % 149), 0, 90, rep, rep % 2, 0));
        }
        cs.rows[n0].start = 0;
        cs.rows[n0].end = (uint32_t)cs.sizes[1];
        std::shuffle(cs.rows.begin(), cs.rows.end(), rng);
        cases.push_back(cs);
    }
    {   // bad rows: the first is reported whatever follows it, and each kind alone
        const Case good = random_case("bad rows", rng, 20000, {500000, 80000});
        for (int only = -1; only < 4; only++) {
            Case cs = good;
            if (only < 0 || only == 0) cs.rows[15000].end = (uint32_t)cs.sizes[cs.rows[15000].chrom] + 1;      // past its chromosome
            if (only < 0 || only == 1) cs.rows[4321].rep = 1000;                                              // no such name: the FIRST bad row
            if (only < 0 || only == 2) cs.rows[19999].chrom = 2;                                              // no such chromosome
            if (only < 0 || only == 3) cs.rows[4322].start = cs.rows[4322].end = 0;                           // empty at 0: fits no bin
            const long want[5] = {4321, 15000, 4321, 19999, 4322};
            if (model_table(cs).bad != want[only + 1]) FAIL("bad rows: the model reports row %ld, expected %ld", model_table(cs).bad, want[only + 1]);
            cases.push_back(cs);
            ++*n_bad;
        }
    }
    for (const Case &cs : cases)
        if (!check_case(cs, rng, n_rows, n_bins)) return false;
    return true;
}

int main(void)
{
    std::mt19937_64 rng(20240607);
    unsigned long bins = 0, ranks = 0, rows = 0, built_rows = 0, built_bins = 0, bad = 0;
    if (!check_bins(rng, &bins) || !check_rank_order(rng, &ranks) || !check_passes() || !check_runs(rng, &rows)) return 1;
    if (!check_host_build(rng, &built_rows, &built_bins, &bad)) return 1;
    printf("ok %lu ranges, %lu ranked rows, %lu scanned rows; host build against the model: %lu rows, %lu bins, %lu bad-row cases\n", bins, ranks, rows, built_rows, built_bins,
           bad);
    return 0;
}
