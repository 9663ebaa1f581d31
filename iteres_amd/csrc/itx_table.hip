// itx_table.hip — builds the device-resident repeat table.
//
// Stands in for rmsk2binKeeperHash's per-chromosome binKeeper (generic.c:1613-1626,
// cuskent/binRange.c:140-186) plus each row's links into hashRep/hashFam/hashCla (generic.c:1631-1693).
// The reference answers "which rows overlap [start,end)" by walking six levels of LIFO bin lists; the
// order in which it RETURNS the hits matters (generic.c:950-960 picks "the last hit whose coverage
// beats the previous hit's"). Here the rows of a chromosome are one start-sorted array with
//   * a binned index `bl` (per 2^shift bp: first row starting in/after the bin, first row whose
//     prefix-max end passes the bin start) bounding the candidate range from both sides in O(1),
//   * a prefix-maximum of the ends of the rows below (pbelow) as the scan-stop bound, and
//   * each row's RANK in binKeeperFind's return order (level coarse->fine, bin descending,
//     insertion ascending — cuskent/binRange.c:209-225) so the kernel can replay the best-hit rule
//     exactly without the bin lists.
// Accumulation is per UNIT = distinct (repName, repFamily, repClass) triple of a row: the reference bumps
// the row's own family/class entries (generic.c:1010-1024), and repName -> family is not functional in
// rmsk, so counting per triple and summing at finish gives all three stat tables from one accumulator.
#include "itx_common.h"
#include "itx_radixsort.h"
#include "itx_tablebuild.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <atomic>
#include <numeric>
#include <thread>
#include <set>
#include <vector>

static thread_local char g_err[512];
void itx_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
extern "C" const char *itx_last_error(void) { return g_err; }
extern "C" int itx_abi_version(void) { return 1005; }
extern "C" int itx_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        itx_set_error("hipGetDeviceCount: %s", hipGetErrorString(e));
        return ITX_E_NO_DEVICE;
    }
    return n;
}

// (level and bin of a row: tb_bin_of_range, itx_tablebuild.h)

// for_each_chrom and for_slices serve the HOST build (ITX_TABLE_HOST=1) only: the device build starts no host thread.
// Runs fn(c) for every chromosome on a few host threads (chromosomes are independent in every sort below).
template <class F>
static void for_each_chrom(int n_chrom, F fn)
{
    unsigned nt = std::thread::hardware_concurrency();
    if (nt > 16) nt = 16;
    if (nt < 1) nt = 1;
    if ((int)nt > n_chrom) nt = n_chrom > 0 ? (unsigned)n_chrom : 1u;
    std::atomic<int> next{0};
    auto work = [&]() {
        for (int c = next.fetch_add(1); c < n_chrom; c = next.fetch_add(1)) fn(c);
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
}

// Runs fn(t, lo, hi) over n items cut into contiguous slices, one per host thread (at most 16, at least `grain` items each).
template <class F>
static size_t for_slices(size_t n, size_t grain, F fn)
{
    unsigned hw = std::thread::hardware_concurrency();
    size_t nt = hw ? hw : 1;
    if (nt > 16) nt = 16;
    if (nt > n / grain + 1) nt = n / grain + 1;
    std::vector<std::thread> th;
    for (size_t t = 1; t < nt; t++) th.emplace_back([&, t]() { fn(t, n * t / nt, n * (t + 1) / nt); });
    fn((size_t)0, (size_t)0, n / nt);
    for (auto &x : th) x.join();
    return nt;
}

struct Carver {
    size_t off = 0;
    size_t take(size_t bytes)
    {
        off = (off + 255) & ~size_t(255);
        size_t o = off;
        off += bytes;
        return o;
    }
};

#include <time.h>
static void tb_tick(const char *what, double *t0)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    const double t = (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
    if (getenv("ITX_TIMING_TABLE")) fprintf(stderr, "[itx timing] table: %s %.3f s\n", what, t - *t0);
    *t0 = t;
}

// ---- what the two builds below share: the checks of the arguments, the units from their triples, the bin width, the table object
static int tb_check_args(const itx_row *rows, size_t n_rows, const int64_t *chrom_size, int n_chrom, const uint32_t *rep_len, uint32_t n_rep, itx_table **out)
{
    if (!out || n_chrom < 0 || (n_rows && !rows) || (n_chrom && !chrom_size) || (n_rep && !rep_len)) {
        itx_set_error("itx_table_create: null argument");
        return ITX_E_ARG;
    }
    if (n_rows >= (1ull << 31)) {
        itx_set_error("itx_table_create: %zu rows exceed the 2^31 row limit", n_rows);
        return ITX_E_LIMIT;
    }
    for (int c = 0; c < n_chrom; c++)
        if (chrom_size[c] < 0 || chrom_size[c] > 0x7fffffffLL) {
            itx_set_error("itx_table_create: chromosome %d size %lld outside int range (binKeeperNew takes int)", c,
                          (long long)chrom_size[c]);
            return ITX_E_LIMIT;
        }
    return ITX_OK;
}

typedef std::array<uint32_t, 3> Triple;                    // (rep, fam, cla)
// The units: the distinct triples in (rep, fam, cla) order — the units of a name are neighbours —, each with its slot range
// (rep_len + 1 slots), where its coverage lands and whether it is its name's only unit.
struct TbUnits {
    std::vector<uint4> ids;                                // (rep, fam, cla, solo)
    std::vector<uint32_t> first;                           // [n_rep + 1] the first unit of every name (names without rows: unused)
    std::vector<uint32_t> slot;                            // [n + 1]
    std::vector<uint64_t> covoff;                          // [n]
    uint32_t n = 0;
    uint64_t slots = 0, cov = 0;
};
static int tb_units(std::vector<Triple> &triples, const uint32_t *rep_len, uint32_t n_rep, TbUnits &U)
{
    std::sort(triples.begin(), triples.end());
    triples.erase(std::unique(triples.begin(), triples.end()), triples.end());
    U.n = (uint32_t)triples.size();
    U.ids.resize(U.n);
    U.first.assign((size_t)n_rep + 1, 0);
    for (size_t k = triples.size(); k-- > 0;) {
        U.ids[k] = make_uint4(triples[k][0], triples[k][1], triples[k][2], 0);
        U.first[triples[k][0]] = (uint32_t)k;
    }
    std::vector<uint64_t> covoff(n_rep + 1);
    for (uint32_t r = 0; r < n_rep; r++) {
        covoff[r] = U.cov;
        U.cov += rep_len[r];
    }
    U.slot.resize((size_t)U.n + 1);
    U.covoff.resize(U.n);
    for (uint32_t u = 0; u < U.n; u++) {
        U.slot[u] = (uint32_t)U.slots;
        U.slots += (uint64_t)rep_len[U.ids[u].x] + 1;
        if (U.slots >= (1ull << 30)) {
            itx_set_error("itx_table_create: consensus slot space exceeds 2^30");
            return ITX_E_LIMIT;
        }
        U.covoff[u] = covoff[U.ids[u].x];
        const bool prev_same = u > 0 && U.ids[u - 1].x == U.ids[u].x;
        const bool next_same = u + 1 < U.n && U.ids[u + 1].x == U.ids[u].x;
        U.ids[u].w = (prev_same || next_same) ? 0u : 1u;     // solo: the name's only unit
    }
    U.slot[U.n] = (uint32_t)U.slots;
    return ITX_OK;
}

// bin width: about one row per bin (128 bp .. 128 kb); bin_off[c]: where chromosome c's bins start
static int tb_bin_shift(size_t n_rows, const int64_t *chrom_size, int n_chrom, std::vector<uint32_t> &bin_off)
{
    uint64_t genome = 0;
    for (int c = 0; c < n_chrom; c++) genome += (uint64_t)chrom_size[c];
    int shift = 7;
    const uint64_t budget = std::max<uint64_t>((uint64_t)n_rows + (uint64_t)n_rows / 2, 1u << 16);
    while (shift < 17 && (genome >> shift) + 2 * (uint64_t)n_chrom > budget) shift++;
    bin_off.assign((size_t)n_chrom + 1, 0);
    for (int c = 0; c < n_chrom; c++) bin_off[c + 1] = bin_off[c] + (uint32_t)(((uint64_t)chrom_size[c] >> shift) + 2);
    return shift;
}

// where the table's arrays lie in its device allocation
struct TbLayout {
    size_t iv, orig, bl, runit, punit, uslot, uids, ucov, bytes, n_win;
};
static TbLayout tb_layout(Carver &cv, size_t n_rows, size_t n_bins, uint64_t slots, uint32_t n_units)
{
    TbLayout L;
    L.n_win = ((size_t)slots >> ITX_LOGW) + 2;             // windows of 2^ITX_LOGW slots (k_hist sums the starts of a window per unit)
    L.iv = cv.take((n_rows + 1) * sizeof(ItxIv));
    L.orig = cv.take((n_rows + 1) * 4);
    L.bl = cv.take((n_bins + 1) * sizeof(uint2));
    L.runit = cv.take((n_rows + 1) * 4);
    L.punit = cv.take(L.n_win * 4);
    L.uslot = cv.take(((size_t)n_units + 1) * 4);
    L.uids = cv.take(((size_t)n_units + 1) * sizeof(uint4));
    L.ucov = cv.take(((size_t)n_units + 1) * 8);
    L.bytes = cv.take(0) + 256;
    return L;
}

// the table object over a filled allocation
static itx_table *tb_object(char *base, const TbLayout &L, int device, int shift, size_t n_rows, const int64_t *chrom_size, int n_chrom, const uint32_t *rep_len, uint32_t n_rep,
                            uint32_t n_fam, uint32_t n_cla, const TbUnits &U, const std::vector<uint32_t> &chrom_off, const std::vector<uint32_t> &bin_off)
{
    itx_table *t = new itx_table();
    memset(t, 0, sizeof *t);
    t->device = device;
    t->n_chrom = n_chrom;
    t->shift = shift;
    t->n_rows = (uint32_t)n_rows;
    t->n_rep = n_rep;
    t->n_fam = n_fam;
    t->n_cla = n_cla;
    t->n_units = U.n;
    t->n_slots = (uint32_t)U.slots;
    t->cov_len = U.cov;
    t->d_all = base;
    t->table_bytes = L.bytes;
    t->dev.iv = (const ItxIv *)(base + L.iv);
    t->dev.orig = (const int32_t *)(base + L.orig);
    t->dev.bl = (const uint2 *)(base + L.bl);
    t->dev.row_unit = (const uint32_t *)(base + L.runit);
    t->dev.unit_slot = (const uint32_t *)(base + L.uslot);
    t->dev.part_unit = (const uint32_t *)(base + L.punit);
    t->dev.shift = shift;
    t->dev.n_rows = (uint32_t)n_rows;
    t->dev.n_units = U.n;
    t->dev.n_slots = (uint32_t)U.slots;
    t->d_unit_slot = (uint32_t *)(base + L.uslot);
    t->d_row_unit = (uint32_t *)(base + L.runit);
    t->d_part_unit = (uint32_t *)(base + L.punit);
    t->d_unit_ids = (uint4 *)(base + L.uids);
    t->d_unit_covoff = (uint64_t *)(base + L.ucov);
    t->h_rep_len = (uint32_t *)malloc(sizeof(uint32_t) * (n_rep + 1));
    if (n_rep) memcpy(t->h_rep_len, rep_len, sizeof(uint32_t) * n_rep);
    t->h_chrom_off = (uint32_t *)malloc(sizeof(uint32_t) * (n_chrom + 1));
    t->h_bin_off = (uint32_t *)malloc(sizeof(uint32_t) * (n_chrom + 1));
    t->h_chrom_size = (int32_t *)malloc(sizeof(int32_t) * (n_chrom + 1));
    memcpy(t->h_chrom_off, chrom_off.data(), sizeof(uint32_t) * (n_chrom + 1));
    memcpy(t->h_bin_off, bin_off.data(), sizeof(uint32_t) * (n_chrom + 1));
    for (int c = 0; c < n_chrom; c++) t->h_chrom_size[c] = (int32_t)chrom_size[c];
    return t;
}

// The host build: every stage on host threads, eight uploads at the end. Kept, unchanged in what it computes, as the oracle of
// the device build below (ITX_TABLE_HOST=1).
static int table_create_host(const itx_row *rows, size_t n_rows, const int64_t *chrom_size, int n_chrom,
                             const uint32_t *rep_len, uint32_t n_rep, uint32_t n_fam, uint32_t n_cla, int device,
                             itx_table **out, size_t *bad_row)
{
    int rc = tb_check_args(rows, n_rows, chrom_size, n_chrom, rep_len, n_rep, out);
    if (rc) return rc;
    double tb0 = 0;
    tb_tick("start", &tb0);
    // validate rows as binKeeperAdd would, bucket by chromosome (slices of the rows in parallel; the FIRST bad row is reported)
    std::vector<uint32_t> chrom_cnt(n_chrom + 1, 0);
    std::vector<int> lvl(n_rows), bin(n_rows);
    {
        std::vector<std::vector<uint32_t>> cnt_t(16, std::vector<uint32_t>((size_t)n_chrom + 1, 0));
        std::vector<size_t> bad_t(16, SIZE_MAX);
        for_slices(n_rows, 65536, [&](size_t t, size_t lo, size_t hi) {
            std::vector<uint32_t> &cc = cnt_t[t];
            for (size_t i = lo; i < hi; i++) {
                const itx_row &r = rows[i];
                bool ok = r.chrom >= 0 && r.chrom < n_chrom && (int)chrom_size[r.chrom] != 0 && r.rep < n_rep && r.fam < n_fam && r.cla < n_cla;
                if (ok) {
                    int s = (int)r.start, e = (int)r.end, maxPos = (int)chrom_size[r.chrom];
                    ok = !(s < 0 || e > maxPos || s > e) && tb_bin_of_range(s, e, &lvl[i], &bin[i]);
                }
                if (!ok) {
                    bad_t[t] = i;
                    return;
                }
                cc[(size_t)r.chrom + 1]++;
            }
        });
        size_t bad = SIZE_MAX;
        for (size_t t = 0; t < 16; t++) bad = std::min(bad, bad_t[t]);
        if (bad != SIZE_MAX) {
            const itx_row &r = rows[bad];
            if (bad_row) *bad_row = bad;
            itx_set_error("itx_table_create: row %zu (chrom %d, %u-%u) is outside its chromosome or has bad ids", bad, r.chrom, r.start, r.end);
            return ITX_E_RANGE;
        }
        for (size_t t = 0; t < 16; t++)
            for (int c = 0; c <= n_chrom; c++) chrom_cnt[(size_t)c] += cnt_t[t][(size_t)c];
    }
    tb_tick("validate + bucket", &tb0);
    // units: distinct (rep, fam, cla) triples, ordered by (rep, fam, cla). Nearly every repName has ONE family and class: a
    // slice of the rows remembers the first (fam, cla) it meets per name in a plain array, and only a row whose name has
    // been seen with another pair goes through a (small) set — no hashing per row (the per-row hash lookups of the first
    // version were 0.17 s of a 0.45 s build). The units of a name are neighbours in sorted order, so a row's unit is its
    // name's first unit plus a scan over that name's handful of units.
    std::vector<uint32_t> unit_of_row(n_rows);
    TbUnits U;
    {
        std::vector<std::vector<Triple>> found(16);
        for_slices(n_rows, 65536, [&](size_t t, size_t lo, size_t hi) {
            std::vector<uint64_t> first_fc((size_t)n_rep, 0);                 // (fam << 32 | cla) + 1 of the name's first row in this slice
            std::set<Triple> extra;                                            // triples beyond a name's first pair (few)
            for (size_t i = lo; i < hi; i++) {
                const uint64_t fc = ((uint64_t)rows[i].fam << 32 | rows[i].cla) + 1;
                uint64_t &f = first_fc[rows[i].rep];
                if (f == fc) continue;
                const Triple k = {rows[i].rep, rows[i].fam, rows[i].cla};
                if (f == 0) {
                    f = fc;
                    found[t].push_back(k);
                } else {
                    extra.insert(k);
                }
            }
            found[t].insert(found[t].end(), extra.begin(), extra.end());
        });
        std::vector<Triple> triples;
        for (auto &f : found) triples.insert(triples.end(), f.begin(), f.end());
        if ((rc = tb_units(triples, rep_len, n_rep, U))) return rc;
        for_slices(n_rows, 65536, [&](size_t, size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) {
                uint32_t u = U.first[rows[i].rep];
                while (U.ids[u].y != rows[i].fam || U.ids[u].z != rows[i].cla) u++;      // (the triple is there: it was collected above)
                unit_of_row[i] = u;
            }
        });
    }
    const uint32_t n_units = U.n;
    const std::vector<uint32_t> &unit_slot = U.slot;

    std::vector<uint32_t> chrom_off(n_chrom + 1, 0);
    for (int c = 0; c < n_chrom; c++) chrom_off[c + 1] = chrom_off[c] + chrom_cnt[c + 1];
    tb_tick("units", &tb0);
    // start-sorted order per chromosome (stable in file order)
    std::vector<uint32_t> order(n_rows);
    {
        std::vector<uint32_t> fill(chrom_off.begin(), chrom_off.end() - 1);
        for (size_t i = 0; i < n_rows; i++) order[fill[rows[i].chrom]++] = (uint32_t)i;
    }
    for_each_chrom(n_chrom, [&](int c) {
        std::stable_sort(order.begin() + chrom_off[c], order.begin() + chrom_off[c + 1],
                         [&](uint32_t a, uint32_t b) { return (int)rows[a].start < (int)rows[b].start; });
    });
    tb_tick("sort by start", &tb0);
    // rank in binKeeperFind's return order: level coarse (5) -> fine (0), bin descending, file order ascending
    std::vector<uint32_t> rank_of_row(n_rows);
    {
        std::vector<uint32_t> canon(n_rows);
        for_each_chrom(n_chrom, [&](int c) {
            uint32_t lo = chrom_off[c], hi = chrom_off[c + 1];
            std::copy(order.begin() + lo, order.begin() + hi, canon.begin() + lo);
            std::sort(canon.begin() + lo, canon.begin() + hi, [&](uint32_t a, uint32_t b) {
                if (lvl[a] != lvl[b]) return lvl[a] > lvl[b];
                if (bin[a] != bin[b]) return bin[a] > bin[b];
                return a < b;
            });
            for (uint32_t k = lo; k < hi; k++) rank_of_row[canon[k]] = k - lo;
        });
    }
    tb_tick("ranks", &tb0);
    std::vector<uint32_t> bin_off;
    const int shift = tb_bin_shift(n_rows, chrom_size, n_chrom, bin_off);
    std::vector<uint2> bl(bin_off[n_chrom]);
    std::vector<ItxIv> iv(n_rows);
    std::vector<int32_t> orig(n_rows);
    std::vector<uint32_t> row_unit(n_rows);
    // rows: slices of the sorted order in parallel. pbelow (the running maximum of the ends of a chromosome's rows below) crosses
    // slice boundaries: a first pass takes every slice's maximum over the rows of its LAST chromosome, a short serial pass turns
    // those into what each slice starts with, the second pass fills the rows. (One thread per chromosome left chr1's 8 % of the
    // rows to one thread: 0.09 s.)
    {
        struct SliceSum {
            int32_t last_chrom, last_max;      // the slice's last chromosome and the maximum end over its rows of it
            bool one_chrom;                    // the whole slice lies in that chromosome
        };
        std::vector<SliceSum> ss(16, SliceSum{-1, INT32_MIN, false});
        const size_t nt = for_slices(n_rows, 32768, [&](size_t t, size_t lo, size_t hi) {
            if (lo >= hi) return;
            const int32_t lc = rows[order[hi - 1]].chrom;
            int32_t mx = INT32_MIN;
            size_t k = hi;
            while (k > lo && rows[order[k - 1]].chrom == lc) {
                mx = std::max(mx, (int32_t)rows[order[k - 1]].end);
                k--;
            }
            ss[t] = SliceSum{lc, mx, k == lo};
        });
        std::vector<int32_t> carry_in(16, INT32_MIN);      // maximum end over the rows of the slice's FIRST chromosome that lie before the slice
        {
            int32_t cur_chrom = -1, cur_max = INT32_MIN;
            for (size_t t = 0; t < nt; t++) {
                const size_t lo = n_rows * t / nt, hi = n_rows * (t + 1) / nt;
                if (lo >= hi) continue;
                const int32_t fc = rows[order[lo]].chrom;
                carry_in[t] = fc == cur_chrom ? cur_max : INT32_MIN;
                if (ss[t].one_chrom && ss[t].last_chrom == cur_chrom) cur_max = std::max(cur_max, ss[t].last_max);
                else {
                    cur_chrom = ss[t].last_chrom;
                    cur_max = ss[t].last_max;
                }
            }
        }
        for_slices(n_rows, 32768, [&](size_t t, size_t lo, size_t hi) {
            int32_t pm = carry_in[t], cur = lo < hi ? rows[order[lo]].chrom : -1;
            for (size_t k = lo; k < hi; k++) {
                const itx_row &r = rows[order[k]];
                if (r.chrom != cur) {
                    cur = r.chrom;
                    pm = INT32_MIN;
                }
                ItxIv &d = iv[k];
                d.s = (int32_t)r.start;
                d.e = (int32_t)r.end;
                d.pbelow = pm;
                pm = std::max(pm, d.e);
                d.cs = r.cons_start;
                const uint32_t len = rep_len[r.rep];
                const uint32_t u = unit_of_row[order[k]];
                d.jcap = std::min(r.cons_end, len);
                d.covslot = unit_slot[u];
                d.zslot = unit_slot[u] + len;
                d.rank = rank_of_row[order[k]];
                orig[k] = (int32_t)order[k];
                row_unit[k] = u;
            }
        });
    }
    // the binned index: slices of ALL bins in parallel; a slice finds its place in the rows by bisection (starts and prefix-max
    // ends both rise along a chromosome) and sweeps on from there
    {
        const size_t n_bins = bin_off[n_chrom];
        auto pmax = [&](uint32_t r) { return std::max(iv[r].pbelow, iv[r].e); };
        for_slices(n_bins, 65536, [&](size_t, size_t g0, size_t g1) {
            int c = (int)(std::upper_bound(bin_off.begin(), bin_off.end(), (uint32_t)g0) - bin_off.begin()) - 1;
            uint32_t k = 0, m = 0;
            bool fresh = true;
            for (size_t g = g0; g < g1; g++) {
                while (g >= bin_off[c + 1]) {
                    c++;
                    fresh = true;
                }
                const uint32_t lo = chrom_off[c], hi = chrom_off[c + 1];
                const int64_t bound = (int64_t)(g - bin_off[c]) << shift;
                if (fresh) {
                    // first row starting at or after the bin; first row whose prefix-max end passes the bin start
                    uint32_t a = lo, b = hi;
                    while (a < b) {
                        const uint32_t mid = a + (b - a) / 2;
                        if ((int64_t)iv[mid].s < bound) a = mid + 1;
                        else b = mid;
                    }
                    k = a;
                    a = lo, b = hi;
                    while (a < b) {
                        const uint32_t mid = a + (b - a) / 2;
                        if ((int64_t)pmax(mid) <= bound) a = mid + 1;
                        else b = mid;
                    }
                    m = a;
                    fresh = false;
                } else {
                    while (k < hi && (int64_t)iv[k].s < bound) k++;
                    while (m < hi && (int64_t)pmax(m) <= bound) m++;
                }
                bl[g] = make_uint2(k, m);
            }
        });
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        itx_set_error("itx_table_create: HIP device %d not available (%d visible)", device, ndev);
        return ITX_E_NO_DEVICE;
    }
    tb_tick("rows + index", &tb0);
    ITX_HIP(hipSetDevice(device));
    Carver cv;
    const TbLayout L = tb_layout(cv, n_rows, bl.size(), U.slots, n_units);
    // first unit reaching into every window of 2^ITX_LOGW slots
    const size_t n_win = L.n_win;
    std::vector<uint32_t> part_unit(n_win, n_units);
    {
        uint32_t u = 0;
        for (size_t w = 0; w < n_win; w++) {
            while (u < n_units && (uint64_t)unit_slot[u + 1] <= ((uint64_t)w << ITX_LOGW)) u++;
            part_unit[w] = u;
        }
    }
    const size_t total = L.bytes;
    char *base = nullptr;
    hipError_t he = hipMalloc((void **)&base, total);
    if (he != hipSuccess) {
        itx_set_error("itx_table_create: hipMalloc(%zu) failed: %s", total, hipGetErrorString(he));
        return ITX_E_NOMEM;
    }
    auto up = [&](size_t off, const void *src, size_t bytes) -> bool {
        if (bytes == 0) return true;
        he = hipMemcpy(base + off, src, bytes, hipMemcpyHostToDevice);
        return he == hipSuccess;
    };
    bool ok = up(L.iv, iv.data(), iv.size() * sizeof(ItxIv)) &&
              up(L.orig, orig.data(), orig.size() * 4) && up(L.bl, bl.data(), bl.size() * sizeof(uint2)) &&
              up(L.runit, row_unit.data(), row_unit.size() * 4) && up(L.punit, part_unit.data(), part_unit.size() * 4) &&
              up(L.uslot, U.slot.data(), U.slot.size() * 4) && up(L.uids, U.ids.data(), U.ids.size() * sizeof(uint4)) &&
              up(L.ucov, U.covoff.data(), U.covoff.size() * 8);
    if (!ok) {
        itx_set_error("itx_table_create: upload failed: %s", hipGetErrorString(he));
        (void)hipFree(base);
        return ITX_E_NO_DEVICE;
    }
    itx_table *t = tb_object(base, L, device, shift, n_rows, chrom_size, n_chrom, rep_len, n_rep, n_fam, n_cla, U, chrom_off, bin_off);
    tb_tick("upload", &tb0);
    *out = t;
    return ITX_OK;
}

// ------------------------------------------------------------------------------------------------ the device build
// The same table, built where it will live: the rows cross the link once, both orders come from itx_sort_run, pbelow is a
// segmented running maximum across workgroups, the binned index one lane per bin. The calling thread validates the rows and
// finds the units in ONE pass (no host thread is started: the reader's copy threads and the decoder's producer need the cores
// at that moment), everything else runs on a stream of the build's own, which is waited for at the end — not the device.
#define TB_RUN_WG 256u
#define TB_RUN_ROWS 32u                                  // rows per thread of k_tb_runs
#define TB_RUN_BLOCK (TB_RUN_WG * TB_RUN_ROWS)

// file order, keyed for binKeeperFind's return order inside a chromosome
static __global__ __launch_bounds__(256) void k_tb_rank_keys(const itx_row *__restrict__ rows, uint32_t n, uint2 *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    int level = 0, bin = 0;
    (void)tb_bin_of_range((int)rows[i].start, (int)rows[i].end, &level, &bin);        // (the host's pass has vouched for the row)
    keys[i] = make_uint2(tb_rank_key(level, bin), i);
}
// file order, keyed by start
static __global__ __launch_bounds__(256) void k_tb_start_keys(const itx_row *__restrict__ rows, uint32_t n, uint2 *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) keys[i] = make_uint2(rows[i].start, i);
}
// the order so far, keyed by chromosome for the last passes
static __global__ __launch_bounds__(256) void k_tb_chrom_keys(const itx_row *__restrict__ rows, uint32_t n, uint2 *__restrict__ keys)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < n) keys[k].x = (uint32_t)rows[keys[k].y].chrom;
}
// rank = place inside the chromosome in the order by (chromosome, level desc, bin desc, file order)
static __global__ __launch_bounds__(256) void k_tb_ranks(const uint2 *__restrict__ keys, uint32_t n, const itx_row *__restrict__ rows,
                                                         const uint32_t *__restrict__ chrom_off, uint32_t *__restrict__ rank)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const uint32_t i = keys[k].y;
    rank[i] = k - chrom_off[rows[i].chrom];
}
// the records in (chromosome, start, file order) order, all but pbelow
static __global__ __launch_bounds__(256) void k_tb_rows(const uint2 *__restrict__ order, uint32_t n, const itx_row *__restrict__ rows, const uint32_t *__restrict__ rep_len,
                                                        const uint32_t *__restrict__ first_unit, const uint4 *__restrict__ unit_ids, const uint32_t *__restrict__ unit_slot,
                                                        uint32_t n_units, const uint32_t *__restrict__ rank, ItxIv *__restrict__ iv, int32_t *__restrict__ orig,
                                                        uint32_t *__restrict__ row_unit, int32_t *__restrict__ schrom)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const uint32_t i = order[k].y;
    const itx_row r = rows[i];
    uint32_t u = first_unit[r.rep];                                    // the units of a name are neighbours; the row's is among them
    while (u + 1 < n_units && (unit_ids[u].y != r.fam || unit_ids[u].z != r.cla)) u++;
    const uint32_t len = rep_len[r.rep];
    ItxIv d;
    d.s = (int32_t)r.start;
    d.e = (int32_t)r.end;
    d.pbelow = TB_NO_END;
    d.rank = rank[i];
    d.cs = r.cons_start;
    d.jcap = r.cons_end < len ? r.cons_end : len;
    d.covslot = unit_slot[u];
    d.zslot = unit_slot[u] + len;
    iv[k] = d;
    orig[k] = (int32_t)i;
    row_unit[k] = u;
    schrom[k] = r.chrom;
}
// pbelow. A workgroup takes TB_RUN_BLOCK sorted rows, a thread TB_RUN_ROWS of them in a row; the stretches' summaries (TbRun)
// are joined across the workgroup. WRITE false: the workgroup's own summary goes to totals; true: with what precedes the
// workgroup (carry, from k_tb_carry) every row gets the maximum end of its chromosome's rows below it.
template <bool WRITE>
static __global__ __launch_bounds__(TB_RUN_WG) void k_tb_runs(ItxIv *__restrict__ iv, const int32_t *__restrict__ schrom, uint32_t n, const TbRun *__restrict__ carry,
                                                              TbRun *__restrict__ totals)
{
    __shared__ TbRun s[TB_RUN_WG];
    const uint32_t t = threadIdx.x;
    const uint64_t lo0 = (uint64_t)blockIdx.x * TB_RUN_BLOCK + (uint64_t)t * TB_RUN_ROWS;
    const uint64_t lo = lo0 < n ? lo0 : n, hi = lo + TB_RUN_ROWS < n ? lo + TB_RUN_ROWS : n;
    TbRun mine = tb_run_empty();
    for (uint64_t k = lo; k < hi; k++) mine = tb_run_push(mine, schrom[k], iv[k].e);
    s[t] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < TB_RUN_WG; d <<= 1) {
        TbRun v = tb_run_empty();
        if (t >= d) v = s[t - d];
        __syncthreads();
        if (t >= d) s[t] = tb_run_join(v, s[t]);
        __syncthreads();
    }
    if (!WRITE) {
        if (t == TB_RUN_WG - 1) totals[blockIdx.x] = s[t];
        return;
    }
    TbRun before = carry[blockIdx.x];
    if (t > 0) before = tb_run_join(before, s[t - 1]);
    for (uint64_t k = lo; k < hi; k++) {
        const int32_t c = schrom[k], e = iv[k].e;
        iv[k].pbelow = tb_run_below(before, c);
        before = tb_run_push(before, c, e);
    }
}
// what precedes every workgroup of k_tb_runs: a few hundred summaries, one thread
static __global__ void k_tb_carry(const TbRun *__restrict__ totals, uint32_t n_blocks, TbRun *__restrict__ carry)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    TbRun acc = tb_run_empty();
    for (uint32_t b = 0; b < n_blocks; b++) {
        carry[b] = acc;
        acc = tb_run_join(acc, totals[b]);
    }
}
// the binned index, one lane per bin: both bounds are bisections (starts and prefix-max ends both rise along a chromosome)
static __global__ __launch_bounds__(256) void k_tb_bins(const ItxIv *__restrict__ iv, const uint32_t *__restrict__ chrom_off, const uint32_t *__restrict__ bin_off, uint32_t n_chrom,
                                                        uint32_t n_bins, int shift, uint2 *__restrict__ bl)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_bins) return;
    uint32_t a = 0, b = n_chrom + 1;                                   // the chromosome: the last whose bins start at or before g
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (bin_off[mid] <= g) a = mid + 1;
        else b = mid;
    }
    const uint32_t c = a - 1;
    const uint32_t lo = chrom_off[c], hi = chrom_off[c + 1];
    const int64_t bound = (int64_t)(g - bin_off[c]) << shift;
    a = lo, b = hi;                                                    // first row starting at or after the bin
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if ((int64_t)iv[mid].s < bound) a = mid + 1;
        else b = mid;
    }
    const uint32_t k = a;
    a = lo, b = hi;                                                    // first row whose prefix-max end passes the bin start
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        const int32_t pm = iv[mid].pbelow > iv[mid].e ? iv[mid].pbelow : iv[mid].e;
        if ((int64_t)pm <= bound) a = mid + 1;
        else b = mid;
    }
    bl[g] = make_uint2(k, a);
}
// first unit reaching into every window of 2^ITX_LOGW slots
static __global__ __launch_bounds__(256) void k_tb_part_unit(const uint32_t *__restrict__ unit_slot, uint32_t n_units, uint32_t n_win, uint32_t *__restrict__ part_unit)
{
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= n_win) return;
    const uint64_t bound = (uint64_t)w << ITX_LOGW;
    uint32_t a = 0, b = n_units;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if ((uint64_t)unit_slot[mid + 1] <= bound) a = mid + 1;
        else b = mid;
    }
    part_unit[w] = a;
}

// the build's stream, its stage events and (until the table owns it) its device memory
struct TbDevice {
    hipStream_t st = nullptr;
    char *base = nullptr;
    std::vector<std::pair<const char *, hipEvent_t>> marks;
    bool timing = getenv("ITX_TIMING_TABLE") != nullptr;
    ~TbDevice()
    {
        if (st) (void)hipStreamSynchronize(st);
        for (auto &m : marks) (void)hipEventDestroy(m.second);
        if (st) (void)hipStreamDestroy(st);
        if (base) (void)hipFree(base);
    }
    int mark(const char *what)
    {
        if (!timing) return ITX_OK;
        hipEvent_t e;
        ITX_HIP(hipEventCreate(&e));
        ITX_HIP(hipEventRecord(e, st));
        marks.emplace_back(what, e);
        return ITX_OK;
    }
    void report()
    {
        for (size_t k = 1; k < marks.size(); k++) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, marks[k - 1].second, marks[k].second) == hipSuccess)
                fprintf(stderr, "[itx timing] table: device %s %.3f ms\n", marks[k].first, (double)ms);
        }
    }
};
#define TB_GRID(n) dim3((unsigned)(((uint64_t)(n) + 255u) / 256u)), dim3(256)

// (chromosome, key) order of the n pairs of `from`, stable: the key's passes, then the chromosome's
static int tb_sort(hipStream_t st, const itx_row *d_rows, uint2 *from, uint2 *other, uint32_t n, uint32_t key_passes, uint32_t chrom_passes, uint32_t *hist,
                   uint2 **sorted)
{
    int rc = itx_sort_run(st, from, other, n, 0, key_passes, hist, sorted);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tb_chrom_keys, TB_GRID(n), 0, st, d_rows, n, *sorted);
    ITX_HIP(hipGetLastError());
    return itx_sort_run(st, *sorted, *sorted == from ? other : from, n, 0, chrom_passes, hist, sorted);
}

static int table_create_device(const itx_row *rows, size_t n_rows, const int64_t *chrom_size, int n_chrom,
                               const uint32_t *rep_len, uint32_t n_rep, uint32_t n_fam, uint32_t n_cla, int device,
                               itx_table **out, size_t *bad_row)
{
    int rc = tb_check_args(rows, n_rows, chrom_size, n_chrom, rep_len, n_rep, out);
    if (rc) return rc;
    int64_t max_size = 0;
    for (int c = 0; c < n_chrom; c++) max_size = std::max(max_size, chrom_size[c]);
    double tb0 = 0;
    tb_tick("start", &tb0);
    // ONE pass of the calling thread: every row validated as binKeeperAdd would (the first bad row is reported), counted into
    // its chromosome, and its (name, family, class) collected as in the host build: the first pair of a name in a plain array,
    // the few rows that disagree in a set
    std::vector<uint32_t> chrom_off(n_chrom + 1, 0);
    std::vector<Triple> triples;
    {
        std::vector<uint64_t> first_fc((size_t)n_rep, 0);
        std::set<Triple> extra;
        for (size_t i = 0; i < n_rows; i++) {
            const itx_row &r = rows[i];
            bool ok = r.chrom >= 0 && r.chrom < n_chrom && (int)chrom_size[r.chrom] != 0 && r.rep < n_rep && r.fam < n_fam && r.cla < n_cla;
            if (ok) {
                int s = (int)r.start, e = (int)r.end, maxPos = (int)chrom_size[r.chrom], level, bin;
                ok = !(s < 0 || e > maxPos || s > e) && tb_bin_of_range(s, e, &level, &bin);
            }
            if (!ok) {
                if (bad_row) *bad_row = i;
                itx_set_error("itx_table_create: row %zu (chrom %d, %u-%u) is outside its chromosome or has bad ids", i, r.chrom, r.start, r.end);
                return ITX_E_RANGE;
            }
            chrom_off[(size_t)r.chrom + 1]++;
            const uint64_t fc = ((uint64_t)r.fam << 32 | r.cla) + 1;
            uint64_t &f = first_fc[r.rep];
            if (f == fc) continue;
            const Triple k = {r.rep, r.fam, r.cla};
            if (f == 0) {
                f = fc;
                triples.push_back(k);
            } else {
                extra.insert(k);
            }
        }
        triples.insert(triples.end(), extra.begin(), extra.end());
    }
    for (int c = 0; c < n_chrom; c++) chrom_off[c + 1] += chrom_off[c];
    tb_tick("validate + count + units' triples (one host pass)", &tb0);
    TbUnits U;
    if ((rc = tb_units(triples, rep_len, n_rep, U))) return rc;
    const uint32_t n_units = U.n;
    std::vector<uint32_t> bin_off;
    const int shift = tb_bin_shift(n_rows, chrom_size, n_chrom, bin_off);
    const size_t n_bins = bin_off[n_chrom];
    tb_tick("units", &tb0);

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        itx_set_error("itx_table_create: HIP device %d not available (%d visible)", device, ndev);
        return ITX_E_NO_DEVICE;
    }
    ITX_HIP(hipSetDevice(device));
    const uint32_t n = (uint32_t)n_rows;
    const uint32_t n_runs = (uint32_t)(((uint64_t)n + TB_RUN_BLOCK - 1) / TB_RUN_BLOCK);
    // the table's arrays where they will live (as the host build lays them out), the build's working memory behind them
    Carver cv;
    const TbLayout L = tb_layout(cv, n_rows, n_bins, U.slots, n_units);
    const size_t n_win = L.n_win;
    cv.take(256);
    const size_t w_rows = cv.take((n_rows + 1) * sizeof(itx_row));
    const size_t w_ka = cv.take((n_rows + 1) * sizeof(uint2)), w_kb = cv.take((n_rows + 1) * sizeof(uint2));
    const size_t w_rank = cv.take((n_rows + 1) * 4), w_schrom = cv.take((n_rows + 1) * 4);
    const size_t w_hist = cv.take(itx_sort_hist_bytes(n_rows) + 1024);
    const size_t w_tot = cv.take(((size_t)n_runs + 1) * sizeof(TbRun)), w_carry = cv.take(((size_t)n_runs + 1) * sizeof(TbRun));
    const size_t w_coff = cv.take(((size_t)n_chrom + 1) * 4), w_boff = cv.take(((size_t)n_chrom + 1) * 4);
    const size_t w_rlen = cv.take(((size_t)n_rep + 1) * 4), w_funit = cv.take(((size_t)n_rep + 1) * 4);
    const size_t total = cv.take(0) + 256;
    TbDevice D;
    ITX_HIP(hipStreamCreateWithFlags(&D.st, hipStreamNonBlocking));
    hipError_t he = hipMalloc((void **)&D.base, total);
    if (he != hipSuccess) {
        D.base = nullptr;
        itx_set_error("itx_table_create: hipMalloc(%zu) failed: %s", total, hipGetErrorString(he));
        return ITX_E_NOMEM;
    }
    char *base = D.base;
    hipStream_t st = D.st;
    itx_row *d_rows = (itx_row *)(base + w_rows);
    uint2 *ka = (uint2 *)(base + w_ka), *kb = (uint2 *)(base + w_kb), *sorted = nullptr;
    uint32_t *d_rank = (uint32_t *)(base + w_rank), *d_hist = (uint32_t *)(base + w_hist);
    int32_t *d_schrom = (int32_t *)(base + w_schrom);
    uint32_t *d_coff = (uint32_t *)(base + w_coff), *d_boff = (uint32_t *)(base + w_boff), *d_rlen = (uint32_t *)(base + w_rlen),
             *d_funit = (uint32_t *)(base + w_funit);
    ItxIv *d_iv = (ItxIv *)(base + L.iv);
    uint32_t *d_uslot = (uint32_t *)(base + L.uslot);
    if ((rc = D.mark("start"))) return rc;
    // the one upload: the rows, and the few per-chromosome, per-name and per-unit numbers the host has just derived
    auto up = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    ITX_HIP(up(d_rows, rows, n_rows * sizeof(itx_row)));
    ITX_HIP(up(d_coff, chrom_off.data(), chrom_off.size() * 4));
    ITX_HIP(up(d_boff, bin_off.data(), bin_off.size() * 4));
    ITX_HIP(up(d_rlen, rep_len, (size_t)n_rep * 4));
    ITX_HIP(up(d_funit, U.first.data(), U.first.size() * 4));
    ITX_HIP(up(d_uslot, U.slot.data(), U.slot.size() * 4));
    ITX_HIP(up(base + L.uids, U.ids.data(), U.ids.size() * sizeof(uint4)));
    ITX_HIP(up(base + L.ucov, U.covoff.data(), U.covoff.size() * 8));
    if ((rc = D.mark("upload"))) return rc;
    const uint32_t chrom_passes = tb_key_passes(n_chrom > 0 ? (uint64_t)n_chrom - 1 : 0);
    if (n) {
        // ranks first: their order is only needed to number the rows, the buffers then serve the order by start
        hipLaunchKernelGGL(k_tb_rank_keys, TB_GRID(n), 0, st, d_rows, n, ka);
        ITX_HIP(hipGetLastError());
        if ((rc = tb_sort(st, d_rows, ka, kb, n, tb_key_passes((1ull << TB_RANK_KEY_BITS) - 1), chrom_passes, d_hist, &sorted))) return rc;
        hipLaunchKernelGGL(k_tb_ranks, TB_GRID(n), 0, st, sorted, n, d_rows, d_coff, d_rank);
        ITX_HIP(hipGetLastError());
        if ((rc = D.mark("ranks (sort by chromosome, level, bin)"))) return rc;
        hipLaunchKernelGGL(k_tb_start_keys, TB_GRID(n), 0, st, d_rows, n, ka);
        ITX_HIP(hipGetLastError());
        if ((rc = tb_sort(st, d_rows, ka, kb, n, tb_key_passes((uint64_t)max_size), chrom_passes, d_hist, &sorted))) return rc;
        if ((rc = D.mark("sort by chromosome, start"))) return rc;
        hipLaunchKernelGGL(k_tb_rows, TB_GRID(n), 0, st, sorted, n, d_rows, d_rlen, d_funit, (const uint4 *)(base + L.uids), d_uslot, n_units, d_rank, d_iv,
                           (int32_t *)(base + L.orig), (uint32_t *)(base + L.runit), d_schrom);
        ITX_HIP(hipGetLastError());
        TbRun *d_tot = (TbRun *)(base + w_tot), *d_carry = (TbRun *)(base + w_carry);
        hipLaunchKernelGGL(k_tb_runs<false>, dim3(n_runs), dim3(TB_RUN_WG), 0, st, d_iv, d_schrom, n, d_carry, d_tot);
        ITX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_tb_carry, dim3(1), dim3(64), 0, st, d_tot, n_runs, d_carry);
        ITX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_tb_runs<true>, dim3(n_runs), dim3(TB_RUN_WG), 0, st, d_iv, d_schrom, n, d_carry, d_tot);
        ITX_HIP(hipGetLastError());
        if ((rc = D.mark("rows + pbelow"))) return rc;
    }
    if (n_bins) {
        hipLaunchKernelGGL(k_tb_bins, TB_GRID(n_bins), 0, st, d_iv, d_coff, d_boff, (uint32_t)n_chrom, (uint32_t)n_bins, shift, (uint2 *)(base + L.bl));
        ITX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_tb_part_unit, TB_GRID(n_win), 0, st, d_uslot, n_units, (uint32_t)n_win, (uint32_t *)(base + L.punit));
    ITX_HIP(hipGetLastError());
    if ((rc = D.mark("binned index + windows' units"))) return rc;
    ITX_HIP(hipStreamSynchronize(st));                                 // the build's own stream: the host arrays above may go, the table may be used
    tb_tick("device build (upload, sorts, rows, index)", &tb0);
    if (D.timing) D.report();

    // (the working memory stays behind the arrays until the table goes: freeing it now would wait for everything else on the device)
    itx_table *t = tb_object(base, L, device, shift, n_rows, chrom_size, n_chrom, rep_len, n_rep, n_fam, n_cla, U, chrom_off, bin_off);
    D.base = nullptr;
    *out = t;
    return ITX_OK;
}

// ITX_TABLE_HOST=1: the host build, the oracle of the device build
extern "C" int itx_table_create(const itx_row *rows, size_t n_rows, const int64_t *chrom_size, int n_chrom,
                                const uint32_t *rep_len, uint32_t n_rep, uint32_t n_fam, uint32_t n_cla, int device,
                                itx_table **out, size_t *bad_row)
{
    const char *h = getenv("ITX_TABLE_HOST");
    return (h && atoi(h) != 0 ? table_create_host : table_create_device)(rows, n_rows, chrom_size, n_chrom, rep_len, n_rep, n_fam, n_cla, device, out, bad_row);
}

extern "C" int itx_table_debug_copy(const itx_table *t, int which, void *dst, size_t cap_bytes, size_t *bytes)
{
    if (!t || !bytes) {
        itx_set_error("itx_table_debug_copy: null argument");
        return ITX_E_ARG;
    }
    const size_t n_win = ((size_t)t->n_slots >> ITX_LOGW) + 2;
    const void *src = nullptr;
    size_t b = 0;
    bool host = false;
    switch (which) {
    case ITX_TABLE_IV: src = t->dev.iv, b = (size_t)t->n_rows * sizeof(ItxIv); break;
    case ITX_TABLE_ORIG: src = t->dev.orig, b = (size_t)t->n_rows * 4; break;
    case ITX_TABLE_BL: src = t->dev.bl, b = (size_t)t->h_bin_off[t->n_chrom] * sizeof(uint2); break;
    case ITX_TABLE_ROW_UNIT: src = t->d_row_unit, b = (size_t)t->n_rows * 4; break;
    case ITX_TABLE_PART_UNIT: src = t->d_part_unit, b = n_win * 4; break;
    case ITX_TABLE_UNIT_SLOT: src = t->d_unit_slot, b = ((size_t)t->n_units + 1) * 4; break;
    case ITX_TABLE_UNIT_IDS: src = t->d_unit_ids, b = (size_t)t->n_units * sizeof(uint4); break;
    case ITX_TABLE_UNIT_COVOFF: src = t->d_unit_covoff, b = (size_t)t->n_units * 8; break;
    case ITX_TABLE_CHROM_OFF: src = t->h_chrom_off, b = ((size_t)t->n_chrom + 1) * 4, host = true; break;
    case ITX_TABLE_BIN_OFF: src = t->h_bin_off, b = ((size_t)t->n_chrom + 1) * 4, host = true; break;
    default: itx_set_error("itx_table_debug_copy: unknown array %d", which); return ITX_E_ARG;
    }
    *bytes = b;
    if (!dst) return ITX_OK;
    if (cap_bytes < b) {
        itx_set_error("itx_table_debug_copy: %zu bytes do not hold array %d (%zu bytes)", cap_bytes, which, b);
        return ITX_E_ARG;
    }
    if (!b) return ITX_OK;
    if (host) {
        memcpy(dst, src, b);
        return ITX_OK;
    }
    ITX_HIP(hipSetDevice(t->device));
    ITX_HIP(hipMemcpy(dst, src, b, hipMemcpyDeviceToHost));
    return ITX_OK;
}

extern "C" void itx_table_destroy(itx_table *t)
{
    if (!t) return;
    if (t->d_all) {
        (void)hipSetDevice(t->device);
        (void)hipFree(t->d_all);
    }
    free(t->h_rep_len);
    free(t->h_chrom_off);
    free(t->h_bin_off);
    free(t->h_chrom_size);
    delete t;
}

extern "C" int itx_table_get_info(const itx_table *t, itx_table_info *o)
{
    if (!t || !o) {
        itx_set_error("itx_table_get_info: null argument");
        return ITX_E_ARG;
    }
    memset(o, 0, sizeof *o);
    o->n_rows = t->n_rows;
    o->n_rep = t->n_rep;
    o->n_fam = t->n_fam;
    o->n_cla = t->n_cla;
    o->cov_len = t->cov_len;
    o->n_units = t->n_units;
    o->n_slots = t->n_slots;
    o->table_bytes = t->table_bytes;
    o->n_chrom = t->n_chrom;
    o->bin_shift = t->shift;
    o->device = t->device;
    return ITX_OK;
}

extern "C" int itx_table_cov_offsets(const itx_table *t, uint64_t *off)
{
    if (!t || !off) {
        itx_set_error("itx_table_cov_offsets: null argument");
        return ITX_E_ARG;
    }
    uint64_t acc = 0;
    for (uint32_t r = 0; r < t->n_rep; r++) {
        off[r] = acc;
        acc += t->h_rep_len[r];
    }
    off[t->n_rep] = acc;
    return ITX_OK;
}
