// itx_tablehost.h — the host's side of the repeat table's build, plain C++ without a HIP call: what both builds do on the host
// (the checks of the arguments, the units from their triples, the bin width, the stage clock) and the HOST build's arrays
// (tb_host_arrays, ITX_TABLE_HOST=1: what every rank of a multi-GPU job runs, and the oracle of the device build), ready for
// csrc/itx_table_host.hip to upload. Every rule of the table comes from itx_tablebuild.h. tests/tablebuild_main.cpp compiles
// this file with g++ alone and holds tb_host_arrays against a model written out there.
#pragma once
#include "itx_tablebuild.h"

#include <time.h>
#include <algorithm>
#include <array>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <thread>
#include <vector>

void itx_set_error(const char *fmt, ...);                 // csrc/itx_basics.hip

// ITX_TIMING_TABLE: a line per stage of the build on stderr
static inline bool tb_timing(void) { return getenv("ITX_TIMING_TABLE") != nullptr; }
// the stage that ends here, on the calling thread's clock since its last tick
static inline void tb_tick(const char *what)
{
    static thread_local double t0 = 0;
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    const double t = (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
    if (tb_timing()) fprintf(stderr, "[itx timing] table: %s %.3f s\n", what, t - t0);
    t0 = t;
}

// for_each_chrom and for_slices serve the HOST build only: the device build starts no host thread.
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

// ---- what the two builds share on the host
static inline int tb_check_args(const itx_row *rows, size_t n_rows, const int64_t *chrom_size, int n_chrom, const uint32_t *rep_len, uint32_t n_rep, const void *out)
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

// row i failed tb_row_ok
static inline int tb_bad_row(const itx_row *rows, size_t i, size_t *bad_row)
{
    if (bad_row) *bad_row = i;
    itx_set_error("itx_table_create: row %zu (chrom %d, %u-%u) is outside its chromosome or has bad ids", i, rows[i].chrom, rows[i].start, rows[i].end);
    return ITX_E_RANGE;
}

typedef std::array<uint32_t, 3> Triple;                    // (rep, fam, cla)
// The distinct triples of the rows it is fed, and a few of them twice: nearly every repName has ONE family and class, so the
// first (fam, cla) met per name is remembered in a plain array and only a row whose name has been seen with another pair goes
// through a (small) set — no hashing per row (the per-row hash lookups of the first version were 0.17 s of a 0.45 s build).
struct TbTriples {
    std::vector<uint64_t> first_fc;                        // (fam << 32 | cla) + 1 of the name's first row
    std::set<Triple> extra;                                // triples beyond a name's first pair (few)
    std::vector<Triple> found;
    explicit TbTriples(uint32_t n_rep) : first_fc((size_t)n_rep, 0) {}
    // (inlined into the caller's loop over the rows, which nearly every row leaves at the first test)
    __attribute__((always_inline)) void add(const itx_row &r)
    {
        const uint64_t fc = ((uint64_t)r.fam << 32 | r.cla) + 1;
        uint64_t &f = first_fc[r.rep];
        if (f == fc) return;
        const Triple k = {r.rep, r.fam, r.cla};
        if (f == 0) {
            f = fc;
            found.push_back(k);
        } else {
            extra.insert(k);
        }
    }
    // everything found, behind what `to` holds
    void append_to(std::vector<Triple> &to) const
    {
        to.insert(to.end(), found.begin(), found.end());
        to.insert(to.end(), extra.begin(), extra.end());
    }
};
// the candidates of rows[lo, hi)
static inline void tb_triples(const itx_row *rows, size_t lo, size_t hi, uint32_t n_rep, std::vector<Triple> &to)
{
    TbTriples T(n_rep);
    for (size_t i = lo; i < hi; i++) T.add(rows[i]);
    T.append_to(to);
}

// The units: the distinct triples in (rep, fam, cla) order — the units of a name are neighbours —, each with its slot range
// (rep_len + 1 slots), where its coverage lands and whether it is its name's only unit.
struct TbUnits {
    std::vector<TbQuad> ids;                               // (rep, fam, cla, solo)
    std::vector<uint32_t> first;                           // [n_rep + 1] the first unit of every name (names without rows: unused)
    std::vector<uint32_t> slot;                            // [n + 1]
    std::vector<uint64_t> covoff;                          // [n]
    uint32_t n = 0;
    uint64_t slots = 0, cov = 0;
};
static inline int tb_units(std::vector<Triple> &triples, const uint32_t *rep_len, uint32_t n_rep, TbUnits &U)
{
    std::sort(triples.begin(), triples.end());
    triples.erase(std::unique(triples.begin(), triples.end()), triples.end());
    U.n = (uint32_t)triples.size();
    U.ids.resize(U.n);
    U.first.assign((size_t)n_rep + 1, 0);
    for (size_t k = triples.size(); k-- > 0;) {
        U.ids[k] = TbQuad{triples[k][0], triples[k][1], triples[k][2], 0};
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
static inline int tb_bin_shift(size_t n_rows, const int64_t *chrom_size, int n_chrom, std::vector<uint32_t> &bin_off)
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

// ------------------------------------------------------------------------------------------------ the host build's arrays
// Every array of the table as the device will hold it (ItxDevTable, itx_table), and what the table object keeps on the host.
struct TbHostArrays {
    std::vector<ItxIv> iv;                                 // [n_rows] (chromosome, start, file order)
    std::vector<int32_t> orig;                             // [n_rows]
    std::vector<TbPair> bl;                                // [bin_off[n_chrom]]
    std::vector<uint32_t> row_unit;                        // [n_rows]
    std::vector<uint32_t> part_unit;                       // [tb_n_windows(U.slots)]
    TbUnits U;
    std::vector<uint32_t> chrom_off, bin_off;              // [n_chrom + 1]
    int shift = 0;
};

// Every stage on host threads. The arguments are itx_table_create's and have passed tb_check_args; an error leaves A half filled.
static inline int tb_host_arrays(const itx_row *rows, size_t n_rows, const int64_t *chrom_size, int n_chrom, const uint32_t *rep_len, uint32_t n_rep, uint32_t n_fam,
                                 uint32_t n_cla, TbHostArrays &A, size_t *bad_row)
{
    int rc;
    tb_tick("start");
    // validate rows as binKeeperAdd would, bucket by chromosome (slices of the rows in parallel; the FIRST bad row is reported)
    std::vector<uint32_t> chrom_cnt(n_chrom + 1, 0);
    std::vector<int> lvl(n_rows), bin(n_rows);
    {
        std::vector<std::vector<uint32_t>> cnt_t(16, std::vector<uint32_t>((size_t)n_chrom + 1, 0));
        std::vector<size_t> bad_t(16, SIZE_MAX);
        for_slices(n_rows, 65536, [&](size_t t, size_t lo, size_t hi) {
            std::vector<uint32_t> &cc = cnt_t[t];
            for (size_t i = lo; i < hi; i++) {
                if (!tb_row_ok(rows[i], chrom_size, n_chrom, n_rep, n_fam, n_cla, &lvl[i], &bin[i])) {
                    bad_t[t] = i;
                    return;
                }
                cc[(size_t)rows[i].chrom + 1]++;
            }
        });
        size_t bad = SIZE_MAX;
        for (size_t t = 0; t < 16; t++) bad = std::min(bad, bad_t[t]);
        if (bad != SIZE_MAX) return tb_bad_row(rows, bad, bad_row);
        for (size_t t = 0; t < 16; t++)
            for (int c = 0; c <= n_chrom; c++) chrom_cnt[(size_t)c] += cnt_t[t][(size_t)c];
    }
    tb_tick("validate + bucket");
    // units: every slice of the rows collects its triples, tb_units orders them; then every row finds its own
    std::vector<uint32_t> unit_of_row(n_rows);
    TbUnits &U = A.U;
    {
        std::vector<std::vector<Triple>> found(16);
        for_slices(n_rows, 65536, [&](size_t t, size_t lo, size_t hi) { tb_triples(rows, lo, hi, n_rep, found[t]); });
        std::vector<Triple> triples;
        for (auto &f : found) triples.insert(triples.end(), f.begin(), f.end());
        if ((rc = tb_units(triples, rep_len, n_rep, U))) return rc;
        for_slices(n_rows, 65536, [&](size_t, size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) unit_of_row[i] = tb_row_unit(rows[i], U.first.data(), U.ids.data(), U.n);
        });
    }
    std::vector<uint32_t> &chrom_off = A.chrom_off;
    chrom_off.assign((size_t)n_chrom + 1, 0);
    for (int c = 0; c < n_chrom; c++) chrom_off[c + 1] = chrom_off[c] + chrom_cnt[c + 1];
    tb_tick("units");
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
    tb_tick("sort by start");
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
    tb_tick("ranks");
    A.shift = tb_bin_shift(n_rows, chrom_size, n_chrom, A.bin_off);
    const std::vector<uint32_t> &bin_off = A.bin_off;
    const int shift = A.shift;
    A.bl.resize(bin_off[n_chrom]);
    A.iv.resize(n_rows);
    A.orig.resize(n_rows);
    A.row_unit.resize(n_rows);
    ItxIv *iv = A.iv.data();
    // rows: slices of the sorted order in parallel. pbelow crosses slice boundaries: a first pass takes every slice's summary
    // (TbRun), a short serial pass joins them into what precedes each slice, the second pass fills the rows. (One thread per
    // chromosome left chr1's 8 % of the rows to one thread: 0.09 s.)
    {
        std::vector<TbRun> sum(16, tb_run_empty()), before_slice(16, tb_run_empty());
        for_slices(n_rows, 32768, [&](size_t t, size_t lo, size_t hi) {
            if (lo >= hi) return;
            // a summary asks for the rows of the slice's LAST chromosome — walked from the end, their order does not matter to the
            // maximum — and whether any row precedes them: one such row stands for all
            const int32_t last = rows[order[hi - 1]].chrom;
            TbRun tail = tb_run_empty();
            size_t k = hi;
            for (; k > lo && rows[order[k - 1]].chrom == last; k--) tail = tb_run_push(tail, last, (int32_t)rows[order[k - 1]].end);
            sum[t] = k > lo ? tb_run_join(tb_run_push(tb_run_empty(), rows[order[k - 1]].chrom, (int32_t)rows[order[k - 1]].end), tail) : tail;
        });
        TbRun acc = tb_run_empty();
        for (size_t t = 0; t < 16; t++) {
            before_slice[t] = acc;
            acc = tb_run_join(acc, sum[t]);
        }
        for_slices(n_rows, 32768, [&](size_t t, size_t lo, size_t hi) {
            TbRun before = before_slice[t];
            for (size_t k = lo; k < hi; k++) {
                const itx_row &r = rows[order[k]];
                const uint32_t u = unit_of_row[order[k]];
                ItxIv d = tb_row_record(r, rep_len[r.rep], U.slot[u], rank_of_row[order[k]]);
                d.pbelow = tb_run_below(before, r.chrom);
                before = tb_run_push(before, r.chrom, d.e);
                iv[k] = d;
                A.orig[k] = (int32_t)order[k];
                A.row_unit[k] = u;
            }
        });
    }
    // the binned index: slices of ALL bins in parallel; a slice finds its place in the rows by bisection at its first bin and at
    // every chromosome's first, and sweeps on from there
    for_slices(bin_off[n_chrom], 65536, [&](size_t, size_t g0, size_t g1) {
        if (g0 >= g1) return;
        uint32_t c = tb_chrom_of_bin(bin_off.data(), (uint32_t)n_chrom, (uint32_t)g0);
        uint32_t k = 0, m = 0;
        bool fresh = true;
        for (size_t g = g0; g < g1; g++) {
            while (g >= bin_off[c + 1]) {
                c++;
                fresh = true;
            }
            const uint32_t lo = chrom_off[c], hi = chrom_off[c + 1];
            const int64_t bound = tb_bin_bound((uint32_t)g, bin_off[c], shift);
            if (fresh) {
                k = tb_first_start(iv, lo, hi, bound);
                m = tb_first_reach(iv, lo, hi, bound);
                fresh = false;
            } else {
                while (k < hi && tb_starts_before(iv[k], bound)) k++;
                while (m < hi && tb_ends_by(iv[m], bound)) m++;
            }
            A.bl[g] = TbPair{k, m};
        }
    });
    // first unit reaching into every window
    A.part_unit.resize(tb_n_windows(U.slots));
    for (size_t w = 0; w < A.part_unit.size(); w++) A.part_unit[w] = tb_window_unit(U.slot.data(), U.n, (uint32_t)w);
    return ITX_OK;
}
