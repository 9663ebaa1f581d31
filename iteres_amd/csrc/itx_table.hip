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
// The rules of the build are stated once in itx_tablebuild.h. The host's side of both builds and the host build's arrays are in
// itx_tablehost.h, the host build's upload in itx_table_host.hip, the device build in itx_table_device.hip; this file holds what
// both builds and the accessors share.
#include "itx_table_priv.h"

#include <cstdlib>
#include <cstring>

// where the table's arrays lie in its device allocation
TbLayout tb_layout(Carver &cv, size_t n_rows, size_t n_bins, uint64_t slots, uint32_t n_units)
{
    TbLayout L;
    L.n_win = tb_n_windows(slots);
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
itx_table *tb_object(char *base, const TbLayout &L, int device, int shift, size_t n_rows, const int64_t *chrom_size, int n_chrom, const uint32_t *rep_len, uint32_t n_rep,
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

// "HIP device %d not available": the device is there and is the calling thread's current one
int tb_device_ready(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        itx_set_error("itx_table_create: HIP device %d not available (%d visible)", device, ndev);
        return ITX_E_NO_DEVICE;
    }
    ITX_HIP(hipSetDevice(device));
    return ITX_OK;
}

// the one allocation of a build; *base is null when it fails
int tb_device_alloc(char **base, size_t bytes)
{
    const hipError_t he = hipMalloc((void **)base, bytes);
    if (he == hipSuccess) return ITX_OK;
    *base = nullptr;
    itx_set_error("itx_table_create: hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(he));
    return ITX_E_NOMEM;
}

// ITX_TABLE_HOST=1: the host build, the oracle of the device build. The arguments are checked here, once for both.
extern "C" int itx_table_create(const itx_row *rows, size_t n_rows, const int64_t *chrom_size, int n_chrom,
                                const uint32_t *rep_len, uint32_t n_rep, uint32_t n_fam, uint32_t n_cla, int device,
                                itx_table **out, size_t *bad_row)
{
    const int rc = tb_check_args(rows, n_rows, chrom_size, n_chrom, rep_len, n_rep, out);
    if (rc) return rc;
    const char *h = getenv("ITX_TABLE_HOST");
    return (h && atoi(h) != 0 ? table_create_host : table_create_device)(rows, n_rows, chrom_size, n_chrom, rep_len, n_rep, n_fam, n_cla, device, out, bad_row);
}

extern "C" int itx_table_debug_copy(const itx_table *t, int which, void *dst, size_t cap_bytes, size_t *bytes)
{
    if (!t || !bytes) {
        itx_set_error("itx_table_debug_copy: null argument");
        return ITX_E_ARG;
    }
    const size_t n_win = tb_n_windows(t->n_slots);
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
