// itx_bamout_annotate.hip — filter -b -a: the table whose rows tag the counted records of the BAM writer (itx_bamout.hip).
// itx_bamout_annotate_enable checks the rows and the three name tables, lays them out as one block (BoAnn, itx_bamout_priv.h) and
// uploads it once; from then on k_bo_measure<true> and k_bo_gather<uint32_t, true> of itx_bamout.hip read it (the tags' rule:
// csrc/itx_reptag.h). No kernel is launched here.
#include "itx_bamout_priv.h"

#include <stdlib.h>
#include <string.h>

// one name table's checks: offsets that ascend, no name of 2^16 bytes or more. Returns ITX_OK, ITX_E_ARG or ITX_E_LIMIT.
static int bo_check_names(const char *what, const uint64_t *off, uint32_t n)
{
    for (uint32_t i = 0; i < n; i++) {
        if (off[i + 1] < off[i]) {
            itx_set_error("itx_bamout_annotate_enable: the offsets of the %s names do not ascend (name %u)", what, i);
            return ITX_E_ARG;
        }
        if (off[i + 1] - off[i] > ITX_REPTAG_MAX_NAME) {
            itx_set_error("itx_bamout_annotate_enable: %s name %u has %llu bytes (a tag's name has at most %u)", what, i, (ull)(off[i + 1] - off[i]), ITX_REPTAG_MAX_NAME);
            return ITX_E_LIMIT;
        }
    }
    return ITX_OK;
}

extern "C" int itx_bamout_annotate_enable(itx_bamout *bo, const itx_row *rows, size_t n_rows, const char *rep_bytes, const uint64_t *rep_off, uint32_t n_rep,
                                          const char *cla_bytes, const uint64_t *cla_off, uint32_t n_cla, const char *fam_bytes, const uint64_t *fam_off, uint32_t n_fam)
{
    if (!bo || (n_rows && !rows) || !rep_bytes || !rep_off || !cla_bytes || !cla_off || !fam_bytes || !fam_off || n_rows >= 0x7fffffffull) {
        itx_set_error("itx_bamout_annotate_enable: bad argument");
        return ITX_E_ARG;
    }
    if (bo_not_begun(bo, "itx_bamout_annotate_enable", bo->annotate) != ITX_OK) return ITX_E_STATE;
    int rc = ITX_OK;
    if ((rc = bo_check_names("repName", rep_off, n_rep)) != ITX_OK || (rc = bo_check_names("repClass", cla_off, n_cla)) != ITX_OK ||
        (rc = bo_check_names("repFamily", fam_off, n_fam)) != ITX_OK)
        return rc;
    for (size_t r = 0; r < n_rows; r++)
        if (rows[r].rep >= n_rep || rows[r].cla >= n_cla || rows[r].fam >= n_fam) {
            itx_set_error("itx_bamout_annotate_enable: row %zu names repName %u of %u, repClass %u of %u, repFamily %u of %u", r, rows[r].rep, n_rep, rows[r].cla, n_cla,
                          rows[r].fam, n_fam);
            return ITX_E_ARG;
        }
    // one block, laid out on the host and uploaded once: the three offset arrays (8-byte aligned), the rows, the three pools.
    // Offsets are rebased to the pool's first used byte, so a caller's off[0] need not be 0.
    const size_t o_rep = 0, o_cla = o_rep + 8 * ((size_t)n_rep + 1), o_fam = o_cla + 8 * ((size_t)n_cla + 1), o_rows = o_fam + 8 * ((size_t)n_fam + 1);
    const size_t b_rep = o_rows + 4 * (size_t)BO_ROW_WORDS * n_rows, b_cla = b_rep + (size_t)(rep_off[n_rep] - rep_off[0]);
    const size_t b_fam = b_cla + (size_t)(cla_off[n_cla] - cla_off[0]), bytes = b_fam + (size_t)(fam_off[n_fam] - fam_off[0]);
    uint8_t *h = (uint8_t *)malloc(bytes + 16), *d = nullptr;
    if (!h) {
        itx_set_error("itx_bamout_annotate_enable: no host memory for a table of %zu bytes", bytes);
        return ITX_E_NOMEM;
    }
    {
        const uint64_t *const offs[3] = {rep_off, cla_off, fam_off};
        const char *const pools[3] = {rep_bytes, cla_bytes, fam_bytes};
        const uint32_t ns[3] = {n_rep, n_cla, n_fam};
        const size_t at_off[3] = {o_rep, o_cla, o_fam}, at_bytes[3] = {b_rep, b_cla, b_fam};
        for (int t = 0; t < 3; t++) {
            ull *o = (ull *)(h + at_off[t]);
            for (uint32_t i = 0; i <= ns[t]; i++) o[i] = offs[t][i] - offs[t][0];
            if (o[ns[t]]) memcpy(h + at_bytes[t], pools[t] + offs[t][0], (size_t)o[ns[t]]);
        }
        uint32_t *w = (uint32_t *)(h + o_rows);
        for (size_t r = 0; r < n_rows; r++) {
            w[BO_ROW_WORDS * r] = rows[r].start;
            w[BO_ROW_WORDS * r + 1] = rows[r].end;
            w[BO_ROW_WORDS * r + 2] = rows[r].rep;
            w[BO_ROW_WORDS * r + 3] = rows[r].cla;
            w[BO_ROW_WORDS * r + 4] = rows[r].fam;
        }
    }
    ITX_TRY(hipSetDevice(bo->device));
    if (hipMalloc((void **)&d, bytes + 16) != hipSuccess) {
        (void)hipGetLastError();
        itx_set_error("itx_bamout_annotate_enable: no device memory for a table of %zu bytes", bytes);
        rc = ITX_E_NOMEM;
        goto out;
    }
    ITX_TRY(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));                 // (synchronous: the caller's arrays and h are free on return)
    bo->ann.rep_off = (const ull *)(d + o_rep);
    bo->ann.cla_off = (const ull *)(d + o_cla);
    bo->ann.fam_off = (const ull *)(d + o_fam);
    bo->ann.rows = (const uint32_t *)(d + o_rows);
    bo->ann.rep = d + b_rep;
    bo->ann.cla = d + b_cla;
    bo->ann.fam = d + b_fam;
    bo->ann.n_rows = (uint32_t)n_rows;
    bo->d_ann = d;
    bo->annotate = 1;
    d = nullptr;
out:
    (void)hipFree(d);                                                      // (the block that was not taken)
    free(h);
    return rc;
}

extern "C" int itx_bamout_annotate_get_stats(const itx_bamout *bo, uint64_t *tag_bytes)
{
    if (!bo || !tag_bytes) {
        itx_set_error("itx_bamout_annotate_get_stats: bad argument");
        return ITX_E_ARG;
    }
    *tag_bytes = bo->tag_bytes;
    return ITX_OK;
}
