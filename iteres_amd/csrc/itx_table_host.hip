// itx_table_host.hip — the host build of the repeat table (ITX_TABLE_HOST=1): the arrays come from tb_host_arrays
// (itx_tablehost.h, plain C++ on host threads); this is their upload into one allocation.
#include "itx_table_priv.h"

static_assert(sizeof(uint2) == sizeof(TbPair) && sizeof(uint4) == sizeof(TbQuad), "the rules' plain structs are uploaded as the device's vector types");

int table_create_host(const itx_row *rows, size_t n_rows, const int64_t *chrom_size, int n_chrom, const uint32_t *rep_len, uint32_t n_rep, uint32_t n_fam, uint32_t n_cla,
                      int device, itx_table **out, size_t *bad_row)
{
    TbHostArrays A;
    int rc = tb_host_arrays(rows, n_rows, chrom_size, n_chrom, rep_len, n_rep, n_fam, n_cla, A, bad_row);
    if (rc) return rc;
    if ((rc = tb_device_ready(device))) return rc;
    tb_tick("rows + index");
    Carver cv;
    const TbLayout L = tb_layout(cv, n_rows, A.bl.size(), A.U.slots, A.U.n);
    char *base = nullptr;
    if ((rc = tb_device_alloc(&base, L.bytes))) return rc;
    hipError_t he = hipSuccess;
    auto up = [&](size_t off, const void *src, size_t bytes) -> bool {
        if (bytes == 0) return true;
        he = hipMemcpy(base + off, src, bytes, hipMemcpyHostToDevice);
        return he == hipSuccess;
    };
    const bool ok = up(L.iv, A.iv.data(), A.iv.size() * sizeof(ItxIv)) && up(L.orig, A.orig.data(), A.orig.size() * 4) &&
                    up(L.bl, A.bl.data(), A.bl.size() * sizeof(TbPair)) && up(L.runit, A.row_unit.data(), A.row_unit.size() * 4) &&
                    up(L.punit, A.part_unit.data(), A.part_unit.size() * 4) && up(L.uslot, A.U.slot.data(), A.U.slot.size() * 4) &&
                    up(L.uids, A.U.ids.data(), A.U.ids.size() * sizeof(TbQuad)) && up(L.ucov, A.U.covoff.data(), A.U.covoff.size() * 8);
    if (!ok) {
        itx_set_error("itx_table_create: upload failed: %s", hipGetErrorString(he));
        (void)hipFree(base);
        return ITX_E_NO_DEVICE;
    }
    *out = tb_object(base, L, device, A.shift, n_rows, chrom_size, n_chrom, rep_len, n_rep, n_fam, n_cla, A.U, A.chrom_off, A.bin_off);
    tb_tick("upload");
    return ITX_OK;
}
