// itx_table_priv.h — what the three files of the repeat table share: itx_table.hip (layout, table object, dispatch, accessors),
// itx_table_host.hip (the host build's upload) and itx_table_device.hip (the device build).
#pragma once
#include "itx_common.h"
#include "itx_tablehost.h"

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

// where the table's arrays lie in its device allocation
struct TbLayout {
    size_t iv, orig, bl, runit, punit, uslot, uids, ucov, bytes, n_win;
};
TbLayout tb_layout(Carver &cv, size_t n_rows, size_t n_bins, uint64_t slots, uint32_t n_units);
// the table object over a filled allocation
itx_table *tb_object(char *base, const TbLayout &L, int device, int shift, size_t n_rows, const int64_t *chrom_size, int n_chrom, const uint32_t *rep_len, uint32_t n_rep,
                     uint32_t n_fam, uint32_t n_cla, const TbUnits &U, const std::vector<uint32_t> &chrom_off, const std::vector<uint32_t> &bin_off);
// the device is there and becomes the calling thread's; the one allocation of a build (*base null when it fails)
int tb_device_ready(int device);
int tb_device_alloc(char **base, size_t bytes);

// the two builds behind itx_table_create, which has checked the arguments (tb_check_args)
int table_create_host(const itx_row *rows, size_t n_rows, const int64_t *chrom_size, int n_chrom, const uint32_t *rep_len, uint32_t n_rep, uint32_t n_fam, uint32_t n_cla,
                      int device, itx_table **out, size_t *bad_row);
int table_create_device(const itx_row *rows, size_t n_rows, const int64_t *chrom_size, int n_chrom, const uint32_t *rep_len, uint32_t n_rep, uint32_t n_fam, uint32_t n_cla,
                        int device, itx_table **out, size_t *bad_row);
