// Host build of the .bai rule (csrc/itx_bairule.h) for tests/test_bai_rule.py.
#include "../iteres_amd/csrc/itx_bairule.h"

extern "C" uint32_t itxb_reg2bin(int64_t beg, int64_t end) { return itx_bai_reg2bin(beg, end); }

// the fields of the record at rec (len = 4 + block_size bytes): out = {tid, pos, n_cigar, end}; returns itx_bai_refuses
extern "C" int itxb_record(const uint8_t *rec, uint32_t len, int32_t n_ref, const int32_t *l_ref, int64_t *out)
{
    ItxBaiRec r;
    itx_bai_fields(rec, len, &r);
    out[0] = r.tid;
    out[1] = r.pos;
    out[2] = r.n_cigar;
    out[3] = r.end;
    return itx_bai_refuses(&r, n_ref, l_ref);
}

extern "C" uint32_t itxb_key(int32_t tid, uint32_t bin) { return itx_bai_key(tid, bin); }
extern "C" uint32_t itxb_win_first(int32_t pos) { return itx_bai_win_first(pos); }
extern "C" uint32_t itxb_win_last(int64_t end) { return itx_bai_win_last(end); }
extern "C" uint32_t itxb_windows(int32_t l_ref) { return itx_bai_windows(l_ref); }
extern "C" uint64_t itxb_voff(uint64_t first, const uint64_t *coff, uint64_t s, uint32_t payload) { return itx_bai_voff(first, coff, s, payload); }
