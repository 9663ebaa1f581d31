// itx_bamidx.h — internal: what the BAM writer (csrc/itx_bamout.hip and, for the members' sizes and the replay of -s,
// itx_bamout_members.hip and itx_bamout_sort.hip) calls in csrc/itx_bamidx.hip when `filter -b -i` asked for the .bai index.
// The index object lives inside the itx_bamout object; every call works on the bamout object's stream `st`.
#pragma once
#include "itx_common.h"

#define ITX_BAMIDX_TILE 256u         // records per workgroup of the entry kernel: the gather's tile (BO_TILE), whose tile bases it uses

#define ITX_BAMIDX_PAYLOAD 8192u      // bytes of the record stream per member: ITX_BAMOUT_PAYLOAD (itx_bamout_priv.h asserts it)

struct itx_bamidx;

// n_ref >= ITX_BAI_MAX_REFS: an object that only remembers why there will be no index
int itx_bamidx_create(int device, int32_t n_ref, const int32_t *l_ref, itx_bamidx **out);
void itx_bamidx_destroy(itx_bamidx *ix);
// room for n_entries more entries and n_members more member sizes; st is idle. ITX_E_NOMEM leaves everything as it was.
int itx_bamidx_reserve(itx_bamidx *ix, hipStream_t st, uint64_t n_entries, uint64_t n_members);
// one entry per record with len_in[i] != 0, behind the entries there are: record i starts at byte
// stream_at + tile_base[2 * tile] + (its place in the tile, itx_tile_offsets) of the record stream; tile_base[2 * tile + 1] counts
// the records of the tiles before. n_counted: how many entries that makes (the measure's total). Enqueued, not waited for.
int itx_bamidx_entries(itx_bamidx *ix, hipStream_t st, const uint8_t *u, const uint32_t *rec_off, uint32_t n, const uint32_t *len_in,
                       const unsigned long long *tile_base, unsigned long long stream_at, uint64_t n_counted);
// the same with 64-bit offsets: the records of one round of filter -b -s, where they lie in the held stream (itx_bamout_sort_next)
int itx_bamidx_entries64(itx_bamidx *ix, hipStream_t st, const uint8_t *u, const unsigned long long *rec_off, uint32_t n, const uint32_t *len_in,
                         const unsigned long long *tile_base, unsigned long long stream_at, uint64_t n_counted);
// the host route: d_bytes (device) holds n whole records one behind the other, h_off[i] where record i starts in them; the
// offsets are uploaded (waited for: h_off is the caller's again), measured, and the same entry kernel runs over them
int itx_bamidx_host_records(itx_bamidx *ix, hipStream_t st, const uint8_t *d_bytes, const uint32_t *h_off, uint32_t n, unsigned long long stream_at);
// the sizes of n members just made (device), behind those of the members before
int itx_bamidx_members(itx_bamidx *ix, hipStream_t st, const uint32_t *d_msize, uint32_t n);
// the device time of the entry kernels enqueued so far is read (their event is waited for)
void itx_bamidx_batch_time(itx_bamidx *ix);
int itx_bamidx_finish(itx_bamidx *ix, hipStream_t st, uint64_t first_member_offset, itx_bamout_index_result *res);
