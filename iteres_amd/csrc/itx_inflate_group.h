// itx_inflate_group.h — one launch of the device decoder over the blocks of several pushes (itx_inflate.hip): where a slot's
// blocks lie among the launch's block indices, and back. Plain C++ that the host compiles too (tests/inflate_group_main.cpp).
//
// A group has up to ITXG_SLOTS slots (pushes). Slot k's blocks take the group-wide indices [first[k], first[k] + n[k]);
// first[k] is a multiple of 64, so the 64 lanes of a pass-1 wave (lane = block) never belong to two slots, and "is there a
// block behind this index" stays a test against the slot's own count. The indices between a slot's last block and the next
// slot's first are padding: no block, nothing to do. An empty slot takes no indices at all.
#ifndef ITX_INFLATE_GROUP_H
#define ITX_INFLATE_GROUP_H
#include <stdint.h>

#ifndef ITXG_FN
#define ITXG_FN static inline
#endif

#define ITXG_SLOTS 4u
#define ITXG_ALIGN 64u

struct itxg_index {
    uint32_t n_slots;
    uint32_t first[ITXG_SLOTS], n[ITXG_SLOTS];
};

// lays the slots out one after the other; returns the span: one more than the last index that holds a block (0: no blocks).
// The counts must be small enough for the sum of their round-ups to fit 32 bits (a push has fewer than 2^31 / 4 blocks).
ITXG_FN uint32_t itxg_layout(itxg_index *x, const uint32_t *counts, uint32_t n_slots)
{
    uint32_t at = 0, span = 0;
    x->n_slots = n_slots;
    for (uint32_t k = 0; k < ITXG_SLOTS; k++) {
        const uint32_t c = k < n_slots ? counts[k] : 0u;
        x->first[k] = at;
        x->n[k] = c;
        if (c) span = at + c;
        at += (c + ITXG_ALIGN - 1u) / ITXG_ALIGN * ITXG_ALIGN;
    }
    return span;
}

// the slot a group-wide index falls into and the index's place among that slot's blocks; false: padding (or beyond the span)
ITXG_FN bool itxg_locate(const itxg_index &x, uint32_t g, uint32_t *slot, uint32_t *local)
{
    uint32_t k = 0, f = x.first[0], n = x.n[0];               // (every array index a constant: the device keeps x in registers)
#pragma unroll
    for (uint32_t j = 1; j < ITXG_SLOTS; j++)
        if (j < x.n_slots && g >= x.first[j]) {               // first[] never decreases: the last slot that starts at or before g
            k = j;
            f = x.first[j];
            n = x.n[j];
        }
    *slot = k;
    *local = g - f;
    return *local < n;
}

#endif
