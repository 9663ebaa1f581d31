// itx_decode_roles.h — the two roles of one fused launch of the device decoder (k_decode, itx_inflate.hip): which workgroup and
// wave does what, and for which block. Plain C++ that the host compiles too (tests/decode_roles_main.cpp).
//
// A launch carries pass 1 of the CURRENT group and pass 2 of the PREVIOUS one (the group whose pass 1 the launch before carried).
// Its workgroups have ITXD_WAVES waves of 64 lanes:
//   workgroups [0, n1)        pass 1: wave 0 takes the 64 group-wide block indices [64 wg, 64 wg + 64) of the current group, a lane
//                             each (as a k_tokens workgroup does); waves 1 .. 3 have nothing to do. They come first: a pass-1
//                             wave is the launch's long pole, and workgroups are dispatched in index order.
//   workgroups [n1, n1 + n2)  pass 2: wave v takes the one group-wide block index 4 (wg - n1) + v of the previous group, all of
//                             its lanes on that block (as a k_resolve workgroup does).
// Either part may be empty. An index below its group's span may still be padding between two slots: itxg_locate
// (itx_inflate_group.h) says so, as for the two kernels this one stands for.
#ifndef ITX_DECODE_ROLES_H
#define ITX_DECODE_ROLES_H
#include <stdint.h>

#ifndef ITXD_FN
#define ITXD_FN static inline
#endif

#define ITXD_WAVES 4u
#define ITXD_THREADS (ITXD_WAVES * 64u)

enum { ITXD_NONE = 0, ITXD_PASS1 = 1, ITXD_PASS2 = 2 };

struct itxd_grid {
    uint32_t n1, n2;                       // workgroups of the two roles
    uint32_t span_cur, span_prev;          // one more than the last block index of the two groups (itxg_layout)
};

// the launch's grid for the two spans (below 2^31 each); returns its workgroups, n1 + n2 (0: nothing to launch)
ITXD_FN uint32_t itxd_layout(itxd_grid *r, uint32_t span_cur, uint32_t span_prev)
{
    r->span_cur = span_cur;
    r->span_prev = span_prev;
    r->n1 = span_cur / 64u + (span_cur % 64u ? 1u : 0u);
    r->n2 = span_prev / ITXD_WAVES + (span_prev % ITXD_WAVES ? 1u : 0u);
    return r->n1 + r->n2;
}

// what wave `wave` of workgroup `wg` does; *first: for ITXD_PASS1 the first of the wave's 64 indices in the current group (lane
// l takes *first + l where that is below span_cur), for ITXD_PASS2 the wave's one index in the previous group
ITXD_FN uint32_t itxd_role(const itxd_grid &r, uint32_t wg, uint32_t wave, uint32_t *first)
{
    *first = 0;
    if (wg < r.n1) {
        if (wave != 0) return ITXD_NONE;
        *first = wg * 64u;
        return ITXD_PASS1;
    }
    if (wg - r.n1 >= r.n2 || wave >= ITXD_WAVES) return ITXD_NONE;
    const uint32_t g = (wg - r.n1) * ITXD_WAVES + wave;
    if (g >= r.span_prev) return ITXD_NONE;
    *first = g;
    return ITXD_PASS2;
}

// ... and a single lane of it: the role, and whether there is an index for this lane (*g, below its group's span)
ITXD_FN uint32_t itxd_lane(const itxd_grid &r, uint32_t wg, uint32_t wave, uint32_t lane, bool *has, uint32_t *g)
{
    uint32_t first;
    const uint32_t role = itxd_role(r, wg, wave, &first);
    *g = role == ITXD_PASS1 ? first + lane : first;
    *has = role == ITXD_PASS2 || (role == ITXD_PASS1 && *g < r.span_cur);
    return role;
}

#endif
