// itx_pushsched.h — the schedule of the device decoder's push pipeline (itx_inflate.hip): which group a push joins, when a group
// is launched, on which compute lane and scratch buffer, whose pass 2 a launch carries, and when a flush is needed. No HIP in
// here: plain C++ that the host compiles too (tests/pushsched_main.cpp walks every interleaving of a few pushes through it).
//
// A SLOT holds one push from begin to end. Pushes with blocks join the OPEN GROUP in push order; the group is closed and launched
// when it has group_size members, or when the first of its members is ended. Closed groups take the compute LANES in turn. Unfused,
// a launch runs both passes of its group on the lane's buffer 0. FUSED (one lane), a launch runs pass 1 of its group into the lane's
// buffer n_launched & 1 and pass 2 of the lane's PENDING group — the one the launch before carried pass 1 of — which is resolved
// by it; the launched group is pending then, until the next launch or a FLUSH (pass 2 alone) resolves it.
//
// A transition answers ITX_E_STATE or the actions its caller has to carry out, in order. It commits only what the attempt itself
// settles (a closed group is no longer open and has its lane, whether or not the launch succeeds); the caller reports every
// action it has carried out with itxp_done, which commits the rest. An action that fails is not reported and the ones behind it are
// dropped: the slots stay busy, and ending them answers ITX_E_STATE.
#ifndef ITX_PUSHSCHED_H
#define ITX_PUSHSCHED_H
#include "../../include/iteres_amd.h"

#define ITXP_GROUP 4                       /* the members a group can have: ITXG_SLOTS of itx_inflate_group.h (itx_inflater.h checks) */

enum { ITXP_LAUNCH = 1, ITXP_FLUSH = 2, ITXP_WAIT = 3 };

struct itxp_action {
    int kind;
    int group;        // LAUNCH: the group whose pass 1 (unfused: both passes) to enqueue; FLUSH: the pending group; WAIT: the group to wait for
    int lane;         // LAUNCH, FLUSH: the compute lane
    int buf;          // LAUNCH: the lane's scratch buffer for the group's tokens
    int carries;      // LAUNCH: the pending group whose pass 2 goes with it and which it finishes (-1: none; unfused: the group itself)
    int slot;         // WAIT: the slot that ends with it
};
struct itxp_actions {
    int n;
    itxp_action a[3];                      // at most a launch, a flush and a wait
};

struct itxp_sched {
    int n_slots, group_size, n_lanes, fused;
    struct {
        int busy, grp, has_blocks;         // grp: the group the push belongs to (-1: none, a push without blocks or one that failed half way)
    } slot[ITX_BAMWIN_LANES];
    struct {
        int n, slot[ITXP_GROUP];          // its members, in push order
        int live;                          // members whose end is still to come (0: the entry is free)
        int lane;                          // the compute lane it was closed for
        int launched, resolved;            // launched: pass 1 is enqueued; resolved: pass 2 and the status copies too
    } grp[ITX_BAMWIN_LANES];
    struct {
        unsigned long n_launched;          // groups launched on this lane
        int pend, pend_buf;                // fused: the group whose pass 2 is still to come (-1: none), and its scratch buffer
    } lane[ITX_BAMWIN_LANES];
    int open_grp;                          // the group that still takes members (-1: none)
    unsigned long grp_seq;                 // groups closed so far: group q runs on compute lane q % n_lanes
};

static inline void itxp_init(itxp_sched *S, int n_slots, int group_size, int n_lanes, int fused)
{
    *S = itxp_sched{n_slots, group_size, n_lanes, fused, {}, {}, {}, -1, 0};
    for (int k = 0; k < ITX_BAMWIN_LANES; k++) S->slot[k].grp = S->lane[k].pend = -1;
}

// the open group is closed and takes the next lane in turn; its launch is the caller's to attempt
static inline void itxp_close(itxp_sched *S, itxp_actions *A)
{
    const int gi = S->open_grp;
    S->open_grp = -1;
    const int cl = S->grp[gi].lane = (int)(S->grp_seq++ % (unsigned long)S->n_lanes);
    A->a[A->n++] = itxp_action{ITXP_LAUNCH, gi, cl, S->fused ? (int)(S->lane[cl].n_launched & 1u) : 0, S->fused ? S->lane[cl].pend : gi, -1};
}

// a push takes slot s. With blocks it is not in a group yet: itxp_join, once its copies are enqueued
static inline int itxp_begin(itxp_sched *S, int s, int has_blocks)
{
    if (S->slot[s].busy) return ITX_E_STATE;
    S->slot[s] = {1, -1, has_blocks};
    return ITX_OK;
}

// ... and joins the open group, in the first free entry if none is open; the group_size-th member closes it
static inline int itxp_join(itxp_sched *S, int s, itxp_actions *A)
{
    A->n = 0;
    if (S->open_grp < 0) {
        int gi = 0;
        while (gi < S->n_slots && S->grp[gi].live) gi++;           // every live group has a busy slot, and this slot was not: one is free
        if (gi == S->n_slots) return ITX_E_STATE;
        S->grp[gi].n = S->grp[gi].live = S->grp[gi].launched = S->grp[gi].resolved = 0;
        S->open_grp = gi;
    }
    auto &G = S->grp[S->open_grp];
    G.slot[G.n++] = s;
    G.live++;
    S->slot[s].grp = S->open_grp;
    if (G.n == S->group_size) itxp_close(S, A);
    return ITX_OK;
}

// the push in slot s ends: its group is closed first if it is still open; fused, a group that has had pass 1 only gets its pass 2
// from the open group, closed short, if that runs on the same lane, else from a flush. A slot without blocks ends at once
static inline int itxp_end(itxp_sched *S, int s, itxp_actions *A)
{
    A->n = 0;
    if (!S->slot[s].busy) return ITX_E_STATE;
    if (!S->slot[s].has_blocks) {
        S->slot[s].busy = 0;
        return ITX_OK;
    }
    const int gi = S->slot[s].grp;
    if (gi < 0) return ITX_E_STATE;                                 // its begin failed half way
    const auto &G = S->grp[gi];
    if (!G.launched) {
        if (S->open_grp != gi) return ITX_E_STATE;                  // (an unlaunched group is the open one, unless its launch failed)
        itxp_close(S, A);
    } else if (!G.resolved && S->lane[G.lane].pend != gi)
        return ITX_E_STATE;
    if (S->fused && !G.resolved) {                                  // pass 1 only, now or before: who brings its pass 2
        if (S->open_grp >= 0 && (int)(S->grp_seq % (unsigned long)S->n_lanes) == G.lane)
            itxp_close(S, A);
        else
            A->a[A->n++] = itxp_action{ITXP_FLUSH, gi, G.lane, 0, -1, -1};
    }
    A->a[A->n++] = itxp_action{ITXP_WAIT, gi, G.lane, 0, -1, s};
    return ITX_OK;
}

// the caller has carried `a` out
static inline void itxp_done(itxp_sched *S, const itxp_action &a)
{
    auto &L = S->lane[a.lane];
    if (a.kind == ITXP_LAUNCH) {
        L.n_launched++;
        S->grp[a.group].launched = 1;
        if (a.carries >= 0) S->grp[a.carries].resolved = 1;
        if (S->fused) {
            L.pend = a.group;
            L.pend_buf = a.buf;
        }
    } else if (a.kind == ITXP_FLUSH) {
        S->grp[a.group].resolved = 1;
        L.pend = -1;
    } else {
        S->grp[a.group].live--;
        S->slot[a.slot].busy = 0;
    }
}

#endif
