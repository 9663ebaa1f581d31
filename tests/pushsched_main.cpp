// Stand-alone check of iteres_amd/csrc/itx_pushsched.h (tests/test_pushsched.py builds and runs it). A model caller carries the
// schedule's actions out on paper — which group has had which pass, on which lane, which scratch buffer holds tokens that no pass 2
// has read yet — and walks EVERY legal order of begins and ends of up to 6 pushes (a push begins on the lowest free slot, so a slot
// is used again after its end; up to two pushes have no blocks), for every configuration with slots in {1, 2, 4, 6}, group size in
// {1, 2, 4} and (lanes, fused) in {(1, 0), (2, 0), (1, 1)}. Orders that lead to the same state of schedule and model are walked on
// from there once. Then the slot sequences of tests/fusedcase.py's scenarios with the (launches, flushes) that
// tests/test_gpu_inflate_fused.py reads off the device's timing line, and the three illegal calls.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <unordered_set>
#include <vector>

#include "../iteres_amd/csrc/itx_pushsched.h"

#define MAX_PUSHES 6
#define FAIL(...)                                                        \
    do {                                                                 \
        fprintf(stderr, __VA_ARGS__);                                    \
        fprintf(stderr, "\n");                                           \
        return false;                                                    \
    } while (0)

struct Model {
    itxp_sched S;
    int n_pushes, begun, ended, zeros;            // pushes of this walk, how many have begun / ended / had no blocks
    int slot_of[MAX_PUSHES];                      // a begun push's slot; -1: not begun, -2: ended
    int pass1[ITX_BAMWIN_LANES], pass2[ITX_BAMWIN_LANES], lane_of[ITX_BAMWIN_LANES];      // per group entry, since it was last free
    int unread[ITX_BAMWIN_LANES][2];              // per lane and scratch buffer: the group whose tokens no pass 2 has read yet (-1: none)
    unsigned long launches, flushes;
};

static void model_init(Model *M, int n_pushes, int slots, int group, int lanes, int fused)
{
    memset(M, 0, sizeof *M);                      // (padding too: the bytes are the walk's memo key)
    itxp_init(&M->S, slots, group, lanes, fused);
    M->n_pushes = n_pushes;
    for (int k = 0; k < MAX_PUSHES; k++) M->slot_of[k] = -1;
    for (int k = 0; k < ITX_BAMWIN_LANES; k++) M->unread[k][0] = M->unread[k][1] = M->lane_of[k] = -1;
}

// pass 2 of group g is issued on `lane`: it has had pass 1, on that lane, and not pass 2; its tokens are read
static bool model_pass2(Model *M, int g, int lane)
{
    if (g < 0 || !M->pass1[g] || M->pass2[g] || M->lane_of[g] != lane) FAIL("pass 2 of group %d on lane %d: pass 1 %d on lane %d, pass 2 %d", g, lane, g < 0 ? 0 : M->pass1[g], g < 0 ? -1 : M->lane_of[g], g < 0 ? 0 : M->pass2[g]);
    M->pass2[g] = 1;
    for (int q = 0; q < 2; q++)
        if (M->unread[lane][q] == g) M->unread[lane][q] = -1;
    return true;
}

// what itx_inflate.hip does with a transition's actions, on paper
static bool model_carry_out(Model *M, const itxp_actions &A)
{
    itxp_sched &S = M->S;
    if (A.n < 0 || A.n > 3) FAIL("%d actions", A.n);
    for (int i = 0; i < A.n; i++) {
        const itxp_action &a = A.a[i];
        if (a.kind == ITXP_LAUNCH) {
            const int g = a.group;
            if (g < 0 || g >= S.n_slots || S.grp[g].n < 1 || S.grp[g].n > S.group_size || S.grp[g].live < 1) FAIL("launch of group %d", g);
            if (M->pass1[g]) FAIL("group %d gets pass 1 twice", g);
            if (a.lane < 0 || a.lane >= S.n_lanes || a.lane != S.grp[g].lane || a.buf < 0 || a.buf > 1) FAIL("launch of group %d on lane %d buffer %d", g, a.lane, a.buf);
            M->pass1[g] = 1;
            M->lane_of[g] = a.lane;
            if (S.fused) {
                if (M->unread[a.lane][a.buf] >= 0) FAIL("lane %d buffer %d goes to group %d while group %d's tokens in it are unread", a.lane, a.buf, g, M->unread[a.lane][a.buf]);
                M->unread[a.lane][a.buf] = g;
                if (a.carries == g) FAIL("fused: group %d gets both passes in one launch", g);
                if (a.carries != S.lane[a.lane].pend) FAIL("the launch carries %d, pending is %d", a.carries, S.lane[a.lane].pend);
                if (a.carries >= 0 && !model_pass2(M, a.carries, a.lane)) return false;
            } else {
                if (a.carries != g || a.buf != 0) FAIL("unfused launch of group %d carries %d on buffer %d", g, a.carries, a.buf);
                if (!model_pass2(M, g, a.lane)) return false;
            }
            M->launches++;
        } else if (a.kind == ITXP_FLUSH) {
            if (!S.fused || a.lane < 0 || a.lane >= S.n_lanes || S.lane[a.lane].pend != a.group) FAIL("flush of group %d on lane %d", a.group, a.lane);
            if (!model_pass2(M, a.group, a.lane)) return false;
            M->flushes++;
        } else if (a.kind == ITXP_WAIT) {
            if (i != A.n - 1 || !S.grp[a.group].resolved || !M->pass2[a.group]) FAIL("wait for group %d, which is not resolved by the actions before", a.group);
        } else
            FAIL("action kind %d", a.kind);
        itxp_done(&S, a);
        if (a.kind == ITXP_WAIT && S.grp[a.group].live == 0) {           // the entry is free again: it had each pass exactly once
            if (!M->pass1[a.group] || !M->pass2[a.group]) FAIL("group %d ended without both passes", a.group);
            M->pass1[a.group] = M->pass2[a.group] = 0;
            M->lane_of[a.group] = -1;
        }
    }
    return true;
}

static bool model_begin(Model *M, int slot, int has_blocks)
{
    itxp_actions A;
    A.n = 0;
    if (itxp_begin(&M->S, slot, has_blocks) != ITX_OK) FAIL("begin on the free slot %d refused", slot);
    if (!has_blocks) return true;
    if (itxp_join(&M->S, slot, &A) != ITX_OK) FAIL("no free group entry for slot %d", slot);
    return model_carry_out(M, A);
}

static bool model_end(Model *M, int slot)
{
    itxp_actions A;
    if (itxp_end(&M->S, slot, &A) != ITX_OK) FAIL("end of the busy slot %d refused", slot);
    const bool with_blocks = M->S.slot[slot].has_blocks != 0;
    if ((A.n != 0) != with_blocks || (with_blocks && (A.a[A.n - 1].kind != ITXP_WAIT || A.a[A.n - 1].slot != slot))) FAIL("end of slot %d: %d actions", slot, A.n);
    if (!model_carry_out(M, A)) return false;
    if (M->S.slot[slot].busy) FAIL("slot %d is busy after its end", slot);
    return true;
}

// after every end: nothing pending, nothing live, nothing open, no tokens unread
static bool model_at_rest(const Model &M)
{
    const itxp_sched &S = M.S;
    if (S.open_grp != -1) FAIL("group %d is open at the end", S.open_grp);
    for (int k = 0; k < ITX_BAMWIN_LANES; k++)
        if (S.slot[k].busy || S.grp[k].live || S.lane[k].pend != -1 || M.pass1[k] || M.pass2[k] || M.unread[k][0] != -1 || M.unread[k][1] != -1)
            FAIL("at the end: slot %d busy %d, group %d live %d, lane %d pending %d", k, S.slot[k].busy, k, S.grp[k].live, k, S.lane[k].pend);
    return true;
}

static std::unordered_set<std::string> g_seen;
static unsigned long g_states, g_transitions, g_ends;

static bool walk(const Model &M)
{
    if (!g_seen.insert(std::string(reinterpret_cast<const char *>(&M), sizeof M)).second) return true;
    g_states++;
    if (M.ended == M.n_pushes) {
        g_ends++;
        return model_at_rest(M);
    }
    if (M.begun < M.n_pushes) {
        int slot = 0;
        while (slot < M.S.n_slots && M.S.slot[slot].busy) slot++;
        if (slot < M.S.n_slots)
            for (int has_blocks = 1; has_blocks >= (M.zeros < 2 ? 0 : 1); has_blocks--) {
                Model N = M;
                N.slot_of[N.begun++] = slot;
                N.zeros += !has_blocks;
                g_transitions++;
                if (!model_begin(&N, slot, has_blocks) || !walk(N)) {
                    fprintf(stderr, "  after begin of push %d (%s blocks) on slot %d\n", M.begun, has_blocks ? "with" : "no", slot);
                    return false;
                }
            }
    }
    for (int k = 0; k < M.begun; k++) {
        if (M.slot_of[k] < 0) continue;
        Model N = M;
        N.slot_of[k] = -2;
        N.ended++;
        g_transitions++;
        if (!model_end(&N, M.slot_of[k]) || !walk(N)) {
            fprintf(stderr, "  after end of push %d on slot %d\n", k, M.slot_of[k]);
            return false;
        }
    }
    return true;
}

// tests/fusedcase.py: 12 slots, groups of 4, one lane, fused; push k takes slot k % 12. order: +k begins push k, -k - 1 ends it
static bool replay(const char *name, const std::vector<int> &blocks, const std::vector<int> &order, unsigned long launches, unsigned long flushes)
{
    Model M;
    model_init(&M, 0, 12, 4, 1, 1);
    for (int op : order) {
        const int k = op >= 0 ? op : -op - 1;
        if (!(op >= 0 ? model_begin(&M, k % 12, blocks[(size_t)k] != 0) : model_end(&M, k % 12))) {
            fprintf(stderr, "  in scenario %s at push %d\n", name, k);
            return false;
        }
    }
    if (!model_at_rest(M)) return false;
    if (M.launches != launches || M.flushes != flushes) FAIL("scenario %s: %lu launches and %lu flushes, expected %lu and %lu", name, M.launches, M.flushes, launches, flushes);
    return true;
}

// what the reader's producer does: begin while a slot is free, else end the oldest
static std::vector<int> in_order(size_t n)
{
    std::vector<int> order;
    size_t begun = 0, ended = 0;
    while (ended < n)
        if (begun < n && begun - ended < 12)
            order.push_back((int)begun++);
        else
            order.push_back(-(int)ended++ - 1);
    return order;
}

static bool scenarios()
{
    static const int kSizes[6] = {1, 63, 64, 65, 129, 0};
    static const int kFlush[4] = {65, 129, 1, 64};
    for (int n : {1, 2, 4})
        if (!replay("flush", std::vector<int>(kFlush, kFlush + n), in_order((size_t)n), 1, 1)) return false;
    for (int g : {2, 3, 5}) {
        std::vector<int> blocks;
        for (int with = 0; with < 4 * (g - 1) + 3;) {
            blocks.push_back(kSizes[blocks.size() % 6]);
            with += blocks.back() != 0;
        }
        if (!replay("groups", blocks, in_order(blocks.size()), (unsigned long)g, 1)) return false;
    }
    {
        const std::vector<int> blocks = {64, 1, 129, 63, 65, 65, 2, 130, 64, 33};
        std::vector<int> order;
        for (int k = 0; k < 10; k++) order.push_back(k);
        for (int k = 9; k >= 0; k--) order.push_back(-k - 1);
        if (!replay("newest_first", blocks, order, 3, 1)) return false;
    }
    {
        std::vector<int> blocks, order;
        for (int k = 0; k < 12; k++) blocks.push_back(kSizes[k % 5]);
        for (int k = 0; k < 12; k++) order.push_back(k);
        for (int k = 0; k < 12; k++) order.push_back(-k - 1);
        if (!replay("all12", blocks, order, 3, 1)) return false;
    }
    return replay("damaged", {64, 65, 1, 63, 40, 65, 33, 64, 65, 129, 1}, in_order(11), 3, 1);
}

static bool illegal()
{
    for (int fused = 0; fused < 2; fused++) {
        itxp_sched S;
        itxp_actions A;
        itxp_init(&S, 4, 2, 1, fused);
        if (itxp_end(&S, 0, &A) != ITX_E_STATE) FAIL("end on an idle slot is not refused");
        if (itxp_begin(&S, 0, 1) != ITX_OK || itxp_join(&S, 0, &A) != ITX_OK || A.n != 0) FAIL("first begin");
        if (itxp_begin(&S, 0, 1) != ITX_E_STATE || itxp_begin(&S, 0, 0) != ITX_E_STATE) FAIL("begin on a busy slot is not refused");
        if (itxp_begin(&S, 1, 1) != ITX_OK) FAIL("second begin");              // ... and fails before it joins a group
        if (itxp_end(&S, 1, &A) != ITX_E_STATE || A.n != 0 || !S.slot[1].busy) FAIL("end after a begin that failed half way is not refused");
        if (itxp_begin(&S, 1, 1) != ITX_E_STATE) FAIL("the slot of a begin that failed half way is not busy");
        if (itxp_end(&S, 0, &A) != ITX_OK || A.n != (fused ? 3 : 2) || A.a[0].kind != ITXP_LAUNCH) FAIL("the other slot's end");
        // the launch fails: the group is closed and not launched, its member stays busy and its end is refused from now on
        if (itxp_end(&S, 0, &A) != ITX_E_STATE || !S.slot[0].busy || S.open_grp != -1) FAIL("end after a launch that failed is not refused");
    }
    return true;
}

int main()
{
    unsigned long configs = 0;
    static const int kLanesFused[3][2] = {{1, 0}, {2, 0}, {1, 1}};
    for (int slots : {1, 2, 4, 6})
        for (int group : {1, 2, 4})
            for (const auto &lf : kLanesFused)
                for (int n_pushes = 1; n_pushes <= MAX_PUSHES; n_pushes++) {
                    Model M;
                    model_init(&M, n_pushes, slots, group, lf[0], lf[1]);
                    g_seen.clear();
                    if (!walk(M)) {
                        fprintf(stderr, "  with %d slots, groups of %d, %d lanes, fused %d, %d pushes\n", slots, group, lf[0], lf[1], n_pushes);
                        return 1;
                    }
                    configs += n_pushes == MAX_PUSHES;
                }
    if (!scenarios()) return 1;
    if (!illegal()) return 1;
    printf("ok %lu configurations %lu states %lu transitions %lu ends\n", configs, g_states, g_transitions, g_ends);
    return 0;
}
