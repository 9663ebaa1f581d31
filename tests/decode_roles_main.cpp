// Stand-alone check of iteres_amd/csrc/itx_decode_roles.h (tests/test_decode_roles.py builds and runs it): for every pair of
// spans from {0, 1, 63, 64, 65, 129, 4 * 64 + 1}, every workgroup, wave and lane of the fused launch's grid (and some beyond it)
// against a literal loop that deals the blocks out: the first workgroups' wave 0 takes the current group's blocks 64 at a time, a
// lane each; the workgroups behind them take the previous group's, a wave each.
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../iteres_amd/csrc/itx_decode_roles.h"

static const uint32_t kSpans[7] = {0, 1, 63, 64, 65, 129, 4 * 64 + 1};

int main()
{
    unsigned long pairs = 0, waves = 0;
    for (uint32_t span_cur : kSpans)
        for (uint32_t span_prev : kSpans) {
            // the literal deal: (role, index) of every (workgroup, wave, lane); index -1: nothing
            std::vector<int> want_role, want_g;
            uint32_t want_wg = 0;
            for (uint32_t b = 0; b < span_cur; b += 64, want_wg++)
                for (uint32_t wave = 0; wave < ITXD_WAVES; wave++)
                    for (uint32_t lane = 0; lane < 64; lane++) {
                        const bool has = wave == 0 && b + lane < span_cur;
                        want_role.push_back(wave == 0 ? ITXD_PASS1 : ITXD_NONE);
                        want_g.push_back(has ? (int)(b + lane) : -1);
                    }
            const uint32_t want_n1 = want_wg;
            for (uint32_t b = 0; b < span_prev; b += ITXD_WAVES, want_wg++)
                for (uint32_t wave = 0; wave < ITXD_WAVES; wave++)
                    for (uint32_t lane = 0; lane < 64; lane++) {
                        const bool has = b + wave < span_prev;
                        want_role.push_back(has ? ITXD_PASS2 : ITXD_NONE);
                        want_g.push_back(has ? (int)(b + wave) : -1);
                    }
            itxd_grid r;
            const uint32_t n_wg = itxd_layout(&r, span_cur, span_prev);
            if (n_wg != want_wg || r.n1 != want_n1 || r.n1 + r.n2 != n_wg || r.span_cur != span_cur || r.span_prev != span_prev) {
                fprintf(stderr, "spans %u, %u: %u + %u workgroups, expected %u of which %u for pass 1\n", span_cur, span_prev, r.n1, r.n2, want_wg, want_n1);
                return 1;
            }
            std::vector<unsigned> hit_cur(span_cur, 0), hit_prev(span_prev, 0);
            for (uint32_t wg = 0; wg < n_wg + 3; wg++)                      // (the three behind the grid: nothing to do there)
                for (uint32_t wave = 0; wave < ITXD_WAVES; wave++) {
                    uint32_t first = 99;
                    const uint32_t wrole = itxd_role(r, wg, wave, &first);
                    for (uint32_t lane = 0; lane < 64; lane++) {
                        bool has = true;
                        uint32_t g = 99;
                        const uint32_t role = itxd_lane(r, wg, wave, lane, &has, &g);
                        const size_t at = ((size_t)wg * ITXD_WAVES + wave) * 64 + lane;
                        const int w_role = at < want_role.size() ? want_role[at] : (int)ITXD_NONE, w_g = at < want_g.size() ? want_g[at] : -1;
                        if (role != wrole || role != (uint32_t)w_role || (role != ITXD_PASS1 && role != ITXD_PASS2 && role != ITXD_NONE) || has != (w_g >= 0) ||
                            (has && g != (uint32_t)w_g)) {
                            fprintf(stderr, "spans %u, %u, workgroup %u wave %u lane %u: role %u %s index %u, expected role %d index %d\n", span_cur, span_prev, wg, wave,
                                    lane, role, has ? "with" : "without", g, w_role, w_g);
                            return 1;
                        }
                        if (role == ITXD_PASS1 && g != first + lane) return 2;
                        if (role == ITXD_PASS2 && g != first) return 2;
                        if (!has) continue;
                        // one role, one index, never beyond the group's span
                        if (role == ITXD_PASS1) {
                            if (g >= span_cur) return 3;
                            hit_cur[g]++;
                        } else {
                            if (g >= span_prev) return 3;
                            if (lane == 0) hit_prev[g]++;                  // a pass-2 wave: all its lanes on the one block
                        }
                    }
                    waves++;
                }
            for (uint32_t g = 0; g < span_cur; g++)
                if (hit_cur[g] != 1) {
                    fprintf(stderr, "spans %u, %u: block %u of the current group is taken %u times\n", span_cur, span_prev, g, hit_cur[g]);
                    return 1;
                }
            for (uint32_t g = 0; g < span_prev; g++)
                if (hit_prev[g] != 1) {
                    fprintf(stderr, "spans %u, %u: block %u of the previous group is taken by %u waves\n", span_cur, span_prev, g, hit_prev[g]);
                    return 1;
                }
            pairs++;
        }
    printf("ok %lu pairs %lu waves\n", pairs, waves);
    return 0;
}
