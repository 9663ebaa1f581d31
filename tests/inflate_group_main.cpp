// Stand-alone check of iteres_amd/csrc/itx_inflate_group.h (tests/test_inflate_group_index.py builds and runs it): every
// group of one to four slots with block counts from {0, 1, 63, 64, 65, 129}, in every order, against a literal loop that
// lays the slots out one after the other.
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../iteres_amd/csrc/itx_inflate_group.h"

static const uint32_t kCounts[6] = {0, 1, 63, 64, 65, 129};

int main()
{
    unsigned long groups = 0, indices = 0;
    for (uint32_t n_slots = 1; n_slots <= ITXG_SLOTS; n_slots++) {
        uint32_t combos = 1;
        for (uint32_t k = 0; k < n_slots; k++) combos *= 6;
        for (uint32_t c = 0; c < combos; c++) {
            uint32_t counts[ITXG_SLOTS] = {0, 0, 0, 0};
            for (uint32_t k = 0, x = c; k < n_slots; k++, x /= 6) counts[k] = kCounts[x % 6];
            // the literal layout: slot and local index of every group-wide index, -1 where there is no block
            std::vector<int> want_slot, want_local;
            uint32_t want_span = 0;
            for (uint32_t k = 0; k < n_slots; k++) {
                while (want_slot.size() % 64) {
                    want_slot.push_back(-1);
                    want_local.push_back(-1);
                }
                for (uint32_t i = 0; i < counts[k]; i++) {
                    want_slot.push_back((int)k);
                    want_local.push_back((int)i);
                }
                if (counts[k]) want_span = (uint32_t)want_slot.size();
            }
            itxg_index x;
            const uint32_t span = itxg_layout(&x, counts, n_slots);
            if (span != want_span || x.n_slots != n_slots) {
                fprintf(stderr, "combination %u of %u slots: span %u, expected %u\n", c, n_slots, span, want_span);
                return 1;
            }
            for (uint32_t k = 0; k < n_slots; k++)
                if (x.first[k] % 64u || x.n[k] != counts[k]) {
                    fprintf(stderr, "combination %u of %u slots: slot %u starts at %u with %u blocks\n", c, n_slots, k, x.first[k], x.n[k]);
                    return 1;
                }
            for (uint32_t g = 0; g < (uint32_t)want_slot.size() + 130u; g++) {
                uint32_t slot = 99, local = 99;
                const bool is_block = itxg_locate(x, g, &slot, &local);
                const int ws = g < want_slot.size() ? want_slot[g] : -1, wl = g < want_slot.size() ? want_local[g] : -1;
                const bool ok = ws < 0 ? !is_block : (is_block && (int)slot == ws && (int)local == wl);
                if (!ok || slot >= n_slots) {
                    fprintf(stderr, "combination %u of %u slots, index %u: got %s slot %u local %u, expected slot %d local %d\n", c, n_slots, g, is_block ? "block" : "padding",
                            slot, local, ws, wl);
                    return 1;
                }
                // a pass-1 wave asks for its first index only: the slot must hold for all 64
                if (is_block && g % 64u) {
                    uint32_t s0, l0;
                    (void)itxg_locate(x, g - g % 64u, &s0, &l0);
                    if (s0 != slot || l0 + g % 64u != local) {
                        fprintf(stderr, "combination %u of %u slots, index %u: its wave starts in slot %u at %u\n", c, n_slots, g, s0, l0);
                        return 1;
                    }
                }
                indices++;
            }
            groups++;
        }
    }
    printf("ok %lu groups %lu indices\n", groups, indices);
    return 0;
}
