/* bwzoomrule_main.c — iteres_amd/csrc/itx_bwzoomrule.h driven with a table of counts, its decisions printed (tests/test_bwzoomrule.py
 * holds them against the restatement in tests/bwsparse.py). Valid as C11 and as C++17, like the header.
 *   bwzoomrule_main <full size> <mean resolution> <chromosomes> [<reduction>:<summaries> ...]
 * A reduction the table lacks ends the run with status 3: the rule asked for a count nobody expected. */
#include <stdio.h>
#include <stdlib.h>

#include "../iteres_amd/csrc/itx_bwzoomrule.h"

static int n_tab;
static long long tab_red[64];
static unsigned long long tab_n[64];

static unsigned long long count(long long red)
{
    for (int i = 0; i < n_tab; i++)
        if (tab_red[i] == red) return tab_n[i];
    printf("missing %lld\n", red);
    exit(3);
}

int main(int argc, char **argv)
{
    if (argc < 4 || argc > 4 + 64) return 2;
    for (int i = 4; i < argc; i++, n_tab++)
        if (sscanf(argv[i], "%lld:%llu", &tab_red[n_tab], &tab_n[n_tab]) != 2) return 2;
    itx_bwzoom Z;
    int w = itx_bwzoom_init(&Z, strtoull(argv[1], NULL, 10), atoi(argv[2]), strtoull(argv[3], NULL, 10));
    while (w == ITX_BWZ_COUNT) {
        printf("try %lld\n", Z.red);
        w = itx_bwzoom_first(&Z, count(Z.red));
    }
    if (w == ITX_BWZ_RANGE) {
        printf("range %lld rounds %u\n", Z.red, Z.reduce_rounds);
        return 0;
    }
    printf("fixed %u rounds %u\n", Z.reduction[0], Z.reduce_rounds);
    while (itx_bwzoom_next(&Z)) {
        const long long red = Z.red;
        const int from = Z.n_levels - 1, keep = itx_bwzoom_keep(&Z, count(red));
        printf("%s %lld from %u\n", keep ? "keep" : "drop", red, Z.reduction[from]);
    }
    printf("levels");
    for (int i = 0; i < Z.n_levels; i++) printf(" %u", Z.reduction[i]);
    printf("\n");
    return 0;
}
