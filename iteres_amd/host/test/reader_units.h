/* reader_units.h — the test tools of this directory are built from the reader's four files, each a translation unit of its
 * own as in the product (tests/hosttool.py names them and defines ALN_SEPARATE_UNITS). The line the tools were built with
 * while the reader was one file, `gcc <tool>.c ../bamio.c ../tables.c -lz -ldl`, still gives a working tool — the tests of
 * earlier revisions, which are run against later trees, use it: without ALN_SEPARATE_UNITS the other three files come in
 * here, as part of the tool's own unit. A tool includes this file before anything else (_GNU_SOURCE); bgzf.c goes last: it
 * keeps struct aln_reader out of its own sight. */
#ifndef ALN_SEPARATE_UNITS
#define _GNU_SOURCE
#include "../bamdev.c"
#include "../samio.c"
#include "../bgzf.c"
#endif
