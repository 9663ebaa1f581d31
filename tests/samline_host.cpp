// samline_host.cpp — the SAM line rule of csrc/itx_samline.h built for the host, for tests/test_samline.py: runs the header's
// function over every body line of a SAM file and prints one line per line of the file,
//   H                                                        the rule calls the line hard
//   tid pos tmpend mapq flag5 mpos isize qname has_xa nm xa  otherwise (xa: the value cut out of the text by offset and length)
// after one "@<tid>\t<name>" line per @SQ line, as iteres_amd/host/test/reader_dump prints them.
// usage: samline_host <file.sam>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../include/iteres_amd.h"
#include "../iteres_amd/csrc/itx_samline.h"

typedef std::unordered_map<std::string, int> name_map;
static int64_t lookup(const void *names, const uint8_t *p, uint32_t n)
{
    const name_map *m = (const name_map *)names;
    auto it = m->find(std::string((const char *)p, n));
    return it == m->end() ? -1 : it->second;
}
ITX_SAMLINE_DEFINE(sam_line_host, const uint8_t *, lookup)

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    std::string text;
    char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, k);
    fclose(f);
    name_map names;
    size_t at = 0;
    int n_sq = 0;
    bool body = false;
    while (at < text.size()) {
        size_t nl = text.find('\n', at);
        const size_t stop = nl == std::string::npos ? text.size() : nl;
        const uint8_t *p = (const uint8_t *)text.data() + at;
        uint32_t len = (uint32_t)(stop - at);
        if (!body && len && p[0] == '@') {
            if (len >= 3 && memcmp(p, "@SQ", 3) == 0) {
                std::string line((const char *)p, len);
                size_t sn = line.find("\tSN:");
                if (sn != std::string::npos) {
                    std::string nm = line.substr(sn + 4, strcspn(line.c_str() + sn + 4, "\t\r\n"));
                    printf("@%d\t%s\n", n_sq, nm.c_str());
                    names.emplace(nm, n_sq);                       // the first occurrence wins a lookup
                    n_sq++;
                }
            }
        } else {
            body = true;
            ITX_SAM_STRIP(p, len);
            ItxSamRec r;
            sam_line_host(p, len, &names, &r);
            if (r.hard) {
                printf("H\n");
            } else {
                printf("%d\t%d\t%d\t%u\t%u\t%d\t%d\t%.*s\t%u\t%d\t%.*s\n", r.tid, r.pos, r.tmpend, (unsigned)r.mapq, (unsigned)ITX_FLAG5(r.flag), r.mpos, r.isize,
                       (int)r.qname_len, (const char *)p, (unsigned)r.has_xa, r.nm, (int)r.xa_len, (const char *)p + r.xa_off);
            }
        }
        at = stop + 1;
    }
    return 0;
}
