// garlic_amd/host/tped_lines.hpp as a stand-alone program: the file `argv[1]` (plain or .gz) through the slab reader with slabs
// of `argv[2]` bytes, cut into lines, the four leading tokens of every line parsed.  Prints per line
//     number <tab> chr <tab> name <tab> gpos <tab> ppos <tab> individuals <tab> offset behind the fourth token
// and "tped_lines_unit ok" at the end.  tests/test_tped_cpu.py compares that with what it wrote, under ASan + UBSan.
#include <cstdio>
#include <cstdlib>

#include "../../garlic_amd/host/tped_lines.hpp"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: tped_lines_unit FILE SLAB_BYTES\n"); return 2; }
    const size_t cap = (size_t)atoll(argv[2]);
    tped::Reader rd;
    if (!rd.open(argv[1], cap)) { fprintf(stderr, "%s\n", rd.error.c_str()); return 1; }
    tped::SlabLines cut;
    size_t used = 0;
    long long lines = 0;
    do {
        if (!rd.next(used)) { fprintf(stderr, "%s\n", rd.error.c_str()); return 1; }
        used = cut.take(rd.slab.data(), rd.have, rd.eof);
        if (!rd.eof && used == 0 && rd.have == rd.slab.size()) { fprintf(stderr, "a line longer than the slab\n"); return 1; }
        for (size_t k = 0; k < cut.begin.size(); k++) {
            const char *line = rd.slab.data() + cut.begin[k];
            const size_t len = (size_t)(cut.end[k] - cut.begin[k]);
            tped::Lead lead;
            const size_t at = tped::parseLead(line, len, lead);
            printf("%lld\t%s\t%s\t%.17g\t%.17g\t%d\t%zu\n", (long long)cut.number[k], lead.chr.c_str(), lead.name.c_str(), lead.gpos, lead.ppos,
                   tped::individualsOf(line, len), at);
            lines++;
        }
    } while (!rd.eof || used < rd.have);
    // a line without tokens, and one with fewer than four
    tped::Lead lead;
    if (tped::parseLead("", 0, lead) != 0 || !lead.chr.empty() || lead.ppos != 0) return 3;
    if (tped::parseLead("7 rs", 4, lead) != 4 || lead.chr != "7" || lead.name != "rs" || lead.gpos != 0) return 3;
    if (tped::individualsOf("1 a 0 5 A C G", 13) != 1 || tped::individualsOf("1 a", 3) != -1) return 3;
    printf("tped_lines_unit ok %lld\n", lines);
    return 0;
}
