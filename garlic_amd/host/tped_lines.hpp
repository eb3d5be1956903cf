// TPED text on the host: everything about a TPED line that is not an allele.  Header-only.
//
// The alleles of a line are parsed, coded and counted on the device (garlic_bed_set_rows_tped); the host reads the file
// through the slab reader and line cutter of text_slabs.hpp (zlib: plain text and .gz; a slab ends wherever the read ended, the
// file's last line needs no '\n', a '\r' before the '\n' belongs to the line and is a blank to the device; empty lines are
// passed over) and of every line parses the four leading tokens
//     chr  name  gpos  ppos
// exactly as parseTpedLine does: the prefix of the line up to the end of its fourth token goes through the same stream
// extraction (`ss >> chr >> name >> gpos >> ppos`, gpos and ppos as doubles), so "1e6" is a position here as it is there and
// what does not parse is 0 here as it is there.  The number of individuals is that of the first data line,
// (countFields - 4) / 2; a later line with another count is refused by the device and the file goes to the host reader.
//
// --tped-counting (feature counts) does not read through this path: a TPED image folds every letter that is not the line's
// first non-missing allele into "A2", so it cannot tell `C C` from `C G` when that allele is A, which the counting needs.
#pragma once
#include <cctype>
#include <cstdint>
#include <cstring>
#include <sstream>
#include <string>

#include "text_slabs.hpp"

namespace tped {

using text::Reader;
using text::SlabLines;

struct Lead {
    std::string chr, name;
    double gpos = 0, ppos = 0;
};

// whitespace-separated fields of [line, line + len): the host reader's countFields
inline int countFields(const char *line, size_t len)
{
    int n = 0;
    bool in = false;
    for (size_t k = 0; k < len; k++) {
        const char c = line[k];
        const bool ws = (c == ' ' || c == '\t' || c == '\r' || c == '\n');
        if (!ws && !in) n++;
        in = !ws;
    }
    return n;
}

// individuals of a line: (fields - 4) / 2 as src/garlic-data.cpp:59-60 has it (below 1: no genotype columns)
inline int individualsOf(const char *line, size_t len) { return (countFields(line, len) - 4) / 2; }

// the four leading tokens of [line, line + len); returns the offset behind the fourth token (where the alleles begin)
inline size_t parseLead(const char *line, size_t len, Lead &lead)
{
    size_t at = 0;
    for (int field = 0; field < 4; field++) {
        while (at < len && isspace((unsigned char)line[at])) at++;
        while (at < len && !isspace((unsigned char)line[at])) at++;
    }
    std::stringstream ss(std::string(line, at));
    lead = Lead();
    ss >> lead.chr >> lead.name >> lead.gpos >> lead.ppos;
    return at;
}

} // namespace tped
