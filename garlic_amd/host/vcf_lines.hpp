// VCF text on the host: everything about a VCF that is not a genotype.  Header-only.
//
// The genotypes of a data line are parsed on the device (garlic_bed_set_rows_vcf); the host reads the file through zlib
// (gzopen: plain text, .gz, and bgzf as multi-member gzip), skips the ## lines, takes the individuals from the #CHROM line,
// and of every data line parses the nine fixed columns into the .bim fields
//     chr = CHROM, name = ID, gpos = 0, ppos = POS, a1 = REF, a2 = ALT
// checking that FORMAT begins with GT.  A line whose REF or ALT is not exactly one character (`,` lists, `.`, `*`, `<...>`
// included) is no biallelic SNP: refused, or under skipNonSnp left out of line_begin and counted.
//
// The text goes to the device in slabs of lines (text_slabs.hpp); a '\r' before the '\n' belongs to the line (the device
// accepts it as the end of a genotype).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "text_slabs.hpp"

namespace vcf {

using text::Reader;          // the names the VCF readers have always used for them
using text::SlabLines;

struct Site {
    std::string chr, name;
    double gpos = 0;
    long long ppos = 0;
    char a1 = 0, a2 = 0;
};

enum LineKind { LINE_SNP = 0, LINE_NOT_SNP = 1, LINE_BAD = 2 };

// the samples of a "#CHROM POS ID REF ALT QUAL FILTER INFO FORMAT s0 s1 ..." line (tab-separated; a trailing \r is dropped)
inline bool parseHeader(const char *line, size_t len, std::vector<std::string> &samples, std::string &err)
{
    while (len && (line[len - 1] == '\n' || line[len - 1] == '\r')) len--;
    std::vector<std::string> cols;
    size_t at = 0;
    while (at <= len) {
        const char *tab = (const char *)memchr(line + at, '\t', len - at);
        const size_t end = tab ? (size_t)(tab - line) : len;
        cols.emplace_back(line + at, end - at);
        at = end + 1;
    }
    if (cols.size() < 10 || cols[0] != "#CHROM" || cols[8] != "FORMAT") {
        err = "the #CHROM line needs the nine fixed columns up to FORMAT and at least one sample";
        return false;
    }
    samples.assign(cols.begin() + 9, cols.end());
    for (const std::string &s : samples)
        if (s.empty()) { err = "the #CHROM line has an empty sample name"; return false; }
    return true;
}

// the nine fixed columns of a data line [line, line + len) (len stops at or before the '\n')
inline LineKind parseFixed(const char *line, size_t len, Site &site, std::string &err)
{
    const char *col[10];
    size_t n = 0, at = 0;
    col[0] = line;
    while (n < 9 && len) {
        const char *tab = (const char *)memchr(line + at, '\t', len - at);
        if (!tab) break;
        at = (size_t)(tab - line) + 1;
        col[++n] = line + at;
    }
    if (n < 9) { err = "fewer than nine fixed columns and one sample"; return LINE_BAD; }
    auto width = [&](int k) { return (size_t)(col[k + 1] - col[k]) - 1; };
    if (width(0) == 0 || width(1) == 0 || width(2) == 0) { err = "empty CHROM, POS or ID"; return LINE_BAD; }
    site.chr.assign(col[0], width(0));
    site.name.assign(col[2], width(2));
    site.gpos = 0;
    const std::string pos(col[1], width(1));
    char *stop = nullptr;
    site.ppos = strtoll(pos.c_str(), &stop, 10);
    if (*stop || site.ppos < 0) { err = "POS '" + pos + "' is no position"; return LINE_BAD; }
    if (width(8) < 2 || col[8][0] != 'G' || col[8][1] != 'T' || (width(8) > 2 && col[8][2] != ':')) {
        err = "FORMAT '" + std::string(col[8], width(8)) + "' does not begin with GT";
        return LINE_BAD;
    }
    auto base = [](char c) { return c != '.' && c != '*' && c != ',' && c != '<' && c != '>'; };
    if (width(3) != 1 || width(4) != 1 || !base(col[3][0]) || !base(col[4][0])) {
        err = "REF '" + std::string(col[3], width(3)) + "' ALT '" + std::string(col[4], width(4)) + "' is no biallelic SNP";
        return LINE_NOT_SNP;
    }
    site.a1 = col[3][0];
    site.a2 = col[4][0];
    return LINE_SNP;
}

// The scalar FORMAT subfield `key` of a data line's sample columns, as the device defines it (csrc/vcf_gl_kernels.hpp): the
// line ends at its first \r or \n; k = the index of the first key of FORMAT (column 8) that equals `key`; sample j is column
// 9 + j and its value is subfield k of the column.  A column without subfield k, an empty one and "." are missing: on a column
// that starts with '.' the value is *missing, or 0 without one; on any other column *missing, or the line is refused.  Every
// other subfield goes through strtod, which must consume all of it and give a finite value: a list (0,12,40), trailing junk, nan
// and inf are refused (hex floats pass, as strtod reads them).
// out[i] = the value of sample cols[i], i < ncols (cols == NULL: sample i).  false: err says why and `sample` names the
// sample column (-1: the line as a whole).
inline bool parseGlValues(const char *line, size_t len, const std::string &key, int nsamples, const int *cols, size_t ncols,
                          const double *missing, double *out, int &sample, std::string &err)
{
    sample = -1;
    for (size_t i = 0; i < len; i++)
        if (line[i] == '\r' || line[i] == '\n') { len = i; break; }
    std::vector<size_t> begin;           // of every column; begin[c + 1] - 1 is where column c ends
    begin.push_back(0);
    for (size_t i = 0; i < len; i++)
        if (line[i] == '\t') begin.push_back(i + 1);
    begin.push_back(len + 1);
    const size_t ncolumns = begin.size() - 1;
    const size_t found = ncolumns > 9 ? ncolumns - 9 : 0;
    if (found < (size_t)nsamples || ncolumns < 10) { err = "too few sample columns (" + std::to_string(found) + ")"; return false; }
    if (found > (size_t)nsamples) { err = "too many sample columns (" + std::to_string(found) + ")"; return false; }
    // subfield `want` of [b, e): false when the column has fewer colons
    auto subfield = [&](size_t b, size_t e, long want, size_t &sb, size_t &se) {
        long at = 0;
        sb = b;
        for (size_t i = b; i <= e; i++) {
            if (i < e && line[i] != ':') continue;
            if (at == want) { se = i; return true; }
            at++;
            sb = i + 1;
        }
        return false;
    };
    long k = -1;
    {
        const size_t b = begin[8], e = begin[9] - 1;
        size_t sb, se;
        for (long at = 0; subfield(b, e, at, sb, se); at++)
            if (se - sb == key.size() && memcmp(line + sb, key.data(), key.size()) == 0) { k = at; break; }
    }
    if (k < 0) { err = "FORMAT '" + std::string(line + begin[8], begin[9] - 1 - begin[8]) + "' does not name " + key; return false; }
    for (size_t i = 0; i < ncols; i++) {
        const int j = cols ? cols[i] : (int)i;
        const size_t b = begin[(size_t)(9 + j)], e = begin[(size_t)(10 + j)] - 1;
        size_t sb = b, se = b;
        const bool have = subfield(b, e, k, sb, se);
        if (!have || se == sb || (se - sb == 1 && line[sb] == '.')) {
            if (missing) out[i] = *missing;
            else if (e > b && line[b] == '.') out[i] = 0.0;
            else { sample = j; err = "a called genotype without " + key + " (--vcf-gl-missing X gives such genotypes the raw value X)"; return false; }
            continue;
        }
        const std::string tok(line + sb, se - sb);
        char *stop = nullptr;
        out[i] = strtod(tok.c_str(), &stop);
        if (stop == tok.c_str() || *stop || tok.size() != strlen(tok.c_str())) {
            sample = j;
            err = key + " '" + tok + "' is no single number" + (tok.find(',') != std::string::npos ? " (a list: only scalar FORMAT fields are read)" : "");
            return false;
        }
        if (!std::isfinite(out[i])) {      // nan, inf, 1e999: strtod reads them, no likelihood is one
            sample = j;
            err = key + " '" + tok + "' is no finite number";
            return false;
        }
    }
    return true;
}

// lines of a file that do not start with '#': the counting pass in front of garlic_bed_create
inline bool countDataLines(const std::string &path, int64_t &nlines, std::string &err)
{
    nlines = 0;
    const text::SlabsEnd end = text::forEachSlab(path, 1 << 22, err, [&](const text::Reader &rd, const text::SlabLines &cut, size_t) {
        for (int64_t b : cut.begin) nlines += rd.slab[(size_t)b] != '#';
        return true;
    });
    if (end == text::SLABS_LONG_LINE) err = "a line longer than the slab";
    return end == text::SLABS_DONE;
}

} // namespace vcf
