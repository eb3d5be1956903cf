// The host side of the feature counts (the reference's src/count_features_in_roh.pl; the counting itself:
// csrc/feature_kernels.hpp through garlic_feature_counts).  Header-only and free of the device library, so a sanitizer
// unit program runs it as it is (tests/host_unit/feature_counts_unit.cpp).
//
// What the script does, and what is kept of it:
//   * feature file: one line per annotated allele, `chrN:pos ref allele effect`, split on whitespace.  The key is
//     (chromosome, position, allele); `ref` is not read in TPED mode; a later line with the same key replaces the earlier
//     one, whose effect still gets its columns; one position may carry different effects for different alleles.
//   * counting genotypes: a TPED / TFAM of its own.  Per line and individual with alleles a1 a2: nothing if a1 is "0",
//     one count if a1 == a2 and (chr, pos, a1) is annotated.  A line whose position is not annotated is passed over after
//     its first four fields.  Matching is by chromosome name and physical position.
//   * the ROH of an individual on a chromosome: the .roh.bed lines under its track line; a position p is inside a line
//     `chr start end class ..` iff start <= p <= end - 1 (the writer puts the last SNP's position in `end`: a variant
//     exactly there is outside).  Inside: the line's class letter; else NONE.
//   * the table: per effect in bytewise order the columns <effect>A <effect>B <effect>C <effect>NONE, every name followed by
//     one space; then per counting individual `IID` and one " count" per column.  With more than three classes the script
//     counts D.. into a hash it never prints; here the columns then run A .. <last letter> NONE.
// Where this reader is stricter than the script: the script takes its chromosome from the file NAME (one file per
// chromosome, *chrN*, from a hard-coded 22 on) and compares positions as strings; here one file holds any chromosomes, its
// first column names them (as writeROHData: "chr" in front unless the name begins with c or C) and positions are
// integers.  A feature line without a colon, with fewer than four fields or with a position that is not a number, and a
// TPED / TFAM / .roh.bed line that is too short, end the run with a message that names file and line: the script goes on
// with undefined values.  Lines of white space alone are passed over.
#pragma once
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <ostream>
#include <regex>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

namespace garlic_host {

struct FeatureInterval {           // garlic_roh_interval of include/garlic_hip.h
    int32_t ind, chr, start, stop, cls;
};

constexpr int FEATURE_PRINTED_CLASSES = 3;      // the script's A, B, C
constexpr int FEATURE_MAX_CLASSES = 8;          // GARLIC_GMM_MAX_K

inline void featureFail(const std::string &file, long long line, const std::string &what)
{
    throw std::runtime_error(file + ":" + std::to_string(line) + ": " + what);
}

// plain or gzip, lines of any length, the end of line cut off
struct FeatureLines {
    gzFile f;
    std::string path;
    long long number = 0;
    explicit FeatureLines(const std::string &p) : f(gzopen(p.c_str(), "rb")), path(p)
    {
        if (!f) throw std::runtime_error("Failed to open " + p);
    }
    ~FeatureLines() { gzclose(f); }
    FeatureLines(const FeatureLines &) = delete;
    FeatureLines &operator=(const FeatureLines &) = delete;
    bool next(std::string &line)
    {
        line.clear();
        char buf[1 << 16];
        bool got = false;
        while (gzgets(f, buf, sizeof buf)) {
            got = true;
            line += buf;
            if (!line.empty() && line.back() == '\n') break;
        }
        if (!got) return false;
        while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
        number++;
        return true;
    }
};

inline bool featureSpace(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v'; }

inline bool featureBlank(const std::string &s)
{
    for (char c : s)
        if (!featureSpace(c)) return false;
    return true;
}

// perl's split(/\s+/, line, limit): a line that begins with white space has an empty first field; limit 0 = no limit
inline std::vector<std::string> featureSplit(const std::string &line, size_t limit = 0)
{
    std::vector<std::string> out;
    size_t i = 0;
    const size_t n = line.size();
    while (i <= n) {
        if (limit && out.size() + 1 == limit) {
            out.push_back(line.substr(i));
            return out;
        }
        size_t j = i;
        while (j < n && !featureSpace(line[j])) j++;
        out.push_back(line.substr(i, j - i));
        if (j >= n) break;
        while (j < n && featureSpace(line[j])) j++;
        if (j >= n) break;              // trailing white space: no empty last field
        i = j;
    }
    return out;
}

inline bool featureNumber(const std::string &s, int32_t *v)
{
    if (s.empty()) return false;
    char *end = nullptr;
    const long long x = strtoll(s.c_str(), &end, 10);
    if (*end || x < 0 || x > 0x7ffffffe) return false;
    *v = (int32_t)x;
    return true;
}

inline std::string featureChrName(const std::string &chr)      // as writeROHData names a chromosome
{
    return (!chr.empty() && (chr[0] == 'c' || chr[0] == 'C')) ? chr : "chr" + chr;
}

struct FeatureAnnotations {
    std::vector<std::string> effects;                                          // bytewise order; an effect's id is its index
    std::map<std::tuple<std::string, int32_t, std::string>, int32_t> allele;   // (chromosome, position, allele) -> effect id
    // the annotated alleles of a site, in key order: [first, last)
    auto site(const std::string &chr, int32_t pos) const
    {
        auto first = allele.lower_bound(std::make_tuple(chr, pos, std::string()));
        auto last = first;
        while (last != allele.end() && std::get<0>(last->first) == chr && std::get<1>(last->first) == pos) ++last;
        return std::make_pair(first, last);
    }
};

inline FeatureAnnotations readFeatureFile(const std::string &path)
{
    FeatureLines in(path);
    std::map<std::tuple<std::string, int32_t, std::string>, std::string> byKey;
    std::map<std::string, int32_t> names;
    std::string line;
    while (in.next(line)) {
        if (featureBlank(line)) continue;
        const std::vector<std::string> f = featureSplit(line);
        if (f.size() < 4) featureFail(path, in.number, "a feature line needs `chrN:pos ref allele effect`");
        const size_t colon = f[0].find(':');
        if (colon == std::string::npos) featureFail(path, in.number, "no colon in `" + f[0] + "` (chrN:pos)");
        const size_t colon2 = f[0].find(':', colon + 1);
        int32_t pos = 0;
        const std::string text = f[0].substr(colon + 1, colon2 == std::string::npos ? std::string::npos : colon2 - colon - 1);
        if (!featureNumber(text, &pos)) featureFail(path, in.number, "position `" + text + "` is not a number");
        byKey[std::make_tuple(featureChrName(f[0].substr(0, colon)), pos, f[2])] = f[3];     // a later line replaces an earlier one
        names[f[3]] = 0;                                                                      // ... whose effect keeps its columns
    }
    FeatureAnnotations a;
    for (auto &kv : names) {           // std::map<std::string>: bytewise order, as perl's sort
        kv.second = (int32_t)a.effects.size();
        a.effects.push_back(kv.first);
    }
    for (const auto &kv : byKey) a.allele[kv.first] = names[kv.second];
    return a;
}

inline std::vector<std::string> readCountingTfam(const std::string &path)
{
    FeatureLines in(path);
    std::vector<std::string> iid;
    std::string line;
    while (in.next(line)) {
        if (featureBlank(line)) continue;
        const std::vector<std::string> f = featureSplit(line, 3);
        if (f.size() < 2) featureFail(path, in.number, "a TFAM line needs a family and an individual id");
        iid.push_back(f[1]);
    }
    return iid;
}

// chromosome names -> the ids the rows and the intervals share (first seen first)
struct FeatureChrIds {
    std::map<std::string, int32_t> id;
    int32_t of(const std::string &name)
    {
        auto it = id.find(name);
        if (it != id.end()) return it->second;
        const int32_t k = (int32_t)id.size();
        id.emplace(name, k);
        return k;
    }
};

// the hom rows of the counting genotypes: one per TPED line and annotated allele of its site, sorted by (chromosome id,
// position); bit i & 7 of byte i >> 3 of a row is individual i
struct FeatureRows {
    int32_t nind = 0;
    int64_t row_bytes = 0;
    std::vector<int32_t> chr, pos, effect;
    std::vector<uint8_t> bits;
    int64_t lines = 0, lines_annotated = 0;
    int64_t nrows() const { return (int64_t)chr.size(); }
};

inline FeatureRows readCountingTped(const std::string &path, const FeatureAnnotations &ann, int32_t nind, FeatureChrIds &chrs)
{
    FeatureLines in(path);
    FeatureRows rows;
    rows.nind = nind;
    rows.row_bytes = ((int64_t)nind + 7) / 8;
    std::vector<int32_t> chr, pos, effect;
    std::vector<uint8_t> bits;
    std::string line;
    while (in.next(line)) {
        if (featureBlank(line)) continue;
        rows.lines++;
        const std::vector<std::string> head = featureSplit(line, 5);       // chr, id, genetic position, position, the genotypes
        if (head.size() < 4) featureFail(path, in.number, "a TPED line needs chromosome, id, genetic position and position");
        int32_t p = 0;
        if (!featureNumber(head[3], &p)) featureFail(path, in.number, "position `" + head[3] + "` is not a number");
        const std::string name = featureChrName(head[0]);
        const auto site = ann.site(name, p);
        if (site.first == site.second) continue;                           // not annotated: the genotypes are not read
        rows.lines_annotated++;
        const std::vector<std::string> g = featureSplit(head.size() > 4 ? head[4] : std::string());
        if ((int64_t)g.size() < 2 * (int64_t)nind) featureFail(path, in.number, "fewer than " + std::to_string(2 * (int64_t)nind) + " alleles");
        const int32_t c = chrs.of(name);
        for (auto it = site.first; it != site.second; ++it) {
            const std::string &allele = std::get<2>(it->first);
            chr.push_back(c);
            pos.push_back(p);
            effect.push_back(it->second);
            const size_t at = bits.size();
            bits.resize(at + (size_t)rows.row_bytes, 0);
            if (allele == "0") continue;                                   // a1 eq '0' is passed over before the look-up
            for (int32_t i = 0; i < nind; i++)
                if (g[2 * (size_t)i] == allele && g[2 * (size_t)i + 1] == allele) bits[at + (size_t)(i >> 3)] |= (uint8_t)(1u << (i & 7));
        }
    }
    // into (chromosome id, position) order; rows of one position keep the order they came in
    const size_t n = chr.size();
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return chr[a] != chr[b] ? chr[a] < chr[b] : pos[a] < pos[b]; });
    rows.chr.resize(n); rows.pos.resize(n); rows.effect.resize(n);
    rows.bits.resize(n * (size_t)rows.row_bytes);
    for (size_t k = 0; k < n; k++) {
        rows.chr[k] = chr[order[k]]; rows.pos[k] = pos[order[k]]; rows.effect[k] = effect[order[k]];
        if (rows.row_bytes) memcpy(&rows.bits[k * (size_t)rows.row_bytes], &bits[order[k] * (size_t)rows.row_bytes], (size_t)rows.row_bytes);
    }
    return rows;
}

struct FeatureBedPlan;     // feature_bed.hpp
struct BedFile;            // garlic_host.hpp

// everything a count needs of the three input files
struct FeatureData {
    FeatureAnnotations ann;
    std::vector<std::string> iid;      // the counting TFAM's (or .fam's) individuals, in file order
    FeatureChrIds chrs;
    FeatureRows rows;
    // the .bed form (feature_bed.hpp): instead of `rows`, which image row and which homozygote every row is, and the open
    // counting file set whose image the device turns into hom rows (one reference, dropped by releaseFeatureCounts)
    std::shared_ptr<const FeatureBedPlan> plan;
    BedFile *bed = nullptr;
};

inline FeatureData loadFeatureData(const std::string &features, const std::string &tped, const std::string &tfam)
{
    FeatureData d;
    d.ann = readFeatureFile(features);
    d.iid = readCountingTfam(tfam);
    if (d.iid.empty()) throw std::runtime_error(tfam + ": no individuals");
    if (d.iid.size() > 0x7fffffff) throw std::runtime_error(tfam + ": too many individuals");
    d.rows = readCountingTped(tped, d.ann, (int32_t)d.iid.size(), d.chrs);
    return d;
}

// the TFAM that goes with a TPED: the script's s/\.tped/\.tfam/g
inline std::string featureTfamOf(std::string tped)
{
    for (size_t at = 0; (at = tped.find(".tped", at)) != std::string::npos; at += 5) tped.replace(at, 5, ".tfam");
    return tped;
}

inline std::map<std::string, int32_t> featureIndividuals(const std::vector<std::string> &iid)
{
    std::map<std::string, int32_t> of;
    for (size_t i = 0; i < iid.size(); i++) of.emplace(iid[i], (int32_t)i);      // a repeated id: its first line
    return of;
}

// (individual, chromosome, start): the order garlic_feature_counts asks for
inline void featureSortIntervals(std::vector<FeatureInterval> &iv)
{
    std::stable_sort(iv.begin(), iv.end(), [](const FeatureInterval &a, const FeatureInterval &b) {
        return std::tie(a.ind, a.chr, a.start) < std::tie(b.ind, b.chr, b.start);
    });
}

// The intervals of a .roh.bed: the script's track-line pattern and columns.  Individuals that the counting TFAM does not
// list are passed over.  *n_classes: 3, or more when a class letter past C occurs.
inline std::vector<FeatureInterval> readRohBed(const std::string &path, const std::vector<std::string> &iid, FeatureChrIds &chrs, int *n_classes)
{
    static const std::regex track("^track .+Ind: (.+) Pop:(.+) ROH.+");
    const std::map<std::string, int32_t> of = featureIndividuals(iid);
    FeatureLines in(path);
    std::vector<FeatureInterval> iv;
    int classes = FEATURE_PRINTED_CLASSES;
    int32_t ind = -1;
    std::string line;
    std::smatch m;
    while (in.next(line)) {
        if (std::regex_match(line, m, track)) {
            auto it = of.find(m[1].str());
            ind = it == of.end() ? -1 : it->second;
            continue;
        }
        if (featureBlank(line)) continue;
        const std::vector<std::string> f = featureSplit(line, 6);
        if (f.size() < 4) featureFail(path, in.number, "a ROH line needs chromosome, start, end and class");
        FeatureInterval v;
        if (!featureNumber(f[1], &v.start) || !featureNumber(f[2], &v.stop)) featureFail(path, in.number, "start or end is not a number");
        if (f[3].size() != 1 || f[3][0] < 'A' || f[3][0] >= 'A' + FEATURE_MAX_CLASSES)
            featureFail(path, in.number, "class `" + f[3] + "` (A to " + std::string(1, (char)('A' + FEATURE_MAX_CLASSES - 1)) + ")");
        if (v.stop < v.start) featureFail(path, in.number, "end before start");
        v.cls = f[3][0] - 'A';
        classes = std::max(classes, v.cls + 1);
        if (ind < 0) continue;
        v.ind = ind;
        v.chr = chrs.of(featureChrName(f[0]));
        iv.push_back(v);
    }
    featureSortIntervals(iv);
    if (n_classes) *n_classes = classes;
    return iv;
}

// writeROHData's class of a size: the first boundary the size lies below; past the last one: the next class
inline int featureSizeClass(double size, const std::vector<double> &bounds)
{
    size_t i = 0;
    while (i < bounds.size() && !(size < bounds[i])) i++;
    return (int)i;
}

// The intervals of calls that are still in memory: per panel individual its id and its segments (chromosome name as the
// map has it, start, stop, size).  Panel individuals map to counting individuals by id; the others are passed over.
struct FeatureCall {
    std::string chr;
    int32_t start, stop;
    double size;
};
inline std::vector<FeatureInterval> buildFeatureIntervals(const std::vector<std::string> &panel_iid, const std::vector<std::vector<FeatureCall>> &calls,
                                                          const std::vector<double> &bounds, const std::vector<std::string> &iid,
                                                          FeatureChrIds &chrs, int *n_classes)
{
    const std::map<std::string, int32_t> of = featureIndividuals(iid);
    std::vector<FeatureInterval> iv;
    for (size_t k = 0; k < panel_iid.size() && k < calls.size(); k++) {
        auto it = of.find(panel_iid[k]);
        if (it == of.end()) continue;
        for (const FeatureCall &c : calls[k])
            iv.push_back(FeatureInterval{it->second, chrs.of(featureChrName(c.chr)), c.start, c.stop, featureSizeClass(c.size, bounds)});
    }
    featureSortIntervals(iv);
    if (n_classes) *n_classes = std::max<int>(FEATURE_PRINTED_CLASSES, (int)bounds.size() + 1);
    return iv;
}

// counts[ind][n_classes + 1][n_effects], class n_classes = NONE
inline void writeFeatureTable(std::ostream &out, const std::vector<std::string> &effects, const std::vector<std::string> &iid,
                              const int64_t *counts, int n_classes)
{
    const size_t ne = effects.size();
    for (const std::string &e : effects) {
        for (int c = 0; c < n_classes; c++) out << e << (char)('A' + c) << ' ';
        out << e << "NONE ";
    }
    out << '\n';
    for (size_t i = 0; i < iid.size(); i++) {
        out << iid[i];
        for (size_t e = 0; e < ne; e++)
            for (int c = 0; c <= n_classes; c++) out << ' ' << counts[(i * (size_t)(n_classes + 1) + (size_t)c) * ne + e];
        out << '\n';
    }
}

} // namespace garlic_host
