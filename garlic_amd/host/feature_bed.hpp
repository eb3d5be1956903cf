// Feature counts from a PLINK .bed: the row plan.  The counting genotypes stay in the file's 2-bit codes and become hom rows
// on the device (garlic_feature_set_rows_bed, csrc/bed_kernels.hpp); the host reads only the .bim and the .fam and says
// which image row and which homozygote every row of the feature set is.  Header-only and free of the device library, like
// feature_counts.hpp (tests/host_unit/feature_bed_unit.cpp).
//
// The semantics are those of the TPED line a .bed row stands for: hom A1 reads `A1 A1`, het `A1 A2`, hom A2 `A2 A2`, missing
// `0 0`.  So, as readCountingTped does per line:
//   * a .bim line whose (chromosome, position) carries annotations gives one row per annotated allele of the site, in key
//     order; a line without annotations gives none;
//   * the row's selector is 0 (hom A1) if the annotated allele is the .bim's A1, 1 (hom A2) if it is A2, 2 (no bit) if it
//     is neither -- and 2 for the annotated allele "0" and for a .bim allele `0` (the absent allele of a monomorphic site):
//     the script passes over a1 eq '0' before it looks the allele up;
//   * chromosomes are named through featureChrName, positions are integers, chromosome ids are given first seen first among
//     the annotated lines, and the rows are sorted by (chromosome id, position), rows of one position in the order they came.
// Refused with file and line: a .bim line without its six columns or with a position that is not a number, an allele of
// more than one character (as the calling .bed path refuses it), an annotated site whose A1 and A2 are the same character
// (one selector could not say "homozygous for it"), a .fam line without its two ids.
#pragma once
#include <memory>

#include "feature_counts.hpp"

namespace garlic_host {

struct FeatureBedPlan {
    int64_t image_rows = 0;                 // lines of the .bim = rows of the .bed image
    std::vector<int64_t> file_row;          // per row of the feature set: the image row ...
    std::vector<uint8_t> allele;            // ... and 0 = hom A1, 1 = hom A2, 2 = none
    std::vector<int32_t> chr, pos, effect;
    int64_t lines = 0, lines_annotated = 0;
    int64_t nrows() const { return (int64_t)file_row.size(); }
};

inline std::vector<std::string> readCountingFam(const std::string &path)      // the IIDs in file order
{
    FeatureLines in(path);
    std::vector<std::string> iid;
    std::string line;
    while (in.next(line)) {
        if (featureBlank(line)) continue;
        const std::vector<std::string> f = featureSplit(line, 3);
        if (f.size() < 2) featureFail(path, in.number, "a .fam line needs a family and an individual id");
        iid.push_back(f[1]);
    }
    return iid;
}

inline uint8_t featureBedSelector(const std::string &annotated, char a1, char a2)
{
    if (annotated == "0" || annotated.size() != 1) return 2;
    if (a1 != '0' && annotated[0] == a1) return 0;
    if (a2 != '0' && annotated[0] == a2) return 1;
    return 2;
}

inline FeatureBedPlan planCountingBim(const std::string &path, const FeatureAnnotations &ann, FeatureChrIds &chrs)
{
    FeatureLines in(path);
    FeatureBedPlan raw;
    std::string line;
    while (in.next(line)) {
        if (featureBlank(line)) continue;
        const int64_t row = raw.image_rows++;
        raw.lines++;
        std::vector<std::string> f = featureSplit(line);
        if (f[0].empty()) f.erase(f.begin());             // white space in front of the first column, as the calling path reads it
        if (f.size() != 6) featureFail(path, in.number, "a .bim line needs the 6 columns chr snpid gpos ppos a1 a2");
        int32_t p = 0;
        if (!featureNumber(f[3], &p)) featureFail(path, in.number, "position `" + f[3] + "` is not a number");
        for (int k = 4; k < 6; k++)
            if (f[(size_t)k].size() != 1)
                featureFail(path, in.number, "allele \"" + f[(size_t)k] + "\" is not a single character (GARLIC's alleles are single characters)");
        const std::string name = featureChrName(f[0]);
        const auto site = ann.site(name, p);
        if (site.first == site.second) continue;
        raw.lines_annotated++;
        const char a1 = f[4][0], a2 = f[5][0];
        if (a1 == a2 && a1 != '0') featureFail(path, in.number, std::string("both alleles are ") + a1);
        const int32_t c = chrs.of(name);
        for (auto it = site.first; it != site.second; ++it) {
            raw.file_row.push_back(row);
            raw.allele.push_back(featureBedSelector(std::get<2>(it->first), a1, a2));
            raw.chr.push_back(c);
            raw.pos.push_back(p);
            raw.effect.push_back(it->second);
        }
    }
    // into (chromosome id, position) order; rows of one position keep the order they came in
    const size_t n = raw.file_row.size();
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return raw.chr[a] != raw.chr[b] ? raw.chr[a] < raw.chr[b] : raw.pos[a] < raw.pos[b]; });
    FeatureBedPlan plan;
    plan.image_rows = raw.image_rows;
    plan.lines = raw.lines;
    plan.lines_annotated = raw.lines_annotated;
    plan.file_row.resize(n); plan.allele.resize(n); plan.chr.resize(n); plan.pos.resize(n); plan.effect.resize(n);
    for (size_t k = 0; k < n; k++) {
        const size_t o = order[k];
        plan.file_row[k] = raw.file_row[o]; plan.allele[k] = raw.allele[o];
        plan.chr[k] = raw.chr[o]; plan.pos[k] = raw.pos[o]; plan.effect[k] = raw.effect[o];
    }
    return plan;
}

// the .bed form of loadFeatureData: the feature file, the counting individuals and the plan; FeatureData::rows stays empty
// and FeatureData::bed is for the caller that opens the .bed (garlic_host.cpp)
inline FeatureData loadFeatureDataBed(const std::string &features, const std::string &bim, const std::string &fam)
{
    FeatureData d;
    d.ann = readFeatureFile(features);
    d.iid = readCountingFam(fam);
    if (d.iid.empty()) throw std::runtime_error(fam + ": no individuals");
    if (d.iid.size() >= ((size_t)1 << 30)) throw std::runtime_error(fam + ": too many individuals");
    d.plan = std::make_shared<const FeatureBedPlan>(planCountingBim(bim, d.ann, d.chrs));
    return d;
}

} // namespace garlic_host
