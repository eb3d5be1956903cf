// Stand-alone check of garlic_amd/host/feature_bed.hpp (built by tests/test_feature_bed_cpu.py with ASan + UBSan): the row
// plan of a hand-written .bim / .fam / feature file -- selectors 0, 1 and 2, a `0` allele on either side, a replaced
// duplicate key, two alleles at one site, chromosome-name prefixing, the (chromosome id, position) order -- and the
// refusals with file and line.  argv[1]: a directory to write into.
#include <cstdio>
#include <fstream>
#include <iostream>

#include "../../garlic_amd/host/feature_bed.hpp"

using namespace garlic_host;

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::cerr << "line " << __LINE__ << ": " #c " fails\n";       \
            failures++;                                                   \
        }                                                                 \
    } while (0)

static void put(const std::string &path, const std::string &text)
{
    std::ofstream f(path.c_str());
    f << text;
}

static std::string refusal(const std::string &bim, const FeatureAnnotations &ann)
{
    FeatureChrIds chrs;
    try {
        planCountingBim(bim, ann, chrs);
    } catch (const std::exception &e) {
        return e.what();
    }
    return "";
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string d = std::string(argv[1]) + "/";
    put(d + "f.txt",
        "chr2:100 N A dam\n"        // A is the .bim's A1: selector 0
        "chr2:100 N G ben\n"        // the second allele of the site, A2: selector 1
        "chr2:200 N T dam\n"        // a duplicate key ...
        "chr2:200 N T lof\n"        // ... replaced: lof; T is neither A nor C: selector 2
        "1:50 N C ben\n"            // the feature file names the chromosome bare, the .bim with chr
        "chr1:70 N 0 dam\n"         // the annotated allele `0`: selector 2
        "chr1:80 N G dam\n"         // A1 of the .bim is 0 (monomorphic), G is A2: selector 1
        "chr1:90 N 0 ben\n"         // annotated `0` on a monomorphic site whose A1 is 0: still 2
        "chr1:90 N T dam\n"         // A2 is 0 and T is A1: selector 0
        "chr3:5 N A lof\n");        // a site the .bim does not have
    put(d + "c.bim",
        "2\trs1\t0\t200\tA\tC\n"       // row 0: chr2 first seen -> chromosome id 0
        "2\trs2\t0\t100\tA\tG\n"       // row 1: out of order in the file, sorted in the plan
        "2\trs3\t0\t150\tA\tG\n"       // row 2: not annotated
        "chr1\trs4\t0\t50\tT\tC\n"     // row 3
        "chr1\trs5\t0\t70\tA\tG\n"     // row 4
        "chr1\trs6\t0\t80\t0\tG\n"     // row 5
        "\n"                            // a blank line is no row
        " chr1 rs7 0 90 T 0\n");       // row 6: white space in front
    put(d + "c.fam", "F1 I1 0 0 0 -9\nF1 I2 0 0 0 -9\n\nF2 I3 0 0 0 -9\n");

    const FeatureAnnotations ann = readFeatureFile(d + "f.txt");
    CHECK(ann.effects.size() == 3 && ann.effects[0] == "ben" && ann.effects[1] == "dam" && ann.effects[2] == "lof");
    const std::vector<std::string> iid = readCountingFam(d + "c.fam");
    CHECK(iid.size() == 3 && iid[0] == "I1" && iid[2] == "I3");
    FeatureChrIds chrs;
    const FeatureBedPlan p = planCountingBim(d + "c.bim", ann, chrs);
    CHECK(p.image_rows == 7 && p.lines == 7 && p.lines_annotated == 6);
    CHECK(chrs.id.size() == 2 && chrs.of("chr2") == 0 && chrs.of("chr1") == 1);
    // (chromosome id, position): chr2:100 A, chr2:100 G, chr2:200 T, chr1:50 C, chr1:70 0, chr1:80 G, chr1:90 0, chr1:90 T
    const int64_t file_row[] = {1, 1, 0, 3, 4, 5, 6, 6};
    const int allele[] = {0, 1, 2, 1, 2, 1, 2, 0};
    const int32_t chr[] = {0, 0, 0, 1, 1, 1, 1, 1};
    const int32_t pos[] = {100, 100, 200, 50, 70, 80, 90, 90};
    const int32_t effect[] = {1, 0, 2, 0, 1, 1, 0, 1};
    CHECK(p.nrows() == 8);
    for (int k = 0; k < 8 && k < p.nrows(); k++) {
        CHECK(p.file_row[(size_t)k] == file_row[k]);
        CHECK(p.allele[(size_t)k] == allele[k]);
        CHECK(p.chr[(size_t)k] == chr[k] && p.pos[(size_t)k] == pos[k] && p.effect[(size_t)k] == effect[k]);
    }
    CHECK(featureBedSelector("A", 'A', 'G') == 0 && featureBedSelector("G", 'A', 'G') == 1 && featureBedSelector("T", 'A', 'G') == 2);
    CHECK(featureBedSelector("0", '0', 'G') == 2 && featureBedSelector("AT", 'A', 'G') == 2);

    // the whole .bed form of loadFeatureData
    const FeatureData data = loadFeatureDataBed(d + "f.txt", d + "c.bim", d + "c.fam");
    CHECK(data.plan && data.plan->nrows() == 8 && data.iid.size() == 3 && data.rows.nrows() == 0 && data.bed == nullptr);

    // refusals, with file and line
    put(d + "two.bim", "2\trs1\t0\t200\tA\tC\n2\trs2\t0\t100\tAT\tG\n");
    std::string e = refusal(d + "two.bim", ann);
    CHECK(e.find("two.bim:2:") != std::string::npos && e.find("\"AT\"") != std::string::npos && e.find("single character") != std::string::npos);
    put(d + "short.bim", "2\trs1\t0\t200\tA\tC\n\n2\trs2\t0\t100\tA\n");
    e = refusal(d + "short.bim", ann);
    CHECK(e.find("short.bim:3:") != std::string::npos && e.find("6 columns") != std::string::npos);
    put(d + "pos.bim", "2\trs1\t0\t2x0\tA\tC\n");
    e = refusal(d + "pos.bim", ann);
    CHECK(e.find("pos.bim:1:") != std::string::npos && e.find("not a number") != std::string::npos);
    put(d + "same.bim", "2\trs1\t0\t150\tA\tA\n2\trs2\t0\t100\tG\tG\n");      // only an annotated site is refused for it
    e = refusal(d + "same.bim", ann);
    CHECK(e.find("same.bim:2:") != std::string::npos && e.find("both alleles are G") != std::string::npos);
    put(d + "bad.fam", "F1 I1 0 0 0 -9\nF1\n");
    try {
        readCountingFam(d + "bad.fam");
        CHECK(false);
    } catch (const std::exception &x) {
        CHECK(std::string(x.what()).find("bad.fam:2:") != std::string::npos);
    }
    try {
        readCountingFam(d + "none.fam");
        CHECK(false);
    } catch (const std::exception &x) {
        CHECK(std::string(x.what()).find("Failed to open") != std::string::npos);
    }
    if (failures) return 1;
    std::cout << "feature_bed_unit ok\n";
    return 0;
}
