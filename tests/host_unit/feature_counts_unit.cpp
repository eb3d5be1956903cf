// garlic_amd/host/feature_counts.hpp without a device: the readers on the golden inputs of tests/golden/features, the two
// interval builders, and the table writer byte for byte against the script's table -- the counting itself done here by a
// plain loop over rows, bits and intervals.  tests/test_feature_counts_cpu.py builds this under -fsanitize=address,undefined.
//
//   feature_counts_unit <work dir> (<features> <tped> <tfam> <roh.bed> <expected table>) ...
//   prints one line per case and "feature_counts_unit ok" at the end
#include "../../garlic_amd/host/feature_counts.hpp"

#include <cstdio>
#include <fstream>
#include <sstream>

namespace gh = garlic_host;

static void die(const std::string &what)
{
    fprintf(stderr, "feature_counts_unit: %s\n", what.c_str());
    exit(1);
}

static std::string slurp(const std::string &path)
{
    std::ifstream f(path.c_str(), std::ios::binary);
    if (!f) die("cannot open " + path);
    std::stringstream s;
    s << f.rdbuf();
    return s.str();
}

static void spit(const std::string &path, const std::string &text)
{
    std::ofstream f(path.c_str(), std::ios::binary);
    f << text;
    if (!f) die("cannot write " + path);
}

// the semantics, as plainly as they can be said
static std::vector<int64_t> count(const gh::FeatureData &d, const std::vector<gh::FeatureInterval> &iv, int n_classes)
{
    const size_t nind = d.iid.size(), ne = d.ann.effects.size();
    std::vector<int64_t> counts(nind * (size_t)(n_classes + 1) * ne, 0);
    for (int64_t r = 0; r < d.rows.nrows(); r++)
        for (size_t i = 0; i < nind; i++) {
            if (!((d.rows.bits[(size_t)r * (size_t)d.rows.row_bytes + (i >> 3)] >> (i & 7)) & 1)) continue;
            int cls = n_classes;
            for (const gh::FeatureInterval &v : iv)
                if (v.ind == (int32_t)i && v.chr == d.rows.chr[(size_t)r] && v.start <= d.rows.pos[(size_t)r] && d.rows.pos[(size_t)r] < v.stop) cls = v.cls;
            counts[(i * (size_t)(n_classes + 1) + (size_t)cls) * ne + (size_t)d.rows.effect[(size_t)r]]++;
        }
    return counts;
}

static bool same(const std::vector<gh::FeatureInterval> &a, const std::vector<gh::FeatureInterval> &b)
{
    if (a.size() != b.size()) return false;
    for (size_t k = 0; k < a.size(); k++)
        if (memcmp(&a[k], &b[k], sizeof a[k])) return false;
    return true;
}

template <class F> static void refused(const char *what, const std::string &needle, F f)
{
    try {
        f();
    } catch (const std::runtime_error &e) {
        if (std::string(e.what()).find(needle) == std::string::npos) die(std::string(what) + ": message `" + e.what() + "` lacks `" + needle + "`");
        return;
    }
    die(std::string(what) + ": not refused");
}

static void golden(const std::string &work, char **f)
{
    const std::string features = f[0], tped = f[1], tfam = f[2], bed = f[3], expected = slurp(f[4]);
    gh::FeatureData d = gh::loadFeatureData(features, tped, tfam);
    for (int64_t r = 1; r < d.rows.nrows(); r++)
        if (std::make_pair(d.rows.chr[(size_t)r], d.rows.pos[(size_t)r]) < std::make_pair(d.rows.chr[(size_t)r - 1], d.rows.pos[(size_t)r - 1])) die("rows are not sorted");
    int n_classes = 0;
    const std::vector<gh::FeatureInterval> iv = gh::readRohBed(bed, d.iid, d.chrs, &n_classes);
    if (n_classes != 3) die("three classes expected");
    std::ostringstream table;
    gh::writeFeatureTable(table, d.ann.effects, d.iid, count(d, iv, n_classes).data(), n_classes);
    if (table.str() != expected) die("table differs from the script's:\n" + table.str());

    // the same calls handed over in memory: sizes on either side of the bounds give the file's classes back
    std::vector<std::string> panel_iid;
    std::vector<std::vector<gh::FeatureCall>> calls;
    const std::vector<double> bounds = {10.0, 20.0};
    {
        static const std::regex track("^track .+Ind: (.+) Pop:(.+) ROH.+");
        gh::FeatureLines in(bed);
        std::string line;
        std::smatch m;
        while (in.next(line)) {
            if (std::regex_match(line, m, track)) {
                panel_iid.push_back(m[1].str());
                calls.emplace_back();
                continue;
            }
            const std::vector<std::string> t = gh::featureSplit(line, 6);
            std::string chr = t[0].substr(3);                      // the map's name: no "chr" in front
            calls.back().push_back(gh::FeatureCall{chr, atoi(t[1].c_str()), atoi(t[2].c_str()), t[3] == "A" ? 5.0 : (t[3] == "B" ? 10.0 : 20.0)});
        }
    }
    int built_classes = 0;
    if (!same(gh::buildFeatureIntervals(panel_iid, calls, bounds, d.iid, d.chrs, &built_classes), iv) || built_classes != 3)
        die("buildFeatureIntervals differs from readRohBed");

    // gzip input reads the same
    const std::string gz = work + "/copy.tped.gz";
    {
        const std::string text = slurp(tped);
        gzFile g = gzopen(gz.c_str(), "wb");
        if (!g || gzwrite(g, text.data(), (unsigned)text.size()) != (int)text.size()) die("cannot write " + gz);
        gzclose(g);
    }
    gh::FeatureData dz = gh::loadFeatureData(features, gz, tfam);
    if (dz.rows.bits != d.rows.bits || dz.rows.pos != d.rows.pos || dz.rows.chr != d.rows.chr || dz.rows.effect != d.rows.effect) die("gzip input differs");

    // a fourth class: the columns run A .. D NONE and nothing is dropped
    std::vector<gh::FeatureInterval> iv4 = iv;
    if (iv4.empty()) die("no intervals");
    iv4[0].cls = 3;
    std::ostringstream wide;
    const std::vector<int64_t> c4 = count(d, iv4, 4), c3 = count(d, iv, 3);
    gh::writeFeatureTable(wide, d.ann.effects, d.iid, c4.data(), 4);
    if (wide.str().find(d.ann.effects[0] + "D " + d.ann.effects[0] + "NONE ") == std::string::npos) die("no D column");
    int64_t s3 = 0, s4 = 0;
    for (int64_t v : c3) s3 += v;
    for (int64_t v : c4) s4 += v;
    if (s3 != s4) die("a genotype was dropped");
    printf("%s: %lld rows, %zu intervals, %zu effects\n", features.c_str(), (long long)d.rows.nrows(), iv.size(), d.ann.effects.size());
}

int main(int argc, char **argv)
{
    if (argc < 2 || (argc - 2) % 5) die("usage: feature_counts_unit <work dir> (<features> <tped> <tfam> <roh.bed> <expected>) ...");
    const std::string work = argv[1];
    for (int k = 2; k < argc; k += 5) golden(work, argv + k);

    // malformed lines name file and line
    const std::string ff = work + "/bad.features", tp = work + "/bad.tped", tf = work + "/bad.tfam", rb = work + "/bad.roh.bed";
    spit(ff, "chr1:10 A G dam\nchr1 20 A G dam\n");
    refused("no colon", "bad.features:2: no colon", [&] { gh::readFeatureFile(ff); });
    spit(ff, "chr1:10 A G dam\n\nchr1:20 A G\n");
    refused("short feature line", "bad.features:3: a feature line needs", [&] { gh::readFeatureFile(ff); });
    spit(ff, "chr1:1x0 A G dam\n");
    refused("non-numeric position", "bad.features:1: position `1x0` is not a number", [&] { gh::readFeatureFile(ff); });
    spit(ff, "chr1: A G dam\n");
    refused("empty position", "is not a number", [&] { gh::readFeatureFile(ff); });
    spit(ff, "chr1:10 A G dam\n  \n1:20 C T ben\n");
    const gh::FeatureAnnotations ann = gh::readFeatureFile(ff);
    if (ann.effects != std::vector<std::string>{"ben", "dam"} || ann.allele.size() != 2) die("feature file with a blank line");
    if (ann.site("chr1", 20).first == ann.site("chr1", 20).second) die("`1:20` is chr1");
    gh::FeatureChrIds chrs;
    spit(tp, "1 rs1 0 10 G G A G\n1 rs2 0\n");
    refused("short TPED line", "bad.tped:2: a TPED line needs", [&] { gh::readCountingTped(tp, ann, 2, chrs); });
    spit(tp, "1 rs1 0 ten G G A G\n");
    refused("TPED position", "bad.tped:1: position `ten`", [&] { gh::readCountingTped(tp, ann, 2, chrs); });
    spit(tp, "1 rs0 0 5 G\n1 rs1 0 10 G G A\n");
    refused("TPED alleles", "bad.tped:2: fewer than 4 alleles", [&] { gh::readCountingTped(tp, ann, 2, chrs); });
    spit(tp, "1 rs0 0 5 G\n1 rs1 0 10 G G A G\n");              // the unannotated line's genotypes are never read
    const gh::FeatureRows rows = gh::readCountingTped(tp, ann, 2, chrs);
    if (rows.nrows() != 1 || rows.bits != std::vector<uint8_t>{1} || rows.lines != 2 || rows.lines_annotated != 1) die("TPED rows");
    spit(tf, "F I1 0 0 0 -9\nF\n");
    refused("short TFAM line", "bad.tfam:2", [&] { gh::readCountingTfam(tf); });
    const std::string track = "track name=\"Ind: I1 Pop:P ROH\" description=\"Ind: I1 Pop:P ROH from GARLIC v1.1.6a\" visibility=2 itemRgb=\"On\"\n";
    spit(rb, track + "chr1\t5\t9\n");
    refused("short ROH line", "bad.roh.bed:2: a ROH line needs", [&] { gh::readRohBed(rb, {"I1"}, chrs, nullptr); });
    spit(rb, track + "chr1\t5\t9\tZ\t5\n");
    refused("class letter", "bad.roh.bed:2: class `Z`", [&] { gh::readRohBed(rb, {"I1"}, chrs, nullptr); });
    spit(rb, track + "chr1\tfive\t9\tA\t5\n");
    refused("ROH start", "bad.roh.bed:2: start or end", [&] { gh::readRohBed(rb, {"I1"}, chrs, nullptr); });
    spit(rb, track + "chr1\t5\t9\tD\t5\n");
    int n_classes = 0;
    if (gh::readRohBed(rb, {"I0", "I1"}, chrs, &n_classes).at(0).ind != 1 || n_classes != 4) die("class D makes four classes");
    if (gh::featureTfamOf("a/b.chr1.tped.gz") != "a/b.chr1.tfam.gz") die("featureTfamOf");
    if (gh::featureSizeClass(5, {10, 20}) != 0 || gh::featureSizeClass(10, {10, 20}) != 1 || gh::featureSizeClass(25, {10, 20}) != 2) die("featureSizeClass");
    printf("feature_counts_unit ok\n");
    return 0;
}
