// vcf::parseGlValues (garlic_amd/host/vcf_lines.hpp) over the lines of a file: a stand-alone program.
//   vcf_gl_lines_unit KEY NSAMPLES MISSING|none FILE [COL ...]
// prints per line `ok v0 v1 ...` (%.17g, the kept columns COL ... or all) or `bad SAMPLE reason`.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>

#include "../../garlic_amd/host/vcf_lines.hpp"

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const std::string key = argv[1];
    const int nsamples = atoi(argv[2]);
    const bool has_missing = std::string(argv[3]) != "none";
    const double missing = has_missing ? atof(argv[3]) : 0;
    std::vector<int> cols;
    for (int i = 5; i < argc; i++) cols.push_back(atoi(argv[i]));
    const size_t n = cols.empty() ? (size_t)nsamples : cols.size();
    std::ifstream in(argv[4], std::ios::binary);
    std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    vcf::SlabLines cut;
    cut.take(text.data(), text.size(), true);
    std::vector<double> out(n);
    for (size_t k = 0; k < cut.begin.size(); k++) {
        // a heap copy of exactly the line's bytes: a read past either end is the sanitizer's to find
        const std::string line(text.data() + cut.begin[k], (size_t)(cut.end[k] - cut.begin[k]));
        std::vector<char> exact(line.begin(), line.end());
        int sample = -1;
        std::string err;
        if (vcf::parseGlValues(exact.data(), exact.size(), key, nsamples, cols.empty() ? nullptr : cols.data(), n, has_missing ? &missing : nullptr,
                               out.data(), sample, err)) {
            printf("ok");
            for (double v : out) printf(" %.17g", v);
            printf("\n");
        } else {
            printf("bad %d %s\n", sample, err.c_str());
        }
    }
    printf("vcf_gl_lines_unit ok\n");
    return 0;
}
