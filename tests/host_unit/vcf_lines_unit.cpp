// garlic_amd/host/vcf_lines.hpp on its own (built by tests/test_vcf_cpu.py under ASan + UBSan): the #CHROM line, the nine
// fixed columns, refused REF / ALT forms, FORMAT, and lines cut out of slabs that end anywhere.
// usage: vcf_lines_unit <scratch directory>
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../../garlic_amd/host/vcf_lines.hpp"

static int failures = 0;
#define CHECK(cond)                                                                                      \
    do {                                                                                                 \
        if (!(cond)) {                                                                                   \
            std::cerr << __FILE__ << ":" << __LINE__ << ": " #cond "\n";                                 \
            failures++;                                                                                  \
        }                                                                                                \
    } while (0)

static vcf::LineKind fixed(const std::string &line, vcf::Site &s, std::string &err)
{
    // an exact-size heap copy: a read past the line is ASan's to report
    std::vector<char> copy(line.begin(), line.end());
    return vcf::parseFixed(copy.data(), copy.size(), s, err);
}

// every data line of `text`, cut in slabs of `cap` bytes fed `step` bytes at a time
static std::vector<std::string> lines_through_slabs(const std::string &text, size_t cap, size_t step)
{
    std::vector<std::string> out;
    std::vector<char> slab(cap);
    vcf::SlabLines cut;
    size_t have = 0, fed = 0;
    bool eof = false;
    while (!eof || have) {
        const size_t n = std::min(std::min(step, cap - have), text.size() - fed);
        memcpy(slab.data() + have, text.data() + fed, n);
        have += n;
        fed += n;
        eof = fed == text.size();
        const size_t used = cut.take(slab.data(), have, eof);
        for (size_t k = 0; k < cut.begin.size(); k++) out.emplace_back(slab.data() + cut.begin[k], (size_t)(cut.end[k] - cut.begin[k]));
        memmove(slab.data(), slab.data() + used, have - used);
        have -= used;
        if (!eof && n == 0) { CHECK(!"a line longer than the slab"); break; }
    }
    return out;
}

int main(int argc, char **argv)
{
    std::string err;
    // ---- the header
    {
        std::vector<std::string> samples;
        const std::string h = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tNA1\tNA 2\tx\r\n";
        CHECK(vcf::parseHeader(h.data(), h.size(), samples, err));
        CHECK(samples.size() == 3 && samples[0] == "NA1" && samples[1] == "NA 2" && samples[2] == "x");
        const std::string none = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\n";
        CHECK(!vcf::parseHeader(none.data(), none.size(), samples, err));
        const std::string wrong = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tGT\ta\n";
        CHECK(!vcf::parseHeader(wrong.data(), wrong.size(), samples, err));
        const std::string hole = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\t\tb\n";
        CHECK(!vcf::parseHeader(hole.data(), hole.size(), samples, err));
    }
    // ---- the nine columns
    {
        vcf::Site s;
        CHECK(fixed("7\t12345\trs9\tA\tG\t.\tPASS\t.\tGT\t0|1", s, err) == vcf::LINE_SNP);
        CHECK(s.chr == "7" && s.name == "rs9" && s.ppos == 12345 && s.gpos == 0 && s.a1 == 'A' && s.a2 == 'G');
        CHECK(fixed("chrX\t1\t.\tt\tc\t50\tq10\tDP=3;AF=0.5\tGT:GQ:PL\t0/1:3:1,2,3\t1/1\r", s, err) == vcf::LINE_SNP);
        CHECK(s.chr == "chrX" && s.name == "." && s.ppos == 1 && s.a1 == 't' && s.a2 == 'c');
        for (const char *alt : {"G,T", ".", "*", "<DEL>", "GA", ""})
            CHECK(fixed(std::string("1\t5\tid\tA\t") + alt + "\t.\t.\t.\tGT\t0|0", s, err) == vcf::LINE_NOT_SNP && !err.empty());
        for (const char *ref : {"AT", ".", "", "<"})
            CHECK(fixed(std::string("1\t5\tid\t") + ref + "\tC\t.\t.\t.\tGT\t0|0", s, err) == vcf::LINE_NOT_SNP);
        CHECK(fixed("1\t5\tid\tA\tC\t.\t.\t.\tDP:GT\t3:0|0", s, err) == vcf::LINE_BAD && err.find("GT") != std::string::npos);
        CHECK(fixed("1\t5\tid\tA\tC\t.\t.\t.\tG\t0|0", s, err) == vcf::LINE_BAD);
        CHECK(fixed("1\t5\tid\tA\tC\t.\t.\t.\tGTX\t0|0", s, err) == vcf::LINE_BAD);
        CHECK(fixed("1\t5\tid\tA\tC\t.\t.\t.\tGT", s, err) == vcf::LINE_BAD);          // no sample column
        CHECK(fixed("1\t5x\tid\tA\tC\t.\t.\t.\tGT\t0|0", s, err) == vcf::LINE_BAD);
        CHECK(fixed("1\t\tid\tA\tC\t.\t.\t.\tGT\t0|0", s, err) == vcf::LINE_BAD);
        CHECK(fixed("", s, err) == vcf::LINE_BAD);
        // a FORMAT that is not GT is reported before a REF / ALT that is no SNP
        CHECK(fixed("1\t5\tid\tA\tC,T\t.\t.\t.\tDP\t3", s, err) == vcf::LINE_BAD);
    }
    // ---- lines out of slabs: CRLF, empty lines, a last line without '\n', every slab size and feeding step
    {
        const std::vector<std::string> want = {"##fileformat=VCFv4.2", "#CHROM\tx", "1\t5\ta\tA\tC\t.\t.\t.\tGT\t0|0\r", "2\t6\tb\tA\tC\t.\t.\t.\tGT\t1|0:44",
                                               "3\t7\tc\tA\tC\t.\t.\t.\tGT\t./."};
        std::string text;
        for (size_t k = 0; k < want.size(); k++) text += want[k] + (k + 1 < want.size() ? "\n" : "");
        std::string with_blank = text;
        with_blank.insert(with_blank.find("#CHROM"), "\n\r\n");
        for (size_t cap : {(size_t)32, (size_t)33, (size_t)47, (size_t)64, (size_t)4096})
            for (size_t step : {(size_t)1, (size_t)3, (size_t)16, (size_t)4096}) {
                CHECK(lines_through_slabs(text, cap, step) == want);
                CHECK(lines_through_slabs(text + "\n", cap, step) == want);
                CHECK(lines_through_slabs(with_blank, cap, step) == want);
            }
        vcf::SlabLines cut;
        const std::string part = "abc\ndef";
        CHECK(cut.take(part.data(), part.size(), false) == 4 && cut.begin.size() == 1 && cut.end[0] == 3);
        CHECK(cut.take(part.data(), part.size(), true) == 7 && cut.begin.size() == 2 && cut.begin[1] == 4 && cut.end[1] == 7);
        CHECK(cut.take(part.data(), 0, true) == 0 && cut.begin.empty());
    }
    // ---- the reader and the counting pass, plain and gzip, with the skip count of the non-SNP lines
    if (argc > 1) {
        const std::string body = "##a\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts0\n"
                                 "1\t5\ta\tA\tC\t.\t.\t.\tGT\t0|0\n1\t6\tb\tA\tC,T\t.\t.\t.\tGT\t0|0\r\n1\t7\tc\tA\tG\t.\t.\t.\tGT\t1|1";
        const std::string plain = std::string(argv[1]) + "/u.vcf", packed = std::string(argv[1]) + "/u.vcf.gz";
        FILE *fp = fopen(plain.c_str(), "wb");
        CHECK(fp && fwrite(body.data(), 1, body.size(), fp) == body.size());
        if (fp) fclose(fp);
        gzFile gz = gzopen(packed.c_str(), "wb");
        CHECK(gz && gzwrite(gz, body.data(), (unsigned)body.size()) == (int)body.size());
        if (gz) gzclose(gz);
        for (const std::string &path : {plain, packed}) {
            int64_t n = -1;
            CHECK(vcf::countDataLines(path, n, err) && n == 3);
            vcf::Reader rd;
            CHECK(rd.open(path, 64));
            vcf::SlabLines cut;
            size_t used = 0;
            int snps = 0, skipped = 0, headers = 0;
            do {
                CHECK(rd.next(used));
                used = cut.take(rd.slab.data(), rd.have, rd.eof);
                if (!rd.eof && used == 0 && rd.have == rd.slab.size()) { CHECK(!"a line longer than the slab"); break; }
                for (size_t k = 0; k < cut.begin.size(); k++) {
                    const char *line = rd.slab.data() + cut.begin[k];
                    const size_t len = (size_t)(cut.end[k] - cut.begin[k]);
                    if (line[0] == '#') { headers++; continue; }
                    vcf::Site s;
                    const vcf::LineKind kind = vcf::parseFixed(line, len, s, err);
                    snps += kind == vcf::LINE_SNP;
                    skipped += kind == vcf::LINE_NOT_SNP;
                }
            } while (!rd.eof || used < rd.have);
            CHECK(headers == 2 && snps == 2 && skipped == 1);
        }
        int64_t n = 0;
        CHECK(!vcf::countDataLines(std::string(argv[1]) + "/missing.vcf", n, err));
        // a .gz cut short is an error, not a shorter file
        {
            std::string big;
            for (int k = 0; k < 4000; k++) big += "1\t" + std::to_string(k * 7919 % 100003) + "\tid\tA\tC\t.\t.\t.\tGT\t0|1\n";
            const std::string whole = std::string(argv[1]) + "/w.vcf.gz", cut = std::string(argv[1]) + "/cut.vcf.gz";
            gzFile g2 = gzopen(whole.c_str(), "wb");
            CHECK(g2 && gzwrite(g2, big.data(), (unsigned)big.size()) == (int)big.size());
            if (g2) gzclose(g2);
            FILE *in = fopen(whole.c_str(), "rb");
            std::vector<char> raw(1 << 20);
            const size_t got = in ? fread(raw.data(), 1, raw.size(), in) : 0;
            if (in) fclose(in);
            CHECK(got > 200);
            FILE *out = fopen(cut.c_str(), "wb");
            CHECK(out && fwrite(raw.data(), 1, got / 2, out) == got / 2);
            if (out) fclose(out);
            CHECK(vcf::countDataLines(whole, n, err) && n == 4000);
            CHECK(!vcf::countDataLines(cut, n, err));
        }
        // line numbers count the empty lines
        {
            vcf::SlabLines cut;
            const std::string t = "a\n\nb\n\r\nc";
            CHECK(cut.take(t.data(), t.size(), true) == t.size() && cut.number == (std::vector<int64_t>{1, 3, 5}));
        }
    }
    if (failures) {
        std::cerr << failures << " checks failed\n";
        return 1;
    }
    std::cout << "vcf_lines_unit ok\n";
    return 0;
}
