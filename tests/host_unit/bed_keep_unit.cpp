// CPU check of garlic_amd/host/bed_keep.hpp (the keep file of --keep, the family IDs of --pops), a stand-alone program:
//   bed_keep_unit <dir>      writes its files into <dir>
#include "../../garlic_amd/host/bed_keep.hpp"

#include <cstdio>
#include <fstream>
#include <iostream>

using namespace garlic_host;

static int failures = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { std::cerr << "FAILED line " << __LINE__ << ": " #cond "\n"; failures++; } \
    } while (0)

static void put(const std::string &path, const std::string &text)
{
    std::ofstream f(path, std::ios::binary);
    f << text;
}

// the message of the error a call ends with; "" when it does not throw
template <class F> static std::string errorOf(F f)
{
    try {
        f();
    } catch (const std::runtime_error &e) {
        return e.what();
    }
    return "";
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const std::string famfile = dir + "/x.fam";
    // three family IDs interleaved; an individual ID that two families share
    put(famfile, "B b1 0 0 0 -9\nA a1 0 0 0 -9\nB b2 0 0 0 -9\nC c1 0 0 0 -9\nA a2 0 0 0 -9\nA b1 0 0 0 -9\n\nC c2 0 0 0 -9\n");
    const std::vector<FamEntry> fam = readFam(famfile);
    CHECK(fam.size() == 7);
    CHECK(fam[0].fid == "B" && fam[0].iid == "b1" && fam[6].fid == "C" && fam[6].iid == "c2");

    // families in first-seen order, members ascending
    const std::vector<FamFamily> fams = famFamilies(fam);
    CHECK(fams.size() == 3);
    CHECK(fams[0].fid == "B" && fams[1].fid == "A" && fams[2].fid == "C");
    CHECK((fams[0].members == std::vector<int>{0, 2}));
    CHECK((fams[1].members == std::vector<int>{1, 4, 5}));
    CHECK((fams[2].members == std::vector<int>{3, 6}));

    // the .fam's order, not the keep file's; a pair twice counts once
    put(dir + "/order.keep", "A a2\nA a1\nA b1\nA a2\n");
    CHECK((readKeepFile(dir + "/order.keep", fam) == std::vector<int>{1, 4, 5}));
    // the pair decides, not the individual ID alone
    put(dir + "/pair.keep", "B b1\n");
    CHECK((readKeepFile(dir + "/pair.keep", fam) == std::vector<int>{0}));
    // further columns ignored, blank lines skipped, tabs, no newline at the end
    put(dir + "/extra.keep", "\nC\tc2  0 0 2 -9 more\n\n   \nB b2 x");
    CHECK((readKeepFile(dir + "/extra.keep", fam) == std::vector<int>{2, 6}));
    // CRLF, in the keep file and in the .fam
    put(dir + "/crlf.keep", "C c1\r\nA a1\r\n\r\n");
    CHECK((readKeepFile(dir + "/crlf.keep", fam) == std::vector<int>{1, 3}));
    put(dir + "/crlf.fam", "P i0 0 0 0 -9\r\nP i1 0 0 0 -9\r\n");
    const std::vector<FamEntry> crlf = readFam(dir + "/crlf.fam");
    CHECK(crlf.size() == 2 && crlf[1].iid == "i1" && crlf[1].fid == "P");
    put(dir + "/crlf2.keep", "P i1\r\n");
    CHECK((readKeepFile(dir + "/crlf2.keep", crlf) == std::vector<int>{1}));

    // an unknown pair: file, line and pair
    put(dir + "/unknown.keep", "A a1\n\nB a1 0\nC c1\n");
    const std::string unknown = errorOf([&] { readKeepFile(dir + "/unknown.keep", fam); });
    std::cerr << unknown << "\n";
    CHECK(unknown.find("unknown.keep") != std::string::npos && unknown.find("line 3") != std::string::npos &&
          unknown.find("B a1") != std::string::npos);
    // a line with one column
    put(dir + "/short.keep", "A a1\nA\n");
    const std::string one = errorOf([&] { readKeepFile(dir + "/short.keep", fam); });
    CHECK(one.find("line 2") != std::string::npos && one.find("2 columns") != std::string::npos);
    // an empty result
    put(dir + "/empty.keep", "\n\r\n   \n");
    const std::string empty = errorOf([&] { readKeepFile(dir + "/empty.keep", fam); });
    std::cerr << empty << "\n";
    CHECK(empty.find("empty.keep") != std::string::npos && empty.find("keeps no individual") != std::string::npos);
    // a file that is not there
    CHECK(errorOf([&] { readKeepFile(dir + "/none.keep", fam); }).find("Failed to open") != std::string::npos);
    CHECK(errorOf([&] { readFam(dir + "/none.fam"); }).find("Failed to open") != std::string::npos);
    // a pair twice in the .fam
    put(dir + "/twice.fam", "A a1 0 0 0 -9\nB a1 0 0 0 -9\nA a1 0 0 0 -9\n");
    const std::string twice = errorOf([&] { readFam(dir + "/twice.fam"); });
    CHECK(twice.find("duplicate") != std::string::npos && twice.find("line 3") != std::string::npos);

    if (failures) return 1;
    std::cout << "bed_keep_unit ok\n";
    return 0;
}
