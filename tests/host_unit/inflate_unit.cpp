// garlic_amd/csrc/inflate.hpp and garlic_amd/host/bgzf_blocks.hpp on the host, under ASan + UBSan (tests/test_bgzf_cpu.py
// builds and runs it).  inflate_unit DIR: DIR holds what the Python test wrote --
//   *.rec        members with what zlib says about them (tests/bgzf_cases.py: records): every member is inflated from a
//                heap copy of exactly its deflate bytes into a heap buffer of exactly ISIZE bytes, so one byte read or written
//                outside either range stops the run; the CRC32 is summed the way the device's 64 lanes sum it
//   walk.bgzf, walk.txt      a BGZF file and its blocks (offset, bytes, ISIZE per line)
//   cut_header.bgzf, past_end.bgzf, then_gzip.bgzf   files whose walk ends in CUT_SHORT, PAST_END and NOT_BGZF
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../garlic_amd/csrc/inflate.hpp"
#include "../../garlic_amd/host/bgzf_blocks.hpp"

using namespace garlic;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                    \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            if (g_fail++ < 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
        }                                                                                   \
    } while (0)

static std::vector<uint8_t> slurp(const std::string &path)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(2); }
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + got);
    fclose(f);
    return v;
}

static uint32_t g_crc_table[256];

// one member: its status (100: the header is no BGZF header for these bytes), its bytes into `out`
static int inflate_member(const uint8_t *m, size_t n, std::vector<uint8_t> &out)
{
    out.clear();
    bgzf::Block b;
    if (bgzf::parseHeader(m, n, b) != bgzf::OK || (size_t)b.bytes != n) return 100;
    const uint8_t *foot = m + n - 8;
    const uint32_t crc = (uint32_t)foot[0] | (uint32_t)foot[1] << 8 | (uint32_t)foot[2] << 16 | (uint32_t)foot[3] << 24;
    const uint32_t isize = (uint32_t)foot[4] | (uint32_t)foot[5] << 8 | (uint32_t)foot[6] << 16 | (uint32_t)foot[7] << 24;
    if (isize > 65536) return 100;
    const size_t n_in = n - (size_t)b.data_at - 8;
    uint8_t *in = (uint8_t *)malloc(n_in ? n_in : 1), *o = (uint8_t *)malloc(isize ? isize : 1);
    memcpy(in, m + b.data_at, n_in);
    InflateTables *t = new InflateTables;
    int rc = inflate_block(in, (uint32_t)n_in, o, isize, *t);
    if (!rc) {
        uint32_t sum = 0;
        for (uint32_t lane = 0; lane < 64; lane++) sum ^= crc32_lane_part(o, isize, lane, 64, g_crc_table);
        if ((sum ^ 0xFFFFFFFFu) != crc) rc = GARLIC_BGZF_BAD_CRC;
        out.assign(o, o + isize);
    }
    delete t;
    free(in);
    free(o);
    return rc;
}

static size_t run_records(const std::string &path)
{
    const std::vector<uint8_t> v = slurp(path);
    size_t at = 0, count = 0;
    std::vector<uint8_t> out;
    while (at < v.size()) {
        uint32_t n, exp_n;
        int32_t expect;
        memcpy(&n, &v[at], 4);
        const uint8_t *m = &v[at + 4];
        memcpy(&expect, &v[at + 4 + n], 4);
        memcpy(&exp_n, &v[at + 8 + n], 4);
        const uint8_t *want = v.data() + at + 12 + n;
        at += 12 + (size_t)n + exp_n;
        const int rc = inflate_member(m, n, out);
        const bool same = !rc && out.size() == exp_n && (exp_n == 0 || memcmp(out.data(), want, exp_n) == 0);
        if (expect == 0) CHECK(same, "%s member %zu: status %d, zlib accepts it", path.c_str(), count, rc);
        else if (expect > 0) CHECK(rc == expect, "%s member %zu: status %d, expected %d", path.c_str(), count, rc, expect);
        else if (expect == -1) CHECK(rc != 0, "%s member %zu: accepted, zlib refuses it", path.c_str(), count);
        else CHECK(rc != 0 || same, "%s member %zu: accepted with other bytes than zlib's", path.c_str(), count);
        count++;
    }
    return count;
}

static void run_walks(const std::string &dir)
{
    bgzf::File file;
    CHECK(file.open(dir + "/walk.bgzf"), "open walk.bgzf");
    CHECK(bgzf::isBgzf(dir + "/walk.bgzf"), "walk.bgzf is BGZF");
    CHECK(!bgzf::isBgzf(dir + "/walk.txt"), "walk.txt is not BGZF");
    std::vector<long long> want;
    FILE *f = fopen((dir + "/walk.txt").c_str(), "r");
    long long a, b, c;
    while (f && fscanf(f, "%lld %lld %lld", &a, &b, &c) == 3) { want.push_back(a); want.push_back(b); want.push_back(c); }
    if (f) fclose(f);
    // in one go, and in slabs of at most 100,000 inflated bytes or 3 blocks
    for (int pass = 0; pass < 2; pass++) {
        std::vector<bgzf::Block> blocks;
        int64_t at = 0;
        bgzf::End e = bgzf::OK;
        while (e == bgzf::OK) {
            const size_t before = blocks.size();
            int64_t inflated = 0;
            e = bgzf::walk(file, at, pass ? 100000 : (int64_t)1 << 40, pass ? 3 : (size_t)1 << 30, blocks, &at);
            for (size_t k = before; k < blocks.size(); k++) inflated += blocks[k].isize;
            if (pass) CHECK(blocks.size() - before <= 3 && (inflated <= 100000 || blocks.size() - before == 1), "slab limits");
            CHECK(e != bgzf::OK || blocks.size() > before, "a walk that goes on takes a block");
        }
        CHECK(e == bgzf::AT_END && at == file.size, "walk.bgzf ends at its end: %d", (int)e);
        CHECK(blocks.size() * 3 == want.size(), "walk.bgzf: %zu blocks, expected %zu", blocks.size(), want.size() / 3);
        for (size_t k = 0; k < blocks.size() && 3 * k + 2 < want.size(); k++)
            CHECK(blocks[k].at == want[3 * k] && blocks[k].bytes == want[3 * k + 1] && (long long)blocks[k].isize == want[3 * k + 2],
                  "walk.bgzf block %zu", k);
    }
    const struct { const char *name; bgzf::End end; } bad[] = {{"cut_header.bgzf", bgzf::CUT_SHORT}, {"past_end.bgzf", bgzf::PAST_END},
                                                               {"then_gzip.bgzf", bgzf::NOT_BGZF}};
    for (const auto &c : bad) {
        bgzf::File g;
        CHECK(g.open(dir + "/" + c.name), "open %s", c.name);
        std::vector<bgzf::Block> blocks;
        int64_t at = 0;
        const bgzf::End e = bgzf::walk(g, 0, (int64_t)1 << 40, (size_t)1 << 30, blocks, &at);
        CHECK(e == c.end, "%s: walk ended with %d, expected %d", c.name, (int)e, (int)c.end);
        CHECK(blocks.size() == 2 && at == blocks[1].at + blocks[1].bytes, "%s: the two whole blocks in front are kept", c.name);
    }
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: inflate_unit DIR\n"); return 2; }
    const std::string dir = argv[1];
    for (uint32_t i = 0; i < 256; i++) g_crc_table[i] = crc32_table_entry(i);
    size_t n = 0;
    for (const char *name : {"clean.rec", "corrupt.rec", "random.rec", "random_corrupt.rec"}) n += run_records(dir + "/" + name);
    run_walks(dir);
    if (g_fail) { fprintf(stderr, "%d failures\n", g_fail); return 1; }
    printf("inflate_unit ok: %zu members\n", n);
    return 0;
}
