// text::forEachSlab and text::LineCursor (garlic_amd/host/text_slabs.hpp) on files written here: a line that ends exactly at the
// slab's end, tails carried over slabs, a last line without '\n', blank and \r-only lines, a line longer than the slab, a .gz,
// a file that is not there, and a walk that is stopped.  usage: text_slabs_unit DIR
#include <cstdio>
#include <iostream>
#include <string>
#include <utility>
#include <vector>

#include "../../garlic_amd/host/text_slabs.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { failures++; std::cerr << "line " << __LINE__ << ": " #c "\n"; } } while (0)

typedef std::vector<std::pair<int64_t, std::string>> Lines;      // (the line's number in the file, its bytes)

// the rule, byte by byte: lines end at '\n' or the file's end; empty and \r-only lines are counted and left out
static Lines rule(const std::string &t)
{
    Lines out;
    int64_t number = 0;
    for (size_t at = 0; at < t.size();) {
        size_t e = t.find('\n', at);
        if (e == std::string::npos) e = t.size();
        const std::string line = t.substr(at, e - at);
        number++;
        if (!line.empty() && line != "\r") out.emplace_back(number, line);
        at = e + 1;
    }
    return out;
}

static void write_file(const std::string &path, const std::string &t, bool gz)
{
    if (gz) {
        gzFile g = gzopen(path.c_str(), "wb");
        CHECK(g && gzwrite(g, t.data(), (unsigned)t.size()) == (int)t.size());
        if (g) gzclose(g);
    } else {
        FILE *f = fopen(path.c_str(), "wb");
        CHECK(f && fwrite(t.data(), 1, t.size(), f) == t.size());
        if (f) fclose(f);
    }
}

static text::SlabsEnd pushed(const std::string &path, size_t cap, Lines &got, size_t *slabs = nullptr, size_t stop_after = 0)
{
    std::string error;
    got.clear();
    size_t seen = 0;
    const text::SlabsEnd end = text::forEachSlab(path, cap, error, [&](const text::Reader &rd, const text::SlabLines &cut, size_t consumed) {
        CHECK(consumed <= rd.have && rd.have <= cap);
        for (size_t k = 0; k < cut.begin.size(); k++) {
            CHECK(cut.begin[k] < cut.end[k] && (size_t)cut.end[k] <= consumed);
            got.emplace_back(cut.number[k], std::string(rd.slab.data() + cut.begin[k], (size_t)(cut.end[k] - cut.begin[k])));
        }
        return ++seen != stop_after;
    });
    if (slabs) *slabs = seen;
    CHECK((end == text::SLABS_NO_FILE || end == text::SLABS_READ_ERROR) == !error.empty());
    return end;
}

static text::SlabsEnd pulled(const std::string &path, size_t cap, Lines &got)
{
    got.clear();
    text::LineCursor in;
    if (!in.rd.open(path, cap)) return text::SLABS_NO_FILE;
    for (size_t k; in.next(k);)
        got.emplace_back(in.lines.number[k], std::string(in.rd.slab.data() + in.lines.begin[k], (size_t)(in.lines.end[k] - in.lines.begin[k])));
    return in.why;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    Lines got;
    // 16-byte slabs: the first line ends exactly at the first slab's end; the third is carried; the last has no '\n'
    const std::string text = "0123456789abcde\nxy\n0123456789\n\n\r\nlast one";
    const Lines want = rule(text);
    for (bool gz : {false, true}) {
        const std::string path = dir + (gz ? "/a.txt.gz" : "/a.txt");
        write_file(path, text, gz);
        for (size_t cap : {(size_t)16, (size_t)17, (size_t)23, (size_t)64, (size_t)4096}) {
            size_t slabs = 0;
            CHECK(pushed(path, cap, got, &slabs) == text::SLABS_DONE && got == want);
            CHECK(cap != 16 || slabs >= 3);
            CHECK(cap != 4096 || slabs == 1);
            CHECK(pulled(path, cap, got) == text::SLABS_DONE && got == want);
        }
        CHECK(want.size() == 4 && want[3] == std::make_pair((int64_t)6, std::string("last one")));
        // a walk that is stopped hands out what it saw until then
        CHECK(pushed(path, 16, got, nullptr, 1) == text::SLABS_STOPPED && got == Lines(want.begin(), want.begin() + 1));
        // a line of 15 bytes and its '\n' fill a slab of 16; a slab of 15 holds no line end
        CHECK(pushed(path, 15, got) == text::SLABS_LONG_LINE && got.empty());
        CHECK(pulled(path, 15, got) == text::SLABS_LONG_LINE && got.empty());
    }
    // a long line behind short ones: they are handed over, then the walk ends
    write_file(dir + "/b.txt", "ab\ncd\n0123456789abcdef0123456789\nef\n", false);
    CHECK(pushed(dir + "/b.txt", 16, got) == text::SLABS_LONG_LINE && got == (Lines{{1, "ab"}, {2, "cd"}}));
    // a final line without '\n' may be one byte short of the slab (the reader sees the file's end only with room to read)
    write_file(dir + "/c.txt", "ab\n0123456789abcde", false);
    CHECK(pushed(dir + "/c.txt", 16, got) == text::SLABS_DONE && got == (Lines{{1, "ab"}, {2, "0123456789abcde"}}));
    // only blank lines, an empty file, a \r before the \n stays with the line
    write_file(dir + "/d.txt", "\n\r\n\n", false);
    CHECK(pushed(dir + "/d.txt", 16, got) == text::SLABS_DONE && got.empty());
    write_file(dir + "/e.txt", "", false);
    CHECK(pushed(dir + "/e.txt", 16, got) == text::SLABS_DONE && got.empty());
    CHECK(pulled(dir + "/e.txt", 16, got) == text::SLABS_DONE && got.empty());
    write_file(dir + "/f.txt", "a b\r\nc d\r\n", false);
    CHECK(pushed(dir + "/f.txt", 16, got) == text::SLABS_DONE && got == (Lines{{1, "a b\r"}, {2, "c d\r"}}));
    CHECK(pushed(dir + "/none.txt", 16, got) == text::SLABS_NO_FILE);
    // many lines through many slabs, plain and packed
    std::string big;
    for (int k = 0; k < 3000; k++) big += std::string((size_t)(k * 7 % 40), (char)('a' + k % 26)) + (k % 11 == 0 ? "\r\n" : "\n");
    for (bool gz : {false, true}) {
        const std::string path = dir + (gz ? "/big.gz" : "/big.txt");
        write_file(path, big, gz);
        for (size_t cap : {(size_t)41, (size_t)100, (size_t)4096}) {
            CHECK(pushed(path, cap, got) == text::SLABS_DONE && got == rule(big));
            CHECK(pulled(path, cap, got) == text::SLABS_DONE && got == rule(big));
        }
    }
    if (failures) {
        std::cerr << failures << " checks failed\n";
        return 1;
    }
    std::cout << "text_slabs_unit ok\n";
    return 0;
}
