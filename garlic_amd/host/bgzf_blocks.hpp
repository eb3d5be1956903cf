// BGZF files on the host: the walk over the blocks' headers and footers.  Header-only, no HIP.
//
// A BGZF file is a series of gzip members of at most 64 KiB, each with an extra subfield 'B' 'C' of length 2 that holds
// BSIZE = the member's size - 1, and with the usual footer, CRC32 and ISIZE.  The walk reads 12 + XLEN bytes of header and
// the 8 bytes of footer per block and nothing of the deflate data: the compressed and inflated offsets of the next blocks
// that fit a slab.  The empty block at the file's end is a block of ISIZE 0.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace bgzf {

constexpr int64_t MEMBER_MAX = 65536;

struct Block {
    int64_t at = 0;            // file offset of the member
    int64_t bytes = 0;         // the member, header and footer included (BSIZE + 1)
    int64_t data_at = 0;       // offset of the deflate data inside the member (12 + XLEN)
    uint32_t crc = 0, isize = 0;
};

// How a header read or a walk ended.
enum End {
    OK = 0,                    // a block (header) / the limits were reached with blocks in hand (walk)
    AT_END,                    // the file ends exactly in front of this block
    NOT_BGZF,                  // a member that is no BGZF block: another magic or method, no FEXTRA, no BC subfield of length 2
    PAST_END,                  // BSIZE runs past the file's end
    CUT_SHORT,                 // the file ends inside the header
    IO_ERROR
};

// The header in p[0, have): have >= 12 + XLEN or the answer is CUT_SHORT (with *need = the bytes it wants, where it knows).
inline End parseHeader(const uint8_t *p, size_t have, Block &b, size_t *need = nullptr)
{
    if (need) *need = 12;
    if (have < 12) return CUT_SHORT;
    if (p[0] != 0x1F || p[1] != 0x8B || p[2] != 8 || p[3] != 4) return NOT_BGZF;       // FLG: FEXTRA and nothing else
    const size_t xlen = (size_t)p[10] | (size_t)p[11] << 8;
    if (need) *need = 12 + xlen;
    if (have < 12 + xlen) return CUT_SHORT;
    int64_t bsize = -1;
    for (size_t at = 12; at + 4 <= 12 + xlen;) {
        const size_t slen = (size_t)p[at + 2] | (size_t)p[at + 3] << 8;
        if (at + 4 + slen > 12 + xlen) return NOT_BGZF;
        if (p[at] == 'B' && p[at + 1] == 'C' && slen == 2 && bsize < 0) bsize = (int64_t)p[at + 4] | (int64_t)p[at + 5] << 8;
        at += 4 + slen;
    }
    if (bsize < 0) return NOT_BGZF;
    b.bytes = bsize + 1;
    b.data_at = 12 + (int64_t)xlen;
    if (b.bytes < b.data_at + 2 + 8) return NOT_BGZF;       // no room for a deflate block and the footer
    return OK;
}

struct File {
    FILE *f = nullptr;
    int64_t size = 0;
    bool open(const std::string &path)
    {
        f = fopen(path.c_str(), "rb");
        if (!f) return false;
        if (fseeko(f, 0, SEEK_END) != 0) return false;
        size = (int64_t)ftello(f);
        return size >= 0;
    }
    bool read(int64_t at, void *dst, size_t n) const { return fseeko(f, (off_t)at, SEEK_SET) == 0 && fread(dst, 1, n, f) == n; }
    void close() { if (f) fclose(f); f = nullptr; }
    ~File() { close(); }
};

// the block at file offset `at`: its header and its footer
inline End readBlock(const File &file, int64_t at, Block &b)
{
    if (at == file.size) return AT_END;
    uint8_t head[12 + 65535];
    size_t have = (size_t)(file.size - at < 12 ? file.size - at : 12), need = 12;
    if (!file.read(at, head, have)) return IO_ERROR;
    End e = parseHeader(head, have, b, &need);
    if (e == CUT_SHORT && have == 12 && need > 12) {
        have = (size_t)((int64_t)need < file.size - at ? (int64_t)need : file.size - at);
        if (!file.read(at, head, have)) return IO_ERROR;
        e = parseHeader(head, have, b, &need);
    }
    if (e != OK) return e;
    b.at = at;
    if (at + b.bytes > file.size) return PAST_END;
    uint8_t foot[8];
    if (!file.read(at + b.bytes - 8, foot, 8)) return IO_ERROR;
    b.crc = (uint32_t)foot[0] | (uint32_t)foot[1] << 8 | (uint32_t)foot[2] << 16 | (uint32_t)foot[3] << 24;
    b.isize = (uint32_t)foot[4] | (uint32_t)foot[5] << 8 | (uint32_t)foot[6] << 16 | (uint32_t)foot[7] << 24;
    if ((int64_t)b.isize > MEMBER_MAX) return NOT_BGZF;
    return OK;
}

inline bool isBgzf(const std::string &path)
{
    File file;
    Block b;
    return file.open(path) && readBlock(file, 0, b) == OK;
}

// From file offset `at`: the next blocks, appended to `blocks`, while their inflated bytes stay within max_inflated and
// their count within max_blocks (at least one block is taken if one is there).  *next = the offset behind the last block
// taken.  OK: a limit stopped the walk; AT_END: the file's end did; anything else: what stands at *next is no whole block
// (the blocks in front of it are in `blocks`).
inline End walk(const File &file, int64_t at, int64_t max_inflated, size_t max_blocks, std::vector<Block> &blocks, int64_t *next)
{
    int64_t inflated = 0;
    size_t taken = 0;
    *next = at;
    for (;;) {
        Block b;
        const End e = readBlock(file, *next, b);
        if (e != OK) return e;
        if (taken && (inflated + (int64_t)b.isize > max_inflated || taken >= max_blocks)) return OK;
        blocks.push_back(b);
        inflated += b.isize;
        taken++;
        *next = b.at + b.bytes;
    }
}

} // namespace bgzf
