// Text files on the host as slabs of lines: what the readers of VCF, TPED and --tgls text share.  Header-only.
//
// The text goes to the device in slabs.  Reader reads a file through zlib (gzopen: plain text, .gz, and bgzf as multi-member
// gzip); SlabLines cuts a slab into lines with memchr: a slab ends wherever the read ended, so the bytes behind its last '\n'
// are carried to the front of the next one; the file's last line needs no '\n', and a '\r' before the '\n' belongs to the
// line.  forEachSlab is the loop over both.
#pragma once
#include <zlib.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace text {

// One slab of text cut into lines.  take(slab, n, last): the lines that are complete in [slab, slab + n) -- all of them when
// `last` (the file has ended: a final line without '\n' counts) -- as begin[k] / end[k] (end: the '\n' or n); returns the
// number of bytes consumed: the caller moves the rest, slab[consumed .. n), to the front of the next slab.  Empty lines
// are passed over.
struct SlabLines {
    std::vector<int64_t> begin, end, number;      // number: the line's 1-based number in the file, empty lines counted
    int64_t seen = 0;                             // lines of the file taken so far
    size_t take(const char *slab, size_t n, bool last)
    {
        begin.clear();
        end.clear();
        number.clear();
        size_t at = 0;
        while (at < n) {
            const char *nl = (const char *)memchr(slab + at, '\n', n - at);
            if (!nl && !last) break;
            const size_t e = nl ? (size_t)(nl - slab) : n;
            const bool blank = e == at || (e == at + 1 && slab[at] == '\r');
            seen++;
            if (!blank) {
                begin.push_back((int64_t)at);
                end.push_back((int64_t)e);
                number.push_back(seen);
            }
            at = nl ? e + 1 : n;
        }
        return at;
    }
};

// A file read through zlib in slabs of at most `cap` bytes.  next() fills the slab behind what the previous one left over;
// false when the file has ended and nothing is left.
struct Reader {
    gzFile f = nullptr;
    std::vector<char> slab;
    size_t have = 0;          // bytes of the slab in use
    bool eof = false;
    std::string error;
    bool open(const std::string &path, size_t cap)
    {
        f = gzopen(path.c_str(), "rb");
        if (!f) { error = "cannot open " + path; return false; }
        gzbuffer(f, 1 << 20);
        slab.resize(cap);
        have = 0;
        eof = false;
        return true;
    }
    // drop the first `consumed` bytes and read on; returns false on a read error (error set) -- at the end of the file it
    // returns true with eof set and have = what was left
    bool next(size_t consumed)
    {
        memmove(slab.data(), slab.data() + consumed, have - consumed);
        have -= consumed;
        while (!eof && have < slab.size()) {
            const size_t want = slab.size() - have;
            const int got = gzread(f, slab.data() + have, (unsigned)(want < (1u << 30) ? want : (1u << 30)));
            if (got < 0) { int e; error = gzerror(f, &e); return false; }
            if (got == 0) {
                // a truncated .gz hands out what it has and leaves Z_BUF_ERROR behind: no clean end of the file
                int e = Z_OK;
                const char *msg = gzerror(f, &e);
                if (e != Z_OK && e != Z_STREAM_END) { error = std::string("read error (truncated file?): ") + msg; return false; }
                eof = true;
            }
            have += (size_t)got;
        }
        return true;
    }
    void close() { if (f) gzclose(f); f = nullptr; }
    ~Reader() { close(); }
};

// How a walk over a file's slabs ended.  The caller words what it tells its user.
enum SlabsEnd {
    SLABS_DONE = 0,           // the file's last line has been handed over
    SLABS_STOPPED,            // onSlab returned false
    SLABS_NO_FILE,            // error: what the reader says about the open
    SLABS_READ_ERROR,         // error: what the reader says about the read
    SLABS_LONG_LINE           // a slab of slabBytes holds no line end
};

// path in slabs of at most slabBytes, cut at line ends: onSlab(reader, lines, consumed) for every slab -- lines.begin /
// end / number index reader.slab, of which the first `consumed` bytes are those lines and reader.have are in use -- until the
// file ends or onSlab returns false.  A slab without a complete line (the file's last, when only empty lines are left) is handed over
// too, with no lines.
template <class OnSlab>
inline SlabsEnd forEachSlab(const std::string &path, size_t slabBytes, std::string &error, OnSlab onSlab)
{
    Reader rd;
    if (!rd.open(path, slabBytes)) { error = rd.error; return SLABS_NO_FILE; }
    SlabLines cut;
    size_t consumed = 0;
    do {
        if (!rd.next(consumed)) { error = rd.error; return SLABS_READ_ERROR; }
        consumed = cut.take(rd.slab.data(), rd.have, rd.eof);
        if (!rd.eof && consumed == 0 && rd.have == rd.slab.size()) return SLABS_LONG_LINE;
        if (!onSlab(rd, cut, consumed)) return SLABS_STOPPED;
    } while (!rd.eof || consumed < rd.have);
    return SLABS_DONE;
}

// The same walk for a caller that is asked for one line at a time.  next(k): the next line is lines.begin / end / number [k]
// of rd.slab (the slab behind it is read where this one is used up); false: `why` says how the walk ended, rd.error the rest.
struct LineCursor {
    Reader rd;
    SlabLines lines;
    size_t consumed = 0, at = 0;      // the bytes of the slab that `lines` covers (none is read yet: 0 of 0); the next line
    SlabsEnd why = SLABS_DONE;
    bool next(size_t &k)
    {
        while (at >= lines.begin.size()) {
            why = SLABS_DONE;
            if (rd.eof && consumed >= rd.have) return false;
            why = SLABS_READ_ERROR;
            if (!rd.next(consumed)) return false;
            consumed = lines.take(rd.slab.data(), rd.have, rd.eof);
            why = SLABS_LONG_LINE;
            if (!rd.eof && consumed == 0 && rd.have == rd.slab.size()) return false;
            at = 0;
        }
        k = at++;
        return true;
    }
};

} // namespace text
