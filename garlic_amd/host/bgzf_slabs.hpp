// A BGZF text file as slabs of lines that stand on the devices: the counterpart of text::Reader + text::SlabLines
// (text_slabs.hpp) for a file that is inflated there.  Header-only; calls the library (garlic_hip.h).
//
// A slab is the carried tail of the previous one (the bytes behind its last '\n', moved device to device into the other of two
// buffers) plus whole BGZF blocks, up to slabBytes: the compressed bytes go to every device of the list and are inflated there
// (garlic_bgzf_inflate), the first device cuts the lines (garlic_text_lines) and hands the host their offsets, numbers and
// heads.  forEach is forEachSlab's loop.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/garlic_hip.h"
#include "bgzf_blocks.hpp"

namespace bgzf {

// one slab, as onSlab gets it
struct DeviceSlab {
    std::vector<int64_t> begin, end, number;      // as text::SlabLines has them
    std::vector<uint8_t> heads;                   // [lines][head_bytes]
    int64_t head_bytes = 0, have = 0;             // have: bytes of the slab in use
    std::vector<garlic_ctx *> ctx;                // per device of the list
    std::vector<char *> text;                     // the slab there
    const char *head(size_t k) const { return (const char *)heads.data() + k * (size_t)head_bytes; }
    size_t headLen(size_t k) const { return (size_t)(end[k] - begin[k] < head_bytes ? end[k] - begin[k] : head_bytes); }
    bool whole(size_t k) const { return end[k] - begin[k] <= head_bytes; }
    // line k from the first device into buf; false: garlic_hip_last_error says why
    bool fetch(size_t k, std::vector<char> &buf) const { return fetchRange(0, begin[k], end[k], buf); }
    bool fetchRange(size_t dev, int64_t from, int64_t to, std::vector<char> &buf) const
    {
        buf.resize((size_t)(to - from));
        return garlic_device_download(ctx[dev], buf.data(), text[dev] + from, to - from) == GARLIC_OK;
    }
};

enum DeviceSlabsEnd {
    DEV_DONE = 0,
    DEV_STOPPED,              // onSlab returned false
    DEV_NO_FILE,
    DEV_NOT_BGZF,             // the file stops being BGZF, or ends inside a block: error says where
    DEV_BAD_BLOCK,            // a block with a bad status: error is the library's message
    DEV_LONG_LINE,            // a slab of slabBytes holds no line end
    DEV_ERROR                 // the library failed otherwise: error is its message
};

struct DeviceSlabs {
    std::vector<garlic_ctx *> ctx;
    std::vector<char *> buf[2];
    int64_t slabBytes = 0, blocks = 0;            // blocks: inflated so far (per device)
    std::string error;

    bool open(const std::vector<int> &devices, int64_t slab_bytes)
    {
        slabBytes = slab_bytes < MEMBER_MAX ? MEMBER_MAX : slab_bytes;
        for (int d : devices) {
            garlic_ctx *c = nullptr;
            if (garlic_ctx_create(d, nullptr, &c) != GARLIC_OK) { error = garlic_hip_last_error(); return false; }
            ctx.push_back(c);
            for (int k = 0; k < 2; k++) {
                void *p = nullptr;
                if (garlic_device_alloc(c, slabBytes + 2 * MEMBER_MAX + 16, &p) != GARLIC_OK) { error = garlic_hip_last_error(); return false; }
                buf[k].push_back((char *)p);
            }
        }
        return true;
    }
    void close()
    {
        for (size_t d = 0; d < ctx.size(); d++) {
            for (int k = 0; k < 2; k++)
                if (d < buf[k].size()) garlic_device_free(ctx[d], buf[k][d]);
            garlic_ctx_destroy(ctx[d]);
        }
        ctx.clear();
        buf[0].clear();
        buf[1].clear();
    }
    ~DeviceSlabs() { close(); }

    template <class OnSlab> DeviceSlabsEnd forEach(const std::string &path, int64_t head_bytes, OnSlab onSlab)
    {
        File file;
        if (!file.open(path)) { error = "cannot open " + path; return DEV_NO_FILE; }
        DeviceSlab slab;
        slab.head_bytes = head_bytes;
        slab.ctx = ctx;
        slab.text.resize(ctx.size());
        std::vector<Block> list;
        std::vector<uint8_t> comp;
        std::vector<int64_t> bb, ob;
        int64_t at = 0, tail = 0, seen = 0, capacity = 1 << 16;
        int cur = 0;
        bool last = false;
        do {
            list.clear();
            int64_t next = at;
            const End e = walk(file, at, slabBytes > tail ? slabBytes - tail : 0, (size_t)1 << 20, list, &next);
            if (e != OK && e != AT_END) {
                error = "byte " + std::to_string(next) + (e == NOT_BGZF ? ": no BGZF block" : e == PAST_END ? ": a block that runs past the file's end"
                                                          : e == CUT_SHORT ? ": the file ends inside a block's header" : ": read error");
                return DEV_NOT_BGZF;
            }
            last = e == AT_END;
            comp.resize((size_t)(next - at));
            if (!comp.empty() && !file.read(at, comp.data(), comp.size())) { error = "byte " + std::to_string(at) + ": read error"; return DEV_NOT_BGZF; }
            bb.assign(1, 0);
            ob.assign(1, 0);
            for (const Block &b : list) {
                bb.push_back(b.at + b.bytes - at);
                ob.push_back(ob.back() + (int64_t)b.isize);
            }
            for (size_t d = 0; d < ctx.size(); d++) {
                const int rc = garlic_bgzf_inflate(ctx[d], comp.data(), (int64_t)comp.size(), bb.data(), (int64_t)list.size(), buf[cur][d] + tail,
                                                   ob.data(), nullptr, GARLIC_HOST);
                if (rc != GARLIC_OK) {
                    error = garlic_hip_last_error();
                    return rc == GARLIC_ERR_INVALID ? DEV_BAD_BLOCK : DEV_ERROR;
                }
                slab.text[d] = buf[cur][d];
            }
            blocks += (int64_t)list.size();
            slab.have = tail + ob.back();
            int64_t n_lines = 0, consumed = 0, seen_out = seen;
            for (;;) {
                slab.begin.resize((size_t)capacity);
                slab.end.resize((size_t)capacity);
                slab.number.resize((size_t)capacity);
                slab.heads.resize((size_t)(capacity * head_bytes));
                const int rc = garlic_text_lines(ctx[0], slab.text[0], slab.have, last ? 1 : 0, seen, head_bytes, capacity, slab.begin.data(),
                                                 slab.end.data(), slab.number.data(), slab.heads.data(), &n_lines, &consumed, &seen_out);
                if (rc == GARLIC_ERR_RANGE) { capacity = n_lines; continue; }
                if (rc != GARLIC_OK) { error = garlic_hip_last_error(); return DEV_ERROR; }
                break;
            }
            slab.begin.resize((size_t)n_lines);
            slab.end.resize((size_t)n_lines);
            slab.number.resize((size_t)n_lines);
            seen = seen_out;
            if (!last && consumed == 0 && slabBytes - slab.have < MEMBER_MAX) return DEV_LONG_LINE;
            if (!onSlab(slab)) return DEV_STOPPED;
            tail = slab.have - consumed;
            for (size_t d = 0; d < ctx.size() && tail; d++)
                if (garlic_device_copy(ctx[d], buf[cur ^ 1][d], buf[cur][d] + consumed, tail) != GARLIC_OK) { error = garlic_hip_last_error(); return DEV_ERROR; }
            cur ^= 1;
            at = next;
        } while (!last);
        return DEV_DONE;
    }
};

} // namespace bgzf
