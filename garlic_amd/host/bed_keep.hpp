// Which individuals of a PLINK .fam a run keeps: the keep file of --keep, the family IDs of --pops.  Header-only, no device.
//
//   readFam       the (FID, IID) pairs of a .fam in file order
//   readKeepFile  a PLINK keep file -- one `FID IID` per line, further columns ignored, blank lines skipped, CRLF accepted --
//                 as the kept individuals' indices in the .FAM's order (not the keep file's).  A pair that is not in the .fam
//                 is an error naming file, line and pair; a pair listed twice counts once; an empty result is an error.
//   famFamilies   the distinct family IDs of a .fam in first-seen order, with their members (ascending indices)
// Errors are std::runtime_error with the whole message.
#pragma once
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace garlic_host {

struct FamEntry {
    std::string fid, iid;
};

struct FamFamily {
    std::string fid;
    std::vector<int> members;      // indices into the .fam, ascending
};

namespace bed_keep_detail {
// the first two whitespace-separated fields of a line; false for a blank line
inline bool firstTwo(const std::string &line, std::string &a, std::string &b, int &nfields)
{
    std::stringstream ss(line);      // (>> skips \r with the other white space: CRLF files read like LF files)
    nfields = 0;
    std::string tok;
    while (ss >> tok) {
        if (nfields == 0) a = tok;
        else if (nfields == 1) b = tok;
        nfields++;
    }
    return nfields > 0;
}
} // namespace bed_keep_detail

inline std::vector<FamEntry> readFam(const std::string &famfile)
{
    std::ifstream in(famfile);
    if (!in) throw std::runtime_error("Failed to open " + famfile);
    std::vector<FamEntry> fam;
    std::map<std::pair<std::string, std::string>, int> seen;
    std::string line;
    int n = 0;
    while (std::getline(in, line)) {
        n++;
        FamEntry e;
        int nf = 0;
        if (!bed_keep_detail::firstTwo(line, e.fid, e.iid, nf)) continue;
        if (nf < 2) throw std::runtime_error("line " + std::to_string(n) + " of " + famfile + " has fewer than 2 columns");
        if (!seen.emplace(std::make_pair(e.fid, e.iid), n).second)
            throw std::runtime_error("Found duplicate individual (" + e.fid + " " + e.iid + ") on line " + std::to_string(n) + " of " + famfile);
        fam.push_back(e);
    }
    return fam;
}

inline std::vector<int> readKeepFile(const std::string &keepfile, const std::vector<FamEntry> &fam)
{
    std::ifstream in(keepfile);
    if (!in) throw std::runtime_error("Failed to open " + keepfile);
    std::map<std::pair<std::string, std::string>, int> at;
    for (size_t i = 0; i < fam.size(); i++) at.emplace(std::make_pair(fam[i].fid, fam[i].iid), (int)i);
    std::vector<char> kept(fam.size(), 0);
    std::string line, fid, iid;
    int n = 0;
    while (std::getline(in, line)) {
        n++;
        int nf = 0;
        if (!bed_keep_detail::firstTwo(line, fid, iid, nf)) continue;
        if (nf < 2) throw std::runtime_error("line " + std::to_string(n) + " of " + keepfile + " has fewer than 2 columns (FID IID)");
        const auto hit = at.find(std::make_pair(fid, iid));
        if (hit == at.end())
            throw std::runtime_error(keepfile + ", line " + std::to_string(n) + ": individual (" + fid + " " + iid + ") is not in the .fam");
        kept[(size_t)hit->second] = 1;
    }
    std::vector<int> idx;
    for (size_t i = 0; i < kept.size(); i++)
        if (kept[i]) idx.push_back((int)i);
    if (idx.empty()) throw std::runtime_error(keepfile + " keeps no individual");
    return idx;
}

inline std::vector<FamFamily> famFamilies(const std::vector<FamEntry> &fam)
{
    std::vector<FamFamily> out;
    std::map<std::string, size_t> at;
    for (size_t i = 0; i < fam.size(); i++) {
        const auto ins = at.emplace(fam[i].fid, out.size());
        if (ins.second) out.push_back({fam[i].fid, {}});
        out[ins.first->second].members.push_back((int)i);
    }
    return out;
}

} // namespace garlic_host
