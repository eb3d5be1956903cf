// CPU check of the PLINK reader (openBedFile: .fam / .bim / .bed header and size) and of the host's view of a bed panel
// (genotypeAt, the site filter editing only the row map, the cache writer's byte table), on files the caller wrote into
// argv[1].  No GPU: the census a device would run is given as arguments of the good case.
#include "../../garlic_amd/host/garlic_host.hpp"

#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>

using namespace garlic_host;

static bool refused(const std::string &dir, const std::string &bed, const std::string &bim)
{
    try {
        BedFile *b = openBedFile(dir + "/" + bed, dir + "/" + bim, dir + "/good.fam");
        closeBedFile(b);
    } catch (...) {
        return true;
    }
    std::cerr << bed << " + " << bim << " was accepted\n";
    return false;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::cerr << "usage: bed_unit dir\n"; return 2; }
    const std::string dir = argv[1];
    // the files the test wrote: good.{bed,bim,fam} (5 individuals, 6 loci on chromosomes 1, 1, 1, 2, 2, chrX), and broken ones
    if (!refused(dir, "badmagic.bed", "good.bim") || !refused(dir, "truncated.bed", "good.bim") ||
        !refused(dir, "indmajor.bed", "good.bim") || !refused(dir, "good.bed", "multichar.bim") ||
        !refused(dir, "toolong.bed", "good.bim") || !refused(dir, "good.bed", "fivecols.bim"))
        return 1;
    try {
        BedFile *b = openBedFile(dir + "/good.bed", dir + "/good.bim", dir + "/good.fam");
        if (b->nind != 5 || b->nrows != 6 || b->row_bytes != 2) { std::cerr << "shape\n"; return 1; }
        if (b->ppos[1] != 1e6 || (int)b->ppos[1] != 1000000) { std::cerr << "ppos 1e6 read as " << b->ppos[1] << "\n"; return 1; }
        if (b->chr[2] != "1" || b->chr[3] != "2" || b->chr[5] != "chrX") { std::cerr << "chr column\n"; return 1; }
        if (b->a1[0] != 'A' || b->a2[0] != 'G' || b->name[4] != "rs4") { std::cerr << "bim columns\n"; return 1; }
        // rows as written by the test: row r, individual i has PLINK code (r + i) % 4
        for (int r = 0; r < 6; r++)
            for (int i = 0; i < 5; i++)
                if (((b->rows[(size_t)r * 2 + (i >> 2)] >> (2 * (i & 3))) & 3) != (unsigned)((r + i) % 4)) { std::cerr << "rows\n"; return 1; }
        // the host's view with a census as the device would give it: first non-missing code of row r is (r % 4 == 1 ? 2 : r % 4)
        b->counted = {0, 0, 0, 1, 0, 0};
        b->counts.assign(12, 0);
        HapData *h = new HapData{nullptr, 5, 6, nullptr, nullptr, nullptr, b, new long long[6]};
        b->refs = 1;
        for (int l = 0; l < 6; l++) h->bedRow[l] = l;
        for (int r = 0; r < 6; r++)
            for (int i = 0; i < 5; i++) {
                const unsigned code = (unsigned)((r + i) % 4);
                const short want = code == 1 ? -9 : code == 2 ? 1 : (code == 3) == (b->counted[r] == 1) ? 2 : 0;
                if (genotypeAt(h, r, i) != want) { std::cerr << "genotypeAt " << r << " " << i << "\n"; return 1; }
            }
        // the filter edits the row map only
        MapData *m = initMapData(6);
        m->chr = "chr1";
        FreqData *f = initFreqData(6);
        const double fr[6] = {0.5, 0.0, 0.25, 1.0, 0.75, 0.5};
        for (int l = 0; l < 6; l++) { f->freq[l] = fr[l]; m->physicalPos[l] = l; m->allele[l] = 'A'; }
        auto *maps = new std::vector<MapData *>{m};
        auto *haps = new std::vector<HapData *>{h};
        auto *freqs = new std::vector<FreqData *>{f};
        std::vector<GenoLikeData *> *gls = nullptr;
        if (filterMonomorphicSites(&maps, &haps, &freqs, &gls, false) != 4) { std::cerr << "filter count\n"; return 1; }
        const long long want_rows[4] = {0, 2, 4, 5};
        HapData *h2 = haps->at(0);
        if (h2->bed != b || h2->nloci != 4 || h2->data || h2->packed) { std::cerr << "filtered HapData\n"; return 1; }
        for (int l = 0; l < 4; l++)
            if (h2->bedRow[l] != want_rows[l] || genotypeAt(h2, l, 3) != bedGenotype(b->counted[want_rows[l]], (unsigned)((want_rows[l] + 3) % 4))) {
                std::cerr << "row map after the filter\n";
                return 1;
            }
        // the cache written from the bed panel loads to the same genotypes
        writeGenotypeCache(dir + "/from_bed.g2b", haps, maps, freqs);
        int nl = 0, ni = 0;
        std::vector<HapData *> *ch = nullptr; std::vector<MapData *> *cm = nullptr; std::vector<FreqData *> *cf = nullptr;
        loadGenotypeCache(dir + "/from_bed.g2b", nl, ni, &ch, &cm, &cf, true);
        if (nl != 4 || ni != 5) { std::cerr << "cache shape\n"; return 1; }
        for (int l = 0; l < 4; l++) {
            for (int i = 0; i < 5; i++)
                if (genotypeAt(ch->at(0), l, i) != genotypeAt(h2, l, i)) { std::cerr << "cache genotypes\n"; return 1; }
            if (ch->at(0)->packed[l][1] & 0xFC) { std::cerr << "cache pad bits\n"; return 1; }
        }
        releaseHapData(ch); releaseMapData(cm); releaseFreqData(cf);
        releaseHapData(haps);      // the last HapData closes the file
        releaseMapData(maps); releaseFreqData(freqs);
    } catch (...) { std::cerr << "exception\n"; return 1; }
    std::cout << "bed_unit ok\n";
    return 0;
}
