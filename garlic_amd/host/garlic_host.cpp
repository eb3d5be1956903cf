// Host adapter: the reference's Phase-I interface on top of libgarlic_hip.so (see garlic_host.hpp).
#include "garlic_host.hpp"
#include "vcf_lines.hpp"
#include "tped_lines.hpp"
#include "bgzf_slabs.hpp"

#include "../../include/garlic_hip.h"

#include <zlib.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <sstream>
#include <random>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <ctime>

namespace garlic_host {

namespace {

struct CentroRow {
    const char *chr;
    int start, end;
};
#include "centromere_tables.inc"

[[noreturn]] void fail(const std::string &msg)
{
    std::cerr << "ERROR: " << msg << "\n";
    throw 0; // the reference's error convention (src/garlic-data.cpp:1619; main catches `...`)
}

// line reader over plain or gzip files (the reference reads everything through gzstream)
class LineReader {
public:
    explicit LineReader(const std::string &path) : f(gzopen(path.c_str(), "rb"))
    {
        if (!f) fail("Failed to open " + path);
        gzbuffer(f, 1 << 20);
    }
    ~LineReader() { if (f) gzclose(f); }
    bool next(std::string &line)
    {
        line.clear();
        char buf[1 << 16];
        while (gzgets(f, buf, sizeof buf)) {
            size_t n = strlen(buf);
            if (n && buf[n - 1] == '\n') {
                line.append(buf, n - 1);
                if (!line.empty() && line.back() == '\r') line.pop_back();
                return true;
            }
            line.append(buf, n);
        }
        return !line.empty();
    }

private:
    gzFile f;
};

int countFields(const std::string &s)
{
    int n = 0;
    bool in = false;
    for (char c : s) {
        bool ws = (c == ' ' || c == '\t' || c == '\r' || c == '\n');
        if (!ws && !in) n++;
        in = !ws;
    }
    return n;
}

LodOptions g_options;

void check(int rc, const char *what)
{
    if (rc != GARLIC_OK) fail(std::string(what) + ": " + garlic_hip_last_error());
}

} // namespace

// ------------------------------------------------------------------------- centromere
std::string checkChrName(std::string chr)
{
    if (chr.empty() || chr[0] != 'c') chr = "chr" + chr;
    return chr;
}

centromere::centromere(const std::string &arg, const std::string &file, const std::string &defaultFileName)
{
    const CentroRow *rows = nullptr;
    size_t n = 0;
    if (arg == "hg18") { rows = k_hg18; n = sizeof k_hg18 / sizeof *k_hg18; }
    else if (arg == "hg19") { rows = k_hg19; n = sizeof k_hg19 / sizeof *k_hg19; }
    else if (arg == "hg38") { rows = k_hg38; n = sizeof k_hg38 / sizeof *k_hg38; }
    for (size_t i = 0; i < n; i++) set(rows[i].chr, rows[i].start, rows[i].end);
    if (!rows && file != defaultFileName) readCustomCentromeres(file);
}

void centromere::set(const std::string &chr, int start, int end)
{
    gapStart[checkChrName(chr)] = start;
    gapEnd[checkChrName(chr)] = end;
}

void centromere::readCustomCentromeres(const std::string &filename)
{
    LineReader in(filename);
    std::string line;
    int rows = 0;
    while (in.next(line)) {
        if (countFields(line) != 3) { std::cerr << "ERROR: Custom centromere file requires three columns.\n"; continue; }
        std::stringstream ss(line);
        std::string chr;
        int s, e;
        ss >> chr >> s >> e;
        set(chr, s, e);
        rows++;
    }
    std::cerr << "Loaded custom centromere limits for " << rows << " chromosomes.\n";
}

int centromere::centromereStart(const std::string &chr)
{
    auto it = gapStart.find(chr);
    if (it == gapStart.end()) { // unknown chromosome: 0 and one warning (garlic-centromeres.cpp:33-45)
        if (!warned[chr]++) std::cerr << "WARNING: No centromere information for chr: " << chr << "\n";
        return 0;
    }
    return it->second;
}

int centromere::centromereEnd(const std::string &chr)
{
    auto it = gapEnd.find(chr);
    if (it == gapEnd.end()) {
        if (!warned[chr]++) std::cerr << "WARNING: No centromere information for chr: " << chr << "\n";
        return 0;
    }
    return it->second;
}

// ------------------------------------------------------------------------- structs
HapData *initHapData(unsigned int nind, unsigned int nloci, bool PHASED)
{
    if (nind < 1 || nloci < 1) fail("Can not allocate HapData object: counts must be positive.");
    HapData *d = new HapData;
    d->nind = nind;
    d->nloci = nloci;
    d->data = new short *[nloci];
    d->firstCopy = PHASED ? new bool *[nloci] : nullptr;
    d->packed = nullptr;
    d->phaseBits = nullptr;
    d->bed = nullptr;
    d->bedRow = nullptr;
    for (unsigned l = 0; l < nloci; l++) {
        d->data[l] = new short[nind];
        std::fill(d->data[l], d->data[l] + nind, (short)MISSING);
        if (PHASED) {
            d->firstCopy[l] = new bool[nind];
            std::fill(d->firstCopy[l], d->firstCopy[l] + nind, false);
        }
    }
    return d;
}
void releaseHapData(HapData *d)
{
    if (!d) return;
    for (int l = 0; l < d->nloci; l++) {
        if (d->data) delete[] d->data[l];
        if (d->firstCopy) delete[] d->firstCopy[l];
        if (d->packed) delete[] d->packed[l];
        if (d->phaseBits) delete[] d->phaseBits[l];
    }
    delete[] d->data;
    delete[] d->firstCopy;
    delete[] d->packed;
    delete[] d->phaseBits;
    delete[] d->bedRow;
    if (d->bed && --d->bed->refs == 0) closeBedFile(d->bed);
    delete d;
}
void releaseHapData(std::vector<HapData *> *v) { for (auto d : *v) releaseHapData(d); delete v; }

MapData *initMapData(int nloci)
{
    if (nloci < 1) fail("number of loci must be positive.");
    MapData *d = new MapData;
    d->nloci = nloci;
    d->physicalPos = new int[nloci];
    d->geneticPos = new double[nloci];
    d->locusName = new std::string[nloci];
    d->allele = new char[nloci];
    d->chr = "--";
    for (int l = 0; l < nloci; l++) { d->physicalPos[l] = MISSING; d->geneticPos[l] = MISSING; d->locusName[l] = "--"; d->allele[l] = '-'; }
    return d;
}
void releaseMapData(MapData *d)
{
    if (!d) return;
    delete[] d->physicalPos; delete[] d->geneticPos; delete[] d->locusName; delete[] d->allele;
    delete d;
}
void releaseMapData(std::vector<MapData *> *v) { for (auto d : *v) releaseMapData(d); delete v; }

FreqData *initFreqData(int nloci)
{
    if (nloci < 1) fail("number of loci must be positive.");
    FreqData *d = new FreqData;
    d->nloci = nloci;
    d->freq = new double[nloci];
    std::fill(d->freq, d->freq + nloci, (double)MISSING);
    return d;
}
void releaseFreqData(FreqData *d) { if (d) { delete[] d->freq; delete d; } }
void releaseFreqData(std::vector<FreqData *> *v) { for (auto d : *v) releaseFreqData(d); delete v; }

static void closeTglsFile(TglsFile *f)
{
    if (!f) return;
    for (auto &o : f->objects) {
        if (o.tgls) garlic_tgls_destroy((garlic_tgls *)o.tgls);
        if (o.ctx) garlic_ctx_destroy((garlic_ctx *)o.ctx);
    }
    delete f;
}

GenoLikeData *initGLData(unsigned int nind, unsigned int nloci)
{
    if (nind < 1 || nloci < 1) fail("Can not allocate GenoLikeData object: counts must be positive.");
    GenoLikeData *d = new GenoLikeData;
    d->nind = nind;
    d->nloci = nloci;
    d->data = new double *[nloci];
    d->codes = nullptr;
    d->values = nullptr;
    d->nvalues = 0;
    d->codes16 = nullptr;
    d->tgls = nullptr;
    d->tglsRow = nullptr;
    for (unsigned l = 0; l < nloci; l++) {
        d->data[l] = new double[nind];
        std::fill(d->data[l], d->data[l] + nind, (double)MISSING);
    }
    return d;
}
void releaseGLData(GenoLikeData *d)
{
    if (!d) return;
    for (int l = 0; l < d->nloci; l++) {
        if (d->data) delete[] d->data[l];
        if (d->codes) delete[] d->codes[l];
        if (d->codes16) delete[] d->codes16[l];
    }
    delete[] d->data;
    delete[] d->codes;
    delete[] d->codes16;
    delete[] d->values;
    delete[] d->tglsRow;
    if (d->tgls && --d->tgls->refs == 0) closeTglsFile(d->tgls);
    delete d;
}
void releaseGLData(std::vector<GenoLikeData *> *v) { for (auto d : *v) releaseGLData(d); delete v; }

LDData *initLDData(int nloci, int winsize)
{
    LDData *d = new LDData;
    d->nloci = nloci;
    d->winsize = winsize;
    d->LD = new double *[nloci];
    for (int l = 0; l < nloci; l++) {
        d->LD[l] = new double[winsize];
        std::fill(d->LD[l], d->LD[l] + winsize, 0.0);
    }
    return d;
}
void releaseLDData(LDData *d)
{
    if (!d) return;
    for (int l = 0; l < d->nloci; l++) delete[] d->LD[l];
    delete[] d->LD;
    delete d;
}

void releaseLDData(std::vector<LDData *> *v)
{
    if (!v) return;
    for (auto d : *v) releaseLDData(d);
    delete v;
}

std::vector<GenoFreqData *> *calculateGenoFreq(std::vector<HapData *> *haps)
{   // garlic-data.cpp:648-676
    std::vector<GenoFreqData *> *out = new std::vector<GenoFreqData *>;
    for (auto h : *haps) {
        GenoFreqData *g = new GenoFreqData;
        g->nloci = h->nloci;
        g->homFreq = new double[h->nloci];
        for (int l = 0; l < h->nloci; l++) {
            double total = 0, hom = 0;
            for (int i = 0; i < h->nind; i++) {
                const short v = genotypeAt(h, l, i);
                if (v != -9) {
                    if (v == 2 || v == 0) hom++;
                    total++;
                }
            }
            hom /= total;
            g->homFreq[l] = hom;
        }
        out->push_back(g);
    }
    return out;
}
void releaseGenoFreq(std::vector<GenoFreqData *> *v)
{
    if (!v) return;
    for (auto g : *v) { delete[] g->homFreq; delete g; }
    delete v;
}

WinData *initWinData(unsigned int nind, unsigned int nloci)
{
    if (nind < 1 || nloci < 1) {
        std::cerr << "ERROR: Can't allocate WinData object.  Number of individuals (" << nind
                  << ") and number of loci (" << nloci << ") must be positive.\n";
        throw 0;
    }
    WinData *d = new WinData;
    d->nind = nind;
    d->nloci = nloci;
    d->data = new double *[nind];
    for (unsigned i = 0; i < nind; i++) d->data[i] = new double[nloci]; // filled by the device result
    return d;
}
std::vector<WinData *> *initWinData(std::vector<MapData *> *maps, int nind)
{
    auto *v = new std::vector<WinData *>;
    for (auto m : *maps) v->push_back(initWinData(nind, m->nloci));
    return v;
}
void releaseWinData(WinData *d)
{
    if (!d) return;
    for (int i = 0; i < d->nind; i++) delete[] d->data[i];
    delete[] d->data;
    delete d;
}
void releaseWinData(std::vector<WinData *> *v) { for (auto d : *v) releaseWinData(d); delete v; }
void releaseDoubleData(DoubleData *d) { if (d) { delete[] d->data; delete d; } }
void releaseIndData(IndData *d) { if (d) { delete[] d->indID; delete d; } }

// ------------------------------------------------------------------------- ingest
namespace {
void flushChromosome(const std::string &chr, std::vector<short *> &hap, std::vector<bool *> &fc, std::vector<double> &gpos,
                     std::vector<double> &ppos, std::vector<std::string> &names, std::vector<char> &allele,
                     std::vector<double> &freq, int numInd, std::vector<HapData *> *haps,
                     std::vector<MapData *> *maps, std::vector<FreqData *> *freqs)
{
    const int n = (int)hap.size();
    MapData *m = initMapData(n);
    m->chr = checkChrName(chr);
    HapData *h = new HapData;
    h->nind = numInd;
    h->nloci = n;
    h->data = new short *[n];
    h->firstCopy = fc.empty() ? nullptr : new bool *[n];
    h->packed = nullptr;
    h->phaseBits = nullptr;
    h->bed = nullptr;
    h->bedRow = nullptr;
    FreqData *f = initFreqData(n);
    for (int l = 0; l < n; l++) {
        if (h->firstCopy) h->firstCopy[l] = fc[l];
        m->physicalPos[l] = (int)ppos[l]; // read as double, stored as int (garlic-data.cpp:41,229)
        m->geneticPos[l] = gpos[l];
        m->locusName[l] = names[l];
        m->allele[l] = allele[l];
        h->data[l] = hap[l];
        f->freq[l] = freq[l];
    }
    maps->push_back(m);
    haps->push_back(h);
    freqs->push_back(f);
    hap.clear(); fc.clear(); gpos.clear(); ppos.clear(); names.clear(); allele.clear(); freq.clear();
}
} // namespace

namespace {
struct TpedLine {          // one parsed TPED line (garlic-data.cpp:56-141)
    std::string chr, name;
    double g = 0, p = 0;
    int numInd = 0;
    short *data = nullptr;
    bool *first = nullptr;
    char one = 0;
    double freq = 0;
    int total = 0;         // non-missing alleles on the line
};

TpedLine parseTpedLine(const std::string &line, char TPED_MISSING, bool PHASED)
{
    TpedLine r;
    r.numInd = (countFields(line) - 4) / 2; // garlic-data.cpp:59-60
    // the four leading fields through a stream (tiny), the allele columns by hand: at 10k
    // individuals a line is 40 KB and formatted extraction of every character dominated the load
    size_t at = 0;
    for (int field = 0; field < 4; field++) {
        while (at < line.size() && isspace((unsigned char)line[at])) at++;
        while (at < line.size() && !isspace((unsigned char)line[at])) at++;
    }
    std::stringstream ss(line.substr(0, at));
    ss >> r.chr >> r.name >> r.g >> r.p;
    const char *cur = line.data() + at, *const end = line.data() + line.size();
    auto next_allele = [&]() -> char {   // `ss >> char`: the next non-blank character, TPED_MISSING at the end
        while (cur < end && (*cur == ' ' || *cur == '\t' || *cur == '\r')) cur++;
        return cur < end ? *cur++ : TPED_MISSING;
    };
    const int n = std::max(r.numInd, 0);
    r.data = new short[n > 0 ? n : 1];
    r.first = PHASED ? new bool[n > 0 ? n : 1] : nullptr;
    char one = TPED_MISSING; // the first non-missing allele on the line is the counted one
    int nalleles = 0, total = 0;
    for (int i = 0; i < n; i++) {
        const char a1 = next_allele(), a2 = next_allele(); // alleles are single characters (garlic-data.cpp:47,111)
        if (one == TPED_MISSING && a1 != TPED_MISSING) one = a1;
        if (one == TPED_MISSING && a2 != TPED_MISSING) one = a2;
        int v = 0;
        for (char a : {a1, a2}) {
            if (a == TPED_MISSING) v += -9;
            else { total++; if (a == one) { v += 1; nalleles++; } }
        }
        r.data[i] = (short)(v < 0 ? -9 : v);
        if (r.first) r.first[i] = (a1 == one);   // garlic-data.cpp:129
    }
    r.one = one;
    r.total = total;
    r.freq = total == 0 ? 0.0 : double(nalleles) / double(total); // garlic-data.cpp:140-141
    return r;
}
} // namespace

void loadTPEDData(const std::string &tpedfile, int &numLoci, int &numInd, std::vector<HapData *> **hapDataByChr,
                  std::vector<MapData *> **mapDataByChr, std::vector<FreqData *> **freqDataByChr,
                  char TPED_MISSING, bool PHASED, int nresample, unsigned long long resampleSeed)
{
    // --resample (garlic-data.cpp:16-20, 142-148): the frequency of every SNP becomes the fraction of
    // nresample uniform draws that fall at or below it, one generator for the whole file, in file order.
    // The reference's generator is GSL's default, mt19937 seeded with time(NULL), gsl_rng_uniform =
    // 32 bits / 2^32: std::mt19937 seeded alike is the same stream (GSL maps seed 0 to 4357), so a run
    // given the reference's seed resamples to the same frequencies.
    const unsigned long long seed0 = resampleSeed ? resampleSeed : (unsigned long long)time(nullptr);
    std::mt19937 resampler((uint32_t)(seed0 & 0xffffffffull) ? (uint32_t)(seed0 & 0xffffffffull) : 4357u);
    LineReader in(tpedfile);
    *hapDataByChr = new std::vector<HapData *>;
    *mapDataByChr = new std::vector<MapData *>;
    *freqDataByChr = new std::vector<FreqData *>;
    std::vector<short *> hap;
    std::vector<bool *> fc;
    std::vector<double> gpos, ppos, freq;
    std::vector<std::string> names;
    std::vector<char> allele;
    std::string chr, prevChr;
    numLoci = 0;
    numInd = 0;
    // Lines are independent: one thread reads (and inflates), batches of lines are parsed on all
    // cores, the results join the chromosomes in file order.
    const unsigned nthreads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const size_t batch_lines = 64 * nthreads;
    std::vector<std::string> lines;
    std::vector<TpedLine> parsed;
    bool more = true;
    while (more) {
        lines.clear();
        std::string line;
        while (lines.size() < batch_lines && (more = in.next(line)))
            if (!line.empty()) lines.push_back(std::move(line));
        parsed.assign(lines.size(), TpedLine());
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nthreads && t < lines.size(); t++)
            th.emplace_back([&, t] {
                for (size_t k = t; k < lines.size(); k += nthreads) parsed[k] = parseTpedLine(lines[k], TPED_MISSING, PHASED);
            });
        for (auto &t : th) t.join();
        for (TpedLine &r : parsed) {
            numLoci++;
            numInd = r.numInd;
            chr = r.chr;
            if (numLoci == 1) prevChr = chr;
            if (chr != prevChr) { // new chromosome when the chr string changes (garlic-data.cpp:68-91)
                flushChromosome(prevChr, hap, fc, gpos, ppos, names, allele, freq, numInd, *hapDataByChr,
                                *mapDataByChr, *freqDataByChr);
                prevChr = chr;
            }
            hap.push_back(r.data);
            if (r.first) fc.push_back(r.first);
            gpos.push_back(r.g);
            ppos.push_back(r.p);
            names.push_back(r.name);
            allele.push_back(r.one);
            if (nresample > 0 && r.total != 0) {
                int count = 0;
                for (int i = 0; i < nresample; i++)
                    if ((double)resampler() / 4294967296.0 <= r.freq) count++;
                r.freq = double(count) / double(nresample);
            }
            freq.push_back(r.freq);
        }
    }
    if (numLoci == 0) fail("no loci in " + tpedfile);
    flushChromosome(chr, hap, fc, gpos, ppos, names, allele, freq, numInd, *hapDataByChr, *mapDataByChr,
                    *freqDataByChr);
}

// ------------------------------------------------------------------------- PLINK .bed/.bim/.fam
void closeBedFile(BedFile *b)
{
    if (!b) return;
    for (auto &im : b->images) {
        if (im.bed) garlic_bed_destroy((garlic_bed *)im.bed);
        if (im.ctx) garlic_ctx_destroy((garlic_ctx *)im.ctx);
    }
    if (b->map) munmap(b->map, b->map_bytes);
    BedFile *parent = b->parent;      // (its contexts carried this file's extracts: it goes after them)
    delete b;
    if (parent) releaseBedFile(parent);
}

void releaseBedFile(BedFile *b)
{
    if (b && --b->refs <= 0) closeBedFile(b);
}

BedFile *openBedFile(const std::string &bedfile, const std::string &bimfile, const std::string &famfile, bool anyPopulations)
{
    std::unique_ptr<BedFile, void (*)(BedFile *)> b(new BedFile, closeBedFile);
    b->path = bedfile;
    std::string pop;
    if (anyPopulations) {
        try {
            b->nind = (int)readFam(famfile).size();
        } catch (const std::exception &e) {
            fail(e.what());
        }
    } else {
        scanIndData3(famfile, b->nind, pop);
    }
    if (b->nind < 1) fail("no individuals in " + famfile);
    b->row_bytes = ((size_t)b->nind + 3) / 4;
    {
        LineReader in(bimfile);
        std::string line;
        int n = 0;
        while (in.next(line)) {
            n++;
            if (line.empty()) continue;
            if (countFields(line) != 6)
                fail("line " + std::to_string(n) + " of " + bimfile + " does not have the 6 columns chr snpid gpos ppos a1 a2");
            std::stringstream ss(line);
            std::string chr, name, a1, a2;
            double g = 0, p = 0;       // ppos as a double, stored as an int later: "1e6" is 1000000 as on the TPED path
            ss >> chr >> name >> g >> p >> a1 >> a2;
            if (ss.fail()) fail("line " + std::to_string(n) + " of " + bimfile + ": cannot read gpos / ppos");
            if (a1.size() != 1 || a2.size() != 1)
                fail("line " + std::to_string(n) + " of " + bimfile + ": allele \"" + (a1.size() != 1 ? a1 : a2) +
                     "\" is not a single character (GARLIC's alleles are single characters)");
            b->chr.push_back(chr); b->name.push_back(name); b->gpos.push_back(g); b->ppos.push_back(p);
            b->a1.push_back(a1[0]); b->a2.push_back(a2[0]);
        }
    }
    b->nrows = (long long)b->chr.size();
    if (b->nrows < 1) fail("no loci in " + bimfile);
    const int fd = open(bedfile.c_str(), O_RDONLY);
    if (fd < 0) fail("Failed to open " + bedfile);
    struct stat st;
    if (fstat(fd, &st) != 0) { close(fd); fail("Failed to stat " + bedfile); }
    unsigned char magic[3] = {0, 0, 0};
    const ssize_t got = pread(fd, magic, 3, 0);
    if (got != 3 || magic[0] != 0x6c || magic[1] != 0x1b) { close(fd); fail(bedfile + " is not a PLINK .bed file (magic bytes 6c 1b 01 expected)"); }
    if (magic[2] == 0x00) { close(fd); fail(bedfile + " is an individual-major .bed (6c 1b 00); only SNP-major files (6c 1b 01) are read"); }
    if (magic[2] != 0x01) { close(fd); fail(bedfile + " is not a PLINK .bed file (magic bytes 6c 1b 01 expected)"); }
    const unsigned long long want = 3ull + (unsigned long long)b->nrows * b->row_bytes;
    if ((unsigned long long)st.st_size != want) {
        close(fd);
        fail(bedfile + ((unsigned long long)st.st_size < want ? " is truncated: " : " is too long: ") + std::to_string((long long)st.st_size) + " bytes, " +
             std::to_string(b->nrows) + " loci x " + std::to_string(b->nind) + " individuals need " + std::to_string(want));
    }
    void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) fail("Failed to map " + bedfile);
    b->map = m;
    b->map_bytes = (size_t)st.st_size;
    b->rows = (const unsigned char *)m + 3;
    return b.release();
}

namespace {
// the slot of `device` in the file's image list, with its context
size_t bedSlotOn(BedFile *b, int device)
{
    for (size_t k = 0; k < b->images.size(); k++)
        if (b->images[k].device == device) return k;
    b->images.push_back({device, nullptr, nullptr});
    if (!b->parent) {      // (an extract lives on its parent's context)
        garlic_ctx *ctx = nullptr;
        check(garlic_ctx_create(device, nullptr, &ctx), "garlic_ctx_create");
        b->images.back().ctx = ctx;
    }
    return b->images.size() - 1;
}

// the image of the whole mapped file on `device` (made and filled chunk by chunk at the first request)
garlic_bed *bedFullImageOn(BedFile *b, int device)
{
    const size_t slot = bedSlotOn(b, device);
    if (b->images[slot].bed) return (garlic_bed *)b->images[slot].bed;
    garlic_bed *bed = nullptr;
    check(garlic_bed_create((garlic_ctx *)b->images[slot].ctx, b->nrows, b->nind, &bed), "garlic_bed_create");
    b->images[slot].bed = bed;
    // chunks of 64 MB through an ordinary buffer (not the read-only file mapping itself: what the runtime does to pin or stage
    // the source of a large copy is then no concern of the mapping)
    const long long chunk = std::max<long long>(1, ((long long)64 << 20) / (long long)b->row_bytes);
    std::vector<unsigned char> buf((size_t)std::min(chunk, b->nrows) * b->row_bytes);
    for (long long r = 0; r < b->nrows; r += chunk) {
        const long long n = std::min(chunk, b->nrows - r);
        memcpy(buf.data(), b->rows + (size_t)r * b->row_bytes, (size_t)n * b->row_bytes);
        check(garlic_bed_set_rows(bed, buf.data(), (int64_t)b->row_bytes, r, n, GARLIC_HOST), "garlic_bed_set_rows");
    }
    if (b->order)      // a VCF or TPED image: its order plane from the host's copy
        check(garlic_bed_set_order_rows(bed, b->order, (int64_t)b->order_row_bytes, 0, b->nrows, GARLIC_HOST), "garlic_bed_set_order_rows");
    if (b->own_census)  // a TPED image: the census its parse wrote on the first device (the image rule cannot recompute it)
        check(garlic_bed_set_census(bed, b->counts.data(), b->counted.data(), GARLIC_HOST), "garlic_bed_set_census");
    return bed;
}

// the image of the file set on `device`, censused at the first request: the whole file's, or -- for a subset -- the extract
// cut from the parent's image there (which then goes, unless the parent holds it for further populations)
garlic_bed *bedImageOn(BedFile *b, int device)
{
    garlic_bed *bed = nullptr;
    if (b->parent) {
        const size_t slot = bedSlotOn(b, device);
        if (!b->images[slot].bed) {
            garlic_bed *full = bedFullImageOn(b->parent, device);
            check(garlic_bed_extract(full, b->keep.data(), (int32_t)b->keep.size(), &bed), "garlic_bed_extract");
            b->images[slot].bed = bed;
            if (!b->parent->hold_images) {
                const size_t ps = bedSlotOn(b->parent, device);
                garlic_bed_destroy((garlic_bed *)b->parent->images[ps].bed);
                b->parent->images[ps].bed = nullptr;
            }
        }
        bed = (garlic_bed *)b->images[slot].bed;
        if (!b->rows) {      // the host's view of the genotypes (genotypeAt, the genotype cache): the subset's own rows
            b->own_rows.resize((size_t)b->nrows * b->row_bytes);
            check(garlic_bed_get_rows(bed, 0, b->nrows, b->own_rows.data(), (int64_t)b->row_bytes, GARLIC_HOST), "garlic_bed_get_rows");
            b->rows = b->own_rows.data();
        }
    } else {
        bed = bedFullImageOn(b, device);
    }
    if (b->counted.empty()) {
        b->counts.resize(2 * (size_t)b->nrows);
        b->counted.resize((size_t)b->nrows);
        check(garlic_bed_census(bed, b->counts.data(), b->counted.data(), GARLIC_HOST), "garlic_bed_census");
    }
    return bed;
}
} // namespace

// the triple of an open file set `b` (the caller's reference on it passes to the HapData, or is dropped on failure)
static void loadBedFile(BedFile *b, int &numLoci, int &numInd, std::vector<HapData *> **hapDataByChr,
                        std::vector<MapData *> **mapDataByChr, std::vector<FreqData *> **freqDataByChr, int nresample,
                        unsigned long long resampleSeed, int device)
{
    const BedFile *bim = b->bim();      // the .bim columns: the parent's for a subset
    *hapDataByChr = new std::vector<HapData *>;
    *mapDataByChr = new std::vector<MapData *>;
    *freqDataByChr = new std::vector<FreqData *>;
    try {
        bedImageOn(b, device);   // the census
        const unsigned long long seed0 = resampleSeed ? resampleSeed : (unsigned long long)time(nullptr);   // as loadTPEDData
        std::mt19937 resampler((uint32_t)(seed0 & 0xffffffffull) ? (uint32_t)(seed0 & 0xffffffffull) : 4357u);
        for (long long r0 = 0; r0 < b->nrows;) {
            long long r1 = r0;
            while (r1 < b->nrows && bim->chr[(size_t)r1] == bim->chr[(size_t)r0]) r1++;   // a new chromosome where the chr string changes
            const int n = (int)(r1 - r0);
            MapData *m = initMapData(n);
            (*mapDataByChr)->push_back(m);
            m->chr = checkChrName(bim->chr[(size_t)r0]);
            FreqData *f = initFreqData(n);
            (*freqDataByChr)->push_back(f);
            HapData *h = new HapData{nullptr, b->nind, n, nullptr, nullptr, nullptr, b, new long long[n]};
            b->refs++;
            (*hapDataByChr)->push_back(h);
            for (int l = 0; l < n; l++) {
                const size_t r = (size_t)(r0 + l);
                h->bedRow[l] = (long long)r;
                m->physicalPos[l] = (int)bim->ppos[r];
                m->geneticPos[l] = bim->gpos[r];
                m->locusName[l] = bim->name[r];
                // what loadTPEDData stores as oneAllele: the counted allele's character, the missing character for none
                m->allele[l] = b->counted[r] == 0 ? bim->a1[r] : b->counted[r] == 1 ? bim->a2[r] : b->none_allele;
                const int nalleles = b->counts[2 * r], total = b->counts[2 * r + 1];
                double freq = total == 0 ? 0.0 : double(nalleles) / double(total);   // garlic-data.cpp:141
                if (nresample > 0 && total != 0) {
                    int count = 0;
                    for (int i = 0; i < nresample; i++)
                        if ((double)resampler() / 4294967296.0 <= freq) count++;
                    freq = double(count) / double(nresample);
                }
                f->freq[l] = freq;
            }
            r0 = r1;
        }
    } catch (...) {
        releaseHapData(*hapDataByChr); releaseMapData(*mapDataByChr); releaseFreqData(*freqDataByChr);
        *hapDataByChr = nullptr; *mapDataByChr = nullptr; *freqDataByChr = nullptr;
        if (--b->refs == 0) closeBedFile(b);
        throw;
    }
    numLoci = (int)b->nrows;
    numInd = b->nind;
    b->refs--;                   // at least one HapData holds the file now
}

void loadBedData(const std::string &bedfile, const std::string &bimfile, const std::string &famfile, int &numLoci, int &numInd,
                 std::vector<HapData *> **hapDataByChr, std::vector<MapData *> **mapDataByChr,
                 std::vector<FreqData *> **freqDataByChr, int nresample, unsigned long long resampleSeed, int device)
{
    BedFile *b = openBedFile(bedfile, bimfile, famfile);
    b->refs = 1;                 // this function's, until the HapData hold theirs
    loadBedFile(b, numLoci, numInd, hapDataByChr, mapDataByChr, freqDataByChr, nresample, resampleSeed, device);
}

[[noreturn]] static void refuseVcfLine(const TglsFile *f, int64_t line, int col, const std::string &why)
{
    fail("line " + std::to_string(line) + " of " + f->path +
         (col >= 0 ? ", sample " + std::to_string(col + 1) + (col < (int)f->vcfSamples.size() ? " (" + f->vcfSamples[(size_t)col] + ")" : std::string()) : std::string()) +
         ": " + why);
}

// One slab of loadVcfData into obj: rows [row, row + n) from the lines lb (n + 1 offsets; ends: where each stops; number: its
// line in the file) of the text that stands on obj's device at d_text and in host memory at h_text.  A row the device defers
// is parsed by vcf::parseGlValues -- from h_text, or where that is NULL (the text stands on the devices only) from the line
// fetched through ctx; a refused line ends the run.  false: the 65,537th distinct raw value.
static bool vcfGlSlab(const TglsFile *f, garlic_ctx *ctx, garlic_tgls *obj, const void *d_text, const char *h_text, int64_t text_bytes,
                      const std::vector<int64_t> &lb, const std::vector<int64_t> &ends, const std::vector<int64_t> &number, long long row)
{
    const int64_t n = (int64_t)lb.size() - 1;
    const double *missing = f->vcfHasMissing ? &f->vcfMissing : nullptr;
    std::vector<int32_t> status((size_t)(2 * n), 0);
    int rc = garlic_tgls_set_rows_vcf(obj, (const char *)d_text, text_bytes, lb.data(), row, n, f->vcfKey.c_str(), missing, status.data(),
                                      GARLIC_DEVICE);
    if (rc == GARLIC_ERR_RANGE) return false;
    if (rc == GARLIC_ERR_INVALID)
        for (int64_t r = 0; r < n; r++) {
            const int code = status[(size_t)(2 * r)], col = status[(size_t)(2 * r + 1)];
            if (code == GARLIC_TGLS_VCF_NO_KEY) refuseVcfLine(f, number[(size_t)r], -1, "FORMAT does not name " + f->vcfKey);
            else if (code == GARLIC_TGLS_VCF_NO_VALUE)
                refuseVcfLine(f, number[(size_t)r], col, "a called genotype without " + f->vcfKey + " (--vcf-gl-missing X gives such genotypes the raw value X)");
            else if (code >= GARLIC_TGLS_FEW_COLUMNS)
                refuseVcfLine(f, number[(size_t)r], -1, code == GARLIC_TGLS_FEW_COLUMNS ? "too few sample columns" : "too many sample columns");
        }
    check(rc, "garlic_tgls_set_rows_vcf");
    std::vector<double> vals((size_t)f->fileInd);
    std::vector<char> fetched;
    std::string err;
    for (int64_t r = 0; r < n; r++) {
        if (status[(size_t)(2 * r)] != GARLIC_TGLS_DEFERRED) continue;
        int sample = -1;
        const size_t len = (size_t)(ends[(size_t)r] - lb[(size_t)r]);
        if (!h_text) {
            fetched.resize(len);
            check(garlic_device_download(ctx, fetched.data(), (const char *)d_text + lb[(size_t)r], (int64_t)len), "garlic_device_download");
        }
        if (!vcf::parseGlValues(h_text ? h_text + lb[(size_t)r] : fetched.data(), len, f->vcfKey, f->fileInd, nullptr, vals.size(), missing,
                                vals.data(), sample, err))
            refuseVcfLine(f, number[(size_t)r], sample, err);
        rc = garlic_tgls_set_rows_values(obj, vals.data(), (int64_t)vals.size(), row + r, 1, GARLIC_HOST);
        if (rc == GARLIC_ERR_RANGE) return false;
        check(rc, "garlic_tgls_set_rows_values");
    }
    return true;
}

// the empty image of a text file's rows on the loader's device, and -- when the parse has filled it -- the host's copies of
// its rows, fetched once: genotypeAt, the phase readers, the genotype cache, and the source of further devices' images
static garlic_bed *createParsedImage(BedFile *b, int device)
{
    const size_t slot = bedSlotOn(b, device);
    garlic_bed *bed = nullptr;
    check(garlic_bed_create((garlic_ctx *)b->images[slot].ctx, b->nrows, b->nind, &bed), "garlic_bed_create");
    b->images[slot].bed = bed;
    return bed;
}

static void fetchParsedRows(BedFile *b, garlic_bed *bed)
{
    b->own_rows.resize((size_t)b->nrows * b->row_bytes);
    b->own_order.resize((size_t)b->nrows * b->order_row_bytes);
    check(garlic_bed_get_rows(bed, 0, b->nrows, b->own_rows.data(), (int64_t)b->row_bytes, GARLIC_HOST), "garlic_bed_get_rows");
    check(garlic_bed_get_order_rows(bed, 0, b->nrows, b->own_order.data(), (int64_t)b->order_row_bytes, GARLIC_HOST), "garlic_bed_get_order_rows");
    b->rows = b->own_rows.data();
    b->order = b->own_order.data();
}

// text::forEachSlab for a loader that gives up on a file it cannot read; longLine: what it says about a line that fills a
// slab.  false: onSlab stopped the walk.
template <class OnSlab>
static bool slabsOrFail(const std::string &path, size_t slabBytes, const std::string &longLine, OnSlab onSlab)
{
    std::string error;
    const text::SlabsEnd end = text::forEachSlab(path, slabBytes, error, onSlab);
    if (end == text::SLABS_NO_FILE) fail(error);
    if (end == text::SLABS_READ_ERROR) fail(path + ": " + error);
    if (end == text::SLABS_LONG_LINE) fail(longLine);
    return end == text::SLABS_DONE;
}

// the loader's slab of text on the devices that parse it: one buffer per likelihood object, freed with the scope
struct VcfDeviceSlabs {
    struct One { garlic_ctx *ctx; garlic_tgls *obj; void *text; };
    std::vector<One> on;
    bool borrowed = false;         // the buffers are a bgzf::DeviceSlabs': named per slab, not freed here
    void release()
    {
        for (One &o : on)
            if (!borrowed) garlic_device_free(o.ctx, o.text);
        on.clear();
    }
    ~VcfDeviceSlabs() { release(); }
};

// One slab of either source, as the two walks of loadVcfData see it: the lines, and their text in host memory (host) or on the
// devices with the lines' heads on the host (dev).
struct VcfSlab {
    const std::vector<int64_t> &begin, &end, &number;
    int64_t have;
    const char *host;
    const bgzf::DeviceSlab *dev;
};

// loadVcfData through the host reader (onDevice false: any file) or through bgzf::DeviceSlabs (a BGZF file inflated on the
// devices).  false, on the device path alone: the file is no BGZF file throughout or holds a bad block; refusal says which,
// nothing has been handed out, and the host reader can take the file.
static bool loadVcfDataThrough(bool onDevice, const std::string &vcffile, bool phased, bool snpsOnly, std::vector<std::string> &samples,
                               int &numLoci, int &numInd, std::vector<HapData *> **hapDataByChr, std::vector<MapData *> **mapDataByChr,
                               std::vector<FreqData *> **freqDataByChr, int nresample, unsigned long long resampleSeed, int device,
                               VcfGlRequest *gl, std::string &refusal)
{
    std::unique_ptr<BedFile, void (*)(BedFile *)> b(new BedFile, closeBedFile);
    b->path = vcffile;
    b->phased = phased;
    size_t SLAB = (size_t)64 << 20;
    const int64_t HEAD = 512;              // bytes of every line that reach the host on the device path
    if (onDevice)
        if (const char *e = getenv("GARLIC_BGZF_SLAB_BYTES")) SLAB = (size_t)std::max<long long>(atoll(e), 65536);   // (tests: many slabs of a small file)
    int64_t blocksInflated = 0;
    // the walk over the file's slabs by either source; false: the device source refused the file
    auto slabsOf = [&](const std::vector<int> &devices, const std::string &longLine, auto onSlab) -> bool {
        if (!onDevice) {
            slabsOrFail(vcffile, SLAB, longLine, [&](const text::Reader &rd, const text::SlabLines &cut, size_t) {
                onSlab(VcfSlab{cut.begin, cut.end, cut.number, (int64_t)rd.have, rd.slab.data(), nullptr});
                return true;
            });
            return true;
        }
        bgzf::DeviceSlabs src;
        if (!src.open(devices, (int64_t)SLAB)) fail(vcffile + ": " + src.error);
        const bgzf::DeviceSlabsEnd end = src.forEach(vcffile, HEAD, [&](const bgzf::DeviceSlab &s) {
            onSlab(VcfSlab{s.begin, s.end, s.number, s.have, nullptr, &s});
            return true;
        });
        blocksInflated = src.blocks / (int64_t)devices.size();
        if (end == bgzf::DEV_NOT_BGZF || end == bgzf::DEV_BAD_BLOCK) { refusal = src.error; return false; }
        if (end == bgzf::DEV_LONG_LINE) fail(longLine);
        if (end != bgzf::DEV_DONE) fail(vcffile + ": " + src.error);
        return true;
    };
    // first pass: the header, the nine fixed columns of every data line, and which lines are kept -- the row count that
    // garlic_bed_create needs.  On the device path a line's head serves where it holds the nine columns; '#CHROM' and a line
    // whose ninth tab lies behind the head are fetched whole.
    std::vector<char> kept;                // per data line
    samples.clear();
    {
        std::string err;
        std::vector<char> fetched;
        const bool read = slabsOf({device}, vcffile + ": a line longer than 64 MB", [&](const VcfSlab &s) {
            for (size_t k = 0; k < s.begin.size(); k++) {
                const char *line = s.host ? s.host + s.begin[k] : s.dev->head(k);
                size_t len = s.host ? (size_t)(s.end[k] - s.begin[k]) : s.dev->headLen(k);
                const std::string where = "line " + std::to_string(s.number[k]) + " of " + vcffile + ": ";
                if (s.dev && !s.dev->whole(k)) {
                    size_t tabs = 0;
                    for (size_t i = 0; i < len && tabs < 9; i++) tabs += line[i] == '\t';
                    if (line[0] == '#' ? (len >= 6 && memcmp(line, "#CHROM", 6) == 0) : tabs < 9) {
                        if (!s.dev->fetch(k, fetched)) fail(where + garlic_hip_last_error());
                        line = fetched.data();
                        len = fetched.size();
                    }
                }
                if (line[0] == '#') {
                    if (len >= 6 && memcmp(line, "#CHROM", 6) == 0 && !vcf::parseHeader(line, len, samples, err)) fail(where + err);
                    continue;
                }
                if (samples.empty()) fail(where + "a data line before the #CHROM line");
                vcf::Site site;
                const vcf::LineKind kind = vcf::parseFixed(line, len, site, err);
                if (kind == vcf::LINE_BAD || (kind == vcf::LINE_NOT_SNP && !snpsOnly))
                    fail(where + err + (kind == vcf::LINE_NOT_SNP ? " (--vcf-biallelic-snps-only leaves such lines out)" : ""));
                kept.push_back(kind == vcf::LINE_SNP);
                if (kind != vcf::LINE_SNP) { b->skipped_non_snp++; continue; }
                b->chr.push_back(site.chr); b->name.push_back(site.name); b->gpos.push_back(0.0); b->ppos.push_back((double)site.ppos);
                b->a1.push_back(site.a1); b->a2.push_back(site.a2);
            }
        });
        if (!read) return false;
    }
    if (samples.empty()) fail("no #CHROM line in " + vcffile);
    b->nind = (int)samples.size();
    b->nrows = (long long)b->chr.size();
    if (b->nrows < 1) fail("no loci in " + vcffile);
    b->row_bytes = ((size_t)b->nind + 3) / 4;
    b->order_row_bytes = ((size_t)b->nind + 7) / 8;
    // second pass: the text to the device in slabs, one parse call per slab
    garlic_bed *bed = createParsedImage(b.get(), device);
    // the likelihoods from the same slabs: one object of every sample's column per distinct device, and a buffer there that
    // the slab is uploaded to once (on the device path: the source's own buffer, where the slab was inflated); on the loader's
    // own device the genotype parse reads that buffer too
    std::unique_ptr<TglsFile, void (*)(TglsFile *)> glFile(nullptr, closeTglsFile);
    VcfDeviceSlabs slabs;          // (behind glFile: its buffers go before the contexts they came from)
    slabs.borrowed = onDevice;
    std::vector<int> devs{device};
    if (gl) {
        gl->file = nullptr;
        gl->overflow = false;
        if (gl->glType != "GQ" && gl->glType != "GL" && gl->glType != "PL") fail("Must choose GQ/GL/PL for genotype likelihood format");
        glFile.reset(new TglsFile);
        glFile->path = vcffile;
        glFile->glType = gl->glType == "GQ" ? GARLIC_GL_GQ : gl->glType == "GL" ? GARLIC_GL_GL : GARLIC_GL_PL;
        glFile->fileInd = b->nind;
        for (int i = 0; i < b->nind; i++) glFile->cols.push_back(i);
        glFile->nrows = b->nrows;
        glFile->vcfKey = gl->key;
        glFile->vcfHasMissing = gl->hasMissing;
        glFile->vcfMissing = gl->missing;
        glFile->vcfSnpsOnly = snpsOnly;
        glFile->vcfSamples = samples;
        for (int d : gl->devices)
            if (std::find(devs.begin(), devs.end(), d) == devs.end()) devs.push_back(d);
        for (int d : devs) {
            glFile->objects.push_back({d, 0, b->nind, nullptr, nullptr});
            garlic_ctx *ctx = nullptr;
            check(garlic_ctx_create(d, nullptr, &ctx), "garlic_ctx_create");
            glFile->objects.back().ctx = ctx;
            garlic_tgls *obj = nullptr;
            check(garlic_tgls_create(ctx, b->nrows, b->nind, glFile->cols.data(), b->nind, &obj), "garlic_tgls_create");
            glFile->objects.back().tgls = obj;
            void *text = nullptr;
            if (!onDevice) check(garlic_device_alloc(ctx, (int64_t)SLAB + 16, &text), "garlic_device_alloc");      // (the last piece lies inside)
            slabs.on.push_back({ctx, obj, text});
        }
    }
    {
        size_t data_line = 0;
        long long row = 0;
        std::vector<int64_t> lb, number, ends;
        std::vector<int32_t> status;
        // (a line longer than the slab: the first pass met none)
        const bool read = slabsOf(devs, vcffile + " changed while it was read", [&](const VcfSlab &s) {
            lb.clear();
            number.clear();
            ends.clear();
            int64_t last_end = 0;
            for (size_t k = 0; k < s.begin.size(); k++) {
                if ((s.host ? s.host[(size_t)s.begin[k]] : s.dev->head(k)[0]) == '#') continue;
                if (data_line >= kept.size()) fail(vcffile + " changed while it was read");
                if (!kept[data_line++]) continue;
                lb.push_back(s.begin[k]);
                number.push_back(s.number[k]);
                ends.push_back(s.end[k]);
                last_end = s.end[k];
            }
            if (lb.empty()) return;
            const int64_t n = (int64_t)lb.size();
            if (row + n > b->nrows) fail(vcffile + " changed while it was read");
            lb.push_back(last_end);
            status.assign((size_t)(2 * n), 0);
            // one upload per device; the first buffer stands on the image's device and serves both parses
            for (size_t k = 0; k < slabs.on.size(); k++) {
                if (s.dev) slabs.on[k].text = s.dev->text[k];
                else check(garlic_device_upload(slabs.on[k].ctx, slabs.on[k].text, s.host, s.have), "garlic_device_upload");
            }
            const int rc = s.dev ? garlic_bed_set_rows_vcf(bed, s.dev->text[0], s.have, lb.data(), row, n, status.data(), GARLIC_DEVICE)
                           : slabs.on.empty()
                               ? garlic_bed_set_rows_vcf(bed, s.host, s.have, lb.data(), row, n, status.data(), GARLIC_HOST)
                               : garlic_bed_set_rows_vcf(bed, (const char *)slabs.on[0].text, s.have, lb.data(), row, n, status.data(),
                                                         GARLIC_DEVICE);
            if (rc == GARLIC_ERR_INVALID) {
                for (int64_t r = 0; r < n; r++)
                    if (status[(size_t)(2 * r)]) {
                        const int col = status[(size_t)(2 * r + 1)];
                        fail("line " + std::to_string(number[(size_t)r]) + " of " + vcffile + ", sample " + std::to_string(col + 1) +
                             (col < b->nind ? " (" + samples[(size_t)col] + ")" : std::string()) + ": " + garlic_hip_last_error());
                    }
            }
            check(rc, "garlic_bed_set_rows_vcf");
            for (size_t k = 0; k < slabs.on.size(); k++)
                if (!vcfGlSlab(glFile.get(), slabs.on[k].ctx, slabs.on[k].obj, slabs.on[k].text, s.host, s.have, lb, ends, number, row)) {
                    // the 65,537th distinct raw value: the objects are of no use; the genotypes go on from the same text
                    slabs.release();
                    glFile.reset();
                    gl->overflow = true;
                    break;
                }
            row += n;
        });
        if (!read) return false;
        if (row != b->nrows) fail(vcffile + " changed while it was read");
    }
    slabs.release();
    if (gl && !gl->overflow) gl->file = glFile.release();
    if (onDevice) fprintf(stderr, "%s: BGZF, %lld blocks inflated on the device\n", vcffile.c_str(), (long long)blocksInflated);
    b->refs = 1;
    fetchParsedRows(b.get(), bed);
    loadBedFile(b.release(), numLoci, numInd, hapDataByChr, mapDataByChr, freqDataByChr, nresample, resampleSeed, device);
    return true;
}

// A BGZF file is inflated and cut into lines on the devices when GARLIC_BGZF_DEVICE_INFLATE=1 asks for it (opt-in: the load
// phase has not been timed against the host reader); GARLIC_BGZF_HOST_INFLATE=1 keeps the host reader whatever else is set.
// A file that stops being BGZF part-way or holds a block with a bad status is read again by the host reader, with one note.
void loadVcfData(const std::string &vcffile, bool phased, bool snpsOnly, std::vector<std::string> &samples, int &numLoci, int &numInd,
                 std::vector<HapData *> **hapDataByChr, std::vector<MapData *> **mapDataByChr, std::vector<FreqData *> **freqDataByChr,
                 int nresample, unsigned long long resampleSeed, int device, VcfGlRequest *gl)
{
    auto set = [](const char *name) { const char *e = getenv(name); return e && *e && strcmp(e, "0") != 0; };
    std::string refusal;
    if (set("GARLIC_BGZF_DEVICE_INFLATE") && !set("GARLIC_BGZF_HOST_INFLATE") && bgzf::isBgzf(vcffile)) {
        if (loadVcfDataThrough(true, vcffile, phased, snpsOnly, samples, numLoci, numInd, hapDataByChr, mapDataByChr, freqDataByChr, nresample,
                               resampleSeed, device, gl, refusal))
            return;
        fprintf(stderr, "%s: %s; the file is read again by the host reader\n", vcffile.c_str(), refusal.c_str());
    }
    loadVcfDataThrough(false, vcffile, phased, snpsOnly, samples, numLoci, numInd, hapDataByChr, mapDataByChr, freqDataByChr, nresample,
                       resampleSeed, device, gl, refusal);
}

bool loadTPEDDataOnDevice(const std::string &tpedfile, int &numLoci, int &numInd, std::vector<HapData *> **hapDataByChr,
                          std::vector<MapData *> **mapDataByChr, std::vector<FreqData *> **freqDataByChr, char TPED_MISSING, bool PHASED,
                          int nresample, unsigned long long resampleSeed, int device, std::string &refusal)
{
    refusal.clear();
    if (TPED_MISSING == ' ' || TPED_MISSING == '\t' || TPED_MISSING == '\r' || TPED_MISSING == '\n') {
        refusal = tpedfile + ": the missing character is a blank";
        return false;
    }
    std::unique_ptr<BedFile, void (*)(BedFile *)> b(new BedFile, closeBedFile);
    b->path = tpedfile;
    b->phased = PHASED;
    b->own_census = true;
    b->none_allele = TPED_MISSING;
    const size_t SLAB = (size_t)64 << 20;
    // first pass: the four leading tokens of every line and the number of individuals -- what garlic_bed_create needs
    {
        std::string error;
        const text::SlabsEnd end = text::forEachSlab(tpedfile, SLAB, error, [&](const text::Reader &rd, const text::SlabLines &cut, size_t) {
            for (size_t k = 0; k < cut.begin.size(); k++) {
                const char *line = rd.slab.data() + cut.begin[k];
                const size_t len = (size_t)(cut.end[k] - cut.begin[k]);
                if (b->chr.empty()) {
                    b->nind = tped::individualsOf(line, len);
                    if (b->nind < 1) {
                        refusal = "line " + std::to_string(cut.number[k]) + " of " + tpedfile + ": no genotype columns";
                        return false;
                    }
                }
                tped::Lead lead;
                tped::parseLead(line, len, lead);
                b->chr.push_back(lead.chr); b->name.push_back(lead.name); b->gpos.push_back(lead.gpos); b->ppos.push_back(lead.ppos);
            }
            return true;
        });
        if (end == text::SLABS_NO_FILE) refusal = error;      // (the host reader says what it says about that)
        if (end == text::SLABS_NO_FILE || end == text::SLABS_STOPPED) return false;
        if (end == text::SLABS_READ_ERROR) fail(tpedfile + ": " + error);
        if (end == text::SLABS_LONG_LINE) fail(tpedfile + ": a line longer than 64 MB");
    }
    b->nrows = (long long)b->chr.size();
    if (b->nrows < 1) fail("no loci in " + tpedfile);
    b->row_bytes = ((size_t)b->nind + 3) / 4;
    b->order_row_bytes = ((size_t)b->nind + 7) / 8;
    b->a1.assign((size_t)b->nrows, TPED_MISSING);
    b->a2.assign((size_t)b->nrows, TPED_MISSING);
    // second pass: the text to the device in slabs, one parse call per slab
    garlic_bed *bed = createParsedImage(b.get(), device);
    {
        long long row = 0;
        std::vector<int64_t> lb;
        std::vector<int32_t> status;
        // (a line longer than the slab: the first pass met none)
        const bool read = slabsOrFail(tpedfile, SLAB, tpedfile + " changed while it was read", [&](const text::Reader &rd, const text::SlabLines &cut, size_t) {
            if (cut.begin.empty()) return true;
            const int64_t n = (int64_t)cut.begin.size();
            if (row + n > b->nrows) fail(tpedfile + " changed while it was read");
            lb.assign(cut.begin.begin(), cut.begin.end());
            lb.push_back(cut.end.back());
            status.assign((size_t)(2 * n), 0);
            const int rc = garlic_bed_set_rows_tped(bed, rd.slab.data(), (int64_t)rd.have, lb.data(), row, n, (uint8_t)TPED_MISSING,
                                                    (uint8_t *)b->a1.data() + row, status.data(), GARLIC_HOST);
            if (rc == GARLIC_ERR_INVALID) {
                for (int64_t r = 0; r < n; r++)
                    if (status[(size_t)(2 * r)]) {
                        refusal = "line " + std::to_string(cut.number[(size_t)r]) + " of " + tpedfile + " is refused by the device reader (code " +
                                  std::to_string(status[(size_t)(2 * r)]) + ": " + garlic_hip_last_error() + ")";
                        return false;
                    }
            }
            check(rc, "garlic_bed_set_rows_tped");
            row += n;
            return true;
        });
        if (!read) return false;       // (refusal says why)
        if (row != b->nrows) fail(tpedfile + " changed while it was read");
    }
    b->refs = 1;
    fetchParsedRows(b.get(), bed);
    loadBedFile(b.release(), numLoci, numInd, hapDataByChr, mapDataByChr, freqDataByChr, nresample, resampleSeed, device);
    return true;
}

void loadBedSubset(BedFile *full, const std::vector<int> &keep, int &numLoci, int &numInd, std::vector<HapData *> **hapDataByChr,
                   std::vector<MapData *> **mapDataByChr, std::vector<FreqData *> **freqDataByChr, int nresample,
                   unsigned long long resampleSeed, int device)
{
    if (keep.empty()) fail("no individuals kept of " + full->path);
    for (size_t i = 0; i < keep.size(); i++)
        if (keep[i] < 0 || keep[i] >= full->nind || (i && keep[i] <= keep[i - 1]))
            fail("kept individuals must be ascending indices into the .fam of " + full->path);
    BedFile *b = new BedFile;
    b->path = full->path;
    b->parent = full;
    full->refs++;
    b->keep = keep;
    b->nind = (int)keep.size();
    b->nrows = full->nrows;
    b->row_bytes = ((size_t)b->nind + 3) / 4;
    b->refs = 1;
    loadBedFile(b, numLoci, numInd, hapDataByChr, mapDataByChr, freqDataByChr, nresample, resampleSeed, device);
}

void scanIndData3(const std::string &filename, int &numInd, std::string &popName)
{
    LineReader in(filename);
    std::map<std::string, int> seen;
    std::string line, pop, ind;
    int n = 0;
    while (in.next(line)) {
        n++;
        if (countFields(line) < 2) fail("line " + std::to_string(n) + " of " + filename + " has fewer than 2 columns");
        std::stringstream ss(line);
        ss >> pop >> ind;
        if (seen.count(ind)) fail("Found duplicate individual ID (" + ind + ") in " + filename);
        seen[ind] = 1;
        if (n == 1) popName = pop;
        else if (pop != popName) fail("Found multiple population IDs (" + pop + ", " + popName + ") in " + filename);
    }
    numInd = n;
}

IndData *indDataOfKept(const std::vector<FamEntry> &fam, const std::vector<int> &keep, const std::string &famfile)
{
    if (keep.empty()) fail("Number of individuals must be positive");
    std::map<std::string, int> seen;
    const std::string pop = fam[(size_t)keep[0]].fid;
    for (int i : keep) {
        const FamEntry &e = fam[(size_t)i];
        if (seen.count(e.iid)) fail("Found duplicate individual ID (" + e.iid + ") in " + famfile);
        seen[e.iid] = 1;
        if (e.fid != pop) fail("Found multiple population IDs (" + e.fid + ", " + pop + ") in " + famfile + " among the kept individuals");
    }
    IndData *d = new IndData;
    d->nind = (int)keep.size();
    d->indID = new std::string[keep.size()];
    for (size_t k = 0; k < keep.size(); k++) d->indID[k] = fam[(size_t)keep[k]].iid;
    d->pop = pop;
    return d;
}

IndData *readIndData3(const std::string &filename, int numInd)
{
    if (numInd < 1) fail("Number of individuals must be positive");
    LineReader in(filename);
    IndData *d = new IndData;
    d->nind = numInd;
    d->indID = new std::string[numInd];
    std::string line, pop, ind;
    for (int i = 0; i < numInd && in.next(line); i++) {
        std::stringstream ss(line);
        ss >> pop >> ind;
        d->indID[i] = ind;
    }
    d->pop = pop;
    return d;
}

// readTGLSData behind the text: nextRow(vals) brings the next locus' raw values, one per kept individual; the conversion and
// the forms (compact: codes that widen at the 257th and the 65,537th value) are what every host reader of likelihoods shares
static std::vector<GenoLikeData *> *readGLRows(int expectedInd, std::vector<MapData *> *maps, const std::string &GL_TYPE, bool compact,
                                               const std::function<void(double *)> &nextRow)
{
    if (GL_TYPE != "GQ" && GL_TYPE != "GL" && GL_TYPE != "PL") fail("Must choose GQ/GL/PL for genotype likelihood format");
    auto *out = new std::vector<GenoLikeData *>;
    std::vector<double> vals((size_t)expectedInd);
    for (auto m : *maps) {
        GenoLikeData *d;
        // compact: one byte per genotype and a table of the distinct converted values, in the order they are first seen;
        // at the 257th value the rows read so far widen to two bytes, at the 65,537th to the doubles themselves
        int width = compact ? 1 : 8;
        std::unordered_map<uint64_t, int> code_of;   // bit pattern of a value -> its code
        if (compact) {
            d = new GenoLikeData{nullptr, expectedInd, m->nloci, new unsigned char *[m->nloci](), new double[256], 0, nullptr};
            code_of.reserve(512);
        } else {
            d = initGLData(expectedInd, m->nloci);
        }
        out->push_back(d);
        for (int l = 0; l < m->nloci; l++) {
            nextRow(vals.data());
            if (compact && width == 1) d->codes[l] = new unsigned char[expectedInd];
            else if (compact && width == 2) d->codes16[l] = new unsigned short[expectedInd];
            else if (compact) d->data[l] = new double[expectedInd];
            uint64_t last_bits = 0;
            int last_code = -1;
            for (int i = 0; i < expectedInd; i++) {
                double gl = vals[(size_t)i];
                // garlic-data.cpp:1557-1576, operation for operation
                if (GL_TYPE == "GQ") { gl /= (-10.0); gl = (gl > -10) ? gl : -10; gl = pow(10, gl); }
                else if (GL_TYPE == "GL") { gl = (gl > -10) ? gl : -10; gl = 1 - pow(10, gl); }
                else { gl /= (-10.0); gl = (gl > -10) ? gl : -10; gl = 1 - pow(10, gl); }
                if (gl <= 0) gl = 0.0000000000000001;
                if (gl > 1) gl = 1;
                if (width == 8) { d->data[l][i] = gl; continue; }
                uint64_t bits;
                memcpy(&bits, &gl, sizeof bits);
                int code;
                if (last_code >= 0 && bits == last_bits) {
                    code = last_code;
                } else {
                    auto hit = code_of.find(bits);
                    code = hit == code_of.end() ? -1 : hit->second;
                }
                if (code < 0 && d->nvalues == 256 && width == 1) {          // rows 0 .. l (this one up to i) widen to 16 bits
                    d->codes16 = new unsigned short *[m->nloci]();
                    for (int r = 0; r <= l; r++) {
                        d->codes16[r] = new unsigned short[expectedInd];
                        const int n = r < l ? expectedInd : i;
                        for (int k = 0; k < n; k++) d->codes16[r][k] = d->codes[r][k];
                        delete[] d->codes[r];
                    }
                    delete[] d->codes;
                    d->codes = nullptr;
                    double *wider = new double[65536];
                    memcpy(wider, d->values, 256 * sizeof(double));
                    delete[] d->values;
                    d->values = wider;
                    code_of.reserve(1 << 17);
                    width = 2;
                }
                if (code < 0 && d->nvalues == 65536) {                      // ... and past 65,536 values to the doubles
                    d->data = new double *[m->nloci]();
                    for (int r = 0; r <= l; r++) {
                        d->data[r] = new double[expectedInd];
                        const int n = r < l ? expectedInd : i;
                        for (int k = 0; k < n; k++) d->data[r][k] = d->values[d->codes16[r][k]];
                        delete[] d->codes16[r];
                    }
                    delete[] d->codes16;
                    d->codes16 = nullptr;
                    delete[] d->values;
                    d->values = nullptr;
                    d->nvalues = 0;
                    code_of.clear();
                    width = 8;
                    d->data[l][i] = gl;
                    continue;
                }
                if (code < 0) {
                    code = d->nvalues;
                    code_of.emplace(bits, code);
                    d->values[d->nvalues++] = gl;
                }
                last_bits = bits;
                last_code = code;
                if (width == 1) d->codes[l][i] = (unsigned char)code;
                else d->codes16[l][i] = (unsigned short)code;
            }
        }
    }
    return out;
}

std::vector<GenoLikeData *> *readTGLSData(const std::string &filename, int /*expectedLoci*/, int expectedInd,
                                          std::vector<MapData *> *maps, const std::string &GL_TYPE, bool compact,
                                          const std::vector<int> *cols, int fileInd)
{
    if (cols && (int)cols->size() != expectedInd) fail("readTGLSData: one column per kept individual is needed");
    std::vector<double> raw(cols ? (size_t)fileInd : 0);
    LineReader in(filename);
    std::string line, junk;
    return readGLRows(expectedInd, maps, GL_TYPE, compact, [&](double *vals) {
        if (!in.next(line)) fail("too few lines in " + filename);
        const int num = countFields(line);
        if (num != (cols ? fileInd : expectedInd) + 4) fail("Incorrect number of columns in tgls file: " + std::to_string(num));
        std::stringstream ss(line);
        ss >> junk >> junk >> junk >> junk;
        for (double &v : raw) ss >> v;      // --keep: the whole line, then the kept columns
        for (int i = 0; i < expectedInd; i++) {
            if (cols) vals[i] = raw[(size_t)(*cols)[(size_t)i]];
            else ss >> vals[i];
        }
    });
}

// ---- the same file through the device (garlic_tgls): slabs of text up, rows of codes there, nothing per genotype here
// The file's first f->nrows lines into obj, whose kept columns are objCols: 64 MB slabs cut at line ends, one
// garlic_tgls_set_rows_text per slab; a row the device defers is parsed here as readTGLSData parses it and handed over through
// garlic_tgls_set_rows_values.  false: the 65,537th distinct raw value.
static bool fillTglsObject(const TglsFile *f, garlic_tgls *obj, const std::vector<int> &objCols)
{
    if (!f->vcfKey.empty()) fail(f->path + ": no likelihood object on this device (loadVcfData fills one per device it is told of)");
    std::vector<int64_t> lb;
    std::vector<int32_t> status;
    std::vector<double> raw((size_t)f->fileInd), vals(objCols.size());
    std::string junk;
    long long done = 0;
    bool overflow = false;
    slabsOrFail(f->path, (size_t)64 << 20, "a line of " + f->path + " is longer than a slab",
                [&](const text::Reader &rd, const text::SlabLines &cut, size_t consumed) {
        const long long n = std::min<long long>((long long)cut.begin.size(), f->nrows - done);
        if (n > 0) {
            lb.assign(cut.begin.begin(), cut.begin.begin() + n);
            lb.push_back((size_t)n < cut.begin.size() ? cut.begin[(size_t)n] : (int64_t)consumed);
            status.assign((size_t)(2 * n), 0);
            int rc = garlic_tgls_set_rows_text(obj, rd.slab.data(), (int64_t)consumed, lb.data(), done, n, status.data(), GARLIC_HOST);
            if (rc == GARLIC_ERR_RANGE) { overflow = true; return false; }
            auto lineOf = [&](long long r) { return std::string(rd.slab.data() + cut.begin[(size_t)r], (size_t)(cut.end[(size_t)r] - cut.begin[(size_t)r])); };
            for (long long r = 0; r < n; r++)
                if (status[(size_t)(2 * r)] >= GARLIC_TGLS_FEW_COLUMNS)
                    fail("Incorrect number of columns in tgls file: " + std::to_string(countFields(lineOf(r))));
            check(rc, "garlic_tgls_set_rows_text");
            for (long long r = 0; r < n; r++) {
                if (status[(size_t)(2 * r)] != GARLIC_TGLS_DEFERRED) continue;
                const std::string line = lineOf(r);
                const int num = countFields(line);
                if (num != f->fileInd + 4) fail("Incorrect number of columns in tgls file: " + std::to_string(num));
                std::stringstream ss(line);
                ss >> junk >> junk >> junk >> junk;
                for (double &v : raw) ss >> v;
                for (size_t k = 0; k < objCols.size(); k++) vals[k] = raw[(size_t)objCols[k]];
                rc = garlic_tgls_set_rows_values(obj, vals.data(), (int64_t)vals.size(), done + r, 1, GARLIC_HOST);
                if (rc == GARLIC_ERR_RANGE) { overflow = true; return false; }
                check(rc, "garlic_tgls_set_rows_values");
            }
            done += n;
        }
        return done < f->nrows;
    });
    if (overflow) return false;
    if (done < f->nrows) fail("too few lines in " + f->path);
    return true;
}

// the object that serves individuals [ind_begin, +nind) on `device`, and where its columns begin in it
static garlic_tgls *tglsObjectOn(TglsFile *f, int device, int ind_begin, int nind, int64_t &ind_offset)
{
    for (auto &o : f->objects)
        if (o.device == device && o.ind_begin <= ind_begin && ind_begin + nind <= o.ind_begin + o.nind) {
            ind_offset = ind_begin - o.ind_begin;
            return (garlic_tgls *)o.tgls;
        }
    f->objects.push_back({device, ind_begin, nind, nullptr, nullptr});
    TglsFile::Object &o = f->objects.back();
    garlic_ctx *ctx = nullptr;
    check(garlic_ctx_create(device, nullptr, &ctx), "garlic_ctx_create");
    o.ctx = ctx;
    const std::vector<int> objCols(f->cols.begin() + ind_begin, f->cols.begin() + ind_begin + nind);
    garlic_tgls *obj = nullptr;
    check(garlic_tgls_create(ctx, f->nrows, f->fileInd, objCols.data(), nind, &obj), "garlic_tgls_create");
    o.tgls = obj;
    if (!fillTglsObject(f, obj, objCols)) fail(f->path + " holds more than 65,536 distinct raw values on a second reading");
    ind_offset = 0;
    return obj;
}

// one GenoLikeData per chromosome that points into f, whose first object is filled; f is theirs from here on
static std::vector<GenoLikeData *> *glDataOfTglsFile(std::unique_ptr<TglsFile, void (*)(TglsFile *)> &f, int expectedInd,
                                                     std::vector<MapData *> *maps)
{
    garlic_tgls *obj = (garlic_tgls *)f->objects.front().tgls;
    auto *out = new std::vector<GenoLikeData *>;
    long long row = 0;
    try {
        for (auto m : *maps) {
            int32_t nvalues = 0;
            check(garlic_tgls_count_values(obj, f->glType, row, m->nloci, &nvalues), "garlic_tgls_count_values");
            GenoLikeData *d = new GenoLikeData{nullptr, expectedInd, m->nloci, nullptr, nullptr, nvalues, nullptr, f.get(), new long long[m->nloci]};
            f->refs++;
            out->push_back(d);
            for (int l = 0; l < m->nloci; l++) d->tglsRow[l] = row++;
        }
    } catch (...) {
        for (auto d : *out) { delete[] d->tglsRow; delete d; }
        delete out;
        throw;
    }
    f.release();
    return out;
}

// f filled on `device` and one GenoLikeData per chromosome that points into it; NULL (f closed): a 65,537th distinct raw value
static std::vector<GenoLikeData *> *tglsFileOnDevice(std::unique_ptr<TglsFile, void (*)(TglsFile *)> &f, int expectedInd,
                                                     std::vector<MapData *> *maps, int device)
{
    for (auto m : *maps) f->nrows += m->nloci;
    f->objects.push_back({device, 0, expectedInd, nullptr, nullptr});
    garlic_ctx *ctx = nullptr;
    check(garlic_ctx_create(device, nullptr, &ctx), "garlic_ctx_create");
    f->objects.back().ctx = ctx;
    garlic_tgls *obj = nullptr;
    check(garlic_tgls_create(ctx, f->nrows, f->fileInd, f->cols.data(), expectedInd, &obj), "garlic_tgls_create");
    f->objects.back().tgls = obj;
    if (!fillTglsObject(f.get(), obj, f->cols)) return nullptr;
    return glDataOfTglsFile(f, expectedInd, maps);
}

std::vector<GenoLikeData *> *loadTGLSFile(const std::string &filename, int expectedInd, std::vector<MapData *> *maps,
                                          const std::string &GL_TYPE, const std::vector<int> *cols, int fileInd, int device)
{
    if (cols && (int)cols->size() != expectedInd) fail("loadTGLSFile: one column per kept individual is needed");
    if (GL_TYPE != "GQ" && GL_TYPE != "GL" && GL_TYPE != "PL") fail("Must choose GQ/GL/PL for genotype likelihood format");
    std::unique_ptr<TglsFile, void (*)(TglsFile *)> f(new TglsFile, closeTglsFile);
    f->path = filename;
    f->glType = GL_TYPE == "GQ" ? GARLIC_GL_GQ : GL_TYPE == "GL" ? GARLIC_GL_GL : GARLIC_GL_PL;
    f->fileInd = cols ? fileInd : expectedInd;
    if (cols) f->cols = *cols;
    else for (int i = 0; i < expectedInd; i++) f->cols.push_back(i);
    for (int c : f->cols)
        if (c < 0 || c >= f->fileInd) fail("loadTGLSFile: a kept column outside the file's columns");
    auto *out = tglsFileOnDevice(f, expectedInd, maps, device);
    if (!out) std::cerr << filename << " holds more than 65,536 distinct values: read by the host reader instead\n";
    return out;
}

// The likelihoods loadVcfData left in `gl`: the GenoLikeData of its device objects, or -- a field of more than 65,536 distinct
// raw values -- the file read once more on the host, line by line through vcf::parseGlValues, into readTGLSData's compact forms
std::vector<GenoLikeData *> *vcfGlData(VcfGlRequest &gl, const std::string &vcffile, bool snpsOnly, const std::vector<std::string> &samples,
                                       std::vector<MapData *> *maps)
{
    const int nind = (int)samples.size();
    if (!gl.overflow) {
        if (!gl.file) fail("vcfGlData: loadVcfData has not run with this request");
        std::unique_ptr<TglsFile, void (*)(TglsFile *)> f(gl.file, closeTglsFile);
        gl.file = nullptr;
        long long rows = 0;
        for (auto m : *maps) rows += m->nloci;
        if (rows != f->nrows) fail("vcfGlData: the maps do not hold the loci that were read");
        return glDataOfTglsFile(f, nind, maps);
    }
    std::cerr << vcffile << ": " << gl.key << " holds more than 65,536 distinct values: read by the host reader instead\n";
    TglsFile names;
    names.path = vcffile;
    names.vcfSamples = samples;
    text::LineCursor in;
    if (!in.rd.open(vcffile, (size_t)64 << 20)) fail(in.rd.error);
    const text::SlabLines &cut = in.lines;
    std::string err;
    const double *missing = gl.hasMissing ? &gl.missing : nullptr;
    return readGLRows(nind, maps, gl.glType, /*compact=*/true, [&](double *vals) {
        for (;;) {
            size_t k = 0;
            if (!in.next(k))
                fail(in.why == text::SLABS_DONE ? vcffile + " changed while it was read"
                     : in.why == text::SLABS_READ_ERROR ? vcffile + ": " + in.rd.error : vcffile + ": a line longer than 64 MB");
            const char *line = in.rd.slab.data() + cut.begin[k];
            const size_t len = (size_t)(cut.end[k] - cut.begin[k]);
            if (line[0] == '#') continue;
            vcf::Site site;
            const vcf::LineKind kind = vcf::parseFixed(line, len, site, err);
            if (kind == vcf::LINE_BAD || (kind == vcf::LINE_NOT_SNP && !snpsOnly)) refuseVcfLine(&names, cut.number[k], -1, err);
            if (kind != vcf::LINE_SNP) continue;
            int sample = -1;
            if (!vcf::parseGlValues(line, len, gl.key, nind, nullptr, (size_t)nind, missing, vals, sample, err))
                refuseVcfLine(&names, cut.number[k], sample, err);
            return;
        }
    });
}

std::vector<FreqData *> *readFreqData(const std::string &freqfile, std::vector<MapData *> *maps)
{
    LineReader in(freqfile);
    auto *out = new std::vector<FreqData *>;
    std::string line, chrom, id;
    in.next(line); // header
    int lineNum = 1;
    for (auto m : *maps) {
        FreqData *f = initFreqData(m->nloci);
        out->push_back(f);
        for (int l = 0; l < m->nloci; l++) {
            lineNum++;
            if (!in.next(line)) fail("at line " + std::to_string(lineNum) + " in " + freqfile + ". Perhaps too few lines?");
            if (countFields(line) < 5) fail("fewer than 5 columns in " + freqfile + " on line " + std::to_string(lineNum));
            std::stringstream ss(line);
            double pos;
            char al;
            ss >> chrom >> id >> pos >> al >> f->freq[l];
            if (m->locusName[l] != id) fail("Loci appear mismatched in: " + freqfile + " at line " + std::to_string(lineNum));
            if (m->allele[l] != al) f->freq[l] = 1 - f->freq[l]; // other allele counted (garlic-data.cpp:1422-1424)
        }
    }
    return out;
}

static std::string gzip_member(const std::string &text);

// The reference's table (garlic-data.cpp:790-826; default ostream formatting = 6 significant digits = %g), lines
// formatted and compressed on all host cores, 100k lines per gzip member, appended in order.
void writeFreqData(const std::string &freqOutfile, std::vector<FreqData *> *freqs, std::vector<MapData *> *maps)
{
    const std::string path = freqOutfile + ".gz";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) fail("Failed to open " + path);
    struct Chunk { size_t c; int l0, l1; };
    std::vector<Chunk> chunks;
    for (size_t c = 0; c < maps->size(); c++)
        for (int l0 = 0; l0 < maps->at(c)->nloci; l0 += 100000)
            chunks.push_back(Chunk{c, l0, std::min(maps->at(c)->nloci, l0 + 100000)});
    const unsigned nthreads = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    std::atomic<bool> failed{false};   // set by the compression threads
    {
        const std::string m = gzip_member("CHR\tSNP\tPOS\tALLELE\tFREQ\n");
        failed = fwrite(m.data(), 1, m.size(), f) != m.size();
    }
    for (size_t k0 = 0; k0 < chunks.size() && !failed; k0 += nthreads) {
        const size_t n = std::min<size_t>(nthreads, chunks.size() - k0);
        std::vector<std::string> members(n);
        std::vector<std::thread> pool;
        for (size_t t = 0; t < n; t++)
            pool.emplace_back([&, t]() {
                const Chunk ch = chunks[k0 + t];
                const MapData *m = maps->at(ch.c);
                const double *fr = freqs->at(ch.c)->freq;
                std::string text;
                text.reserve((size_t)(ch.l1 - ch.l0) * 48);
                char num[64];
                for (int l = ch.l0; l < ch.l1; l++) {
                    text += m->chr; text += '\t';
                    text += m->locusName[l]; text += '\t';
                    text.append(num, (size_t)snprintf(num, sizeof num, "%d\t%c\t%g\n", m->physicalPos[l], m->allele[l], fr[l]));
                }
                try { members[t] = gzip_member(text); } catch (...) { failed = true; }
            });
        for (auto &th : pool) th.join();
        for (const std::string &m : members)
            if (!failed && fwrite(m.data(), 1, m.size(), f) != m.size()) failed = true;
    }
    fclose(f);
    if (failed) fail("Failed to write " + path);
}

namespace {
// keeps the SNPs with keep[l] != 0 in map / hap / freq / GL together
void filterSites(size_t c, const std::vector<char> &keep, std::vector<MapData *> *maps, std::vector<HapData *> *haps,
                 std::vector<FreqData *> *freqs, std::vector<GenoLikeData *> *gls)
{
    int n = 0;
    for (char k : keep) n += k != 0;
    MapData *m = maps->at(c);
    HapData *h = haps->at(c);
    FreqData *f = freqs->at(c);
    GenoLikeData *g = gls ? gls->at(c) : nullptr;
    if (n == m->nloci) return;
    if (n < 1) fail("no sites left on " + m->chr + " after filtering");
    MapData *m2 = initMapData(n);
    m2->chr = m->chr;
    HapData *h2 = new HapData{h->data ? new short *[n] : nullptr, h->nind, n, h->firstCopy ? new bool *[n] : nullptr,
                              h->packed ? new unsigned char *[n] : nullptr, h->phaseBits ? new unsigned char *[n] : nullptr,
                              h->bed, h->bed ? new long long[n] : nullptr};      // (a bed panel: only the row map is edited)
    FreqData *f2 = initFreqData(n);
    GenoLikeData *g2 = nullptr;
    if (g) {
        g2 = new GenoLikeData{g->data ? new double *[n] : nullptr, g->nind, n, g->codes ? new unsigned char *[n] : nullptr,
                              g->values, g->nvalues, g->codes16 ? new unsigned short *[n] : nullptr,
                              g->tgls, g->tgls ? new long long[n] : nullptr};      // (a device-held file: only the row map is edited)
        if (g->values) g->values = nullptr;   // the table moves on with the kept rows
    }
    int j = 0;
    for (int l = 0; l < m->nloci; l++) {
        if (!keep[l]) {
            if (h->data) delete[] h->data[l];
            if (h->packed) delete[] h->packed[l];
            if (h->firstCopy) delete[] h->firstCopy[l];
            if (h->phaseBits) delete[] h->phaseBits[l];
            if (g && g->data) delete[] g->data[l];
            if (g && g->codes) delete[] g->codes[l];
            if (g && g->codes16) delete[] g->codes16[l];
            continue;
        }
        m2->physicalPos[j] = m->physicalPos[l]; m2->geneticPos[j] = m->geneticPos[l];
        m2->locusName[j] = m->locusName[l]; m2->allele[j] = m->allele[l];
        if (h->data) h2->data[j] = h->data[l];
        if (h->packed) h2->packed[j] = h->packed[l];
        if (h->firstCopy) h2->firstCopy[j] = h->firstCopy[l];
        if (h->phaseBits) h2->phaseBits[j] = h->phaseBits[l];
        if (h->bed) h2->bedRow[j] = h->bedRow[l];
        f2->freq[j] = f->freq[l];
        if (g && g->data) g2->data[j] = g->data[l];
        if (g && g->codes) g2->codes[j] = g->codes[l];
        if (g && g->codes16) g2->codes16[j] = g->codes16[l];
        if (g && g->tgls) g2->tglsRow[j] = g->tglsRow[l];
        j++;
    }
    delete[] h->data; delete[] h->firstCopy; delete[] h->packed; delete[] h->phaseBits; delete[] h->bedRow; delete h;
    if (g) { delete[] g->data; delete[] g->codes; delete[] g->codes16; delete[] g->tglsRow; delete g; (*gls)[c] = g2; }
    releaseMapData(m); releaseFreqData(f);
    (*maps)[c] = m2; (*haps)[c] = h2; (*freqs)[c] = f2;
}
} // namespace

int filterMonomorphicSites(std::vector<MapData *> **maps, std::vector<HapData *> **haps,
                           std::vector<FreqData *> **freqs, std::vector<GenoLikeData *> **gls, bool USE_GL)
{
    int total = 0;
    for (size_t c = 0; c < (*maps)->size(); c++) {
        const FreqData *f = (*freqs)->at(c);
        std::vector<char> keep(f->nloci);
        for (int l = 0; l < f->nloci; l++) keep[l] = (f->freq[l] > 0 && f->freq[l] < 1); // garlic-data.cpp:871-914
        filterSites(c, keep, *maps, *haps, *freqs, USE_GL ? *gls : nullptr);
        total += (*maps)->at(c)->nloci;
    }
    return total;
}

// genetic-map scaffold: 4 columns chr snpid gpos ppos, one block per chromosome in file order
// (garlic-data.cpp:760-844)
std::vector<GenMapScaffold *> *loadMapScaffold(const std::string &mapfile, centromere *centro)
{
    std::vector<GenMapScaffold *> *out = new std::vector<GenMapScaffold *>;
    LineReader in(mapfile);
    std::string line, chr, id;
    int n = 0;
    while (in.next(line)) {
        n++;
        if (countFields(line) != 4)
            fail("line " + std::to_string(n) + " of " + mapfile + " does not have the 4 expected columns");
        std::stringstream ss(line);
        double g;
        int p;
        ss >> chr >> id >> g >> p;
        chr = checkChrName(chr);
        if (out->empty() || out->back()->chr != chr) {
            GenMapScaffold *sc = new GenMapScaffold;
            sc->chr = chr;
            sc->centroStart = centro->centromereStart(chr);
            sc->centroEnd = centro->centromereEnd(chr);
            out->push_back(sc);
        }
        out->back()->physicalPos.push_back(p);
        out->back()->geneticPos.push_back(g);
    }
    return out;
}
void releaseGenMapScaffold(std::vector<GenMapScaffold *> *v)
{
    if (!v) return;
    for (auto s : *v) delete s;
    delete v;
}

// --weighted keeps a site iff its frequency is in (0,1), it lies inside the scaffold's span and
// not strictly inside the centromere (garlic-data.cpp:1066-1098)
int filterMonomorphicAndOOBSites(std::vector<MapData *> **maps, std::vector<HapData *> **haps,
                                 std::vector<FreqData *> **freqs, std::vector<GenoLikeData *> **gls,
                                 std::vector<GenMapScaffold *> *scaffold, bool USE_GL)
{
    int total = 0;
    for (size_t c = 0; c < (*maps)->size(); c++) {
        const FreqData *f = (*freqs)->at(c);
        const MapData *m = (*maps)->at(c);
        const GenMapScaffold *sc = scaffold->at(c);
        std::vector<char> keep(f->nloci);
        for (int l = 0; l < f->nloci; l++) {
            const int q = m->physicalPos[l];
            keep[l] = (f->freq[l] > 0 && f->freq[l] < 1) && !(q < sc->physicalPos.front()) &&
                      !(q > sc->physicalPos.back()) && !(q > sc->centroStart && q < sc->centroEnd);
        }
        filterSites(c, keep, *maps, *haps, *freqs, USE_GL ? *gls : nullptr);
        total += (*maps)->at(c)->nloci;
    }
    return total;
}

// exact scaffold positions take the scaffold's value, the others are linearly interpolated between
// their neighbours with the reference's expression (garlic-data.cpp:718-757)
int interpolateGeneticmap(std::vector<MapData *> *maps, std::vector<GenMapScaffold *> *scaffold)
{
    int interpolated = 0;
    for (size_t c = 0; c < maps->size(); c++) {
        MapData *m = maps->at(c);
        const GenMapScaffold *sc = scaffold->at(c);
        const std::vector<int> &pp = sc->physicalPos;
        size_t k = 0;
        for (int l = 0; l < m->nloci; l++) {
            const int q = m->physicalPos[l];
            if (q < pp.front() || q > pp.back())
                fail("Sites outside of map scaffold should have been filtered out.");
            while (k + 1 < pp.size() && pp[k + 1] <= q) k++;
            if (pp[k] == q) { m->geneticPos[l] = sc->geneticPos[k]; continue; }
            const double x0 = pp[k], y0 = sc->geneticPos[k], x1 = pp[k + 1], y1 = sc->geneticPos[k + 1];
            m->geneticPos[l] = (((y1 - y0) / (x1 - x0)) * q + (y0 - ((y1 - y0) / (x1 - x0)) * x0));
            interpolated++;
        }
    }
    return interpolated;
}

// ------------------------------------------------------------------------- genotype cache
namespace {
const char CACHE_MAGIC[8] = {'G', 'A', 'R', 'L', 'I', 'C', '2', 'B'};
const uint32_t CACHE_VERSION = 2;       // 2: a flags word after the chromosome count
const uint32_t CACHE_FLAG_PHASE = 1;    // HapData::firstCopy rows (1 bit each) follow every chromosome's genotypes

struct CacheOut {
    FILE *f;
    explicit CacheOut(const std::string &p) : f(fopen(p.c_str(), "wb")) { if (!f) fail("cannot write " + p); }
    ~CacheOut() { if (f) fclose(f); }
    void put(const void *p, size_t n) { if (n && fwrite(p, 1, n, f) != n) fail("short write to genotype cache"); }
    template <class T> void val(T v) { put(&v, sizeof v); }
    void str(const std::string &s) { val<uint32_t>((uint32_t)s.size()); put(s.data(), s.size()); }
};
struct CacheIn {
    FILE *f;
    explicit CacheIn(const std::string &p) : f(fopen(p.c_str(), "rb")) { if (!f) fail("cannot read " + p); }
    ~CacheIn() { if (f) fclose(f); }
    void get(void *p, size_t n) { if (n && fread(p, 1, n, f) != n) fail("genotype cache is truncated"); }
    template <class T> T val() { T v; get(&v, sizeof v); return v; }
    std::string str()
    {
        const uint32_t n = val<uint32_t>();
        if (n > (1u << 20)) fail("genotype cache is corrupt (string length)");
        std::string s(n, '\0');
        get(&s[0], n);
        return s;
    }
};
} // namespace

// four PLINK codes -> four cache codes (0/1/2 copies of the counted allele, 3 = missing), per counted[row]
static const uint8_t *bedByteTable(unsigned counted)
{
    static uint8_t table[3][256];
    static std::once_flag once;
    std::call_once(once, [] {
        for (unsigned c = 0; c < 3; c++)
            for (unsigned b = 0; b < 256; b++) {
                unsigned out = 0;
                for (int k = 0; k < 4; k++) {
                    const short g = bedGenotype(c, (b >> (2 * k)) & 3u);
                    out |= (g < 0 ? 3u : (unsigned)g) << (2 * k);
                }
                table[c][b] = (uint8_t)out;
            }
    });
    return table[counted];
}

void writeGenotypeCache(const std::string &path, std::vector<HapData *> *haps, std::vector<MapData *> *maps,
                        std::vector<FreqData *> *freqs)
{
    CacheOut o(path);
    const int nind = haps->at(0)->nind;
    o.put(CACHE_MAGIC, 8);
    o.val<uint32_t>(CACHE_VERSION);
    o.val<uint32_t>((uint32_t)nind);
    o.val<uint32_t>((uint32_t)maps->size());
    bool phased = true;
    for (auto h : *haps) phased = phased && hasPhase(h);
    o.val<uint32_t>(phased ? CACHE_FLAG_PHASE : 0u);
    const size_t row = ((size_t)nind + 3) / 4, prow = ((size_t)nind + 7) / 8;
    std::vector<uint8_t> bits(row), pbits(prow);
    for (size_t c = 0; c < maps->size(); c++) {
        const MapData *m = maps->at(c);
        const HapData *h = haps->at(c);
        o.str(m->chr);
        o.val<uint32_t>((uint32_t)m->nloci);
        o.put(m->physicalPos, sizeof(int) * m->nloci);
        o.put(m->geneticPos, sizeof(double) * m->nloci);
        o.put(m->allele, (size_t)m->nloci);
        o.put(freqs->at(c)->freq, sizeof(double) * m->nloci);
        for (int l = 0; l < m->nloci; l++) o.str(m->locusName[l]);
        for (int l = 0; l < m->nloci; l++) {
            if (h->packed) { o.put(h->packed[l], row); continue; }
            if (h->bed) {   // the row in the cache's codes: a 256-entry byte table per counted allele
                const size_t r = (size_t)h->bedRow[l];
                const uint8_t *t = bedByteTable(h->bed->counted[r]);
                const unsigned char *src = h->bed->rows + r * row;
                for (size_t k = 0; k < row; k++) bits[k] = t[src[k]];
                if (nind & 3) bits[row - 1] &= (uint8_t)((1u << (2 * (nind & 3))) - 1);   // the unused bits 0, as below
                o.put(bits.data(), row);
                continue;
            }
            std::fill(bits.begin(), bits.end(), 0);
            for (int i = 0; i < nind; i++) {
                const short g = h->data[l][i];
                const unsigned code = (g == 0 || g == 1 || g == 2) ? (unsigned)g : 3u;   // -9 = missing
                bits[i >> 2] |= (uint8_t)(code << (2 * (i & 3)));
            }
            o.put(bits.data(), row);
        }
        if (phased)
            for (int l = 0; l < m->nloci; l++) {   // HapData::firstCopy, one bit per individual: bit i & 7 of byte i >> 3
                if (h->phaseBits) { o.put(h->phaseBits[l], prow); continue; }
                std::fill(pbits.begin(), pbits.end(), 0);
                if (h->bed) {      // a VCF image: firstCopy from the order plane
                    for (int i = 0; i < nind; i++)
                        if (bedFirstCopy(h->bed, (size_t)h->bedRow[l], i)) pbits[i >> 3] |= (uint8_t)(1u << (i & 7));
                    o.put(pbits.data(), prow);
                    continue;
                }
                for (int i = 0; i < nind; i++)
                    if (h->firstCopy[l][i]) pbits[i >> 3] |= (uint8_t)(1u << (i & 7));
                o.put(pbits.data(), prow);
            }
    }
}

void loadGenotypeCache(const std::string &path, int &numLoci, int &numInd, std::vector<HapData *> **haps,
                       std::vector<MapData *> **maps, std::vector<FreqData *> **freqs, bool keepPacked)
{
    CacheIn in(path);
    char magic[8];
    in.get(magic, 8);
    if (memcmp(magic, CACHE_MAGIC, 8) != 0) fail(path + " is not a GARLIC genotype cache");
    if (in.val<uint32_t>() != CACHE_VERSION) fail(path + ": unsupported genotype cache version");
    const int nind = (int)in.val<uint32_t>();
    const uint32_t nchr = in.val<uint32_t>();
    const uint32_t flags = in.val<uint32_t>();
    if (nind < 1 || nchr < 1 || nchr > 100000 || (flags & ~CACHE_FLAG_PHASE))
        fail(path + ": corrupt genotype cache header");
    const bool phased = (flags & CACHE_FLAG_PHASE) != 0;
    *haps = new std::vector<HapData *>;
    *maps = new std::vector<MapData *>;
    *freqs = new std::vector<FreqData *>;
    const size_t row = ((size_t)nind + 3) / 4, prow = ((size_t)nind + 7) / 8;
    std::vector<uint8_t> bits(row), pbits(prow);
    static const short DECODE[4] = {0, 1, 2, -9};
    numLoci = 0;
    try {
        for (uint32_t c = 0; c < nchr; c++) {
            const std::string chr = in.str();
            const int n = (int)in.val<uint32_t>();
            if (n < 1) fail(path + ": corrupt genotype cache (empty chromosome)");
            // each object joins its container as soon as it exists (rows still NULL), so that a
            // file that ends early leaves nothing behind
            MapData *m = initMapData(n);
            (*maps)->push_back(m);
            m->chr = chr;
            in.get(m->physicalPos, sizeof(int) * n);
            in.get(m->geneticPos, sizeof(double) * n);
            in.get(m->allele, (size_t)n);
            FreqData *f = initFreqData(n);
            (*freqs)->push_back(f);
            in.get(f->freq, sizeof(double) * n);
            for (int l = 0; l < n; l++) m->locusName[l] = in.str();
            HapData *h = new HapData{keepPacked ? nullptr : new short *[n](), nind, n, phased ? new bool *[n]() : nullptr,
                                     keepPacked ? new unsigned char *[n]() : nullptr,
                                     phased && keepPacked ? new unsigned char *[n]() : nullptr};
            (*haps)->push_back(h);
            for (int l = 0; l < n; l++) {
                if (keepPacked) {   // the rows as stored: the engine uploads them 2-bit
                    h->packed[l] = new unsigned char[row];
                    in.get(h->packed[l], row);
                    continue;
                }
                in.get(bits.data(), row);
                short *d = h->data[l] = new short[nind];
                for (int i = 0; i < nind; i++) d[i] = DECODE[(bits[i >> 2] >> (2 * (i & 3))) & 3];
            }
            for (int l = 0; phased && l < n; l++) {
                in.get(pbits.data(), prow);
                if (keepPacked) {   // the phase rows as stored, next to firstCopy (which the host's readers use): the engine uploads them 1-bit
                    if (nind & 7) pbits[prow - 1] &= (uint8_t)((1u << (nind & 7)) - 1);
                    h->phaseBits[l] = new unsigned char[prow];
                    memcpy(h->phaseBits[l], pbits.data(), prow);
                }
                bool *d = h->firstCopy[l] = new bool[nind];
                for (int i = 0; i < nind; i++) d[i] = (pbits[i >> 3] >> (i & 7)) & 1;
            }
            numLoci += n;
        }
    } catch (...) {
        releaseHapData(*haps); releaseMapData(*maps); releaseFreqData(*freqs);
        *haps = nullptr; *maps = nullptr; *freqs = nullptr;
        throw;
    }
    numInd = nind;
}

// ------------------------------------------------------------------------- the path
void setLodOptions(const LodOptions &o) { g_options = o; }

struct LodEngine::Impl {
    struct Shard {
        int device, ind_begin, nind;
        garlic_ctx *ctx = nullptr;
        garlic_panel *panel = nullptr;
    };
    std::vector<Shard> shards;
    std::vector<int32_t> chr_nloci;
    std::vector<MapData *> *maps;
    int nind = 0;
    bool use_gl = false;
    bool have_phase = false;   // every HapData carries firstCopy: the panels hold the phase planes
    int kde_multi_shards = 0;  // LodEngine::kdeMultiShards
};

LodEngine::LodEngine(std::vector<HapData *> *haps, std::vector<FreqData *> *freqs, std::vector<MapData *> *maps,
                     std::vector<GenoLikeData *> *gls, centromere *centro, bool USE_GL,
                     const std::vector<int> &devices)
    : impl(new Impl)
{
    try {
        upload(haps, freqs, maps, gls, centro, USE_GL, devices);
    } catch (...) {   // a constructor that throws runs no destructor: release what was created
        release();
        throw;
    }
}

void LodEngine::release()
{
    for (auto &s : impl->shards) {
        if (s.panel) garlic_panel_destroy(s.panel);
        if (s.ctx) garlic_ctx_destroy(s.ctx);
    }
    delete impl;
    impl = nullptr;
}

void LodEngine::upload(std::vector<HapData *> *haps, std::vector<FreqData *> *freqs, std::vector<MapData *> *maps,
                       std::vector<GenoLikeData *> *gls, centromere *centro, bool USE_GL,
                       const std::vector<int> &devices)
{
    const int nchr = (int)maps->size();
    impl->maps = maps;
    impl->nind = haps->at(0)->nind;
    impl->use_gl = USE_GL;
    int64_t nloci = 0;
    for (auto m : *maps) { impl->chr_nloci.push_back(m->nloci); nloci += m->nloci; }
    std::vector<int32_t> pos(nloci), cs(nchr), ce(nchr);
    std::vector<double> gpos(nloci), freq(nloci);
    int64_t o = 0;
    for (int c = 0; c < nchr; c++) {
        const MapData *m = maps->at(c);
        cs[c] = centro->centromereStart(m->chr);   // garlic-roh.cpp:36-37
        ce[c] = centro->centromereEnd(m->chr);
        for (int l = 0; l < m->nloci; l++, o++) {
            pos[o] = m->physicalPos[l];
            gpos[o] = m->geneticPos[l];
            freq[o] = freqs->at(c)->freq[l];
        }
    }
    std::vector<int> devs = devices.empty() ? std::vector<int>{0} : devices;
    const int nd = std::min<int>((int)devs.size(), impl->nind);
    const int per = (impl->nind + nd - 1) / nd; // contiguous blocks in TFAM order
    for (int d = 0; d < nd; d++) {
        if (std::min(per, impl->nind - d * per) < 1) break;
        impl->shards.emplace_back();
        Impl::Shard &s = impl->shards.back();
        s.device = devs[d];
        s.ind_begin = d * per;
        s.nind = std::min(per, impl->nind - s.ind_begin);
        check(garlic_ctx_create(s.device, nullptr, &s.ctx), "garlic_ctx_create");
        check(garlic_panel_create(s.ctx, nchr, impl->chr_nloci.data(), s.nind, &s.panel), "garlic_panel_create");
        check(garlic_panel_set_map(s.panel, pos.data(), gpos.data(), cs.data(), ce.data()), "garlic_panel_set_map");
        check(garlic_panel_set_freq(s.panel, freq.data()), "garlic_panel_set_freq");
        if (USE_GL && g_options.tgls_term_bytes != 0)      // --tgls-term-gb: the term matrix of each shard in slabs (weighted calls too)
            check(garlic_panel_set_tgls_term_budget(s.panel, g_options.tgls_term_bytes), "garlic_panel_set_tgls_term_budget");
    }
    // a .bed panel: every shard's context fills its column block from the image on its device, through the row map the
    // site filters left
    if (haps->at(0)->bed) {
        BedFile *b = haps->at(0)->bed;
        std::vector<int64_t> dest((size_t)b->nrows, -1);
        int64_t at = 0;
        for (int c = 0; c < nchr; c++) {
            const HapData *h = haps->at(c);
            if (h->bed != b) fail("the chromosomes come from different .bed files");
            for (int l = 0; l < h->nloci; l++) dest[(size_t)h->bedRow[l]] = at++;
        }
        for (auto &s : impl->shards) {
            check(garlic_panel_set_genotypes_bed(s.panel, bedImageOn(b, s.device), s.ind_begin, dest.data()),
                  "garlic_panel_set_genotypes_bed");
            if (hasPhase(haps->at(0)))      // a phased VCF: firstCopy from the image's order plane, device to device
                check(garlic_panel_set_phase_bed(s.panel, bedImageOn(b, s.device), s.ind_begin, dest.data()), "garlic_panel_set_phase_bed");
        }
    }
    // likelihoods held on the devices (loadTGLSFile): every shard's panel takes its columns from the object on its device,
    // through the row map the site filters left
    const bool gl_on_device = USE_GL && gls->at(0)->tgls;
    if (gl_on_device) {
        TglsFile *f = gls->at(0)->tgls;
        std::vector<int64_t> dest((size_t)f->nrows, -1);
        int64_t at = 0;
        for (int c = 0; c < nchr; c++) {
            const GenoLikeData *g = gls->at(c);
            if (g->tgls != f) fail("the chromosomes' likelihoods come from different files");
            for (int l = 0; l < g->nloci; l++) dest[(size_t)g->tglsRow[l]] = at++;
        }
        for (auto &s : impl->shards) {
            int64_t ind_offset = 0;
            garlic_tgls *obj = tglsObjectOn(f, s.device, s.ind_begin, s.nind, ind_offset);
            check(garlic_panel_set_gl_tgls(s.panel, obj, f->glType, ind_offset, dest.data()), "garlic_panel_set_gl_tgls");
        }
    }
    // genotype rows are separate allocations in HapData: stage a slab of SNP rows at a time
    const int64_t slab = std::max<int64_t>(1, ((int64_t)64 << 20) / (2 * (int64_t)impl->nind));
    std::vector<int16_t> stage;
    std::vector<uint8_t> stage2, stage_glc;
    std::vector<uint16_t> stage_glc16;
    std::vector<double> stage_gl;
    // one chromosome with 16-bit codes: the one-byte chromosomes go up widened too, so the panel's table merges them all
    // (one-byte uploads alone that pass 256 values between them would turn the panel continuous)
    bool wide_codes = false;
    if (USE_GL) for (auto g : *gls) wide_codes = wide_codes || g->codes16;
    std::vector<uint8_t> stage_fc, stage_fcbits;
    impl->have_phase = true;
    for (auto h : *haps) impl->have_phase = impl->have_phase && hasPhase(h);
    o = 0;
    for (int c = 0; c < nchr; c++) {
        const HapData *h = haps->at(c);
        for (int l0 = 0; l0 < h->nloci; l0 += (int)slab) {
            const int rows = (int)std::min<int64_t>(slab, h->nloci - l0);
            const size_t row_bytes = ((size_t)impl->nind + 3) / 4;
            if (h->bed) {   // (uploaded above)
            } else if (h->packed) {
                stage2.resize((size_t)rows * row_bytes);
                for (int r = 0; r < rows; r++) memcpy(&stage2[(size_t)r * row_bytes], h->packed[l0 + r], row_bytes);
            } else {
                stage.resize((size_t)rows * impl->nind);
                for (int r = 0; r < rows; r++)
                    memcpy(&stage[(size_t)r * impl->nind], h->data[l0 + r], sizeof(short) * impl->nind);
            }
            const GenoLikeData *gld = USE_GL && !gl_on_device ? gls->at(c) : nullptr;   // (on the device: filled above)
            const bool gl16 = gld && (gld->codes16 || (gld->codes && wide_codes));
            if (gl16) {
                stage_glc16.resize((size_t)rows * impl->nind);
                for (int r = 0; r < rows; r++)
                    for (int i = 0; i < impl->nind; i++)
                        stage_glc16[(size_t)r * impl->nind + i] = gld->codes16 ? gld->codes16[l0 + r][i] : gld->codes[l0 + r][i];
            } else if (gld && gld->codes) {
                stage_glc.resize((size_t)rows * impl->nind);
                for (int r = 0; r < rows; r++) memcpy(&stage_glc[(size_t)r * impl->nind], gld->codes[l0 + r], impl->nind);
            } else if (gld) {
                stage_gl.resize((size_t)rows * impl->nind);
                for (int r = 0; r < rows; r++)
                    memcpy(&stage_gl[(size_t)r * impl->nind], gld->data[l0 + r], sizeof(double) * impl->nind);
            }
            const size_t prow_bytes = ((size_t)impl->nind + 7) / 8;
            if (h->bed) {   // (filled above)
            } else if (impl->have_phase && h->phaseBits) {   // one bit per genotype, as the cache holds them
                stage_fc.resize((size_t)rows * prow_bytes);
                for (int r = 0; r < rows; r++) memcpy(&stage_fc[(size_t)r * prow_bytes], h->phaseBits[l0 + r], prow_bytes);
            } else if (impl->have_phase) {
                stage_fc.resize((size_t)rows * impl->nind);
                for (int r = 0; r < rows; r++)
                    for (int i = 0; i < impl->nind; i++)
                        stage_fc[(size_t)r * impl->nind + i] = h->firstCopy[l0 + r][i];
            }
            for (auto &s : impl->shards) {
                if (h->bed) {
                } else if (h->packed)
                    check(garlic_panel_set_genotypes_2bit(s.panel, stage2.data(), (int64_t)row_bytes, s.ind_begin, o + l0,
                                                          rows, GARLIC_HOST), "garlic_panel_set_genotypes_2bit");
                else
                    check(garlic_panel_set_genotypes(s.panel, stage.data() + s.ind_begin, impl->nind, o + l0, rows,
                                                     GARLIC_HOST), "garlic_panel_set_genotypes");
                if (h->bed) {
                } else if (impl->have_phase && h->phaseBits && (s.ind_begin & 7) == 0) {
                    check(garlic_panel_set_phase_bits(s.panel, stage_fc.data() + s.ind_begin / 8, (int64_t)prow_bytes, o + l0, rows,
                                                      GARLIC_HOST), "garlic_panel_set_phase_bits");
                } else if (impl->have_phase && h->phaseBits) {   // a shard that begins inside a byte: its bits moved down
                    const size_t sb = ((size_t)s.nind + 7) / 8;
                    stage_fcbits.assign((size_t)rows * sb, 0);
                    for (int r = 0; r < rows; r++)
                        for (int i = 0; i < s.nind; i++) {
                            const int g = s.ind_begin + i;
                            if ((stage_fc[(size_t)r * prow_bytes + (g >> 3)] >> (g & 7)) & 1)
                                stage_fcbits[(size_t)r * sb + (i >> 3)] |= (uint8_t)(1u << (i & 7));
                        }
                    check(garlic_panel_set_phase_bits(s.panel, stage_fcbits.data(), (int64_t)sb, o + l0, rows, GARLIC_HOST),
                          "garlic_panel_set_phase_bits");
                } else if (impl->have_phase) {
                    check(garlic_panel_set_phase(s.panel, stage_fc.data() + s.ind_begin, impl->nind, o + l0, rows,
                                                 GARLIC_HOST), "garlic_panel_set_phase");
                }
                if (gl16)
                    check(garlic_panel_set_gl_codes16(s.panel, stage_glc16.data() + s.ind_begin, impl->nind, o + l0, rows,
                                                      gld->values, gld->nvalues, GARLIC_HOST), "garlic_panel_set_gl_codes16");
                else if (gld && gld->codes)
                    check(garlic_panel_set_gl_codes(s.panel, stage_glc.data() + s.ind_begin, impl->nind, o + l0, rows,
                                                    gld->values, gld->nvalues, GARLIC_HOST), "garlic_panel_set_gl_codes");
                else if (gld)
                    check(garlic_panel_set_gl(s.panel, stage_gl.data() + s.ind_begin, impl->nind, o + l0, rows,
                                              GARLIC_HOST), "garlic_panel_set_gl");
            }
        }
        o += h->nloci;
    }
}

LodEngine::~LodEngine() { release(); }

// ---- feature counts per ROH class (feature_counts.hpp)
FeatureData *loadFeatureCounts(const std::string &features, const std::string &tpedCounting, const std::string &tfamCounting)
{
    try {
        FeatureData *d = new FeatureData(loadFeatureData(features, tpedCounting, tfamCounting));
        std::cerr << "Feature counts: " << d->ann.allele.size() << " annotated alleles, " << d->ann.effects.size() << " effects; "
                  << d->rows.lines_annotated << " of " << d->rows.lines << " counting loci annotated, " << d->iid.size() << " individuals\n";
        return d;
    } catch (const std::exception &e) {
        fail(e.what());
    }
}

// the .bed form: the plan from the .bim and the .fam, and the counting file set opened (its image is made where the count runs)
FeatureData *loadFeatureCountsBed(const std::string &features, const std::string &bedCounting, const std::string &bimCounting,
                                  const std::string &famCounting)
{
    std::unique_ptr<FeatureData, void (*)(FeatureData *)> d(nullptr, releaseFeatureCounts);
    try {
        d.reset(new FeatureData(loadFeatureDataBed(features, bimCounting, famCounting)));
    } catch (const std::exception &e) {
        fail(e.what());
    }
    d->bed = openBedFile(bedCounting, bimCounting, famCounting, /*anyPopulations=*/true);
    d->bed->refs = 1;
    if (d->bed->nrows != d->plan->image_rows || (size_t)d->bed->nind != d->iid.size())
        fail(bimCounting + " / " + famCounting + ": " + std::to_string(d->plan->image_rows) + " loci x " + std::to_string(d->iid.size()) +
             " individuals in the row plan, " + std::to_string(d->bed->nrows) + " x " + std::to_string(d->bed->nind) + " in the file set");
    std::cerr << "Feature counts: " << d->ann.allele.size() << " annotated alleles, " << d->ann.effects.size() << " effects; "
              << d->plan->lines_annotated << " of " << d->plan->lines << " counting loci annotated, " << d->iid.size() << " individuals\n";
    return d.release();
}

void releaseFeatureCounts(FeatureData *data)
{
    if (!data) return;
    releaseBedFile(data->bed);
    delete data;
}

namespace {
// the hom rows onto the device, the count, the table
// (`device`: the one `ctx` is on.)  The .bed form uploads the counting file's image there, has the device build the hom rows
// from it and lets the image go before the count.
void featureCountsOn(garlic_ctx *ctx, int device, const FeatureData &d, const std::vector<FeatureInterval> &iv, int n_classes,
                     const std::string &outfile)
{
    static_assert(sizeof(FeatureInterval) == sizeof(garlic_roh_interval), "one interval");
    const size_t nind = d.iid.size(), ne = d.ann.effects.size();
    const int64_t nrows = d.plan ? d.plan->nrows() : d.rows.nrows();
    std::vector<int64_t> counts(nind * (size_t)(n_classes + 1) * std::max<size_t>(ne, 1), 0);
    if (ne > 0) {
        garlic_feature_set *fs = nullptr;
        check(garlic_feature_set_create(ctx, nrows, (int32_t)nind, &fs), "garlic_feature_set_create");
        int rc = GARLIC_OK;
        const char *what = "";
        std::string error;
        if (d.plan && nrows > 0) {
            try {
                what = "garlic_feature_set_rows_bed";
                rc = garlic_feature_set_rows_bed(fs, bedFullImageOn(d.bed, device), d.plan->file_row.data(), d.plan->allele.data(), 0, nrows);
            } catch (...) {      // (the upload's own failure: its message is out already)
                error = "the counting .bed did not reach the device";
            }
            if (rc != GARLIC_OK) error = std::string(what) + ": " + garlic_hip_last_error();
            const size_t slot = bedSlotOn(d.bed, device);
            garlic_bed_destroy((garlic_bed *)d.bed->images[slot].bed);
            d.bed->images[slot].bed = nullptr;
            if (!error.empty()) {
                garlic_feature_set_destroy(fs);
                fail(error);
            }
        } else if (nrows > 0) {
            what = "garlic_feature_set_rows";
            rc = garlic_feature_set_rows(fs, d.rows.bits.data(), d.rows.row_bytes, 0, nrows);
        }
        if (rc == GARLIC_OK) {
            what = "garlic_feature_set_sites";
            rc = d.plan ? garlic_feature_set_sites(fs, d.plan->chr.data(), d.plan->pos.data(), d.plan->effect.data())
                        : garlic_feature_set_sites(fs, d.rows.chr.data(), d.rows.pos.data(), d.rows.effect.data());
        }
        if (rc == GARLIC_OK) {
            what = "garlic_feature_counts";
            rc = garlic_feature_counts(fs, (const garlic_roh_interval *)iv.data(), (int64_t)iv.size(), n_classes, (int32_t)ne, counts.data(), GARLIC_HOST);
        }
        if (rc != GARLIC_OK) error = std::string(what) + ": " + garlic_hip_last_error();
        garlic_feature_set_destroy(fs);
        if (!error.empty()) fail(error);
    }
    std::ofstream out(outfile.c_str());
    if (out.fail()) fail("Failed to open " + outfile);
    writeFeatureTable(out, d.ann.effects, d.iid, counts.data(), n_classes);
    out.close();
    std::cerr << "Feature counts: " << outfile << " (" << nrows << " hom rows, " << iv.size() << " ROH, " << n_classes << " classes)\n";
}
} // namespace

void featureCountsFromBed(FeatureData *data, const std::string &rohBed, const std::string &outfile, int device)
{
    if (!data) fail("featureCountsFromBed: no feature data");
    int n_classes = 0;
    std::vector<FeatureInterval> iv;
    try {
        iv = readRohBed(rohBed, data->iid, data->chrs, &n_classes);
    } catch (const std::exception &e) {
        fail(e.what());
    }
    garlic_ctx *ctx = nullptr;
    check(garlic_ctx_create(device, nullptr, &ctx), "garlic_ctx_create");
    try {
        featureCountsOn(ctx, device, *data, iv, n_classes, outfile);
    } catch (...) {
        garlic_ctx_destroy(ctx);
        throw;
    }
    garlic_ctx_destroy(ctx);
}

void LodEngine::featureCounts(FeatureData *data, std::vector<ROHData *> *rohDataByInd, std::vector<MapData *> *mapDataByChr,
                              const std::vector<double> &bounds, const std::string &outfile)
{
    if (!data || !rohDataByInd || !mapDataByChr) fail("featureCounts: feature data, ROH calls and maps are required");
    if ((int)bounds.size() + 1 > FEATURE_MAX_CLASSES) fail("featureCounts: at most " + std::to_string(FEATURE_MAX_CLASSES) + " size classes");
    std::vector<std::string> panel_iid;
    std::vector<std::vector<FeatureCall>> calls;
    for (const ROHData *r : *rohDataByInd) {
        panel_iid.push_back(r->indID);
        calls.emplace_back();
        for (size_t k = 0; k < r->chr.size(); k++)       // start / stop as writeROHData prints them
            calls.back().push_back(FeatureCall{mapDataByChr->at((size_t)r->chr[k])->chr, int(r->start[k]), int(r->stop[k]), r->length[k]});
    }
    int n_classes = 0;
    const std::vector<FeatureInterval> iv = buildFeatureIntervals(panel_iid, calls, bounds, data->iid, data->chrs, &n_classes);
    featureCountsOn(impl->shards[0].ctx, impl->shards[0].device, *data, iv, n_classes, outfile);
}

void LodEngine::tglsTermSlabs(int *slab_blocks, int *n_slabs)
{
    int32_t sb = 0, ns = 0;
    if (!impl->shards.empty())
        check(garlic_panel_tgls_terms_info(impl->shards[0].panel, nullptr, nullptr, &sb, &ns), "garlic_panel_tgls_terms_info");
    if (slab_blocks) *slab_blocks = sb;
    if (n_slabs) *n_slabs = ns;
}

std::vector<WinData *> *LodEngine::lodWindows(int winsize, double error, int MAX_GAP)
{
    return run(false, winsize, error, MAX_GAP, 0, 0.0);
}

std::vector<WinData *> *LodEngine::wlodWindows(std::vector<LDData *> *lds, int winsize, double error, int MAX_GAP,
                                               int M, double mu)
{
    // LDData rows are separate allocations: flatten to [locus][winsize] and hand to every device
    int64_t nloci = 0;
    for (int n : impl->chr_nloci) nloci += n;
    std::vector<double> flat((size_t)nloci * winsize);
    int64_t o = 0;
    for (size_t c = 0; c < lds->size(); c++)
        for (int l = 0; l < lds->at(c)->nloci; l++, o++)
            memcpy(&flat[(size_t)o * winsize], lds->at(c)->LD[l], sizeof(double) * winsize);
    for (auto &s : impl->shards) check(garlic_panel_set_ld(s.panel, winsize, flat.data(), GARLIC_HOST), "garlic_panel_set_ld");
    return run(true, winsize, error, MAX_GAP, M, mu);
}

std::vector<WinData *> *LodEngine::wlodWindowsResident(int winsize, double error, int MAX_GAP, int M, double mu)
{
    return run(true, winsize, error, MAX_GAP, M, mu);
}

// LodOptions::feed_sorted: the shards' ascending feeds into `out` (feed_merge.hpp)
static void mergeShardFeeds(const std::vector<std::vector<double>> &feeds, double *out)
{
    std::vector<const double *> parts;
    std::vector<int64_t> sizes;
    for (const auto &f : feeds) {
        parts.push_back(f.data());
        sizes.push_back((int64_t)f.size());
    }
    mergeSortedFeeds(parts, sizes, out);
}

DoubleData *LodEngine::lodFeed(int winsize, double error, int MAX_GAP, int step, bool weighted, int M, double mu,
                               const std::vector<int> *kdeSubsample)
{
    std::cerr << "Calculating LOD scores with winsize " << winsize << " (thinned on the device, step " << step << ").\n";
    const int nchr = (int)impl->chr_nloci.size();
    const size_t ns = impl->shards.size();
    // --kde-subsample (convertSubsetWinData2DoubleData, garlic-data.cpp:2071-2150): panel-wide indices in
    // increasing order (what gsl_ran_choose returns), so that the shards' feeds -- each over its own part
    // of the list -- merge per chromosome in shard order exactly as for the whole panel
    const bool subset = kdeSubsample && !kdeSubsample->empty();
    if (subset)
        for (size_t i = 1; i < kdeSubsample->size(); i++)
            if ((*kdeSubsample)[i] <= (*kdeSubsample)[i - 1]) fail("KDE subsample must be in increasing order");
    const bool sorted = g_options.feed_sorted;
    std::vector<std::vector<double>> feeds(ns);
    std::vector<std::vector<int64_t>> per_chr(ns, std::vector<int64_t>(nchr, 0));
    std::vector<std::string> errors(ns);
    std::vector<std::thread> th;
    for (size_t k = 0; k < ns; k++)
        th.emplace_back([&, k] {
            auto &s = impl->shards[k];
            std::vector<int32_t> mine;
            if (subset) {
                for (int g : *kdeSubsample)
                    if (g >= s.ind_begin && g < s.ind_begin + s.nind) mine.push_back(g - s.ind_begin);
                if (mine.empty()) { feeds[k].clear(); return; }      // no listed individual lives here
            }
            const int64_t rows = subset ? (int64_t)mine.size() : s.nind;
            int64_t cap = 0, n = 0;
            for (int c = 0; c < nchr; c++) cap += ((int64_t)impl->chr_nloci[c] + step - 1) / step * rows;
            feeds[k].resize((size_t)std::max<int64_t>(cap, 1));
            if (garlic_panel_set_feed_order(s.panel, sorted ? GARLIC_FEED_ORDER_SORTED : GARLIC_FEED_ORDER_REFERENCE) != GARLIC_OK ||
                garlic_lod_feed_subset(s.panel, winsize, error, MAX_GAP, impl->use_gl, weighted, M, mu, step,
                                       subset ? mine.data() : nullptr, (int32_t)mine.size(), feeds[k].data(), cap, &n,
                                       per_chr[k].data()) != GARLIC_OK)
                errors[k] = garlic_hip_last_error();
            else
                feeds[k].resize((size_t)n);
        });
    for (auto &t : th) t.join();
    for (auto &e : errors)
        if (!e.empty()) fail("garlic_lod_feed: " + e);
    // merge in the reference's order: chromosome -> individual (= shard order) -> locus
    int64_t total = 0;
    for (auto &f : feeds) total += (int64_t)f.size();
    if (total > 0x7fffffff) fail("KDE feed has more than 2^31 values: DoubleData::size is an int");
    DoubleData *d = new DoubleData;
    d->size = (int)total;
    d->data = new double[total > 0 ? total : 1];
    if (sorted) {       // every shard's feed is ascending: their merge is the ascending feed of the whole panel
        mergeShardFeeds(feeds, d->data);
        return d;
    }
    std::vector<int64_t> off(ns, 0);
    int64_t o = 0;
    for (int c = 0; c < nchr; c++)
        for (size_t k = 0; k < ns; k++) {
            memcpy(d->data + o, feeds[k].data() + off[k], sizeof(double) * (size_t)per_chr[k][c]);
            o += per_chr[k][c];
            off[k] += per_chr[k][c];
        }
    return d;
}

// computeKDE of the feed lodFeed would return, sorted (garlic_hip.h: garlic_lod_kde).  One shard: the feed never leaves the
// device.  Several: the shards' sorted feeds merged on the host as for LodOptions::feed_sorted, then garlic_feed_kde on
// the first context -- every feed value crosses PCIe twice and one device computes all the sums.
// LodOptions::kde_on_shards: every shard with KDE individuals leaves its sorted feed on its device as one garlic_kde_part
// (on the shards' threads, as assembleROHWindows runs them) and garlic_kde_parts reduces them where they lie: the moments
// and the Gaussian sums add over the shards, the quartiles come from rank queries (kde_parts.hpp).  One shard: one part,
// garlic_lod_kde's bits.
KdeData LodEngine::lodKde(int winsize, double error, int MAX_GAP, int step, bool weighted, int M, double mu,
                             const std::vector<int> *kdeSubsample)
{
    static_assert(sizeof(KdeData) == sizeof(garlic_kde) && KDE_POINTS == GARLIC_KDE_POINTS, "KdeData mirrors garlic_kde");
    garlic_kde gk;
    auto result = [&] { KdeData k; memcpy(&k, &gk, sizeof k); return k; };
    const bool subset = kdeSubsample && !kdeSubsample->empty();
    if (g_options.kde_on_shards) {
        if (subset)
            for (size_t i = 1; i < kdeSubsample->size(); i++)
                if ((*kdeSubsample)[i] <= (*kdeSubsample)[i - 1]) fail("KDE subsample must be in increasing order");
        const size_t ns = impl->shards.size();
        std::vector<garlic_kde_part *> made(ns, nullptr);
        std::vector<std::string> errors(ns);
        std::vector<std::thread> th;
        for (size_t k = 0; k < ns; k++)
            th.emplace_back([&, k] {
                auto &s = impl->shards[k];
                std::vector<int32_t> mine;
                if (subset) {
                    for (int g : *kdeSubsample)
                        if (g >= s.ind_begin && g < s.ind_begin + s.nind) mine.push_back(g - s.ind_begin);
                    if (mine.empty()) return;          // no listed individual lives here: no part
                }
                if (garlic_lod_kde_part(s.panel, winsize, error, MAX_GAP, impl->use_gl, weighted, M, mu, step, subset ? mine.data() : nullptr,
                                        (int32_t)mine.size(), &made[k], nullptr) != GARLIC_OK)
                    errors[k] = garlic_hip_last_error();
            });
        for (auto &t : th) t.join();
        std::vector<garlic_kde_part *> parts;
        for (garlic_kde_part *p : made)
            if (p) parts.push_back(p);
        std::string error_text;
        for (auto &e : errors)
            if (!e.empty() && error_text.empty()) error_text = "garlic_lod_kde_part: " + e;
        if (error_text.empty()) {
            std::cerr << "KDE on " << parts.size() << " shards\n";
            if (parts.empty()) error_text = "garlic_kde_parts: no shard holds a KDE individual";
            else if (garlic_kde_parts(parts.data(), (int32_t)parts.size(), &gk) != GARLIC_OK)
                error_text = std::string("garlic_kde_parts: ") + garlic_hip_last_error();
        }
        for (garlic_kde_part *p : parts) garlic_kde_part_destroy(p);
        if (!error_text.empty()) fail(error_text);
        return result();
    }
    if (impl->shards.size() == 1) {
        auto &s = impl->shards[0];
        std::cerr << "Calculating LOD scores with winsize " << winsize << " (thinned on the device, step " << step << ", KDE on the device).\n";
        std::vector<int32_t> mine;
        if (subset)
            for (size_t i = 0; i < kdeSubsample->size(); i++) {
                if (i && (*kdeSubsample)[i] <= (*kdeSubsample)[i - 1]) fail("KDE subsample must be in increasing order");
                mine.push_back((*kdeSubsample)[i] - s.ind_begin);
            }
        if (garlic_lod_kde(s.panel, winsize, error, MAX_GAP, impl->use_gl, weighted, M, mu, step, subset ? mine.data() : nullptr,
                           (int32_t)mine.size(), &gk, nullptr) != GARLIC_OK)
            fail(std::string("garlic_lod_kde: ") + garlic_hip_last_error());
        return result();
    }
    const bool was = g_options.feed_sorted;
    g_options.feed_sorted = true;
    DoubleData *feed = nullptr;
    try {
        feed = lodFeed(winsize, error, MAX_GAP, step, weighted, M, mu, kdeSubsample);
    } catch (...) {
        g_options.feed_sorted = was;
        throw;
    }
    g_options.feed_sorted = was;
    const int rc = garlic_feed_kde(impl->shards[0].ctx, feed->data, feed->size, GARLIC_HOST, &gk);
    releaseDoubleData(feed);
    if (rc != GARLIC_OK) fail(std::string("garlic_feed_kde: ") + garlic_hip_last_error());
    return result();
}

// one shard on one device (garlic_lod_kde_multi), or LodOptions::kde_on_shards on any number of shards (one
// garlic_kde_part_set per shard, garlic_kde_parts_multi)
bool LodEngine::kdeMultiInOneCall() const { return impl->shards.size() == 1 || g_options.kde_on_shards; }

int LodEngine::kdeMultiShards() const { return impl->kde_multi_shards; }

std::vector<KdeData> LodEngine::lodKdeMulti(const std::vector<int> &winsizes, double error, int MAX_GAP, const std::vector<int> *steps,
                                            const std::vector<int> *kdeSubsample, std::vector<int> *status)
{
    const size_t m = winsizes.size();
    std::vector<KdeData> out(m);
    std::vector<int32_t> st(m);
    for (size_t i = 0; i < m; i++) st[i] = steps ? (*steps)[i] : winsizes[i];
    if (status) status->assign(m, 0);
    static_assert(KDE_MAX_FEEDS == GARLIC_KDE_MAX_FEEDS, "one limit");
    impl->kde_multi_shards = 0;
    if (!kdeMultiInOneCall() || m > (size_t)GARLIC_KDE_MAX_FEEDS) {
        for (size_t i = 0; i < m; i++) out[i] = lodKde(winsizes[i], error, MAX_GAP, st[i], false, 0, 0.0, kdeSubsample);
        return out;
    }
    if (m == 0) return out;
    if (g_options.kde_on_shards) {
        // lodKde's sharded path for all sizes at once: every shard with KDE individuals leaves the sorted feeds of all sizes
        // on its device as one garlic_kde_part_set (on the shards' threads), garlic_kde_parts_multi reduces them where they lie
        const bool subset = kdeSubsample && !kdeSubsample->empty();
        if (subset)
            for (size_t i = 1; i < kdeSubsample->size(); i++)
                if ((*kdeSubsample)[i] <= (*kdeSubsample)[i - 1]) fail("KDE subsample must be in increasing order");
        const size_t ns = impl->shards.size();
        std::cerr << "Calculating LOD scores with winsizes";
        for (size_t i = 0; i < m; i++) std::cerr << (i ? ", " : " ") << winsizes[i];
        std::cerr << " (thinned on the devices, KDE of all sizes on the shards in one call).\n";
        std::vector<int32_t> sizes(winsizes.begin(), winsizes.end()), code(m, 0);
        std::vector<garlic_kde_part_set *> made(ns, nullptr);
        std::vector<std::string> errors(ns);
        std::vector<std::thread> th;
        for (size_t k = 0; k < ns; k++)
            th.emplace_back([&, k] {
                auto &s = impl->shards[k];
                std::vector<int32_t> mine;
                if (subset) {
                    for (int g : *kdeSubsample)
                        if (g >= s.ind_begin && g < s.ind_begin + s.nind) mine.push_back(g - s.ind_begin);
                    if (mine.empty()) return;          // no listed individual lives here: no set
                }
                if (garlic_lod_kde_part_set(s.panel, sizes.data(), st.data(), (int32_t)m, error, MAX_GAP, impl->use_gl, subset ? mine.data() : nullptr,
                                            (int32_t)mine.size(), &made[k], nullptr) != GARLIC_OK)
                    errors[k] = garlic_hip_last_error();
            });
        for (auto &t : th) t.join();
        std::vector<garlic_kde_part_set *> sets;
        for (garlic_kde_part_set *p : made)
            if (p) sets.push_back(p);
        std::string error_text;
        for (auto &e : errors)
            if (!e.empty() && error_text.empty()) error_text = "garlic_lod_kde_part_set: " + e;
        std::vector<garlic_kde> gk(m);
        if (error_text.empty()) {
            if (sets.empty()) error_text = "garlic_kde_parts_multi: no shard holds a KDE individual";
            else if (garlic_kde_parts_multi(sets.data(), (int32_t)sets.size(), gk.data(), status ? code.data() : nullptr) != GARLIC_OK)
                error_text = std::string("garlic_kde_parts_multi: ") + garlic_hip_last_error();
        }
        impl->kde_multi_shards = (int)sets.size();
        for (garlic_kde_part_set *p : sets) garlic_kde_part_set_destroy(p);
        if (!error_text.empty()) fail(error_text);
        for (size_t i = 0; i < m; i++) {
            if (status) (*status)[i] = code[i];
            if (!code[i]) memcpy(&out[i], &gk[i], sizeof out[i]);
        }
        return out;
    }
    if (m == 0) return out;
    auto &s = impl->shards[0];
    const bool subset = kdeSubsample && !kdeSubsample->empty();
    std::cerr << "Calculating LOD scores with winsizes";
    for (size_t i = 0; i < m; i++) std::cerr << (i ? ", " : " ") << winsizes[i];
    std::cerr << " (thinned on the device, KDE of all sizes on the device in one call).\n";
    std::vector<int32_t> mine;
    if (subset)
        for (size_t i = 0; i < kdeSubsample->size(); i++) {
            if (i && (*kdeSubsample)[i] <= (*kdeSubsample)[i - 1]) fail("KDE subsample must be in increasing order");
            mine.push_back((*kdeSubsample)[i] - s.ind_begin);
        }
    std::vector<garlic_kde> gk(m);
    std::vector<int32_t> sizes(winsizes.begin(), winsizes.end()), code(m, 0);
    if (garlic_lod_kde_multi(s.panel, sizes.data(), st.data(), (int32_t)m, error, MAX_GAP, impl->use_gl, subset ? mine.data() : nullptr,
                             (int32_t)mine.size(), gk.data(), status ? code.data() : nullptr, nullptr) != GARLIC_OK)
        fail(std::string("garlic_lod_kde_multi: ") + garlic_hip_last_error());
    for (size_t i = 0; i < m; i++) {
        if (status) (*status)[i] = code[i];
        if (!code[i]) memcpy(&out[i], &gk[i], sizeof out[i]);
    }
    return out;
}

// ---- ROH calls
std::vector<ROHData *> *initROHData(IndData *indData)
{
    auto *v = new std::vector<ROHData *>;
    for (int ind = 0; ind < indData->nind; ind++) v->push_back(new ROHData);
    return v;
}

void releaseROHData(std::vector<ROHData *> *rohDataByInd)
{
    if (!rohDataByInd) return;
    for (ROHData *r : *rohDataByInd) delete r;
    rohDataByInd->clear();
    delete rohDataByInd;
}

ROHLength *initROHLength(int size, std::string pop)
{
    ROHLength *r = new ROHLength;
    r->pop = pop;
    r->length = new double[size > 0 ? size : 1];
    r->size = size;
    return r;
}

void releaseROHLength(ROHLength *rohLength)
{
    if (!rohLength) return;
    delete[] rohLength->length;
    delete rohLength;
}

// garlic-roh.cpp:574-648
void writeROHData(const std::string &outfile, std::vector<ROHData *> *rohDataByInd, std::vector<MapData *> *mapDataByChr,
                  const std::vector<double> &bounds, const std::string &popName, const std::string &version, bool CM)
{
    static const char *colors[9] = {"228,26,28", "77,175,74", "55,126,184", "152,78,163", "255,127,0",
                                    "255,255,51", "166,86,40", "247,129,191", "153,153,153"};
    std::ofstream out(outfile.c_str());
    if (out.fail()) fail("Failed to open " + outfile);
    for (size_t ind = 0; ind < rohDataByInd->size(); ind++) {
        const ROHData *rohData = rohDataByInd->at(ind);
        out << "track name=\"Ind: " + rohData->indID + " Pop:" + popName + " ROH\" description=\"Ind: " + rohData->indID +
                   " Pop:" + popName + " ROH from GARLIC v" + version + "\" visibility=2 itemRgb=\"On\"\n";
        for (size_t roh = 0; roh < rohData->chr.size(); roh++) {
            const double size = rohData->length[roh];
            // the first boundary the size lies below names the class (A, B, ..); past the last one: the next letter
            size_t i = 0;
            while (i < bounds.size() && !(size < bounds[i])) i++;
            const char sizeClass = (char)('A' + i);
            const char *color = colors[i <= 8 ? i : 8];
            std::string chr = mapDataByChr->at((size_t)rohData->chr[roh])->chr;
            if (chr[0] != 'c' && chr[0] != 'C') chr = "chr" + chr;
            out << chr << "\t" << int(rohData->start[roh]) << "\t" << int(rohData->stop[roh]) << "\t" << sizeClass << "\t";
            if (CM) out << size;
            else out << int(size);
            out << "\t.\t0\t0\t" << color << std::endl;
        }
    }
    out.close();
    std::cerr << "ROH calls: " << outfile << "\n";
}

// assembleROHWindows, garlic-roh.cpp:409-545: the device returns every segment as (individual, chromosome, first SNP,
// last SNP) in the reference's order; positions, sizes and the pooled length list are filled in here as :470-520 do
// (size in cM from geneticPos with CM, else stop - start + 1 in bp; start / stop are the SNPs' physical positions)
std::vector<ROHData *> *LodEngine::assembleROHWindows(IndData *indData, double lodScoreCutoff, ROHLength **rohLength,
                                                      int winSize, double error, int MAX_GAP, double OVERLAP_FRAC, bool CM,
                                                      bool weighted, int M, double mu)
{
    if (!indData || indData->nind != impl->nind) fail("assembleROHWindows: IndData does not match the panel");
    std::cerr << "Assembling ROH windows on the device (winsize " << winSize << ").\n";
    const size_t ns = impl->shards.size();
    std::vector<std::vector<garlic_roh_segment>> segs(ns);
    std::vector<std::string> errors(ns);
    std::vector<std::thread> th;
    for (size_t k = 0; k < ns; k++)
        th.emplace_back([&, k] {
            auto &s = impl->shards[k];
            int64_t n = 0;
            // a first guess of room for 64 segments per individual; the call says how many there are
            segs[k].resize((size_t)std::max<int64_t>(1024, 64 * (int64_t)s.nind));
            for (int attempt = 0; attempt < 2; attempt++) {
                if (garlic_roh_segments(s.panel, winSize, error, MAX_GAP, impl->use_gl, weighted, M, mu, lodScoreCutoff, OVERLAP_FRAC,
                                        segs[k].data(), (int64_t)segs[k].size(), &n) != GARLIC_OK) {
                    errors[k] = garlic_hip_last_error();
                    return;
                }
                if (n <= (int64_t)segs[k].size()) break;
                segs[k].resize((size_t)n);
            }
            segs[k].resize((size_t)n);
        });
    for (auto &t : th) t.join();
    for (auto &e : errors)
        if (!e.empty()) fail("garlic_roh_segments: " + e);
    std::vector<ROHData *> *rohDataByInd = initROHData(indData);
    std::vector<double> lengths;
    for (size_t k = 0; k < ns; k++) {           // shards hold the individuals in order, each list is sorted by individual
        const auto &s = impl->shards[k];
        for (const garlic_roh_segment &g : segs[k]) {
            const MapData *map = impl->maps->at((size_t)g.chr);
            ROHData *r = rohDataByInd->at((size_t)(s.ind_begin + g.ind));
            const int winStart = map->physicalPos[g.start], winStop = map->physicalPos[g.stop];
            const double size = CM ? map->geneticPos[g.stop] - map->geneticPos[g.start] : winStop - winStart + 1;
            lengths.push_back(size);
            r->length.push_back(size);
            r->chr.push_back(g.chr);
            r->start.push_back(winStart);
            r->stop.push_back(winStop);
        }
    }
    for (int ind = 0; ind < indData->nind; ind++) rohDataByInd->at((size_t)ind)->indID = indData->indID[ind];
    ROHLength *rl = initROHLength((int)lengths.size(), indData->pop);
    for (size_t i = 0; i < lengths.size(); i++) rl->length[i] = lengths[i];
    if (rohLength) *rohLength = rl;
    else releaseROHLength(rl);
    return rohDataByInd;
}

// selectSizeClasses, garlic-roh.cpp:935-1003: the initial guess on the host (one pass over doubles it already holds), the
// EM fit on the first device, ordering, log lines and boundaries on the host (size_classes.hpp)
std::vector<double> LodEngine::selectSizeClasses(const ROHLength *rohLength, int nclust)
{
    static_assert(GMM_MAX_K == GARLIC_GMM_MAX_K, "one K limit");
    if (!rohLength || rohLength->size < 1) fail("selectSizeClasses: no ROH segments to fit size classes to");
    if (nclust < 1 || nclust > GMM_MAX_K) fail("selectSizeClasses: " + std::to_string(nclust) + " size classes (1 to " + std::to_string(GMM_MAX_K) + ")");
    const int64_t n = (int64_t)rohLength->size;
    double a[GMM_MAX_K], mean[GMM_MAX_K], var[GMM_MAX_K];
    sizeClassInit(rohLength->length, n, nclust, a, mean, var);
    garlic_gmm g;
    if (garlic_gmm_fit(impl->shards[0].ctx, rohLength->length, n, GARLIC_HOST, nclust, a, mean, var, GMM_MAX_ITER, GMM_PRECISION, &g) != GARLIC_OK)
        fail(std::string("garlic_gmm_fit: ") + garlic_hip_last_error());
    std::cerr << "GMM with " << nclust << " Gaussians on the device: " << g.iterations << " EM iterations"
              << (g.converged ? "" : " (not converged)") << ", log likelihood " << g.loglik << "\n";
    std::cerr << sizeClassLines(g.a, g.mean, g.var, nclust);
    std::vector<double> bounds;
    std::string why;
    if (!sizeClassBounds(g.a, g.mean, g.var, nclust, &bounds, &why)) fail(why);
    return bounds;
}

// The callers that sweep window sizes on one data set -- exploreWinsizes (garlic-roh.cpp:726-751), selectWinsize
// (:798-837), selectWinsizeFromList (:881-920) -- through garlic_lod_feed_multi (unweighted --error scores) or, when the
// engine holds per-genotype likelihoods (USE_GL; the sweeps run with --tgls as with --error), garlic_lod_feed_multi_tgls.  The
// thinning step of a size is the size itself (convertWinData2DoubleData(.., winsize), :735,743,817,900) unless `steps` says otherwise.
std::vector<DoubleData *> LodEngine::lodFeedMulti(const std::vector<int> &winsizes, double error, int MAX_GAP,
                                                  const std::vector<int> *steps, const std::vector<int> *kdeSubsample)
{
    const int nchr = (int)impl->chr_nloci.size();
    const size_t ns = impl->shards.size(), nw = winsizes.size();
    if (nw == 0) return {};
    if (steps && steps->size() != nw) fail("lodFeedMulti: one thinning step per window size");
    std::cerr << "Calculating LOD scores with winsizes";
    for (int W : winsizes) std::cerr << " " << W;
    std::cerr << " (thinned on the device).\n";
    const bool subset = kdeSubsample && !kdeSubsample->empty();
    if (subset)
        for (size_t i = 1; i < kdeSubsample->size(); i++)
            if ((*kdeSubsample)[i] <= (*kdeSubsample)[i - 1]) fail("KDE subsample must be in increasing order");
    const bool sorted = g_options.feed_sorted;
    std::vector<int32_t> W32(winsizes.begin(), winsizes.end()), S32(nw);
    for (size_t i = 0; i < nw; i++) S32[i] = steps ? (*steps)[i] : winsizes[i];
    // feeds[shard][size], per_chr[shard][size * nchr + c]
    std::vector<std::vector<std::vector<double>>> feeds(ns, std::vector<std::vector<double>>(nw));
    std::vector<std::vector<int64_t>> per_chr(ns, std::vector<int64_t>(nw * (size_t)nchr, 0));
    std::vector<std::string> errors(ns);
    std::vector<std::thread> th;
    for (size_t k = 0; k < ns; k++)
        th.emplace_back([&, k] {
            auto &s = impl->shards[k];
            std::vector<int32_t> mine;
            if (subset) {
                for (int g : *kdeSubsample)
                    if (g >= s.ind_begin && g < s.ind_begin + s.nind) mine.push_back(g - s.ind_begin);
                if (mine.empty()) return;      // no listed individual lives here
            }
            const int64_t rows = subset ? (int64_t)mine.size() : s.nind;
            std::vector<double *> ptrs(nw);
            std::vector<int64_t> cap(nw, 0), n(nw, 0);
            for (size_t i = 0; i < nw; i++) {
                for (int c = 0; c < nchr; c++) cap[i] += ((int64_t)impl->chr_nloci[c] + S32[i] - 1) / S32[i] * rows;
                feeds[k][i].resize((size_t)std::max<int64_t>(cap[i], 1));
                ptrs[i] = feeds[k][i].data();
            }
            int rc = garlic_panel_set_feed_order(s.panel, sorted ? GARLIC_FEED_ORDER_SORTED : GARLIC_FEED_ORDER_REFERENCE);
            if (rc == GARLIC_OK)
                rc = impl->use_gl
                               ? garlic_lod_feed_multi_tgls(s.panel, W32.data(), S32.data(), (int32_t)nw, MAX_GAP, subset ? mine.data() : nullptr,
                                                            (int32_t)mine.size(), ptrs.data(), cap.data(), n.data(), per_chr[k].data())
                               : garlic_lod_feed_multi(s.panel, W32.data(), S32.data(), (int32_t)nw, error, MAX_GAP, subset ? mine.data() : nullptr,
                                                       (int32_t)mine.size(), ptrs.data(), cap.data(), n.data(), per_chr[k].data());
            if (rc != GARLIC_OK)
                errors[k] = garlic_hip_last_error();
            else
                for (size_t i = 0; i < nw; i++) feeds[k][i].resize((size_t)n[i]);
        });
    for (auto &t : th) t.join();
    for (auto &e : errors)
        if (!e.empty()) fail(std::string(impl->use_gl ? "garlic_lod_feed_multi_tgls: " : "garlic_lod_feed_multi: ") + e);
    // merge per size in the reference's order: chromosome -> individual (= shard order) -> locus
    std::vector<DoubleData *> out(nw, nullptr);
    for (size_t i = 0; i < nw; i++) {
        int64_t total = 0;
        for (size_t k = 0; k < ns; k++) total += (int64_t)feeds[k][i].size();
        if (total > 0x7fffffff) fail("KDE feed has more than 2^31 values: DoubleData::size is an int");
        DoubleData *d = new DoubleData;
        d->size = (int)total;
        d->data = new double[total > 0 ? total : 1];
        out[i] = d;
        if (sorted) {
            std::vector<std::vector<double>> of_size(ns);
            for (size_t k = 0; k < ns; k++) of_size[k].swap(feeds[k][i]);
            mergeShardFeeds(of_size, d->data);
            continue;
        }
        std::vector<int64_t> off(ns, 0);
        int64_t o = 0;
        for (int c = 0; c < nchr; c++)
            for (size_t k = 0; k < ns; k++) {
                const int64_t m = feeds[k][i].empty() ? 0 : per_chr[k][i * (size_t)nchr + c];
                memcpy(d->data + o, feeds[k][i].data() + off[k], sizeof(double) * (size_t)m);
                o += m;
                off[k] += m;
            }
    }
    return out;
}

std::vector<LDData *> *LodEngine::ldWeights(int winsize, const std::vector<int> &subsample, bool want_host,
                                            bool phased)
{
    if (phased && !impl->have_phase) fail("--phased: the genotypes were loaded without phase (HapData::firstCopy)");
    const int32_t ph = phased ? 1 : 0;
    std::cerr << "Calculating LD weights with winsize " << winsize << ".\n";
    int64_t nloci = 0;
    for (int n : impl->chr_nloci) nloci += n;
    // every shard counts over its own individuals; the counts are integers, so their sum over
    // shards is exact whatever the order (with one process per GPU this is an RCCL all-reduce)
    std::vector<int32_t> loc((size_t)nloci * 2, 0), pair((size_t)nloci * winsize * 2, 0);
    const size_t ns = impl->shards.size();
    std::vector<std::string> errors(ns);
    std::mutex sum_lock;
    auto count_shard = [&](size_t k) {   // one host thread per GPU, as for the scores
        auto &s = impl->shards[k];
        std::vector<int32_t> sub;
        for (int g : subsample)
            if (g >= s.ind_begin && g < s.ind_begin + s.nind) sub.push_back(g - s.ind_begin);
        std::vector<int32_t> l1, p1;
        std::vector<int32_t> &lo = ns == 1 ? loc : l1, &pa = ns == 1 ? pair : p1;
        lo.resize(loc.size()); pa.resize(pair.size());
        // subsample given: the shard's part of it, possibly empty (a non-NULL pointer with n_sub = 0 means
        // "none of them": pair counts zero, the homFreq counts still over every individual)
        static const int32_t no_index = 0;
        const int32_t *sub_ptr = subsample.empty() ? nullptr : (sub.empty() ? &no_index : sub.data());
        if (garlic_ld_counts(s.panel, winsize, ph, sub_ptr, (int32_t)sub.size(), lo.data(), pa.data(), GARLIC_HOST) !=
            GARLIC_OK) {
            errors[k] = garlic_hip_last_error();
            return;
        }
        if (ns == 1) return;
        std::lock_guard<std::mutex> hold(sum_lock);
        for (size_t i = 0; i < loc.size(); i++) loc[i] += lo[i];
        for (size_t i = 0; i < pair.size(); i++) pair[i] += pa[i];
    };
    {
        std::vector<std::thread> th;
        for (size_t k = 0; k < ns; k++) th.emplace_back(count_shard, k);
        for (auto &t : th) t.join();
    }
    for (auto &e : errors)
        if (!e.empty()) fail("garlic_ld_counts: " + e);
    std::vector<double> flat;
    if (want_host) flat.resize((size_t)nloci * winsize);
    {
        std::vector<std::thread> th;
        for (size_t k = 0; k < ns; k++)
            th.emplace_back([&, k] {
                if (garlic_ld_finish(impl->shards[k].panel, winsize, ph, loc.data(), pair.data(),
                                     (want_host && k == 0) ? flat.data() : nullptr, GARLIC_HOST) != GARLIC_OK)
                    errors[k] = garlic_hip_last_error();
            });
        for (auto &t : th) t.join();
    }
    for (auto &e : errors)
        if (!e.empty()) fail("garlic_ld_finish: " + e);
    if (!want_host) return nullptr;
    std::vector<LDData *> *out = new std::vector<LDData *>;
    int64_t o = 0;
    for (int n : impl->chr_nloci) {
        LDData *d = initLDData(n, winsize);
        for (int l = 0; l < n; l++, o++) memcpy(d->LD[l], &flat[(size_t)o * winsize], sizeof(double) * winsize);
        out->push_back(d);
    }
    return out;
}

bool LodEngine::ldWeightsMulti(const std::vector<int> &sizes, const std::vector<int> &subsample, bool phased)
{
    if (sizes.empty()) return true;
    if (phased && !impl->have_phase) fail("--phased: the genotypes were loaded without phase (HapData::firstCopy)");
    const int32_t ph = phased ? 1 : 0;
    std::cerr << "Calculating LD weights with winsizes";
    for (int W : sizes) std::cerr << " " << W;
    std::cerr << " (one LD computation for " << sizes.size() << " window sizes).\n";
    const std::vector<int32_t> ws(sizes.begin(), sizes.end());
    const int32_t wmax = *std::max_element(ws.begin(), ws.end());
    int64_t nloci = 0;
    for (int n : impl->chr_nloci) nloci += n;
    const size_t ns = impl->shards.size();
    std::vector<std::string> errors(ns);
    std::vector<int> codes(ns, GARLIC_OK);
    auto shard_sub = [&](size_t k, std::vector<int32_t> &sub) -> const int32_t * {
        auto &s = impl->shards[k];
        for (int g : subsample)
            if (g >= s.ind_begin && g < s.ind_begin + s.nind) sub.push_back(g - s.ind_begin);
        static const int32_t no_index = 0;
        return subsample.empty() ? nullptr : (sub.empty() ? &no_index : sub.data());
    };
    if (ns == 1) {      // every individual's counts are on the one device: pair stage and shared sums in one call
        std::vector<int32_t> sub;
        const int32_t *sub_ptr = shard_sub(0, sub);
        const int rc = garlic_panel_compute_ld_multi(impl->shards[0].panel, ws.data(), (int32_t)ws.size(), ph, sub_ptr, (int32_t)sub.size(),
                                                     nullptr, GARLIC_HOST);
        if (rc == GARLIC_ERR_NOMEM) return false;
        if (rc != GARLIC_OK) fail(std::string("garlic_panel_compute_ld_multi: ") + garlic_hip_last_error());
        return true;
    }
    // the integer counts at the largest size, summed over the shards, serve every size
    std::vector<int32_t> loc((size_t)nloci * 2, 0), pair((size_t)nloci * wmax * 2, 0);
    std::mutex sum_lock;
    {
        std::vector<std::thread> th;
        for (size_t k = 0; k < ns; k++)
            th.emplace_back([&, k] {
                std::vector<int32_t> sub, lo(loc.size()), pa(pair.size());
                const int32_t *sub_ptr = shard_sub(k, sub);
                if (garlic_ld_counts(impl->shards[k].panel, wmax, ph, sub_ptr, (int32_t)sub.size(), lo.data(), pa.data(), GARLIC_HOST) !=
                    GARLIC_OK) {
                    errors[k] = garlic_hip_last_error();
                    return;
                }
                std::lock_guard<std::mutex> hold(sum_lock);
                for (size_t i = 0; i < loc.size(); i++) loc[i] += lo[i];
                for (size_t i = 0; i < pair.size(); i++) pair[i] += pa[i];
            });
        for (auto &t : th) t.join();
    }
    for (auto &e : errors)
        if (!e.empty()) fail("garlic_ld_counts: " + e);
    {
        std::vector<std::thread> th;
        for (size_t k = 0; k < ns; k++)
            th.emplace_back([&, k] {
                codes[k] = garlic_ld_finish_multi(impl->shards[k].panel, ws.data(), (int32_t)ws.size(), ph, loc.data(), pair.data(), nullptr,
                                                  GARLIC_HOST);
                if (codes[k] != GARLIC_OK) errors[k] = garlic_hip_last_error();
            });
        for (auto &t : th) t.join();
    }
    bool nomem = false;
    for (size_t k = 0; k < ns; k++) {
        if (codes[k] == GARLIC_ERR_NOMEM) nomem = true;
        else if (codes[k] != GARLIC_OK) fail("garlic_ld_finish_multi: " + errors[k]);
    }
    return !nomem;
}

std::vector<WinData *> *LodEngine::run(bool weighted, int winsize, double error, int MAX_GAP, int M, double mu)
{
    std::cerr << "Calculating LOD scores with winsize " << winsize << ".\n";
    std::vector<WinData *> *win = initWinData(impl->maps, impl->nind);
    const int nchr = (int)impl->chr_nloci.size();
    std::vector<std::string> errors(impl->shards.size());
    std::vector<std::thread> th;
    for (size_t k = 0; k < impl->shards.size(); k++) {
        th.emplace_back([&, k] { // one host thread per GPU; no collective, just a gather of rows
            auto &s = impl->shards[k];
            std::vector<int64_t> base(nchr), pitch(nchr);
            int64_t total = 0;
            // individuals come back in chunks so the host never stages more than ~1 GiB
            int64_t per_ind = 0;
            for (int c = 0; c < nchr; c++) per_ind += impl->chr_nloci[c];
            const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(s.nind, ((int64_t)1 << 27) / std::max<int64_t>(1, per_ind)));
            std::vector<double> buf;
            for (int i0 = 0; i0 < s.nind; i0 += chunk) {
                const int n = std::min(chunk, s.nind - i0);
                if (garlic_lod_out_layout(s.panel, 1, n, base.data(), pitch.data(), &total) != GARLIC_OK ||
                    (buf.resize((size_t)total), false) ||
                    (weighted ? garlic_wlod_windows(s.panel, winsize, error, MAX_GAP, impl->use_gl, M, mu, i0, n, 1,
                                                    buf.data(), GARLIC_HOST)
                              : garlic_lod_windows(s.panel, winsize, error, MAX_GAP, impl->use_gl, i0, n, 1,
                                                   buf.data(), GARLIC_HOST)) != GARLIC_OK) {
                    errors[k] = garlic_hip_last_error();
                    return;
                }
                for (int c = 0; c < nchr; c++)
                    for (int i = 0; i < n; i++)
                        memcpy(win->at(c)->data[s.ind_begin + i0 + i], &buf[base[c] + (int64_t)i * pitch[c]],
                               sizeof(double) * impl->chr_nloci[c]);
            }
        });
    }
    for (auto &t : th) t.join();
    for (auto &e : errors)
        if (!e.empty()) { releaseWinData(win); fail("garlic_lod_windows: " + e); }
    return win;
}

std::vector<int> drawLdSubsample(int nind, int ldSubsample, unsigned long long seed)
{
    std::vector<int> out;
    if (ldSubsample >= nind || ldSubsample <= 0) return out;   // all (garlic-data.cpp:351-356)
    // selection sampling: ldSubsample of nind, each subset equally likely, indices ascending --
    // the contract of gsl_ran_choose; the stream itself cannot match a time-seeded GSL generator
    std::mt19937_64 rng(seed ? seed : (unsigned long long)time(nullptr));
    int need = ldSubsample;
    for (int i = 0; i < nind && need > 0; i++) {
        const double u = std::generate_canonical<double, 53>(rng);
        if ((double)(nind - i) * u < (double)need) { out.push_back(i); need--; }
    }
    return out;
}

std::vector<int> drawKdeSubsample(int nind, int kdeSubsample, unsigned long long seed)
{   // garlic-data.cpp:2081-2096: everyone when the subsample is not smaller than the panel (here: empty list)
    return drawLdSubsample(nind, kdeSubsample, seed ? seed ^ 0x6B64655F73756273ull : 0);
}

std::vector<LDData *> *calcLDData(std::vector<HapData *> *haps, std::vector<FreqData *> *freqs,
                                  std::vector<MapData *> *maps, std::vector<GenoFreqData *> * /*genoFreq*/,
                                  centromere *centro, int winsize, int /*MAX_GAP*/, bool PHASED,
                                  int /*numThreads*/, int ldSubsample)
{
    LodEngine engine(haps, freqs, maps, nullptr, centro, false, g_options.devices);
    return engine.ldWeights(winsize, drawLdSubsample(haps->at(0)->nind, ldSubsample, g_options.ld_seed), true,
                            PHASED);
}

std::vector<WinData *> *calcLODWindows(std::vector<HapData *> *haps, std::vector<FreqData *> *freqs,
                                       std::vector<MapData *> *maps, std::vector<GenoLikeData *> *gls,
                                       centromere *centro, int winsize, double error, int MAX_GAP, bool USE_GL)
{
    // GLDataByChr may be an uninitialised pointer when !USE_GL (garlic-roh.cpp:713,720): never touched then
    LodEngine engine(haps, freqs, maps, USE_GL ? gls : nullptr, centro, USE_GL, g_options.devices);
    return engine.lodWindows(winsize, error, MAX_GAP);
}

std::vector<WinData *> *calcwLODWindows(std::vector<HapData *> *haps, std::vector<FreqData *> *freqs,
                                        std::vector<MapData *> *maps, std::vector<GenoLikeData *> *gls,
                                        std::vector<LDData *> *lds, centromere *centro, int winsize, double error,
                                        int MAX_GAP, bool USE_GL, int M, double mu, int /*numThreads*/)
{
    // numThreads only partitions loci in the reference (garlic-data.cpp:538); the result does not depend on it
    LodEngine engine(haps, freqs, maps, USE_GL ? gls : nullptr, centro, USE_GL, g_options.devices);
    return engine.wlodWindows(lds, winsize, error, MAX_GAP, M, mu);
}

// ------------------------------------------------------------------------- consumers
DoubleData *convertWinData2DoubleData(std::vector<WinData *> *wins, int step)
{
    // garlic-data.cpp:2026-2069: chr -> ind -> every step-th locus; MISSING and NaN are dropped
    int size = 0;
    for (auto w : *wins)
        for (int i = 0; i < w->nind; i++)
            for (int l = 0; l < w->nloci; l += step) {
                const double x = w->data[i][l];
                if (x != MISSING && !std::isnan(x)) size++;
            }
    DoubleData *d = new DoubleData;
    d->size = size;
    d->data = new double[size > 0 ? size : 1];
    int k = 0;
    for (auto w : *wins)
        for (int i = 0; i < w->nind; i++)
            for (int l = 0; l < w->nloci; l += step) {
                const double x = w->data[i][l];
                if (x != MISSING && !std::isnan(x)) d->data[k++] = x;
            }
    return d;
}

DoubleData *convertSubsetWinData2DoubleData(std::vector<WinData *> *wins, const std::vector<int> &randInd, int step)
{
    // garlic-data.cpp:2071-2150 with the draw supplied: chr -> randInd[0..] -> every step-th locus
    int size = 0;
    for (auto w : *wins)
        for (int i : randInd) {
            if (i < 0 || i >= w->nind) { std::cerr << "ERROR: KDE subsample index " << i << " outside the panel.\n"; throw 0; }
            for (int l = 0; l < w->nloci; l += step) {
                const double x = w->data[i][l];
                if (x != MISSING && !std::isnan(x)) size++;
            }
        }
    DoubleData *d = new DoubleData;
    d->size = size;
    d->data = new double[size > 0 ? size : 1];
    int k = 0;
    for (auto w : *wins)
        for (int i : randInd)
            for (int l = 0; l < w->nloci; l += step) {
                const double x = w->data[i][l];
                if (x != MISSING && !std::isnan(x)) d->data[k++] = x;
            }
    return d;
}

// one gzip member holding `text` (members may simply follow each other in a .gz file)
static std::string gzip_member(const std::string &text)
{
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, Z_DEFAULT_COMPRESSION, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) throw -1;
    std::string out;
    out.resize(deflateBound(&z, (uLong)text.size()) + 64);
    z.next_in = reinterpret_cast<Bytef *>(const_cast<char *>(text.data()));
    z.avail_in = (uInt)text.size();
    z.next_out = reinterpret_cast<Bytef *>(&out[0]);
    z.avail_out = (uInt)out.size();
    const int rc = deflate(&z, Z_FINISH);
    out.resize(out.size() - z.avail_out);
    deflateEnd(&z);
    if (rc != Z_STREAM_END) throw -1;
    return out;
}

// The reference's text (garlic-data.cpp:1722-1745: one line per individual, "NA" for MISSING, operator<<'s six
// significant digits = printf's %g), written the way a GPU-sized panel needs it: the individuals' lines are formatted and
// compressed on all host cores, a few lines per gzip member, and appended in order (formatted through one
// ostringstream and one gz stream, 20 M values took 8 s).
void writeWinData(std::vector<WinData *> *wins, IndData *indData, std::vector<MapData *> *maps,
                  const std::string &outfile)
{
    const unsigned nthreads = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    for (size_t c = 0; c < maps->size(); c++) {
        const std::string path = outfile + "." + indData->pop + "." + maps->at(c)->chr + ".raw.lod.windows.gz";
        FILE *f = fopen(path.c_str(), "wb");
        if (!f) { std::cerr << "ERROR: Failed to open " << path << " for writing.\n"; throw -1; }
        const WinData *w = wins->at(c);
        // rows per member: ~4 MB of text each; a wave of members = one per thread
        const int per = std::max(1, (int)(((size_t)4 << 20) / ((size_t)std::max(1, w->nloci) * 8 + 1)));
        for (int i0 = 0; i0 < w->nind; i0 += per * (int)nthreads) {
            const int ntasks = std::min<int>((int)nthreads, (w->nind - i0 + per - 1) / per);
            std::vector<std::string> members((size_t)ntasks);
            std::vector<std::thread> pool;
            std::atomic<bool> failed{false};   // set by the compression threads
            for (int t = 0; t < ntasks; t++)
                pool.emplace_back([&, t]() {
                    std::string text;
                    text.reserve((size_t)per * ((size_t)w->nloci * 9 + 1));
                    char buf[40];
                    const int a = i0 + t * per, b = std::min(w->nind, a + per);
                    for (int i = a; i < b; i++) {
                        for (int l = 0; l < w->nloci; l++) {
                            if (w->data[i][l] == MISSING) text += "NA";               // garlic-data.cpp:1736
                            else text.append(buf, (size_t)snprintf(buf, sizeof buf, "%g", w->data[i][l]));
                            if (l < w->nloci - 1) text += ' ';
                        }
                        text += '\n';
                    }
                    try { members[(size_t)t] = gzip_member(text); } catch (...) { failed = true; }
                });
            for (auto &th : pool) th.join();
            if (failed) { fclose(f); std::cerr << "ERROR: Failed to compress " << path << "\n"; throw -1; }
            for (const std::string &m : members)
                if (fwrite(m.data(), 1, m.size(), f) != m.size()) { fclose(f); std::cerr << "ERROR: Failed to write " << path << "\n"; throw -1; }
        }
        if (w->nind == 0) { const std::string m = gzip_member(""); fwrite(m.data(), 1, m.size(), f); }
        fclose(f);
        std::cerr << "Wrote " << path << "\n";
    }
}

} // namespace garlic_host
