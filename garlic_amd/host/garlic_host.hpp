// Host-side mirror of the reference's Phase-I interface, on top of the C ABI (include/garlic_hip.h).
//
// The reference is a C++ program with no plugin layer: its boundary for this path is
//     calcLODWindows   src/garlic-roh.h:96-102
//     calcwLODWindows  src/garlic-roh.h:104-112
// and the structs those borrow (src/garlic-data.h:32-108).  This header re-declares structs of
// the same shape and the two entry points with the same argument meaning and error behaviour
// (`throw 0`, src/garlic-data.cpp:1619), so GARLIC's callers -- main, exploreWinsizes,
// selectWinsize, selectWinsizeFromList -- can be pointed here unchanged.
// Also: the ingest GARLIC does before the path (tped/tfam/tgls/freq/map/centromere) and the
// two consumers right after it (raw LOD writer, KDE feed flattening).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "bed_keep.hpp"
#include "feature_bed.hpp"
#include "feature_counts.hpp"
#include "feed_merge.hpp"
#include "kde_select.hpp"
#include "size_classes.hpp"

namespace garlic_host {

const int MISSING = -9999; // src/garlic-data.h:24

// A PLINK .bed/.bim/.fam triple (openBedFile): the .bed mapped read-only, the .bim columns per file row, and -- once
// loadBedData has run the census on a device -- every row's counted allele and the two integers of its frequency.  The
// genotypes stay in the file's codes (00 hom A1, 01 missing, 10 het, 11 hom A2; 4 per byte): the devices hold the image
// (garlic_bed), the host reads single values through genotypeAt when a consumer needs them.
struct BedFile {
    std::string path;
    int nind = 0;
    long long nrows = 0;
    size_t row_bytes = 0;                 // (nind + 3) / 4
    const unsigned char *rows = nullptr;  // row r at rows + r * row_bytes (behind the three magic bytes)
    void *map = nullptr;
    size_t map_bytes = 0;
    std::vector<std::string> chr, name;
    std::vector<double> gpos, ppos;
    std::vector<char> a1, a2;
    std::vector<unsigned char> counted;   // per row: 0 = A1, 1 = A2, 2 = none (every genotype missing)
    std::vector<int> counts;              // per row: nalleles, total
    struct Image { int device; void *ctx; void *bed; };
    std::vector<Image> images;            // the image on each device that has asked for it (bedImageOn)
    int refs = 0;                         // HapData that point here; the last one released closes the file
    // --keep / --pops (subsetBedFile): this is the file set that holds only the individuals `keep` of `parent` (indices into
    // its .fam, ascending).  nind / row_bytes / counted / counts are the subset's; `rows` points into own_rows, the subset
    // image fetched back from the first device (garlic_bed_get_rows); `images` holds the extracts (garlic_bed_extract, made on
    // the parent's contexts: ctx NULL here); the .bim columns are read through bim().  A subset holds one reference on its
    // parent.  On a parent, hold_images keeps the full image of a device after an extract was cut from it (--pops: one
    // upload serves every population); without it the full image of a device goes as soon as the extract exists.
    BedFile *parent = nullptr;
    std::vector<int> keep;
    std::vector<unsigned char> own_rows;
    bool hold_images = false;
    // VCF input (loadVcfData): nothing is mapped; `rows` points into own_rows, the image fetched back once after the parse on
    // the first device, and `order` into own_order, its order plane (one bit per genotype: the first allele is A2; row r at
    // order + r * order_row_bytes).  Further devices get both through garlic_bed_set_rows / garlic_bed_set_order_rows.  With
    // `phased` the plane is also the phase: HapData::firstCopy is firstCopyAt.
    const unsigned char *order = nullptr;
    size_t order_row_bytes = 0;           // (nind + 7) / 8
    std::vector<unsigned char> own_order;
    bool phased = false;
    long long skipped_non_snp = 0;        // --vcf-biallelic-snps-only: lines left out
    // TPED input (loadTPEDDataOnDevice): as VCF input, and a1 holds each line's counted allele (garlic_bed_set_rows_tped's
    // row_allele).  own_census: counts / counted are what the parse on the first device wrote (half-missing genotypes count
    // in total, which no rule recounts from the image); further devices get them through garlic_bed_set_census.
    bool own_census = false;
    char none_allele = '0';               // MapData::allele of a row without a counted allele: the missing character
    const BedFile *bim() const { return parent ? parent : this; }
};
// HapData::firstCopy of file row r, individual i of a VCF image: non-missing && (order bit == (counted == A2)); all true on a
// row without a counted allele
inline bool bedFirstCopy(const BedFile *b, size_t r, int i)
{
    const unsigned c = b->counted[r];
    if (c >= 2) return true;
    const unsigned code = (b->rows[r * b->row_bytes + (i >> 2)] >> (2 * (i & 3))) & 3u;
    const unsigned bit = (b->order[r * b->order_row_bytes + (i >> 3)] >> (i & 7)) & 1u;
    return code != 1u && bit == c;
}
// copies of the counted allele by counted[row] and PLINK code; -9 = missing
inline short bedGenotype(unsigned counted, unsigned code)
{
    static const short T[3][4] = {{2, -9, 1, 0}, {0, -9, 1, 2}, {-9, -9, -9, -9}};
    return T[counted][code];
}

struct HapData {           // src/garlic-data.h:32-38
    short **data;          // [locus][ind]: copies of the counted allele, -9 = missing
    int nind;
    int nloci;
    bool **firstCopy;      // --phased only (else NULL): the first allele of the pair is the counted one
    // Extension: rows straight from the genotype cache, 4 genotypes per byte (0/1/2, 3 = missing),
    // (nind + 3) / 4 bytes each; then `data` is NULL.  Everything in this adapter takes either form
    // (genotypeAt reads one value); the engine uploads the packed rows as they are.
    unsigned char **packed;
    // Extension: the firstCopy rows as the genotype cache stores them, 1 bit per genotype (bit i & 7 of byte i >> 3 is
    // individual i, the bits past the last individual 0), (nind + 7) / 8 bytes each; NULL unless the cache was loaded with
    // keepPacked.  `firstCopy` stays filled next to them for the host's readers; the engine uploads these rows as they are
    // (garlic_panel_set_phase_bits: an eighth of the bytes, no staging expansion).
    unsigned char **phaseBits;
    // Extension: the genotypes are rows of a .bed file (loadBedData): `data` and `packed` are NULL, locus l is file row
    // bedRow[l] of `bed`.  The site filters only edit bedRow; the engine fills its panels from the image on the device
    // (garlic_panel_set_genotypes_bed).
    BedFile *bed;
    long long *bedRow;
};
inline bool hasPhase(const HapData *h) { return h->firstCopy || h->phaseBits || (h->bed && h->bed->order && h->bed->phased); }
inline short genotypeAt(const HapData *h, int locus, int ind)
{
    if (h->data) return h->data[locus][ind];
    if (h->bed) {
        const long long r = h->bedRow[locus];
        return bedGenotype(h->bed->counted[(size_t)r], (h->bed->rows[(size_t)r * h->bed->row_bytes + (ind >> 2)] >> (2 * (ind & 3))) & 3u);
    }
    const unsigned code = (h->packed[locus][ind >> 2] >> (2 * (ind & 3))) & 3u;
    return code == 3u ? (short)-9 : (short)code;
}
struct MapData {           // src/garlic-data.h:51-60
    int *physicalPos;
    double *geneticPos;
    std::string *locusName;
    char *allele;          // the allele that is counted
    int nloci;
    std::string chr;
};
struct IndData {           // src/garlic-data.h:62-67
    std::string pop;
    std::string *indID;
    int nind;
};
struct FreqData {          // src/garlic-data.h:69-73
    double *freq;
    int nloci;
};
// A --tgls file whose likelihoods live on the devices only (loadTGLSFile): parsed from the text and dictionary-coded there
// (garlic_tgls), one object per device.  The first device's object holds every kept column -- it also answers how many
// distinct values a chromosome has -- a further device's object holds its shard's columns, read from the file when the engine
// first asks for it.  No per-genotype likelihood exists on the host.
struct TglsFile {
    std::string path;
    int glType = 0;               // GARLIC_GL_GQ / _GL / _PL
    int fileInd = 0;              // sample columns of a line
    std::vector<int> cols;        // the kept columns of a line, in the panel's order of individuals
    long long nrows = 0;          // lines read: the loci before any site filter
    int refs = 0;                 // GenoLikeData that point here
    struct Object { int device, ind_begin, nind; void *ctx, *tgls; };
    std::vector<Object> objects;
    // a VCF as the source (loadVcfData with a VcfGlRequest): the FORMAT key read, the raw value of a called genotype without one (if any),
    // whether lines that are no biallelic SNPs are left out, and the header's sample names for messages
    std::string vcfKey;
    bool vcfHasMissing = false, vcfSnpsOnly = false;
    double vcfMissing = 0;
    std::vector<std::string> vcfSamples;
};
struct VcfGlRequest {
    std::string key, glType;      // the FORMAT key; GQ / GL / PL
    bool hasMissing = false;      // `missing` is the raw value of a called genotype without one (else such a line ends the run)
    double missing = 0;
    std::vector<int> devices;     // every device that will hold a shard (loadVcfData's own is added if it is not among them)
    TglsFile *file = nullptr;     // out: the filled objects, one per distinct device; vcfGlData takes it over
    bool overflow = false;        // out: a 65,537th distinct raw value was met; no objects, vcfGlData reads on the host
};
struct GenoLikeData {      // src/garlic-data.h:89-95
    double **data;         // [locus][ind]: per-genotype error probability
    int nind;
    int nloci;
    // Extension (readTGLSData with compact = true): the same values dictionary-coded, one byte per
    // genotype -- codes[locus][ind] indexes values[0 .. nvalues) -- and `data` NULL.  GQ / PL / GL
    // files hold a few dozen distinct values; the engine uploads the codes as they are.
    // A chromosome with more than 256 distinct values (GL / PL columns of printed numbers) has codes16
    // instead, two bytes per genotype and up to 65,536 values; one with more than that has `data` and
    // no table.  Exactly one of data / codes / codes16 is set.
    unsigned char **codes;
    double *values;
    int nvalues;
    unsigned short **codes16;
    // Extension (loadTGLSFile): the likelihoods are rows of a file held on the devices: data, codes and codes16 are NULL,
    // locus l is row tglsRow[l] of `tgls`, nvalues the number of distinct converted values the chromosome had when it was
    // read.  The site filters only edit tglsRow; the engine fills its panels device to device (garlic_panel_set_gl_tgls).
    // likelihoodAt has nothing to read here.
    TglsFile *tgls;
    long long *tglsRow;
};
inline double likelihoodAt(const GenoLikeData *g, int locus, int ind)
{
    if (g->data) return g->data[locus][ind];
    return g->values[g->codes16 ? g->codes16[locus][ind] : g->codes[locus][ind]];
}
// "one-byte codes", "16-bit codes" or "doubles": how a chromosome's likelihoods are held
inline const char *likelihoodForm(const GenoLikeData *g)
{
    if (g->tgls) return g->nvalues > 256 ? "16-bit codes" : "one-byte codes";      // what the host reader's counts decide
    return g->data ? "doubles" : g->codes16 ? "16-bit codes" : "one-byte codes";
}
struct LDData {            // src/garlic-data.h:103-108
    double **LD;           // [locus][winsize]
    int nloci;
    int winsize;
};
struct GenoFreqData {      // src/garlic-data.h:75-79
    double *homFreq;       // fraction of homozygous genotypes among the non-missing, per locus
    int nloci;
};
struct WinData {           // src/garlic-data.h:81-87
    double **data;         // [ind][locus], MISSING where no score
    int nind;
    int nloci;
};
struct DoubleData {        // src/garlic-data.h:97-101
    double *data;
    int size;
};

// src/garlic-centromeres.h: only centromereStart/End are used on the path (garlic-roh.cpp:36-37)
class centromere {
public:
    centromere() {}
    // arg: hg18 | hg19 | hg38 | none ; file: custom "chr start end" table (garlic-centromeres.cpp:64)
    centromere(const std::string &arg, const std::string &file, const std::string &defaultFileName);
    int centromereStart(const std::string &chr);
    int centromereEnd(const std::string &chr);
    void readCustomCentromeres(const std::string &filename);
    void set(const std::string &chr, int start, int end);

private:
    std::map<std::string, int> gapStart, gapEnd;
    std::map<std::string, int> warned;
};

std::string checkChrName(std::string chr); // "1" -> "chr1" (garlic-data.cpp:1886-1891)

// ---- allocation helpers with the reference's semantics
HapData *initHapData(unsigned int nind, unsigned int nloci, bool PHASED = false);   // garlic-data.cpp:1749
void releaseHapData(HapData *d);
void releaseHapData(std::vector<HapData *> *v);
MapData *initMapData(int nloci);
void releaseMapData(MapData *d);
void releaseMapData(std::vector<MapData *> *v);
FreqData *initFreqData(int nloci);
void releaseFreqData(FreqData *d);
void releaseFreqData(std::vector<FreqData *> *v);
GenoLikeData *initGLData(unsigned int nind, unsigned int nloci);
void releaseGLData(GenoLikeData *d);
void releaseGLData(std::vector<GenoLikeData *> *v);
LDData *initLDData(int nloci, int winsize);
void releaseLDData(LDData *d);
void releaseLDData(std::vector<LDData *> *v);
std::vector<GenoFreqData *> *calculateGenoFreq(std::vector<HapData *> *hapDataByChr);   // garlic-data.cpp:648
void releaseGenoFreq(std::vector<GenoFreqData *> *v);
WinData *initWinData(unsigned int nind, unsigned int nloci);          // throws 0 on empty shapes
std::vector<WinData *> *initWinData(std::vector<MapData *> *mapDataByChr, int nind);
void releaseWinData(WinData *d);
void releaseWinData(std::vector<WinData *> *v);
void releaseDoubleData(DoubleData *d);
void releaseIndData(IndData *d);

// ---- ingest (what main does before the path, src/garlic-main.cpp:216-279)
void loadTPEDData(const std::string &tpedfile, int &numLoci, int &numInd,
                  std::vector<HapData *> **hapDataByChr, std::vector<MapData *> **mapDataByChr,
                  std::vector<FreqData *> **freqDataByChr, char TPED_MISSING,
                  bool PHASED = false, int nresample = 0,
                  unsigned long long resampleSeed = 0);                          // garlic-data.cpp:10
// nresample > 0 (--resample, garlic-data.cpp:142-148): binomial resampling of every frequency, one mt19937
// stream in file order; resampleSeed 0 = time(NULL) as in the reference, else the stream GSL gives that seed
// PLINK input.  openBedFile reads the .fam (already the TFAM format) for the individual count and the .bim
// (chr snpid gpos ppos a1 a2; ppos is read as a double like the TPED's), maps the .bed and checks it: the magic bytes
// 6c 1b 01 (anything else, the individual-major 6c 1b 00 included, is refused), its size against rows x individuals, alleles
// of one character (GARLIC's alleles are single characters: a longer one is an error that names the line).  No GPU needed.
// anyPopulations (--keep / --pops): the .fam may carry several family IDs; the single-population check is then the caller's,
// over the individuals it keeps.
BedFile *openBedFile(const std::string &bedfile, const std::string &bimfile, const std::string &famfile, bool anyPopulations = false);
void closeBedFile(BedFile *b);
void releaseBedFile(BedFile *b);          // one reference less; the last one closes the file
// The (hap, map, freq) triple of the file set that holds only the individuals `keep` of `full` (ascending indices into its
// .fam): the full image goes to `device` (once per device and parent), garlic_bed_extract cuts the subset out of it, and
// census, frequencies, row map, shards and the host's view of the genotypes are the subset image's from there on.
// VCF input: the genotype text is parsed on `device` (garlic_bed_set_rows_vcf) into an image with an order plane; the host reads
// the header and the nine fixed columns (vcf_lines.hpp).  tfam "": family 0 and the header's names; otherwise its count must
// match.  samples: the header's names.  snpsOnly: lines whose REF / ALT is not one base are left out and counted
// (BedFile::skipped_non_snp) instead of ending the run.
// gl: the scalar FORMAT field gl->key of every sample column as likelihoods, from the same slabs (garlic_tgls_set_rows_vcf):
// the file is read once, and each slab goes once to every device of gl->devices -- into a device buffer of the loader's that
// both parse calls read with where = GARLIC_DEVICE -- where an object of all the samples' columns is filled.
void loadVcfData(const std::string &vcffile, bool phased, bool snpsOnly, std::vector<std::string> &samples, int &numLoci, int &numInd,
                 std::vector<HapData *> **hapDataByChr, std::vector<MapData *> **mapDataByChr, std::vector<FreqData *> **freqDataByChr,
                 int nresample, unsigned long long resampleSeed, int device, VcfGlRequest *gl = nullptr);
void loadBedSubset(BedFile *full, const std::vector<int> &keep, int &numLoci, int &numInd, std::vector<HapData *> **hapDataByChr,
                   std::vector<MapData *> **mapDataByChr, std::vector<FreqData *> **freqDataByChr, int nresample,
                   unsigned long long resampleSeed, int device);
// TPED input on the device: the same triple as loadTPEDData, the alleles parsed, coded and counted on `device`
// (garlic_bed_set_rows_tped, 64 MB slabs, .gz included) into an image with an order plane and the census of the parse; the host
// parses the four leading tokens of every line (tped_lines.hpp) and runs the --resample draws in file order from the census
// counts.  HapData::bed / ::bedRow instead of ::data; with PHASED the plane is the phase.  false: the device refused a line
// (an allele longer than one character, a column count that differs from the first line's, \v \f NUL) -- `refusal` names the
// first such line and its code, nothing is loaded, and the caller reads the file with loadTPEDData, whose leniency is unchanged.
bool loadTPEDDataOnDevice(const std::string &tpedfile, int &numLoci, int &numInd, std::vector<HapData *> **hapDataByChr,
                          std::vector<MapData *> **mapDataByChr, std::vector<FreqData *> **freqDataByChr, char TPED_MISSING, bool PHASED,
                          int nresample, unsigned long long resampleSeed, int device, std::string &refusal);
// IndData of the kept individuals of a .fam (readFam order): their single family ID is the population name; several among
// them fail like scanIndData3 ("Found multiple population IDs"), as does an individual ID twice
IndData *indDataOfKept(const std::vector<FamEntry> &fam, const std::vector<int> &keep, const std::string &famfile);
// The same (hap, map, freq) triple as loadTPEDData from a .bed/.bim/.fam: the rows go to `device` in chunks, the census there
// (garlic_bed_census) finds every row's counted allele -- the first non-missing allele of the TPED line the row stands for,
// on which a het reads "A1 A2" -- and the two integers of its frequency; the division is the host's, :141.  HapData::bed /
// ::bedRow instead of ::data.  A .bed carries no phase.
void loadBedData(const std::string &bedfile, const std::string &bimfile, const std::string &famfile, int &numLoci, int &numInd,
                 std::vector<HapData *> **hapDataByChr, std::vector<MapData *> **mapDataByChr,
                 std::vector<FreqData *> **freqDataByChr, int nresample = 0, unsigned long long resampleSeed = 0,
                 int device = 0);
void scanIndData3(const std::string &filename, int &numInd, std::string &popName);  // :1893
IndData *readIndData3(const std::string &filename, int numInd);                     // :1963
// The same file read through the device (TglsFile): the GenoLikeData per chromosome carry rows, not values.  cols / fileInd as
// for readTGLSData.  NULL when the file holds more than 65,536 distinct raw values: it needs readTGLSData (one line on stderr).
std::vector<GenoLikeData *> *loadTGLSFile(const std::string &filename, int expectedInd, std::vector<MapData *> *maps,
                                          const std::string &GL_TYPE, const std::vector<int> *cols, int fileInd, int device);
// The likelihoods of a VCF's own lines, asked of loadVcfData through its last argument (VcfGlRequest, above): vcfGlData
// turns what the load left in the request into the GenoLikeData per chromosome -- rows of the device objects, or, past 65,536
// distinct raw values, the file read once more on the host (vcf::parseGlValues per line; one line on stderr) into the forms of
// readTGLSData(compact = true).  A refused line ends the run naming file, line, sample and reason.
std::vector<GenoLikeData *> *vcfGlData(VcfGlRequest &gl, const std::string &vcffile, bool snpsOnly, const std::vector<std::string> &samples,
                                       std::vector<MapData *> *maps);
std::vector<GenoLikeData *> *readTGLSData(const std::string &filename, int expectedLoci, int expectedInd,
                                          std::vector<MapData *> *mapDataByChr,
                                          const std::string &GL_TYPE,
                                          bool compact = false,    // compact: ::codes / ::codes16 where the values allow, else ::data   // :1516
                                          // --keep: the file has fileInd + 4 fields per line and individual i is its column cols[i]
                                          const std::vector<int> *cols = nullptr, int fileInd = 0);
std::vector<FreqData *> *readFreqData(const std::string &freqfile,
                                      std::vector<MapData *> *mapDataByChr);        // :1345
void writeFreqData(const std::string &freqOutfile, std::vector<FreqData *> *freqDataByChr,
                   std::vector<MapData *> *mapDataByChr);                           // :1442
int filterMonomorphicSites(std::vector<MapData *> **mapDataByChr, std::vector<HapData *> **hapDataByChr,
                           std::vector<FreqData *> **freqDataByChr,
                           std::vector<GenoLikeData *> **GLDataByChr, bool USE_GL); // :871
// genetic map for --weighted: scaffold of 4 columns chr snpid gpos ppos (:760-844), out-of-bounds /
// centromere / monomorphic filter (:916-960, 1066-1098), linear interpolation (:702-757)
struct GenMapScaffold {
    std::vector<int> physicalPos;
    std::vector<double> geneticPos;
    std::string chr;
    int centroStart = 0, centroEnd = 0;
};
std::vector<GenMapScaffold *> *loadMapScaffold(const std::string &mapfile, centromere *centro);
void releaseGenMapScaffold(std::vector<GenMapScaffold *> *v);
int filterMonomorphicAndOOBSites(std::vector<MapData *> **mapDataByChr, std::vector<HapData *> **hapDataByChr,
                                 std::vector<FreqData *> **freqDataByChr,
                                 std::vector<GenoLikeData *> **GLDataByChr,
                                 std::vector<GenMapScaffold *> *scaffoldMapByChr, bool USE_GL);
int interpolateGeneticmap(std::vector<MapData *> *mapDataByChr, std::vector<GenMapScaffold *> *scaffoldMapByChr);

// Binary sidecar of what loadTPEDData produces: parsing a 10M x 10k TPED is ~400 GB
// of text and dwarfs the GPU time; the cache holds the same genotypes at 2 bits each (4 per byte,
// SNP-major; 3 = missing), positions, genetic positions, locus names, counted alleles and
// frequencies, and loads at memory speed; if the genotypes were read with PHASED, also
// HapData::firstCopy at 1 bit each.  Same (hap, map, freq) triple as the TPED path, so everything
// downstream is unchanged.  `throw 0` on I/O or format errors.
void writeGenotypeCache(const std::string &path, std::vector<HapData *> *hapDataByChr,
                        std::vector<MapData *> *mapDataByChr, std::vector<FreqData *> *freqDataByChr);
void loadGenotypeCache(const std::string &path, int &numLoci, int &numInd,
                       std::vector<HapData *> **hapDataByChr, std::vector<MapData *> **mapDataByChr,
                       std::vector<FreqData *> **freqDataByChr,
                       bool keepPacked = false);   // keepPacked: HapData::packed instead of ::data

// ---- ROH calls (src/garlic-roh.h:43-57)
struct ROHData {
    std::string indID;
    std::vector<int> chr;
    std::vector<double> start, stop, length;
};
struct ROHLength {
    std::string pop;
    double *length;
    double size;
};
std::vector<ROHData *> *initROHData(IndData *indData);                 // garlic-roh.cpp:387-397
void releaseROHData(std::vector<ROHData *> *rohDataByInd);             // :399-407
ROHLength *initROHLength(int size, std::string pop);                   // :547-554
void releaseROHLength(ROHLength *rohLength);                           // :556-560
// the .roh.bed file (garlic-roh.cpp:574-648): a track line per individual, then chr / start / stop / size class /
// size / colour per segment; bounds: the size-class boundaries (--size-bounds, or GARLIC's GMM stage)
void writeROHData(const std::string &outfile, std::vector<ROHData *> *rohDataByInd, std::vector<MapData *> *mapDataByChr,
                  const std::vector<double> &bounds, const std::string &popName, const std::string &version, bool CM);

// ---- feature counts per ROH class (the reference's src/count_features_in_roh.pl; feature_counts.hpp holds the readers and
// the writer, csrc/feature_kernels.hpp the counting).  loadFeatureCounts reads the feature file and the counting TPED /
// TFAM once; `throw 0` with a message that names file and line for what feature_counts.hpp refuses.
// featureCountsFromBed: the table of an existing .roh.bed on `device`, no panel needed.  The table has the script's
// columns A B C NONE per effect; with more than three classes A .. <last letter> NONE.
// loadFeatureCountsBed: the counting genotypes as a PLINK .bed / .bim / .fam instead (feature_bed.hpp): only the .bim and the
// .fam are read, into a row plan; the .bed is opened and its image becomes hom rows on the device where the count runs
// (garlic_feature_set_rows_bed).  The counting individuals are the .fam's, whatever --keep / --pops select of the run's.
FeatureData *loadFeatureCounts(const std::string &features, const std::string &tpedCounting, const std::string &tfamCounting);
FeatureData *loadFeatureCountsBed(const std::string &features, const std::string &bedCounting, const std::string &bimCounting,
                                  const std::string &famCounting);
void releaseFeatureCounts(FeatureData *data);
void featureCountsFromBed(FeatureData *data, const std::string &rohBed, const std::string &outfile, int device);

// ---- the path (drop-in signatures)
struct LodOptions {
    std::vector<int> devices;   // HIP device ordinals; empty = {0}.  Individuals shard contiguously.
    // --ld-subsample draw: the reference seeds its generator with time(NULL)
    // (garlic-data.cpp:346); 0 does the same here, any other value makes the draw repeatable.
    unsigned long long ld_seed = 0;
    // garlic_panel_set_tgls_term_budget for every shard's panel (dictionary-coded likelihoods): 0 the whole term matrix or
    // none, > 0 bytes (the matrix in slabs when it is larger), -1 whole if it fits, else slabs from the free memory
    long long tgls_term_bytes = 0;
    // LodEngine::lodFeed / lodFeedMulti return every feed ascending instead of in the reference's chromosome -> individual
    // -> locus order: the array nrd0's gsl_sort (garlic-kde.cpp:132) would make of it.  Sorted on the devices
    // (garlic_panel_set_feed_order on every shard's panel), the shards' arrays merged on the host (feed_merge.hpp).
    bool feed_sorted = false;
    // LodEngine::lodKde: the KDE of a sharded panel from one garlic_kde_part per shard (garlic_kde_parts) instead of the
    // shards' feeds merged on the host and one device's garlic_feed_kde.  Off by default until a node has measured it.
    bool kde_on_shards = false;
};
void setLodOptions(const LodOptions &o);

std::vector<WinData *> *calcLODWindows(std::vector<HapData *> *hapDataByChr,
                                       std::vector<FreqData *> *freqDataByChr,
                                       std::vector<MapData *> *mapDataByChr,
                                       std::vector<GenoLikeData *> *GLDataByChr, centromere *centro,
                                       int winsize, double error, int MAX_GAP, bool USE_GL);

std::vector<WinData *> *calcwLODWindows(std::vector<HapData *> *hapDataByChr,
                                        std::vector<FreqData *> *freqDataByChr,
                                        std::vector<MapData *> *mapDataByChr,
                                        std::vector<GenoLikeData *> *GLDataByChr,
                                        std::vector<LDData *> *ldDataByChr, centromere *centro,
                                        int winsize, double error, int MAX_GAP, bool USE_GL, int M,
                                        double mu, int numThreads);

// LD weights of wLOD (garlic-data.cpp:330-375).  Same arguments as the reference; the counts come
// from the device(s), so genoFreqDataByChr is not read (the device recomputes the same fractions
// from the genotypes) and numThreads is ignored.  PHASED (calcR2LD) needs HapData::firstCopy
// (loadTPEDData with PHASED), else `throw 0`.
std::vector<LDData *> *calcLDData(std::vector<HapData *> *hapDataByChr, std::vector<FreqData *> *freqDataByChr,
                                  std::vector<MapData *> *mapDataByChr,
                                  std::vector<GenoFreqData *> *genoFreqDataByChr, centromere *centro,
                                  int winsize, int MAX_GAP, bool PHASED, int numThreads, int ldSubsample);
// the individuals calcLDData would use: all when ldSubsample <= 0 or >= nind, else ldSubsample
// distinct indices in increasing order (what gsl_ran_choose returns, garlic-data.cpp:361-362)
std::vector<int> drawLdSubsample(int nind, int ldSubsample, unsigned long long seed);
// the individuals convertSubsetWinData2DoubleData would use (garlic-data.cpp:2081-2096; time-seeded
// there): empty = everyone (kdeSubsample <= 0 or >= nind), else kdeSubsample distinct indices, increasing
std::vector<int> drawKdeSubsample(int nind, int kdeSubsample, unsigned long long seed);

constexpr int KDE_MAX_FEEDS = 32;    // GARLIC_KDE_MAX_FEEDS: the most window sizes one LodEngine::lodKdeMulti call hands the library
// garlic_kde of include/garlic_hip.h on this side (the same layout): LodEngine::lodKde's result
struct KdeData {
    int64_t n;
    double h, sd, q25, q75, lo, hi;
    double x[KDE_POINTS], y[KDE_POINTS], raw[KDE_POINTS];
};

// A panel kept on the device(s) across window sizes (exploreWinsizes / selectWinsize call the
// path once per candidate winsize on the same data, garlic-roh.cpp:726-751,798-837,881-920).
class LodEngine {
public:
    LodEngine(std::vector<HapData *> *hapDataByChr, std::vector<FreqData *> *freqDataByChr,
              std::vector<MapData *> *mapDataByChr, std::vector<GenoLikeData *> *GLDataByChr,
              centromere *centro, bool USE_GL, const std::vector<int> &devices);
    ~LodEngine();
    std::vector<WinData *> *lodWindows(int winsize, double error, int MAX_GAP);
    std::vector<WinData *> *wlodWindows(std::vector<LDData *> *ldDataByChr, int winsize, double error,
                                        int MAX_GAP, int M, double mu);
    // LD weights for winsize from the resident genotypes (subsample: panel-wide individual indices,
    // empty = all); they stay installed on the device(s) for wlodWindowsResident.  Returns the
    // reference-shaped host copy when want_host is set, else NULL.
    // phased: calcR2LD (r2 from HapData::firstCopy and FreqData::freq) instead of calcHR2LD.
    std::vector<LDData *> *ldWeights(int winsize, const std::vector<int> &subsample, bool want_host = true,
                                     bool phased = false);
    // The LD weights of every listed window size from shared passes (garlic_panel_compute_ld_multi; several shards:
    // garlic_ld_counts at the largest size, the host sum, garlic_ld_finish_multi on every shard); all of them stay
    // installed for wlodWindowsResident / lodFeed / assembleROHWindows.  false: the sets do not fit the device memory
    // (nothing is installed: go on with ldWeights per size).
    bool ldWeightsMulti(const std::vector<int> &sizes, const std::vector<int> &subsample, bool phased = false);
    std::vector<WinData *> *wlodWindowsResident(int winsize, double error, int MAX_GAP, int M, double mu);
    // What exploreWinsizes / selectWinsize keep of a window size (garlic-roh.cpp:741-745, 816-823):
    // convertWinData2DoubleData(calcLODWindows(...), step), with the scores thinned on the device(s)
    // -- 8/step bytes per window come back instead of 8.  weighted: wLOD from the resident LD weights.
    // kdeSubsample (convertSubsetWinData2DoubleData, garlic-data.cpp:2071-2150: selectLODCutoff with
    // --kde-subsample): the feed of these individuals only, panel-wide indices in increasing order (what
    // gsl_ran_choose draws); NULL or empty = everyone.  Only their 64-individual blocks are scored.
    DoubleData *lodFeed(int winsize, double error, int MAX_GAP, int step, bool weighted = false, int M = 0,
                        double mu = 0.0, const std::vector<int> *kdeSubsample = nullptr);
    // computeKDE (garlic-kde.cpp:14-140) of the ascending feed of lodFeed's arguments, on the device (garlic_lod_kde: exact
    // Gaussian sums, not FIGTree's approximation).  One shard: no feed value crosses PCIe; several shards or devices: the
    // sorted feeds merged on the host, then garlic_feed_kde.  kde_select.hpp turns the result into a cutoff.
    KdeData lodKde(int winsize, double error, int MAX_GAP, int step, bool weighted = false, int M = 0, double mu = 0.0,
                      const std::vector<int> *kdeSubsample = nullptr);
    // lodKde of several window sizes of a sweep (unweighted scores; steps NULL: the sizes).  One shard on one device: one
    // garlic_lod_kde_multi -- one pass over the panel for all feeds, six KDE launches and two waits for all sizes -- and
    // every result equals lodKde's bit for bit.  status given: status->at(i) != 0 marks a size the library refused (its
    // result is not set; lodKde of that size says why), the others stand; NULL: any refused size fails the call.
    // LodOptions::kde_on_shards, any number of shards: one garlic_lod_kde_part_set per shard that holds KDE individuals and
    // one garlic_kde_parts_multi -- every result equals the sharded lodKde's bit for bit, status as above; the caller prints
    // lodKde's "KDE on <P> shards" per size it uses, <P> = kdeMultiShards().  Several shards without kde_on_shards, or more sizes
    // than KDE_MAX_FEEDS (kdeMultiInOneCall() false): a loop over lodKde, which fails at the first refused size.
    std::vector<KdeData> lodKdeMulti(const std::vector<int> &winsizes, double error, int MAX_GAP, const std::vector<int> *steps = nullptr,
                                     const std::vector<int> *kdeSubsample = nullptr, std::vector<int> *status = nullptr);
    bool kdeMultiInOneCall() const;
    int kdeMultiShards() const;      // the shards the last lodKdeMulti reduced on their devices (0: it took another path)
    // several window sizes in one call (unweighted --error scores): the feeds of exploreWinsizes / selectWinsize /
    // selectWinsizeFromList (garlic-roh.cpp:726-751, 798-837, 881-920), one DoubleData per size; steps NULL: the sizes
    std::vector<DoubleData *> lodFeedMulti(const std::vector<int> &winsizes, double error, int MAX_GAP,
                                           const std::vector<int> *steps = nullptr,
                                           const std::vector<int> *kdeSubsample = nullptr);
    // assembleROHWindows (garlic-roh.cpp:409-545) for the resident panel, from the genotypes to rohData->start / stop /
    // length without the window scores or the per-SNP coverage counts in memory (garlic_roh_segments): what main needs of
    // calcLODWindows + assembleROHWindows when --raw-lod is not asked for (garlic-main.cpp:346-420).  Same arguments as
    // the reference's function after the data; weighted: wLOD from the resident LD weights (ldWeights).
    std::vector<ROHData *> *assembleROHWindows(IndData *indData, double lodScoreCutoff, ROHLength **rohLength, int winSize,
                                               double error, int MAX_GAP, double OVERLAP_FRAC, bool CM, bool weighted = false,
                                               int M = 0, double mu = 0.0);
    // selectSizeClasses (garlic-roh.cpp:935-1003): the nclust-component Gaussian mixture of the pooled lengths that
    // assembleROHWindows returns (individual order, bp or cM), fitted by EM on the engine's first device (garlic_gmm_fit),
    // and the nclust - 1 boundaries between the classes ordered by mean (size_classes.hpp).  The fit is a function of the
    // lengths alone, so one shard or several give the same bits.  Prints the reference's "Gaussian class" lines to stderr;
    // `throw 0` where the reference aborts (no sign change between two means, no convergence of the root search).
    std::vector<double> selectSizeClasses(const ROHLength *rohLength, int nclust);
    // The feature counts of calls that are still in memory (what writeROHData was given): the intervals get writeROHData's
    // classes from `bounds`, panel individuals map to the counting TFAM's by id, and the table is written to outfile.  Runs
    // on the engine's first device: the counts are per individual of the COUNTING file, which no shard splits.
    void featureCounts(FeatureData *data, std::vector<ROHData *> *rohDataByInd, std::vector<MapData *> *mapDataByChr,
                       const std::vector<double> &bounds, const std::string &outfile);
    // garlic_panel_tgls_terms_info of the first shard: the slabs of its last call with likelihoods, weighted or not (n_slabs 0: none)
    void tglsTermSlabs(int *slab_blocks, int *n_slabs);
    LodEngine(const LodEngine &) = delete;
    LodEngine &operator=(const LodEngine &) = delete;

private:
    std::vector<WinData *> *run(bool weighted, int winsize, double error, int MAX_GAP, int M, double mu);
    void upload(std::vector<HapData *> *haps, std::vector<FreqData *> *freqs, std::vector<MapData *> *maps,
                std::vector<GenoLikeData *> *gls, centromere *centro, bool USE_GL, const std::vector<int> &devices);
    void release();
    struct Impl;
    Impl *impl;
};

// ---- consumers right after the path
DoubleData *convertWinData2DoubleData(std::vector<WinData *> *winDataByChr, int step); // :2026
// :2071 with the drawn individuals (randInd[], any order) supplied instead of a time-seeded gsl_ran_choose
DoubleData *convertSubsetWinData2DoubleData(std::vector<WinData *> *winDataByChr, const std::vector<int> &randInd,
                                            int step);
void writeWinData(std::vector<WinData *> *winDataByChr, IndData *indData,
                  std::vector<MapData *> *mapDataByChr, const std::string &outfile);      // :1704

} // namespace garlic_host
