// CPU unit checks of readTGLSData(compact = true): the three forms a chromosome's likelihoods can take -- one-byte codes up
// to 256 distinct converted values, 16-bit codes up to 65,536, the doubles themselves beyond -- each describing exactly the
// doubles of compact = false, before and after the monomorphic-site filter.  The one-byte form is also compared with the
// coding the reader had before the wider forms existed (first-seen order, found by a linear scan).  The inputs are written
// here: GL-typed columns, 7 individuals, a monomorphic SNP every fifth row.
#include "../../garlic_amd/host/garlic_host.hpp"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <set>
#include <string>
#include <vector>

using namespace garlic_host;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::cerr << "FAILED " << __LINE__ << ": " #cond "\n"; return 1; } \
    } while (0)

static const int NIND = 7;

// chromosome c gets exactly distinct[c] different printed values, visited in a scrambled order
static void write_inputs(const std::string &tped, const std::string &tgls, const std::vector<int> &distinct, std::vector<int> &rows)
{
    FILE *a = fopen(tped.c_str(), "w"), *b = fopen(tgls.c_str(), "w");
    unsigned x = 2463534242u;
    for (size_t c = 0; c < distinct.size(); c++) {
        const int T = distinct[c];
        rows.push_back((T + NIND - 1) / NIND + 3);
        for (int l = 0; l < rows[c]; l++) {
            fprintf(a, "%d s%d_%d 0 %d", (int)c + 1, (int)c, l, 1000 + 100 * l);
            fprintf(b, "%d s%d_%d 0 %d", (int)c + 1, (int)c, l, 1000 + 100 * l);
            for (int i = 0; i < NIND; i++) {
                x ^= x << 13; x ^= x >> 17; x ^= x << 5;
                if (l % 5 == 4) fprintf(a, " 1 1");
                else fprintf(a, " %d %d", 1 + (int)(x & 1), 1 + (int)((x >> 1) & 1));
                const long long k = ((long long)(l * NIND + i) * 7919) % T;      // 7919 is prime: every k < T turns up
                fprintf(b, " -%.4f", (double)k * 1e-4);                         // k = 0: 1 - 10^0 = 0, clamped to 1e-16
            }
            fprintf(a, "\n");
            fprintf(b, "\n");
        }
    }
    fclose(a);
    fclose(b);
}

static bool same_values(std::vector<GenoLikeData *> *g, std::vector<GenoLikeData *> *gc)
{
    if (g->size() != gc->size()) return false;
    for (size_t c = 0; c < g->size(); c++) {
        if (g->at(c)->nloci != gc->at(c)->nloci) return false;
        for (int l = 0; l < g->at(c)->nloci; l++)
            for (int i = 0; i < NIND; i++) {
                const double p = likelihoodAt(g->at(c), l, i), q = likelihoodAt(gc->at(c), l, i);
                if (memcmp(&p, &q, sizeof p) != 0) return false;
            }
    }
    return true;
}

static int run_case(const std::string &tmp, const std::string &name, const std::vector<int> &distinct, const std::vector<int> &width)
{
    const std::string tped = tmp + "/" + name + ".tped", tgls = tmp + "/" + name + ".tgls";
    std::vector<int> rows;
    write_inputs(tped, tgls, distinct, rows);
    int nl = 0, ni = 0, nl2 = 0, ni2 = 0;
    std::vector<HapData *> *h, *h2;
    std::vector<MapData *> *m, *m2;
    std::vector<FreqData *> *f, *f2;
    loadTPEDData(tped, nl, ni, &h, &m, &f, '0', false);
    loadTPEDData(tped, nl2, ni2, &h2, &m2, &f2, '0', false);
    CHECK(ni == NIND && m->size() == distinct.size());
    std::vector<GenoLikeData *> *g = readTGLSData(tgls, nl, ni, m, "GL", false);
    std::vector<GenoLikeData *> *gc = readTGLSData(tgls, nl2, ni2, m2, "GL", true);
    for (size_t c = 0; c < distinct.size(); c++) {
        const GenoLikeData *d = gc->at(c), *full = g->at(c);
        CHECK(full->data && !full->codes && !full->codes16 && full->nloci == rows[c]);
        std::set<uint64_t> seen;
        for (int l = 0; l < rows[c]; l++)
            for (int i = 0; i < NIND; i++) {
                uint64_t bits;
                memcpy(&bits, &full->data[l][i], sizeof bits);
                seen.insert(bits);
            }
        CHECK((int)seen.size() == distinct[c]);                  // the printed values stay distinct through the conversion
        CHECK((d->data != nullptr) + (d->codes != nullptr) + (d->codes16 != nullptr) == 1);
        if (width[c] == 1) {
            CHECK(d->codes && d->nvalues == distinct[c] && d->nvalues <= 256);
            CHECK(std::string(likelihoodForm(d)) == "one-byte codes");
            // the coding before the wider forms: first-seen order, a linear scan per genotype
            std::vector<double> table;
            for (int l = 0; l < rows[c]; l++)
                for (int i = 0; i < NIND; i++) {
                    size_t code = 0;
                    while (code < table.size() && memcmp(&table[code], &full->data[l][i], sizeof(double)) != 0) code++;
                    if (code == table.size()) table.push_back(full->data[l][i]);
                    CHECK(d->codes[l][i] == (unsigned char)code);
                }
            CHECK((int)table.size() == d->nvalues && memcmp(table.data(), d->values, table.size() * sizeof(double)) == 0);
        } else if (width[c] == 2) {
            CHECK(d->codes16 && d->nvalues == distinct[c] && d->nvalues > 256 && d->nvalues <= 65536);
            CHECK(std::string(likelihoodForm(d)) == "16-bit codes");
            int next = 0;                                        // first-seen order here too
            for (int l = 0; l < rows[c]; l++)
                for (int i = 0; i < NIND; i++) {
                    CHECK(d->codes16[l][i] <= next);
                    if (d->codes16[l][i] == next) next++;
                }
            CHECK(next == d->nvalues);
        } else {
            CHECK(d->data && !d->values && d->nvalues == 0 && distinct[c] > 65536);
            CHECK(std::string(likelihoodForm(d)) == "doubles");
        }
    }
    CHECK(same_values(g, gc));
    const int k1 = filterMonomorphicSites(&m, &h, &f, &g, true);
    const int k2 = filterMonomorphicSites(&m2, &h2, &f2, &gc, true);
    CHECK(k1 == k2 && k1 < nl && k1 > 0);
    CHECK(same_values(g, gc));
    for (size_t c = 0; c < distinct.size(); c++) {               // the filter keeps each chromosome's form and table
        const GenoLikeData *d = gc->at(c);
        CHECK((width[c] == 1 ? d->codes != nullptr : width[c] == 2 ? d->codes16 != nullptr : d->data != nullptr));
        CHECK(width[c] == 8 || d->nvalues == distinct[c]);
    }
    releaseGLData(g); releaseGLData(gc);
    releaseHapData(h); releaseHapData(h2);
    releaseMapData(m); releaseMapData(m2);
    releaseFreqData(f); releaseFreqData(f2);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::cerr << "usage: tgls_forms_unit tmpdir\n"; return 2; }
    const std::string tmp = argv[1];
    try {
        if (run_case(tmp, "a", {256, 300}, {1, 2})) return 1;        // 256 values: one byte, as before; forms are per chromosome
        if (run_case(tmp, "b", {257, 40}, {2, 1})) return 1;         // the 257th value widens the rows read so far
        if (run_case(tmp, "c", {65536, 65537}, {2, 8})) return 1;    // a full 16-bit table; one value more: doubles
    } catch (const std::exception &e) {
        std::cerr << "exception: " << e.what() << "\n";
        return 1;
    }
    std::cout << "tgls_forms_unit ok\n";
    return 0;
}
