// garlic-lod: GARLIC's Phase I (window LOD scores) as a stand-alone tool on MI355X.
// Keeps the reference's ingest (tped/tfam/tgls/freq/map/centromere) and the Phase-I part of its
// command line (src/garlic-cli.cpp), and writes what GARLIC's next stage consumes:
//   <out>.<pop>.<chr>.raw.lod.windows.gz   with --raw-lod   (src/garlic-data.cpp:1704)
//   <out>.<W>SNPs.lod.f64                  the KDE feed: convertWinData2DoubleData's doubles
//                                          (src/garlic-data.cpp:2026), thinned to every W-th window
//                                          unless --no-kde-thinning
//   <out>.<W>SNPs.lod.sorted.f64           instead, with --sorted-feed: the same doubles ascending -- the array
//                                          computeKDE's nrd0 makes of the feed first (gsl_sort, src/garlic-kde.cpp:132),
//                                          sorted on the device
// Input besides the reference's tped/tfam: a VCF (--vcf F[.gz], parsed on the device, phase included) or
// a PLINK .bed/.bim/.fam (--bfile PREFIX, or --bed F --bim F --fam F).  The rows go
// to the device as they are; the counted allele of every SNP and its frequency come from a census there, and the genotypes
// never exist on the host as anything but the mapped file.
//   <out>.<W>SNPs.kde                      with --kde: computeKDE's density of the feed (src/garlic-kde.cpp:14-140; the exact
//                                          Gaussian sums on the device, not FIGTree's approximation), the feed itself is
//                                          not written; "Selected LOD score cutoff: X" on stderr (get_min_btw_modes), and
//                                          with --size-bounds and no --lod-cutoff the ROH calls at that cutoff.  With
//                                          --auto-winsize the tool runs selectWinsize / selectWinsizeFromList itself.
// --nclust K (GARLIC's flag) instead of --size-bounds: selectSizeClasses (src/garlic-roh.cpp:935-1003) -- a K-component
// Gaussian mixture fitted to the ROH lengths by EM on the device, the class boundaries from a root search on the host;
// the "Gaussian class" and "Selected ROH size boundaries" lines go to stderr.  Without --nclust nothing changes:
// --size-bounds is then required for ROH calls.
#include "garlic_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

using namespace garlic_host;

namespace {
struct Args {
    std::string tped, tfam, out = "outfile", build = "none", centromere = "none", tgls = "none",
                gl_type = "none", freq_file = "none", map = "none", cache = "none", bed, bim, fam, bfile, vcf;
    char tped_missing = '0';       // src/garlic-cli.cpp:114
    double error = -1;             // :34 (must be in (0,1) unless TGLS)
    int winsize = 0;               // :38
    std::vector<int> winsize_multi;
    bool auto_winsize = false, weighted = false, raw_lod = false, kde_thinning = true, phased = false, vcf_snps_only = false;
    bool sorted_feed = false;      // extension: the feeds ascending, <out>.<W>SNPs.lod.sorted.f64 (the device sorts them)
    bool kde_sharded = false;      // extension: with --kde, the KDE of a sharded panel on the shards' devices (garlic_kde_parts)
    bool kde = false;              // extension: the KDE, the LOD cutoff and (--auto-winsize) the window size in this tool
    bool winsize_stream = false;   // extension: further window sizes from stdin (the loop of selectWinsize, driven by the KDE's owner)
    int auto_winsize_step = 10, max_gap = 200000, M = 7, threads = 1, kde_subsample = 20, gpus = 1;
    std::vector<int> devices;      // --devices; empty = 0 .. gpus-1
    int ld_subsample = 0;          // src/garlic-cli.cpp:137
    int resample = 0;              // src/garlic-cli.cpp:62-64: resamples for the allele frequencies
    unsigned long long resample_seed = 0;   // extension: 0 = time-seeded like the reference
    unsigned long long ld_seed = 0; // extension: 0 = time-seeded like the reference
    std::string vcf_gl_field;      // extension: with --vcf, the likelihoods are this scalar FORMAT field of the VCF's own lines
    bool have_vcf_gl_missing = false;
    double vcf_gl_missing = 0;     // --vcf-gl-missing: the raw value of a called genotype without the field
    double tgls_term_gb = 0;       // extension: garlic_panel_set_tgls_term_budget in GB (0 whole matrix or none, -1 automatic)
    unsigned long long kde_seed = 0; // extension: the --kde-subsample draw, 0 = time-seeded like the reference
    double mu = 1e-9, overlap_frac = 0.25;
    bool have_cutoff = false, cm = false;   // --lod-cutoff (src/garlic-cli.cpp:101), --cm (:167)
    double lod_cutoff = 0.0;
    std::vector<double> size_bounds;        // --size-bounds (:107)
    int nclust = 0;                         // --nclust (:163): the size classes from the GMM of the ROH lengths; 0 = not given
    // --features / --tped-counting / --tfam-counting (:177-189, declared there and never wired in: the reference leaves the
    // stage to src/count_features_in_roh.pl); --roh-bed: extension, count on an existing calls file and exit
    // --bfile-counting / --bed-counting --bim-counting --fam-counting: extension, the counting genotypes as a PLINK file set
    std::string features, tped_counting, tfam_counting, roh_bed;
    std::string bfile_counting, bed_counting, bim_counting, fam_counting;
    // extensions, PLINK input only: --keep F runs the individuals listed in F (a PLINK keep file) as if the file set held
    // only them; --pops all | NAME ... runs every listed family ID of the .fam in turn, each as --keep of its members with
    // --out <out>.<NAME>
    std::string keep;
    std::vector<std::string> pops;
};

[[noreturn]] void usage(const char *msg)
{
    std::cerr << "ERROR: " << msg << "\n"
              << "usage: garlic-lod (--tped F --tfam F | --bfile PREFIX | --bed F --bim F --fam F) --out P\n"
                 "         (--build hg18|hg19|hg38 | --centromere F)\n"
                 "         (--error E | --tgls F --gl-type GQ|GL|PL) (--winsize W | --winsize-multi W1 W2 ...)\n"
                 "         [--auto-winsize] [--auto-winsize-step N] [--winsize-stream] [--max-gap N] [--overlap-frac X]\n"
                 "         [--freq-file F] [--tped-missing C] [--raw-lod] [--kde-subsample N] [--kde-seed S] [--no-kde-thinning]\n"
                 "         [--weighted --map F --M N --mu X --ld-subsample N --ld-seed S --threads N]\n"
                 "         [--resample N --resample-seed S] [--gpus N | --devices 0,1,...] [--genotype-cache F] [--tgls-term-gb X]\n"
                 "         (--tgls-term-gb X: at most X GB of TGLS terms per device, built and read in slabs; binds --weighted --tgls too)\n"
                 "         [--sorted-feed]   (the KDE feeds ascending, as nrd0's gsl_sort leaves them: <out>.<W>SNPs.lod.sorted.f64)\n"
                 "         [--lod-cutoff X --size-bounds B1 B2 ... [--cm]]   (ROH calls: <out>.roh.bed)\n"
                 "         [--nclust K]   (instead of --size-bounds: K size classes, 1 to 8, from a Gaussian mixture fitted to the ROH\n"
                 "                         lengths on the device; with --lod-cutoff or --kde)\n"
                 "         [--kde]   (<out>.<W>SNPs.kde and the LOD cutoff from the KDE on the device instead of the feed files; with\n"
                 "                    --size-bounds and no --lod-cutoff the ROH calls use it; with --auto-winsize the window size too)\n"
                 "         [--kde-sharded]   (with --kde: every shard's feed stays on its device, the KDE is reduced over the shards)\n"
                 "         [--features F --tped-counting T [--tfam-counting M]]   (with a run that writes ROH calls: per individual of T / M\n"
                 "                    the homozygous genotypes of F's annotated alleles (lines `chrN:pos ref allele effect`) inside ROH of\n"
                 "                    each size class and outside any, <out>[.<W>SNPs].feature.counts, counted on the device; M defaults\n"
                 "                    to T with .tped replaced by .tfam.  The columns are count_features_in_roh.pl's <effect>A B C NONE;\n"
                 "                    with more than three size classes they run A .. <last letter> NONE, so nothing is dropped)\n"
                 "         [--roh-bed F --features F --tped-counting T [--tfam-counting M] --out P]   (no genotype input: the same table\n"
                 "                    for the calls of an existing .roh.bed, <out>.feature.counts, then exit)\n"
                 "         [--bfile-counting PREFIX | --bed-counting F --bim-counting F --fam-counting F]   (instead of --tped-counting /\n"
                 "                    --tfam-counting, wherever those go: the counting genotypes as a PLINK SNP-major file set; only the\n"
                 "                    .bim and the .fam are read on the host, the hom rows are built from the .bed image on the device; the\n"
                 "                    counting individuals are the .fam's, also under --keep / --pops)\n"
                 "         [--vcf F[.gz] [--tfam T] [--vcf-biallelic-snps-only]]   (VCF input wherever --bfile goes: the genotypes and the phase\n"
                 "          are parsed on the device, --phased is allowed; without --tfam the family is 0 and the IDs are the header's;\n"
                 "          a REF / ALT that is not one base ends the run, or is left out and counted under --vcf-biallelic-snps-only;\n"
                 "          not with --keep / --pops / --bfile / --bed / --bim / --fam / --tped)\n"
                 "         [--vcf F[.gz] --vcf-gl-field KEY --gl-type GQ|GL|PL [--vcf-gl-missing X]]   (instead of --tgls: the likelihoods\n"
                 "          are the scalar FORMAT field KEY of the VCF's own sample columns, parsed and coded on the device; a missing\n"
                 "          genotype needs no value; a called genotype without one ends the run, or takes the raw value X; under\n"
                 "          --gl-type GQ a raw 0 makes every LOD term of the genotype 0, the neutral X; lists (GL / PL triples) are refused)\n"
                 "         (--bfile / --bed --bim --fam: PLINK SNP-major .bed input, read on the device; not with --tped / --tfam /\n"
                 "          --phased; --genotype-cache F is then written from the .bed, never read)\n"
                 "         [--keep F]   (with PLINK input: the run is that of a file set holding only the individuals of F, a PLINK keep\n"
                 "                       file of `FID IID` lines, in the .fam's order; they must share one family ID, the population's\n"
                 "                       name; the subset is cut out of the image on the device)\n"
                 "         [--pops all | NAME [NAME ...]]   (with PLINK input: every listed family ID of the .fam in turn -- all: every\n"
                 "                       distinct one, first seen first -- each as --keep of its members with --out <out>.<NAME>; one\n"
                 "                       upload of the file per device serves all; stops at the first population that fails; not with\n"
                 "                       --keep, --freq-file, --genotype-cache or --roh-bed)\n";
    exit(1);
}

Args parse(int argc, char **argv)
{
    Args a;
    for (int i = 1; i < argc; i++) {
        const std::string f = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) usage(("missing value for " + f).c_str()); return argv[++i]; };
        if (f == "--tped") a.tped = val();
        else if (f == "--tfam") a.tfam = val();
        else if (f == "--bfile") a.bfile = val();
        else if (f == "--vcf") a.vcf = val();
        else if (f == "--vcf-biallelic-snps-only") a.vcf_snps_only = true;
        else if (f == "--vcf-gl-field") a.vcf_gl_field = val();
        else if (f == "--vcf-gl-missing") {
            const std::string v = val();
            char *stop = nullptr;
            a.vcf_gl_missing = strtod(v.c_str(), &stop);
            if (v.empty() || *stop || !std::isfinite(a.vcf_gl_missing)) usage("--vcf-gl-missing takes one finite number");
            a.have_vcf_gl_missing = true;
        }
        else if (f == "--bed") a.bed = val();
        else if (f == "--bim") a.bim = val();
        else if (f == "--fam") a.fam = val();
        else if (f == "--out") a.out = val();
        else if (f == "--build") a.build = val();
        else if (f == "--centromere") a.centromere = val();
        else if (f == "--tgls") a.tgls = val();
        else if (f == "--gl-type") a.gl_type = val();
        else if (f == "--freq-file") a.freq_file = val();
        else if (f == "--map") a.map = val();
        else if (f == "--genotype-cache") a.cache = val();   // extension: binary sidecar of the parsed TPED
        else if (f == "--tped-missing") a.tped_missing = val()[0];
        else if (f == "--error") a.error = atof(val().c_str());
        else if (f == "--winsize") a.winsize = atoi(val().c_str());
        else if (f == "--winsize-multi") {
            while (i + 1 < argc && argv[i + 1][0] != '-') a.winsize_multi.push_back(atoi(argv[++i]));
        }
        else if (f == "--auto-winsize") a.auto_winsize = !a.auto_winsize; // bool flags toggle (param_t.cpp:278)
        else if (f == "--auto-winsize-step") a.auto_winsize_step = atoi(val().c_str());
        else if (f == "--winsize-stream") a.winsize_stream = !a.winsize_stream;
        else if (f == "--sorted-feed") a.sorted_feed = !a.sorted_feed;
        else if (f == "--kde") a.kde = !a.kde;
        else if (f == "--kde-sharded") a.kde_sharded = !a.kde_sharded;
        else if (f == "--max-gap") a.max_gap = atoi(val().c_str());
        else if (f == "--overlap-frac") a.overlap_frac = atof(val().c_str());
        else if (f == "--weighted") a.weighted = !a.weighted;
        else if (f == "--lod-cutoff") { a.lod_cutoff = atof(val().c_str()); a.have_cutoff = true; }
        else if (f == "--cm") a.cm = !a.cm;
        else if (f == "--size-bounds") {
            while (i + 1 < argc && (isdigit((unsigned char)argv[i + 1][0]) || argv[i + 1][0] == '.')) a.size_bounds.push_back(atof(argv[++i]));
        }
        else if (f == "--nclust") {
            a.nclust = atoi(val().c_str());
            if (a.nclust <= 0) usage("Must choose positive number for number of GMM clusters.");   // checkNCLUST
            if (a.nclust > GMM_MAX_K) usage("--nclust: at most 8 GMM clusters");
        }
        else if (f == "--features") a.features = val();
        else if (f == "--tped-counting") a.tped_counting = val();
        else if (f == "--tfam-counting") a.tfam_counting = val();
        else if (f == "--roh-bed") a.roh_bed = val();
        else if (f == "--bfile-counting") a.bfile_counting = val();
        else if (f == "--bed-counting") a.bed_counting = val();
        else if (f == "--bim-counting") a.bim_counting = val();
        else if (f == "--fam-counting") a.fam_counting = val();
        else if (f == "--keep") a.keep = val();
        else if (f == "--pops") {
            while (i + 1 < argc && !(argv[i + 1][0] == '-' && argv[i + 1][1] == '-')) a.pops.push_back(argv[++i]);
            if (a.pops.empty()) usage("--pops needs all, or family IDs of the .fam");
        }
        else if (f == "--M") a.M = atoi(val().c_str());
        else if (f == "--mu") a.mu = atof(val().c_str());
        else if (f == "--threads") a.threads = atoi(val().c_str());
        else if (f == "--ld-subsample") a.ld_subsample = atoi(val().c_str());
        else if (f == "--ld-seed") a.ld_seed = strtoull(val().c_str(), nullptr, 10);
        else if (f == "--phased") a.phased = !a.phased;
        else if (f == "--raw-lod") a.raw_lod = !a.raw_lod;
        else if (f == "--kde-subsample") a.kde_subsample = atoi(val().c_str());
        else if (f == "--kde-seed") a.kde_seed = strtoull(val().c_str(), nullptr, 10);
        else if (f == "--resample") a.resample = atoi(val().c_str());
        else if (f == "--resample-seed") a.resample_seed = strtoull(val().c_str(), nullptr, 10);
        else if (f == "--no-kde-thinning") a.kde_thinning = !a.kde_thinning;
        else if (f == "--gpus") a.gpus = atoi(val().c_str());
        else if (f == "--tgls-term-gb") a.tgls_term_gb = atof(val().c_str());
        else if (f == "--devices") {   // explicit HIP ordinals, e.g. 0,1,2,3 (an ordinal may repeat: shards share that GPU)
            std::stringstream ss(val());
            std::string tok;
            while (std::getline(ss, tok, ',')) a.devices.push_back(atoi(tok.c_str()));
        }
        else usage(("unknown flag " + f).c_str());
    }
    if (!a.bfile_counting.empty()) {
        if (!a.bed_counting.empty() || !a.bim_counting.empty() || !a.fam_counting.empty())
            usage("--bfile-counting and --bed-counting / --bim-counting / --fam-counting exclude each other");
        a.bed_counting = a.bfile_counting + ".bed"; a.bim_counting = a.bfile_counting + ".bim"; a.fam_counting = a.bfile_counting + ".fam";
    }
    if (!a.bed_counting.empty() || !a.bim_counting.empty() || !a.fam_counting.empty()) {
        if (!a.tped_counting.empty() || !a.tfam_counting.empty())
            usage("--bfile-counting / --bed-counting and --tped-counting / --tfam-counting exclude each other");
        if (a.bed_counting.empty() || a.bim_counting.empty() || a.fam_counting.empty()) usage("--bed-counting, --bim-counting and --fam-counting go together");
        if (a.features.empty()) usage("feature counts need --features and --tped-counting");
    } else if (!a.features.empty() || !a.tped_counting.empty() || !a.tfam_counting.empty() || !a.roh_bed.empty()) {
        if (a.features.empty() || a.tped_counting.empty()) usage("feature counts need --features and --tped-counting");
        if (a.tfam_counting.empty()) a.tfam_counting = featureTfamOf(a.tped_counting);
    }
    if (!a.keep.empty() && !a.pops.empty()) usage("--keep and --pops exclude each other (--pops is --keep of every listed population in turn)");
    if (!a.pops.empty() && !a.roh_bed.empty()) usage("--pops with --roh-bed: --roh-bed counts on existing calls and reads no populations");
    if (!a.roh_bed.empty()) {      // counts on an existing calls file: nothing else is read
        if (!a.tped.empty() || !a.tfam.empty() || !a.bfile.empty() || !a.bed.empty() || !a.vcf.empty()) usage("--roh-bed counts on existing calls and takes no genotype input");
        if (a.devices.empty()) a.devices.push_back(0);
        return a;
    }
    // validators of src/garlic-cli.cpp:240-462 that concern Phase I
    if (a.vcf_snps_only && a.vcf.empty()) usage("--vcf-biallelic-snps-only needs --vcf");
    if (!a.vcf_gl_field.empty() && a.vcf.empty()) usage("--vcf-gl-field reads a FORMAT field of the --vcf file and needs --vcf");
    if (!a.vcf_gl_field.empty() && a.tgls != "none") usage("--vcf-gl-field and --tgls exclude each other (the likelihoods come from one of them)");
    if (a.have_vcf_gl_missing && a.vcf_gl_field.empty()) usage("--vcf-gl-missing needs --vcf-gl-field");
    if (!a.vcf_gl_field.empty()) {
        bool ok = a.vcf_gl_field.size() <= 16 && a.vcf_gl_field != "GT";
        for (char c : a.vcf_gl_field) ok = ok && (isalnum((unsigned char)c) || c == '_' || c == '.');
        if (!ok) usage("--vcf-gl-field takes a FORMAT key of 1 to 16 characters of [A-Za-z0-9_.] other than GT");
    }
    if (!a.vcf.empty()) {
        if (!a.bfile.empty() || !a.bed.empty() || !a.bim.empty() || !a.fam.empty() || !a.tped.empty())
            usage("--vcf and --bfile / --bed / --bim / --fam / --tped exclude each other");
        if (!a.keep.empty() || !a.pops.empty()) usage("--vcf with --keep / --pops: a column subset of a VCF image is not built");
    }
    if (!a.vcf.empty()) {
    } else if (!a.bfile.empty()) {
        if (!a.bed.empty() || !a.bim.empty() || !a.fam.empty()) usage("--bfile and --bed / --bim / --fam exclude each other");
        a.bed = a.bfile + ".bed"; a.bim = a.bfile + ".bim"; a.fam = a.bfile + ".fam";
    }
    if (!a.vcf.empty()) {
    } else if (!a.bed.empty() || !a.bim.empty() || !a.fam.empty()) {
        if (a.bed.empty() || a.bim.empty() || a.fam.empty()) usage("--bed, --bim and --fam go together");
        if (!a.tped.empty() || !a.tfam.empty()) usage("--bfile / --bed and --tped / --tfam exclude each other");
        if (a.phased) usage("--phased with --bfile: a .bed carries no phase");
        a.tfam = a.fam;      // the .fam is the TFAM format
    } else if (!a.keep.empty() || !a.pops.empty()) {
        usage("--keep / --pops select individuals of a PLINK .fam and need --bfile (or --bed --bim --fam), not --tped");
    } else if (a.tped.empty() || a.tfam.empty()) usage("--tped and --tfam (or --bfile) are required");
    if (!a.pops.empty() && a.freq_file != "none") usage("--pops with --freq-file: one frequency file cannot serve several populations");
    if (!a.pops.empty() && a.cache != "none") usage("--pops with --genotype-cache: one cache file cannot hold several populations");
    if (a.build == "none" && a.centromere == "none") usage("must provide --build or --centromere (garlic-cli.cpp:285-291)");
    if ((a.error <= 0 || a.error >= 1) && a.tgls == "none" && a.vcf_gl_field.empty())
        usage("Genotype error rate must be > 0 and < 1, or a TGLS file must be provided.");
    if ((a.tgls != "none" || !a.vcf_gl_field.empty()) && a.gl_type != "GQ" && a.gl_type != "GL" && a.gl_type != "PL")
        usage("Must choose GQ/GL/PL for genotype likelihood format.");
    if (a.winsize <= 1 && a.winsize_multi.empty()) usage("SNP window size must be > 1.");
    for (int w : a.winsize_multi) if (w <= 1) usage("SNP window sizes must be > 1.");
    if (a.max_gap < 0) usage("Max gap must be > 0.");
    if (a.overlap_frac < 0 || a.overlap_frac > 1) usage("Overlap fraction must be >= 0 and <= 1.");
    if (a.weighted && a.map == "none") usage("--weighted needs --map");
    if (a.cm && a.map == "none") usage("--cm needs --map");
    if (a.nclust && !a.size_bounds.empty()) usage("--nclust and --size-bounds exclude each other (the size classes are fitted, or given)");
    if (a.nclust && !a.have_cutoff && !a.kde) usage("--nclust classifies ROH calls and needs --lod-cutoff or --kde");
    if (a.have_cutoff && a.size_bounds.empty() && !a.nclust)
        usage("--lod-cutoff writes the ROH calls and needs --size-bounds (the size classes otherwise come from GARLIC's GMM stage, "
              "Phase II, not part of this tool)");
    if (!a.features.empty() && !((a.have_cutoff || a.kde) && (!a.size_bounds.empty() || a.nclust)))
        usage("--features counts inside ROH calls: give --roh-bed, or a run that writes them (--lod-cutoff or --kde, with --size-bounds or --nclust)");
    if (a.kde_sharded && !a.kde) usage("--kde-sharded needs --kde (it says where the KDE of --kde is computed)");
    if (a.kde && a.raw_lod) usage("--kde and --raw-lod exclude each other (the KDE path keeps the scores on the device)");
    if (a.kde && a.sorted_feed) usage("--kde and --sorted-feed exclude each other (with --kde no feed file is written)");
    if (a.kde && a.winsize_stream) usage("--kde and --winsize-stream exclude each other (with --kde the tool owns the KDE and runs --auto-winsize itself)");
    for (size_t k = 1; k < a.size_bounds.size(); k++)
        if (!(a.size_bounds[k] > a.size_bounds[k - 1])) usage("--size-bounds must increase");
    return a;
}

void writeFeed(const std::string &path, const DoubleData *d)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) { std::cerr << "ERROR: cannot write " << path << "\n"; throw 0; }
    fwrite(d->data, sizeof(double), (size_t)d->size, f);
    fclose(f);
    std::cerr << "Wrote " << path << " (" << d->size << " window scores)\n";
}

// One run of the tool on one population: everything from the ingest to the last output of `a`.  `features`: the loaded
// --features table or NULL.  With `keep` (--keep / --pops) the population is the individuals `keep` (ascending indices into
// `fam`, the .fam's lines) of the open PLINK file set `full`; otherwise the inputs are read as `a` names them.
int run(const Args &a, FeatureData *features, BedFile *full, const std::vector<FamEntry> *fam, const std::vector<int> *keep)
{
    try {
        centromere centro(a.build, a.centromere, "none");
        int numLoci = 0, numInd = 0;
        std::vector<HapData *> *haps = nullptr; std::vector<MapData *> *maps = nullptr;
        std::vector<FreqData *> *freqs = nullptr; std::vector<GenoLikeData *> *gls = nullptr;
        IndData *ind = nullptr;
        struct Owner {   // the reference-shaped containers are raw pointers: release them on every way out
            std::vector<HapData *> *&haps; std::vector<MapData *> *&maps; std::vector<FreqData *> *&freqs;
            std::vector<GenoLikeData *> *&gls; IndData *&ind;
            ~Owner()
            {
                if (ind) releaseIndData(ind);
                if (haps) releaseHapData(haps);
                if (maps) releaseMapData(maps);
                if (freqs) releaseFreqData(freqs);
                if (gls) releaseGLData(gls);
            }
        } owner{haps, maps, freqs, gls, ind};
        std::vector<int> devices = a.devices;
        if (devices.empty())
            for (int d = 0; d < a.gpus; d++) devices.push_back(d);
        FILE *probe = a.cache == "none" || !a.bed.empty() || !a.vcf.empty() ? nullptr : fopen(a.cache.c_str(), "rb");
        std::vector<std::string> vcf_samples;
        VcfGlRequest vcf_gl;
        if (keep) ind = indDataOfKept(*fam, *keep, a.fam);      // the single-population check, over the kept individuals
        if (!a.vcf.empty()) {   // VCF input: parsed on the first device; the cache, if asked for, is written from the image
            // --vcf-gl-field: the likelihoods from the same slabs, on every device that will hold a shard
            vcf_gl.key = a.vcf_gl_field;
            vcf_gl.glType = a.gl_type;
            vcf_gl.hasMissing = a.have_vcf_gl_missing;
            vcf_gl.missing = a.vcf_gl_missing;
            vcf_gl.devices = devices;
            loadVcfData(a.vcf, a.phased, a.vcf_snps_only, vcf_samples, numLoci, numInd, &haps, &maps, &freqs, a.resample, a.resample_seed,
                        devices[0], a.vcf_gl_field.empty() ? nullptr : &vcf_gl);
            if (a.vcf_snps_only)
                std::cerr << "Left out " << haps->at(0)->bed->skipped_non_snp << " lines of " << a.vcf << " that are no biallelic SNPs\n";
            if (a.resample > 0) std::cerr << "Allele frequencies resampled: " << a.resample << "\n";
            if (a.cache != "none") {
                writeGenotypeCache(a.cache, haps, maps, freqs);
                std::cerr << "Wrote genotype cache " << a.cache << "\n";
            }
        } else if (!a.bed.empty()) {   // PLINK input: census on the first device; the cache, if asked for, is written from it
            if (keep) loadBedSubset(full, *keep, numLoci, numInd, &haps, &maps, &freqs, a.resample, a.resample_seed, devices[0]);
            else loadBedData(a.bed, a.bim, a.fam, numLoci, numInd, &haps, &maps, &freqs, a.resample, a.resample_seed, devices[0]);
            if (a.resample > 0) std::cerr << "Allele frequencies resampled: " << a.resample << "\n";
            if (a.cache != "none") {
                writeGenotypeCache(a.cache, haps, maps, freqs);
                std::cerr << "Wrote genotype cache " << a.cache << "\n";
            }
        } else if (probe) {   // parsed before: load the 2-bit sidecar instead of the text
            fclose(probe);
            loadGenotypeCache(a.cache, numLoci, numInd, &haps, &maps, &freqs, /*keepPacked=*/true);
            std::cerr << "Loaded genotype cache " << a.cache << "\n";
            if (a.phased && !hasPhase(haps->at(0))) {
                std::cerr << "ERROR: --phased, but " << a.cache << " was written without phase; delete it to re-read the tped\n";
                return 1;
            }
        } else {
            // GARLIC_TPED_DEVICE_READER=1: parsed, coded and counted on the first device.  The host reader is the default: on the
            // one shape measured (profiles/tped_parse_ab.txt) the load phase through the device reader was the slower one.
            // GARLIC_TPED_HOST_READER=1, or a file with a line the device refuses, keeps the host reader in any case
            const char *host_reader = getenv("GARLIC_TPED_HOST_READER"), *device_reader = getenv("GARLIC_TPED_DEVICE_READER");
            bool on_device = device_reader && *device_reader && strcmp(device_reader, "0") && !(host_reader && *host_reader && strcmp(host_reader, "0"));
            if (on_device) {
                std::string refusal;
                on_device = loadTPEDDataOnDevice(a.tped, numLoci, numInd, &haps, &maps, &freqs, a.tped_missing, a.phased, a.resample,
                                                 a.resample_seed, devices[0], refusal);
                if (!on_device) std::cerr << "TPED device reader: " << refusal << "; reading the file again with the host reader\n";
                else std::cerr << "TPED parsed on device " << devices[0] << "\n";
            }
            if (!on_device)
                loadTPEDData(a.tped, numLoci, numInd, &haps, &maps, &freqs, a.tped_missing, a.phased, a.resample,
                             a.resample_seed);
            if (a.resample > 0) std::cerr << "Allele frequencies resampled: " << a.resample << "\n";   // garlic-main.cpp:91
            if (a.cache != "none") {
                writeGenotypeCache(a.cache, haps, maps, freqs);
                std::cerr << "Wrote genotype cache " << a.cache << "\n";
            }
        }
        if (!a.vcf.empty() && a.tfam.empty()) {      // the .tfam vcf2tped.pl writes: family 0, the header's names
            ind = new IndData;
            ind->nind = numInd;
            ind->pop = "0";
            ind->indID = new std::string[numInd];
            for (int i = 0; i < numInd; i++) ind->indID[i] = vcf_samples[(size_t)i];
        } else if (!keep) {
            std::string pop;
            int nindFam = 0;
            scanIndData3(a.tfam, nindFam, pop);
            if (nindFam != numInd) { std::cerr << "ERROR: tfam lists " << nindFam << " individuals, tped has " << numInd << "\n"; return 1; }
            ind = readIndData3(a.tfam, numInd);
        }
        std::cerr << "Loaded " << numLoci << " loci x " << numInd << " individuals (" << maps->size() << " chromosomes)\n";

        const bool USE_GL = a.tgls != "none" || !a.vcf_gl_field.empty();
        if (USE_GL && !a.vcf_gl_field.empty()) {
            // the VCF's own FORMAT field, parsed and coded by loadVcfData from the slabs of the genotype parse
            gls = vcfGlData(vcf_gl, a.vcf, a.vcf_snps_only, vcf_samples, maps);
            std::cerr << "Genotype likelihoods (" << a.gl_type << ", FORMAT field " << a.vcf_gl_field << " of " << a.vcf << "):";
            for (size_t c = 0; c < gls->size(); c++)
            {
                std::cerr << (c ? ", " : " ") << maps->at(c)->chr << " as " << likelihoodForm(gls->at(c));
                if (!gls->at(c)->data) std::cerr << " (" << gls->at(c)->nvalues << " values)";
            }
            std::cerr << "\n";
        } else if (USE_GL) {
            // rows in pre-filter TPED order; under --keep the kept individuals' columns of the whole .fam's
            // parsed and coded on the first device, no likelihood on the host; GARLIC_TGLS_HOST_READER=1, or a file of more
            // than 65,536 distinct values, keeps the host reader
            const char *host_reader = getenv("GARLIC_TGLS_HOST_READER");
            if (!(host_reader && *host_reader && strcmp(host_reader, "0")))
                gls = loadTGLSFile(a.tgls, numInd, maps, a.gl_type, keep, keep ? (int)fam->size() : 0, devices[0]);
            if (!gls)
                gls = readTGLSData(a.tgls, numLoci, numInd, maps, a.gl_type, /*compact=*/true, keep, keep ? (int)fam->size() : 0);
            // the form each chromosome took: one byte per genotype up to 256 distinct values, two up to 65,536, else doubles
            std::cerr << "Genotype likelihoods (" << a.gl_type << "):";
            for (size_t c = 0; c < gls->size(); c++) {
                std::cerr << (c ? ", " : " ") << maps->at(c)->chr << " as " << likelihoodForm(gls->at(c));
                if (!gls->at(c)->data) std::cerr << " (" << gls->at(c)->nvalues << " values)";
            }
            std::cerr << "\n";
        }
        if (a.freq_file != "none") { releaseFreqData(freqs); freqs = nullptr; freqs = readFreqData(a.freq_file, maps); }
        else writeFreqData(a.out + ".freq", freqs, maps);                        // garlic-main.cpp:245-253
        int kept;
        if (a.weighted) {   // garlic-main.cpp:233-239, 267-276
            std::vector<GenMapScaffold *> *scaffold = loadMapScaffold(a.map, &centro);
            if (scaffold->size() != maps->size()) {
                std::cerr << "ERROR: Scaffold genetic map does not have the same number of chromosomes as data.\n";
                releaseGenMapScaffold(scaffold);
                return 1;
            }
            kept = filterMonomorphicAndOOBSites(&maps, &haps, &freqs, &gls, scaffold, USE_GL);
            const int ni = interpolateGeneticmap(maps, scaffold);
            std::cerr << "Number of genetic map locations interpolated: " << ni << "\n";
            releaseGenMapScaffold(scaffold);
        } else {
            kept = filterMonomorphicSites(&maps, &haps, &freqs, &gls, USE_GL);
        }
        std::cerr << "Filtered monomorphic" << (a.weighted ? " or out of bounds" : "") << " sites: " << kept << " loci kept\n";

        std::vector<int> sizes = a.winsize_multi.empty() ? std::vector<int>{a.winsize} : a.winsize_multi;
        if (a.tgls_term_gb != 0 || a.sorted_feed || a.kde_sharded) {
            LodOptions lo;
            lo.devices = devices;
            // per device: the TGLS term matrix in slabs when it is larger than this
            if (a.tgls_term_gb != 0) lo.tgls_term_bytes = a.tgls_term_gb < 0 ? -1 : (long long)(a.tgls_term_gb * 1e9);
            lo.feed_sorted = a.sorted_feed;      // every feed of the engine arrives ascending
            lo.kde_on_shards = a.kde_sharded;    // LodEngine::lodKde prints "KDE on <P> shards"
            setLodOptions(lo);
        }
        auto feed_file = [&](int W) { return a.out + "." + std::to_string(W) + (a.sorted_feed ? "SNPs.lod.sorted.f64" : "SNPs.lod.f64"); };
        LodEngine engine(haps, freqs, maps, gls, &centro, USE_GL, devices); // one upload, many window sizes
        const std::vector<int> ldsub = a.weighted ? drawLdSubsample(numInd, a.ld_subsample, a.ld_seed) : std::vector<int>();
        // selectLODCutoff (garlic-roh.cpp:674-675): the KDE sees --kde-subsample individuals (default 20,
        // garlic-cli.cpp:131), 0 = everyone.  The ROH stage scores everyone; --raw-lod still writes all rows.
        const std::vector<int> kdesub = drawKdeSubsample(numInd, a.kde_subsample, a.kde_seed);
        if (!kdesub.empty()) {
            std::cerr << "Individuals used for KDE:";
            for (int i : kdesub) std::cerr << " " << ind->indID[i];
            std::cerr << "\n";
        }
        if (!a.kde && !a.raw_lod && !a.weighted && sizes.size() > 1) {
            // --winsize-multi, feeds only, unweighted: all sizes in one call (their kernels and downloads overlap; with --tgls
            // the sizes share passes over the term matrix: garlic_lod_feed_multi_tgls)
            std::vector<int> steps;
            for (int W : sizes) steps.push_back(a.kde_thinning ? W : 1);
            std::vector<DoubleData *> feeds = engine.lodFeedMulti(sizes, a.error, a.max_gap, &steps, &kdesub);
            for (size_t i = 0; i < sizes.size(); i++) {
                writeFeed(feed_file(sizes[i]), feeds[i]);
                releaseDoubleData(feeds[i]);
            }
            sizes.clear();
        }
        // --lod-cutoff: the ROH calls (garlic-main.cpp:346-420 with a user cutoff and user size classes): assembleROHWindows
        // on the device(s), straight from the genotypes -- no window scores, no per-SNP counts -- then the .roh.bed
        auto term_report = [&] {
            if (!USE_GL || a.tgls_term_gb == 0) return;
            int slab_blocks = 0, n_slabs = 0;
            engine.tglsTermSlabs(&slab_blocks, &n_slabs);
            std::cerr << "TGLS terms (--tgls-term-gb " << a.tgls_term_gb << "): last call in " << n_slabs << " slabs of " << slab_blocks
                      << " blocks on the first device (0: the whole matrix, or terms looked up)\n";
        };
        auto roh_calls_at = [&](int W, bool single, double cutoff) {
            ROHLength *len = nullptr;
            std::vector<ROHData *> *roh = engine.assembleROHWindows(ind, cutoff, &len, W, a.error, a.max_gap, a.overlap_frac,
                                                                    a.cm, a.weighted, a.M, a.mu);
            std::cerr << "ROH segments: " << (long long)len->size << " (garlic-lod, MI355X; .roh.bed in the format of garlic 1.1.6a)\n";
            std::vector<double> bounds = a.size_bounds;
            if (a.nclust) {      // garlic-main.cpp:393-398
                try {
                    bounds = engine.selectSizeClasses(len, a.nclust);
                } catch (...) {
                    releaseROHData(roh);
                    releaseROHLength(len);
                    throw;
                }
                std::cerr << sizeBoundsLine(bounds);
            }
            const std::string stem = single ? a.out : a.out + "." + std::to_string(W) + "SNPs";
            writeROHData(stem + ".roh.bed", roh, maps, bounds, ind->pop,
                         "1.1.6a", a.cm);      // the track lines name the format's version (garlic VERSION); this tool says who it is on stderr
            if (features) {
                try {
                    engine.featureCounts(features, roh, maps, bounds, stem + ".feature.counts");
                } catch (...) {
                    releaseROHData(roh);
                    releaseROHLength(len);
                    throw;
                }
            }
            releaseROHData(roh);
            releaseROHLength(len);
        };
        auto roh_calls = [&](int W, bool single) {
            if (a.have_cutoff) roh_calls_at(W, single, a.lod_cutoff);
        };
        if (a.kde) {
            // selectLODCutoff / selectWinsize / selectWinsizeFromList (garlic-roh.cpp:660-700, 766-930) with the KDE of every
            // size made on the device (LodEngine::lodKde); kde_select.hpp holds what the reference does with the density
            const bool single = a.winsize_multi.empty();
            auto kde_of = [&](int W) {
                if (a.weighted) engine.ldWeights(W, ldsub, false, a.phased);
                return engine.lodKde(W, a.error, a.max_gap, a.kde_thinning ? W : 1, a.weighted, a.M, a.mu, &kdesub);
            };
            auto finish = [&](int W, const KdeData &k, double scale, bool single_out) {
                const std::string path = a.out + "." + std::to_string(W) + "SNPs.kde";
                std::vector<double> y(k.y, k.y + KDE_POINTS);
                for (double &v : y) v = scale == 1.0 ? v : v * scale;
                if (!writeKde(path, k.x, y.data(), KDE_POINTS)) { std::cerr << "ERROR: Failed to open " << path << "\n"; throw 0; }
                std::cerr << "Wrote KDE results to " << path << " (" << (long long)k.n << " window scores, bandwidth " << k.h << ")\n";
                double cutoff = 0;
                std::string why;
                if (!kdeMinBetweenModes(k.x, y.data(), KDE_POINTS, W, &cutoff, nullptr, &why)) {
                    std::cerr << "ERROR: no LOD score cutoff from the KDE of winsize " << W << ": " << why << "\n";
                    throw 0;
                }
                std::cerr << "Selected LOD score cutoff: " << cutoff << "\n";
                if (!a.size_bounds.empty() || a.nclust) roh_calls_at(W, single_out, a.have_cutoff ? a.lod_cutoff : cutoff);
            };
            // Unweighted sweeps on one device, or under --kde-sharded on any number of shards: the KDEs of several sizes from
            // one call (LodEngine::lodKdeMulti) -- a whole
            // --winsize-multi list, or the next SWEEP_BATCH sizes of the stepping search, where the sizes past the selected
            // one are computed ahead of need: one that the library refuses fails the run only when the loop reaches it, with
            // the per-size call's message.  GARLIC_KDE_MULTI_OFF: the per-size loop (same files, same selection lines).
            const bool batched = !a.weighted && !getenv("GARLIC_KDE_MULTI_OFF") && engine.kdeMultiInOneCall() && (!single || a.auto_winsize);
            constexpr int SWEEP_BATCH = 4;
            std::vector<int> batch_sizes, batch_status;
            std::vector<KdeData> batch;
            auto kde_batch = [&](const std::vector<int> &ws) {
                std::vector<int> steps;
                for (int W : ws) steps.push_back(a.kde_thinning ? W : 1);
                batch_sizes = ws;
                batch = engine.lodKdeMulti(ws, a.error, a.max_gap, &steps, &kdesub, &batch_status);
            };
            auto from_batch = [&](size_t j) -> KdeData {
                if (batch_status[j]) return kde_of(batch_sizes[j]);      // refused: the per-size call says why, and fails
                if (engine.kdeMultiShards()) std::cerr << "KDE on " << engine.kdeMultiShards() << " shards\n";      // as lodKde, per size used
                return batch[j];
            };
            if (!a.auto_winsize) {
                if (batched) {
                    for (size_t i0 = 0; i0 < sizes.size(); i0 += KDE_MAX_FEEDS) {
                        kde_batch(std::vector<int>(sizes.begin() + (long)i0, sizes.begin() + (long)std::min(sizes.size(), i0 + KDE_MAX_FEEDS)));
                        for (size_t j = 0; j < batch_sizes.size(); j++) finish(batch_sizes[j], from_batch(j), 1.0, single);
                    }
                } else {
                    for (int W : sizes) finish(W, kde_of(W), 1.0, single);
                }
                term_report();
                return 0;
            }
            if (a.weighted) { std::cerr << "Not currently supported.\n"; return 1; }    // as the reference's selectWinsize says
            const double threshold = 0.50;
            std::cerr << "Searching for acceptable window size, smoothness threshold: " << threshold << "\nwinsize\tsmoothness\n";
            size_t batch0 = 0;                  // the loop index of the batch's first size
            for (size_t i = 0;; i++) {      // selectWinsize: from --winsize in steps; selectWinsizeFromList: the list, the last size if none passes
                const int W = single ? a.winsize + (int)i * a.auto_winsize_step : sizes[i];
                if (batched && (i == 0 || i - batch0 >= batch_sizes.size())) {
                    std::vector<int> ws;
                    const size_t want = single ? (size_t)SWEEP_BATCH : std::min<size_t>(sizes.size() - i, KDE_MAX_FEEDS);
                    for (size_t j = 0; j < want; j++) ws.push_back(single ? a.winsize + (int)(i + j) * a.auto_winsize_step : sizes[i + j]);
                    batch0 = i;
                    kde_batch(ws);
                }
                const KdeData k = batched ? from_batch(i - batch0) : kde_of(W);
                const double mse = kdeWiggle(k.x, k.y, KDE_POINTS);
                std::cerr << W << "\t" << mse << "\n";
                if (mse <= threshold || (!single && i + 1 == sizes.size())) {
                    // calculateWiggle scales y by 100 in place before the reference writes and reads the density again
                    std::cerr << "Selected window size: " << W << "\n";
                    finish(W, k, 100.0, true);
                    term_report();
                    return 0;
                }
            }
        }
        const bool single_size = a.winsize_multi.empty();
        if (a.have_cutoff && !a.weighted)
            for (int W : a.winsize_multi.empty() ? std::vector<int>{a.winsize} : a.winsize_multi) roh_calls(W, single_size);
        // --weighted --winsize-multi: the LD weights of all sizes from shared passes, once; where the sets do not fit the
        // device, per size as before
        const bool ld_shared = a.weighted && sizes.size() > 1 && engine.ldWeightsMulti(sizes, ldsub, a.phased);
        if (a.weighted && sizes.size() > 1 && !ld_shared)
            std::cerr << "NOTE: the LD weights of all window sizes do not fit the device memory; computing them per size\n";
        for (int W : sizes) {
            if (a.weighted && !ld_shared) engine.ldWeights(W, ldsub, false, a.phased);   // garlic-main.cpp:346-357: LD weights per window size
            if (a.weighted) roh_calls(W, single_size);
            const std::string feed_path = feed_file(W);
            if (!a.raw_lod) {   // only the KDE feed is wanted: thin on the device, no full-score download
                DoubleData *feed = engine.lodFeed(W, a.error, a.max_gap, a.kde_thinning ? W : 1, a.weighted, a.M, a.mu, &kdesub);
                writeFeed(feed_path, feed);
                releaseDoubleData(feed);
                continue;
            }
            std::vector<WinData *> *win = a.weighted ? engine.wlodWindowsResident(W, a.error, a.max_gap, a.M, a.mu)
                                                     : engine.lodWindows(W, a.error, a.max_gap);
            writeWinData(win, ind, maps, sizes.size() == 1 ? a.out : a.out + "." + std::to_string(W) + "SNPs");
            DoubleData *feed = kdesub.empty() ? convertWinData2DoubleData(win, a.kde_thinning ? W : 1)
                                              : convertSubsetWinData2DoubleData(win, kdesub, a.kde_thinning ? W : 1);
            if (a.sorted_feed) std::sort(feed->data, feed->data + feed->size);   // host scores: the same file as the device's sort
            writeFeed(feed_path, feed);
            releaseDoubleData(feed);
            releaseWinData(win);
        }
        if (a.winsize_stream) {
            // selectWinsize (garlic-roh.cpp:766-850) computes a window size, looks at the KDE of its scores and, if that is
            // not smooth enough, goes on with winsize + --auto-winsize-step on the same data.  The KDE is Phase II and not
            // part of this tool, so its owner drives that loop: one window size per line on stdin ("+" = the previous size
            // + --auto-winsize-step), the feed of each on the resident panel, one line "FEED <winsize> <file> <values>"
            // on stdout when it is written; end of input or 0 ends the run.
            int last = a.winsize_multi.empty() ? a.winsize : a.winsize_multi.back();
            std::string line;
            while (std::getline(std::cin, line)) {
                while (!line.empty() && isspace((unsigned char)line.back())) line.pop_back();
                if (line.empty()) continue;
                const int W = line == "+" ? last + a.auto_winsize_step : atoi(line.c_str());
                if (W == 0) break;
                if (W <= 1) { std::cerr << "ERROR: SNP window size must be > 1.\n"; return 1; }
                if (a.weighted) engine.ldWeights(W, ldsub, false, a.phased);
                DoubleData *feed = engine.lodFeed(W, a.error, a.max_gap, a.kde_thinning ? W : 1, a.weighted, a.M, a.mu, &kdesub);
                const std::string path = feed_file(W);
                writeFeed(path, feed);
                std::cout << "FEED " << W << " " << path << " " << feed->size << std::endl;
                releaseDoubleData(feed);
                last = W;
            }
        } else if (a.auto_winsize)
            std::cerr << "NOTE: --auto-winsize picks among the feeds above in GARLIC's KDE stage (Phase II, not part of this tool); "
                         "--winsize-stream lets that stage ask for further window sizes on the resident panel\n";
        term_report();
    } catch (...) {
        return 1;
    }
    return 0;
}
} // namespace

int main(int argc, char **argv)
{
    const Args a = parse(argc, argv);
    try {
        struct FeatureOwner {
            FeatureData *d = nullptr;
            ~FeatureOwner() { releaseFeatureCounts(d); }
        } fdata;
        if (!a.features.empty())
            fdata.d = a.bed_counting.empty() ? loadFeatureCounts(a.features, a.tped_counting, a.tfam_counting)
                                             : loadFeatureCountsBed(a.features, a.bed_counting, a.bim_counting, a.fam_counting);
        if (!a.roh_bed.empty()) {
            featureCountsFromBed(fdata.d, a.roh_bed, a.out + ".feature.counts", a.devices[0]);
            return 0;
        }
        if (a.keep.empty() && a.pops.empty()) return run(a, fdata.d, nullptr, nullptr, nullptr);
        // --keep / --pops: the whole file set is opened once; every run extracts its individuals from the image on the device
        std::vector<FamEntry> fam;
        std::vector<int> kept;
        std::vector<FamFamily> todo;
        try {
            fam = readFam(a.fam);
            if (!a.keep.empty()) kept = readKeepFile(a.keep, fam);
            else {
                const std::vector<FamFamily> all = famFamilies(fam);
                if (a.pops.size() == 1 && a.pops[0] == "all") todo = all;
                else
                    for (const std::string &name : a.pops) {
                        size_t k = 0;
                        while (k < all.size() && all[k].fid != name) k++;
                        if (k == all.size()) throw std::runtime_error("--pops: no family ID " + name + " in " + a.fam);
                        todo.push_back(all[k]);
                    }
                if (todo.empty()) throw std::runtime_error("no individuals in " + a.fam);
            }
        } catch (const std::exception &e) {
            std::cerr << "ERROR: " << e.what() << "\n";
            return 1;
        }
        struct FileOwner {
            BedFile *b = nullptr;
            ~FileOwner() { releaseBedFile(b); }
        } file;
        file.b = openBedFile(a.bed, a.bim, a.fam, /*anyPopulations=*/true);
        file.b->refs = 1;
        if (!a.keep.empty()) return run(a, fdata.d, file.b, &fam, &kept);
        file.b->hold_images = true;      // one upload per device serves every population
        for (const FamFamily &f : todo) {
            Args one = a;
            one.out = a.out + "." + f.fid;
            std::cerr << "Population " << f.fid << ": " << f.members.size() << " individuals, --out " << one.out << "\n";
            const int rc = run(one, fdata.d, file.b, &fam, &f.members);
            if (rc) {
                std::cerr << "ERROR: population " << f.fid << " failed; stopping\n";
                return rc;
            }
        }
    } catch (...) {
        return 1;
    }
    return 0;
}
