"""Deterministic synthetic SNP x individual panels for bench.py and the
full-size property tests.  Not part of the hot path.

Per-SNP data (positions, allele frequencies, genetic map) are made on the host with numpy;
genotypes are drawn chunk by chunk with torch on whatever device is asked for (the GPU for the
bench, so a 1M x 1k panel never exists as host memory).
"""
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

HG19_LEN = [249250621, 243199373, 198022430, 191154276, 180915260, 171115067, 159138663,
            146364022, 141213431, 135534747, 135006516, 133851895, 115169878, 107349540,
            102531392, 90354753, 81195210, 78077248, 59128983, 63025520, 48129895, 51304566]


def hg19_centromeres():
    with open(os.path.join(_HERE, "centromeres.json")) as f:
        t = json.load(f)["hg19"]
    return [tuple(t["chr%d" % (c + 1)]) for c in range(22)]


class PanelSpec:
    """Per-SNP description of a synthetic panel: 22 autosomes, SNP counts proportional to the
    hg19 chromosome lengths, exponential spacing, no SNP inside a centromere, one injected
    > max_gap hole per chromosome, allele frequency U(0.05, 0.95), 1 cM/Mb +-20 % genetic map."""

    def __init__(self, nloci, seed, max_gap=200000, nchr=22):
        rng = np.random.default_rng(seed)
        lens = np.array(HG19_LEN[:nchr], dtype=np.float64)
        counts = np.maximum(1, np.floor(nloci * lens / lens.sum()).astype(np.int64))
        counts[0] += nloci - counts.sum()
        assert counts.sum() == nloci and counts.min() >= 1
        cen = hg19_centromeres()[:nchr]
        pos, gpos = [], []
        for c in range(nchr):
            n = int(counts[c])
            cs, ce = cen[c]
            usable = HG19_LEN[c] - (ce - cs + 1) - max_gap - 2000
            gaps = rng.exponential(1.0, size=n)
            gaps *= 0.97 * usable / gaps.sum()
            p = np.cumsum(np.maximum(1, gaps).astype(np.int64))
            if n > 4:  # one hole wider than max_gap
                k = int(rng.integers(n // 4, 3 * n // 4))
                p[k:] += max_gap + 1000
            p = np.where(p >= cs, p + (ce - cs + 1), p)  # nothing inside the centromere
            assert (np.diff(p) > 0).all() and p[-1] < 2**31
            pos.append(p.astype(np.int32))
            rate = 1e-6 * rng.uniform(0.8, 1.2, size=n)  # cM per bp
            gpos.append(np.cumsum(np.diff(p, prepend=0) * rate))
        self.nchr = nchr
        self.chr_nloci = counts.astype(np.int32)
        self.chr_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.pos = np.concatenate(pos)
        self.gpos = np.concatenate(gpos)
        self.centro_start = np.array([c[0] for c in cen], dtype=np.int32)
        self.centro_end = np.array([c[1] for c in cen], dtype=np.int32)
        self.freq = rng.uniform(0.05, 0.95, size=nloci)
        self.nloci = int(nloci)
        self.seed = int(seed)
        self.max_gap = int(max_gap)


def genotype_chunks(spec, nind, device, chunk=65536, ind_offset=0, miss=0.01, tracts=8):
    """Yields (locus_begin, int16 tensor [rows][nind]) : HWE draws from spec.freq with `miss`
    missing (-9) and `tracts` planted homozygous tracts per individual (hets forced to the
    nearer homozygote) so the LOD distribution is bimodal.  ind_offset makes shards of one big
    panel distinct (rank r draws individuals [r*nind, (r+1)*nind))."""
    import torch

    g = torch.Generator(device=device)
    g.manual_seed(spec.seed * 1000003 + ind_offset)
    freq = torch.from_numpy(spec.freq).to(device)
    # tract [start, start+len) in global SNP coordinates, per individual
    t_start = torch.randint(0, max(1, spec.nloci - 1), (tracts, nind), generator=g, device=device)
    t_len = torch.randint(500, 3000, (tracts, nind), generator=g, device=device)
    for l0 in range(0, spec.nloci, chunk):
        l1 = min(spec.nloci, l0 + chunk)
        p = freq[l0:l1, None]
        u = torch.rand((l1 - l0, nind), generator=g, device=device, dtype=torch.float32)
        q0 = ((1 - p) * (1 - p)).float()
        q1 = (q0 + 2 * p * (1 - p)).float()
        geno = (u >= q0).to(torch.int16) + (u >= q1).to(torch.int16)
        loc = torch.arange(l0, l1, device=device)[:, None]
        in_tract = torch.zeros((l1 - l0, nind), dtype=torch.bool, device=device)
        for k in range(tracts):
            in_tract |= (loc >= t_start[k][None, :]) & (loc < (t_start[k] + t_len[k])[None, :])
        hom = torch.where(p > 0.5, 2, 0).to(torch.int16).expand(-1, nind)
        geno = torch.where(in_tract & (geno == 1), hom, geno)
        m = torch.rand((l1 - l0, nind), generator=g, device=device, dtype=torch.float32) < miss
        geno = torch.where(m, torch.full_like(geno, -9), geno)
        yield l0, geno.contiguous()


def bed_rows(codes, pad_bits=0):
    """PLINK codes (uint8 [nrows][nind]: 0 hom A1, 1 missing, 2 het, 3 hom A2) -> .bed rows, uint8 [nrows][(nind + 3) // 4],
    individual j at bits 2 * (j % 4) of byte j // 4; the unused bits of the last byte take those of pad_bits."""
    codes = np.asarray(codes, dtype=np.uint8)
    nrows, nind = codes.shape
    rb = (nind + 3) // 4
    padded = np.empty((nrows, 4 * rb), dtype=np.uint8)
    padded[:, :nind] = codes
    for k in range(nind, 4 * rb):
        padded[:, k] = (pad_bits >> (2 * (k % 4))) & 3
    q = padded.reshape(nrows, rb, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)


def write_bed_and_tped(prefix, codes, chrs, pos, a1="A", a2="G", gpos=None, names=None, pop="POP", pad_bits=0):
    """One genotype matrix as PLINK .bed/.bim/.fam and as the twin .tped/.tfam.  codes: PLINK codes [nrows][nind] (see
    bed_rows); chrs / pos: chromosome string and physical position per row; a1 / a2: one character each, or a list per row.
    The TPED line of a row reads "A1 A1" for hom A1, "A1 A2" for a het, "A2 A2" for hom A2 and "0 0" for missing -- the
    convention under which the bed reader's counted allele is GARLIC's first non-missing allele of the line."""
    codes = np.asarray(codes, dtype=np.uint8)
    nrows, nind = codes.shape
    a1 = [a1] * nrows if isinstance(a1, str) else list(a1)
    a2 = [a2] * nrows if isinstance(a2, str) else list(a2)
    gpos = np.zeros(nrows) if gpos is None else np.asarray(gpos, dtype=np.float64)
    names = ["rs%d" % r for r in range(nrows)] if names is None else list(names)
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(bed_rows(codes, pad_bits).tobytes())
    with open(prefix + ".bim", "w") as f:
        for r in range(nrows):
            f.write("%s\t%s\t%.10g\t%d\t%s\t%s\n" % (chrs[r], names[r], gpos[r], pos[r], a1[r], a2[r]))
    fam = "".join("%s ind%d 0 0 0 -9\n" % (pop, i) for i in range(nind))
    for ext in (".fam", ".tfam"):
        with open(prefix + ext, "w") as f:
            f.write(fam)
    with open(prefix + ".tped", "w") as f:
        for r in range(nrows):
            pair = ["%s %s" % (a1[r], a1[r]), "0 0", "%s %s" % (a1[r], a2[r]), "%s %s" % (a2[r], a2[r])]
            f.write("%s %s %.10g %d %s\n" % (chrs[r], names[r], gpos[r], pos[r], " ".join(pair[c] for c in codes[r])))


def vcf_gt(code, order, sep="|"):
    """the GT of one genotype: PLINK code (0 hom REF, 1 missing, 2 het, 3 hom ALT) and order bit (1: the first allele is ALT,
    which tells `1|0` from `0|1`; it is what the code says for a homozygote and 0 for a missing genotype)"""
    a, b = (("0", "0"), (".", "."), ("1", "0") if order else ("0", "1"), ("1", "1"))[int(code)]
    return a + sep + b


def write_vcf_and_tped(prefix, codes, order, chrs, pos, a1="A", a2="G", sep="|", extra_subfields=None, names=None, samples=None,
                       meta=("##fileformat=VCFv4.2",), newline="\n", last_newline=True):
    """One phased genotype matrix as prefix.vcf and as the twin prefix.tped / prefix.tfam that vcf2tped.pl writes from it.
    codes: PLINK codes [nrows][nind] with A1 = REF, A2 = ALT; order: [nrows][nind], 1 where the genotype's first allele is
    ALT (only a het's bit is free).  sep: "|" or "/", one string or an array [nrows][nind] of them.  extra_subfields: None, or
    f(r, j) -> the text behind the GT of genotype (r, j) ("" = bare GT; otherwise FORMAT reads GT:X and the field GT:text).
    The TPED line: CHROM ID 0 POS, then the two letters of every sample in the VCF's own allele order, tab-separated; the TFAM
    line: 0 IID 0 0 0 0."""
    codes = np.asarray(codes, dtype=np.uint8)
    order = np.asarray(order, dtype=np.uint8)
    nrows, nind = codes.shape
    a1 = [a1] * nrows if isinstance(a1, str) else list(a1)
    a2 = [a2] * nrows if isinstance(a2, str) else list(a2)
    names = ["rs%d" % r for r in range(nrows)] if names is None else list(names)
    samples = ["ind%d" % i for i in range(nind)] if samples is None else list(samples)
    seps = np.full((nrows, nind), sep) if isinstance(sep, str) else np.asarray(sep)
    lines = list(meta) + ["\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + samples)]
    tped = []
    for r in range(nrows):
        fields, letters = [], []
        for j in range(nind):
            gt = vcf_gt(codes[r, j], order[r, j], str(seps[r, j]))
            more = extra_subfields(r, j) if extra_subfields else ""
            fields.append(gt + (":" + more if more else ""))
            letters += [{"0": a1[r], "1": a2[r], ".": "0"}[gt[0]], {"0": a1[r], "1": a2[r], ".": "0"}[gt[2]]]
        lines.append("\t".join([str(chrs[r]), "%d" % pos[r], names[r], a1[r], a2[r], ".", "PASS", ".",
                                "GT:X" if extra_subfields else "GT"] + fields))
        tped.append("\t".join([str(chrs[r]), names[r], "0", "%d" % pos[r]] + letters))
    with open(prefix + ".vcf", "w", newline="") as f:
        f.write(newline.join(lines) + (newline if last_newline else ""))
    with open(prefix + ".tped", "w") as f:
        f.write("".join(t + "\n" for t in tped))
    with open(prefix + ".tfam", "w") as f:
        f.write("".join("0\t%s\t0\t0\t0\t0\n" % s for s in samples))
