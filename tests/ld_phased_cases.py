"""Cases and restatements for the phased LD weights on the matrix cores (ld_pair_mfma_kernel<.., PHASED>) and the phase
uploaded as bit rows (garlic_panel_set_phase_bits); importable without a GPU.

  pair_kernel_phased   which pair kernel a PHASED LD call picks -- a RESTATEMENT of the rule in ld_form (LdForm::pair,
                       garlic_amd/csrc/garlic_hip.hip); ld_wide_cases.pair_kernel states the rule phased calls follow under
                       GARLIC_LD_PAIR_NO_MFMA (and followed always before the phased MFMA form existed)
  haplotype_planes     A = T | (O & F), B = T | (O & ~F) as 0 / 1 matrices, and x11 from them
  pack_phase_rows      uint8 [nloci][nind] -> the bit rows of garlic_panel_set_phase_bits (the genotype cache's layout)
  plane_words_*        the [blk][nloci] 64-bit plane words from the byte layout and from the bit rows
  panel / oracle_weights   the case table of tests/test_gpu_ld_phased_mfma.py, built once
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import ld_wide_cases as lw

LDM_COUNT_MAX = 1 << 22        # ld_kernels.hpp: counts a tile of f32 accumulators may reach
MFMA_MAX_NJ = 5

# the form codes of garlic_panel_ld_form_info (include/garlic_hip.h)
PAIR_CODE = {"plain": 0, "plain_phased": 0, "mfma": 1, "lane": 2, "tiled": 3, "flat": 4}


def pair_kernel_phased(winsize, nblk, switches=None):
    """'mfma' | 'lane' | 'tiled' | 'flat' | 'plain_phased': phased calls take the matrix-core form under the conditions
    unphased ones do -- 16 < W, NJ = 1 + (30 + W) / 32 <= 5, not flat, none of GARLIC_LD_PAIR_NO_MFMA / _TILED / _L2 -- and
    while the haplotype counts, up to 2 * nind_pad, stay below 2^22; everything else as before"""
    sw = switches or {}
    w = int(winsize)
    flat = "GARLIC_LD_PAIR_FLAT" in sw and w <= 32
    off = any(k in sw for k in ("GARLIC_LD_PAIR_NO_MFMA", "GARLIC_LD_PAIR_TILED", "GARLIC_LD_PAIR_L2"))
    nj = 1 + (30 + w) // 32
    if not flat and not off and w > lw.LD_SMALL_MAX_W and nj <= MFMA_MAX_NJ and 2 * lw.WAVE * int(nblk) < LDM_COUNT_MAX:
        return "mfma"
    no_mfma = dict(sw)
    no_mfma["GARLIC_LD_PAIR_NO_MFMA"] = "1"
    return lw.pair_kernel(w, True, nblk, no_mfma)


def mfma_nj(winsize):
    return 1 + (30 + int(winsize)) // 32


# ---------------------------------------------------------------------------------------------------- the haplotype identity

def haplotype_planes(geno, phase, sub=None):
    """(M, A, B) as bool [nloci][nind]: non-missing and sampled; first / second haplotype carries the counted allele"""
    nind = geno.shape[1]
    insub = np.zeros(nind, dtype=bool)
    insub[lw._sel(nind, sub)] = True
    t = (geno == 2) & insub[None, :]
    o = (geno == 1) & insub[None, :]
    f = phase != 0
    return (geno != -9) & insub[None, :], t | (o & f), t | (o & ~f)


def haplotype_pair_counts(geno, phase, w, sub=None):
    """[nloci][w][2] = {2 |M_i & M_j|, |A_i & A_j| + |B_i & B_j|} of ONE chromosome: what the three Gram products give"""
    m, a, b = haplotype_planes(geno, phase, sub)
    return np.stack([lw._band(2 * lw._gram(m), w), lw._band(lw._gram(a) + lw._gram(b), w)], axis=2)


# ----------------------------------------------------------------------------------------------------------- the bit rows

def pack_phase_rows(phase, row_bytes=None, fill=0):
    """bit (i & 7) of byte (i >> 3) of a row is individual i; row_bytes > (nind + 7) / 8: the rest of a row holds `fill`"""
    phase = np.asarray(phase) != 0
    rows = np.packbits(phase, axis=1, bitorder="little")
    if row_bytes is None or row_bytes == rows.shape[1]:
        return np.ascontiguousarray(rows)
    assert row_bytes > rows.shape[1]
    out = np.full((rows.shape[0], row_bytes), fill, dtype=np.uint8)
    out[:, :rows.shape[1]] = rows
    return out


def plane_words_from_bytes(phase, nblk):
    """[nblk][nloci] uint64: bit k of word [blk][l] = individual 64 blk + k (what garlic_panel_set_phase makes)"""
    phase = np.asarray(phase) != 0
    nloci, nind = phase.shape
    out = np.zeros((nblk, nloci), dtype=np.uint64)
    for i in range(nind):
        out[i >> 6] |= phase[:, i].astype(np.uint64) << np.uint64(i & 63)
    return out


def plane_words_from_rows(rows, nind, nblk):
    """the same from bit rows: a word is 8 consecutive bytes of a row, little-endian, never read past (nind + 7) / 8 bytes,
    the bits past the last individual cleared"""
    rows = np.asarray(rows, dtype=np.uint8)
    nloci = rows.shape[0]
    nbytes = (nind + 7) // 8
    padded = np.zeros((nloci, nblk * 8), dtype=np.uint8)
    padded[:, :nbytes] = rows[:, :nbytes]
    words = padded.reshape(nloci, nblk, 8).astype(np.uint64)
    out = np.zeros((nloci, nblk), dtype=np.uint64)
    for k in range(8):
        out |= words[:, :, k] << np.uint64(8 * k)
    for blk in range(nblk):
        left = nind - 64 * blk
        if left < 64:
            out[:, blk] &= np.uint64((1 << left) - 1 if left > 0 else 0)
    return np.ascontiguousarray(out.T)


# -------------------------------------------------------------------------------------------------------------- the cases
# W = 17, 40, 100, 129: NJ = 2, 3, 5, 5 (129: the widest window of the form).  nind = 1, 64, 65, 130, 200: 1, 1, 2, 3 and 4
# blocks that hold somebody, 1, 2, 2, 4 and 5 blocks in the panel (lw.nblk_of: 64 individuals already take a pad block) -- the
# block pipeline without prefetch, with the prefetch only, and in its steady state fetch(b + 2) / stage(b + 1) / multiply(b).
WINSIZES = [17, 40, 100, 129]
NINDS = [1, 64, 65, 130, 200]
SUBS = ["all", "third", "one_blk"]
CASES = [(nind, w) for nind in NINDS for w in WINSIZES]


def chrom_sizes(w):
    """the 128-SNP tiles' edges, a single SNP, one short of a window, exactly one window, one more, and a few hundred"""
    return [127, 128, 129, 1, w - 1, w, w + 1, 300]


def subsamples(rng, nind):
    blk = np.arange(nind) // lw.WAVE
    only = min(1, lw.real_blocks(nind) - 1)                    # the second block where there is one
    subs = {"all": None,
            "third": np.sort(rng.choice(nind, size=nind // 3, replace=False)),      # (one individual: nobody)
            "one_blk": np.flatnonzero(blk == only)}
    return {k: (None if v is None else v.astype(np.int32)) for k, v in subs.items()}


@functools.lru_cache(maxsize=None)
def panel(nind, w):
    """(chroms, phase uint8 [nloci][nind], subsamples); built once, never written to"""
    rng = np.random.default_rng(77000 + 1000 * w + nind)
    chroms = lw.wide_chroms(rng, chrom_sizes(w), nind)
    nloci = sum(c[0].shape[0] for c in chroms)
    phase = rng.integers(0, 2, size=(nloci, nind)).astype(np.uint8)
    return chroms, phase, subsamples(rng, nind)


_weights = {}


def oracle_weights(nind, w, subname):
    """the oracle's phased weights of a case (ld_wide_cases.oracle_r2); computed once -- the three subsamples of a case side
    by side, the oracle runs outside the interpreter lock -- and never written to"""
    if (nind, w, subname) not in _weights:
        chroms, phase, subs = panel(nind, w)
        with ThreadPoolExecutor(max_workers=len(SUBS)) as pool:
            got = list(pool.map(lambda name: lw.oracle_r2(chroms, phase, w, subs[name]), SUBS))
        for name, ld in zip(SUBS, got):
            ld.setflags(write=False)
            _weights[(nind, w, name)] = ld
    return _weights[(nind, w, subname)]


def special_panel():
    """One chromosome of 60 SNPs x 70 individuals, W = 17, for the values the r2 formula treats specially:
      SNPs 4 / 6    no individual is genotyped at both: total = 0, x11 / total = 0/0 -> the x86 NaN, sign set
      SNPs 10 / 11  allele frequency 0 and 1: r2 = 0 with every partner
      SNPs 20 / 21  everybody homozygous for the counted allele (x11 / total = 1) at a stated frequency of 0.02:
                    D = 1 - 0.0004, r2 = D^2 / 0.02^2 0.98^2 >> 1 -> clamped to 1
    returns (chroms, phase, W)"""
    rng = np.random.default_rng(4242)
    nloci, nind, w = 60, 70, 17
    chroms = lw.wide_chroms(rng, [nloci], nind)
    g, f, p, cs, ce = chroms[0]
    f[:] = rng.uniform(0.1, 0.9, size=nloci)
    g[4, :35] = -9
    g[6, 35:] = -9
    f[10], f[11] = 0.0, 1.0
    g[20, :] = 2
    g[21, :] = 2
    f[20] = f[21] = 0.02
    phase = rng.integers(0, 2, size=(nloci, nind)).astype(np.uint8)
    return chroms, phase, w
