"""Cases, restatements and plain references for the LD weights on panels wider than six 64-individual blocks; importable
without a GPU.

  nblk_of        the block count garlic_panel_create gives a panel (nind_pad / 64), restated
  pair_kernel    which pair kernel an LD call picks -- a RESTATEMENT of the rule in ld_form (LdForm::pair,
                 garlic_amd/csrc/garlic_hip.hip), kept here so that the case table can be checked without a GPU; when the rule
                 there changes, this one follows it
  staging        the block-staging paths of ld_kernels.hpp / ld_pair_mfma_kernel a (kernel, nblk) reaches, restated likewise
  wide_chroms    panels whose 64-individual blocks differ from one another, so that a block swapped, skipped or repeated
                 changes the integer counts
  locus_counts / pair_counts / phased_pair_counts
                 the integer counts of include/garlic_hip.h (and the head of ld_kernels.hpp) in plain numpy: products of
                 0 / 1 matrices, no bit planes, no blocks
  ld_from_counts the floating-point part in numpy float64, in the reference's operation order
"""
import functools

import numpy as np

import oracle_lib as ol

WAVE = 64
LD_SMALL_MAX_W = 16        # ld_kernels.hpp
LD_LANE_T = 256
LD_PAIR_BLK = 8
LD_LANE_STAGE = 4          # ld_form's default of GARLIC_LD_LANE_STAGE
PLANES_TRIP = 32           # ld_planes_kernel: 4 waves x 8 blocks per outer trip

PAIR_SWITCHES = ["GARLIC_LD_PAIR_TILED", "GARLIC_LD_PAIR_L2", "GARLIC_LD_PAIR_NO_MFMA", "GARLIC_LD_PAIR_FLAT",
                 "GARLIC_LD_LANE_STAGE", "GARLIC_LD_NO_PLANE_CACHE"]


def nblk_of(nind):
    """64-individual blocks of a panel of nind: nind_pad = (nind + 126) / 64 * 64 (a pad block when nind leaves less than
    one free)"""
    return (int(nind) + 126) // 64


def real_blocks(nind):
    """blocks that hold an individual"""
    return (int(nind) + 63) // 64


def lane_stage_of(nblk, switches=None):
    sw = switches or {}
    return min(nblk, int(sw["GARLIC_LD_LANE_STAGE"]) if "GARLIC_LD_LANE_STAGE" in sw else LD_LANE_STAGE)


def pair_kernel(winsize, phased, nblk, switches=None):
    """'mfma' | 'lane' | 'tiled' | 'flat' | 'plain' | 'plain_phased': the pair kernel ld_form picks (LdPair).  switches: {name:
    value} of the GARLIC_LD_* variables that are set (a set variable counts whatever its value, as getenv() != NULL does)"""
    sw = switches or {}
    w = int(winsize)
    flat = "GARLIC_LD_PAIR_FLAT" in sw and w <= 32
    tiled_sw, l2_sw = "GARLIC_LD_PAIR_TILED" in sw, "GARLIC_LD_PAIR_L2" in sw
    mfma_nj = 1 + (30 + w) // 32
    mfma = (not phased and not flat and w > LD_SMALL_MAX_W and mfma_nj <= 5 and "GARLIC_LD_PAIR_NO_MFMA" not in sw
            and not tiled_sw and not l2_sw)
    lane_lds = 8 * (4 if phased else 2) * lane_stage_of(nblk, sw) * (LD_LANE_T + w - 1)
    lane = not mfma and not flat and w - 1 <= 256 and lane_lds <= 150 * 1024 and not tiled_sw and not l2_sw
    tiled = not mfma and not flat and not lane and w - 1 <= 256 and not l2_sw
    if mfma:
        return "mfma"
    if flat:
        return "flat"
    if lane:
        return "lane"
    if tiled:
        return "tiled"
    return "plain_phased" if phased else "plain"


def staging(winsize, phased, nblk, switches=None):
    """the set of staging paths a call reaches, as labels:
      planes_u2        ld_planes_kernel: a wave takes a third block in one trip (u >= 2)
      planes_trip2     ld_planes_kernel: the second outer trip (blk0 += 32)
      lane_partial     ld_pair_lane_kernel: a last stage of fewer than nb_stage blocks
      lane_stages3     ld_pair_lane_kernel: three or more stages
      lane_restaged    ld_pair_lane_kernel: more than one pass over the distances, every pass staging again
      tiled_chunk2     ld_pair_tiled_kernel: a second chunk of LD_PAIR_BLK blocks
      mfma_steady      ld_pair_mfma_kernel: the fetch(b+2) / stage(b+1) / multiply(b) steady state beyond a handful of blocks
    """
    w = int(winsize)
    out = set()
    if nblk > 8:
        out.add("planes_u2")
    if nblk > PLANES_TRIP:
        out.add("planes_trip2")
    k = pair_kernel(w, phased, nblk, switches)
    if k == "lane":
        st = lane_stage_of(nblk, switches)
        nst = (nblk + st - 1) // st
        if nblk % st:
            out.add("lane_partial")
        if nst >= 3:
            out.add("lane_stages3")
        if st < nblk and w - 1 > (16 if w - 1 <= 16 else 32):
            out.add("lane_restaged")
    if k == "tiled" and nblk > LD_PAIR_BLK:
        out.add("tiled_chunk2")
    if k == "mfma" and nblk >= 21:
        out.add("mfma_steady")
    return out


# ------------------------------------------------------------------------------------------------------------- the cases
# widths from the code's thresholds:   nind  nblk
#    385     7   the last real block holds one individual; the lane kernel's second stage is partial
#    577    10   the tiled kernel's second chunk; three lane stages; u = 2 of the planes kernel
#   1250    21   the benchmark's width; the last block is all padding
#   2113    34   the planes kernel's second outer trip (waves 0 and 1)
# window sizes on both sides of every pair-kernel boundary: unphased 16 | 17 (lane | mfma), 129 | 130 (mfma | lane), 257 | 258
# (lane | plain); phased 257 | 258.  The oracle costs starts x W^2 x individuals: the widest panels take a pruned list (the
# plain kernels, which stage nothing, stop at 21 blocks; 34 blocks take W = 130, nine lane stages restaged per distance pass).
UNPHASED = {385: [10, 17, 130], 577: [10, 16, 17, 40, 100, 129, 130, 257, 258], 1250: [10, 40, 100, 130, 258],
            2113: [16, 40, 130]}
PHASED = {385: [9, 40], 577: [9, 40, 257, 258], 1250: [40], 2113: [9]}
NINDS = sorted(UNPHASED)
CASES = [(nind, w, False) for nind in NINDS for w in UNPHASED[nind]] + \
        [(nind, w, True) for nind in NINDS for w in PHASED[nind]]
SWITCH_NINDS = [577, 1250]
MULTI_SIZES = [40, 100, 200, 300]
MULTI_CHROMS = [41, 101, 201, 300, 1]
MID = 300                  # "a few hundred SNPs": window starts of the middle chromosome, where the oracle can afford them
ORACLE_VISITS = 1.5e8       # the oracle visits starts x W^2 x individuals genotype pairs (it takes every pair of a window anew)


def sizes_of(nind):
    return sorted(set(UNPHASED[nind]) | set(PHASED[nind]))


def starts_of(sizes, w):
    return sum(max(0, n - w + 1) for n in sizes)


def chrom_sizes(nind, w):
    """as test_ld_matches_oracle: 1, W-1, W, W+1 SNPs, then -- while the oracle's cost of the case stays within ORACLE_VISITS --
    127 / 128 / 129 (the MFMA kernel's 128-SNP tiles) or 255 / 256 / 257 (the lane kernel's 256-SNP tiles) and a middle
    chromosome of up to MID window starts, which comes first"""
    sizes = [1, w - 1, w, w + 1]
    left = int(ORACLE_VISITS // (w * w * nind)) - starts_of(sizes, w)
    nblk = nblk_of(nind)
    kernels = {pair_kernel(w, False, nblk), pair_kernel(w, True, nblk)}
    edges = ([127, 128, 129] if "mfma" in kernels else []) + ([255, 256, 257] if "lane" in kernels else [])
    for n in edges:
        if n not in sizes and 0 < starts_of([n], w) <= left:
            sizes.append(n)
            left -= starts_of([n], w)
    if left >= 2:
        sizes.insert(0, w - 1 + min(left, MID))
    return sizes


def wide_chroms(rng, sizes, nind):
    """random_panel chromosomes (no gaps) whose blocks differ: missingness rises and heterozygosity falls with the block
    index, one middle block is all-missing at a few SNPs of every chromosome, and the first chromosome has a monomorphic, an
    all-heterozygous and an all-missing SNP"""
    nreal = real_blocks(nind)
    blk = np.arange(nind) // WAVE
    miss = 0.01 + 0.25 * blk / max(1, nreal - 1)              # per individual, by its block
    het = 0.30 * (1.0 - blk / max(1, nreal - 1))
    dead = nreal // 2
    chroms = []
    for n in sizes:
        g, f, p, cs, ce = ol.random_panel(rng, n, nind, max_gap=10 ** 9, gaps=0, miss=0.0)
        g[rng.random((n, nind)) < het[None, :]] = 1
        g[rng.random((n, nind)) < miss[None, :]] = -9
        for l in (2, 3, 7):
            if l < n:
                g[l, blk == dead] = -9
        chroms.append((g, f, p, cs, ce))
    g0 = chroms[0][0]
    if g0.shape[0] > 13:
        g0[5, :] = 2
        g0[9, :] = 1
        g0[13, :] = -9
    return chroms


def subsamples(rng, nind):
    """{name: int32 indices, ascending; None = everyone}"""
    nreal = real_blocks(nind)
    blk = np.arange(nind) // WAVE
    upper = np.flatnonzero(blk >= 4)
    subs = {
        "all": None,
        "third": np.sort(rng.choice(nind, size=nind // 3, replace=False)),
        "from_blk4": np.sort(rng.choice(upper, size=max(1, upper.shape[0] // 2), replace=False)),
        "last_blk": np.flatnonzero(blk == nreal - 1),
        "one_per_blk": np.array([rng.choice(np.flatnonzero(blk == b)) for b in range(nreal)]),
        "empty": np.zeros(0, dtype=np.int32),
    }
    return {k: (None if v is None else v.astype(np.int32)) for k, v in subs.items()}


@functools.lru_cache(maxsize=None)
def panel(nind, w):
    """(chroms, phase uint8 [nloci][nind], subsamples) of a width and window size; built once, never written to"""
    rng = np.random.default_rng(9000 * w + nind)
    chroms = wide_chroms(rng, chrom_sizes(nind, w), nind)
    nloci = sum(c[0].shape[0] for c in chroms)
    phase = rng.integers(0, 2, size=(nloci, nind)).astype(np.uint8)
    return chroms, phase, subsamples(rng, nind)


@functools.lru_cache(maxsize=None)
def multi_panel():
    """the 1250-wide panel of the multi-size tests (chromosomes around MULTI_SIZES)"""
    rng = np.random.default_rng(9001)
    chroms = wide_chroms(rng, MULTI_CHROMS, 1250)
    return chroms, subsamples(rng, 1250)


def oracle_ld(chroms, w, sub=None):
    return np.concatenate([ol.oracle_hr2_ld(c[0], w, idx=sub) for c in chroms], axis=0)


def oracle_r2(chroms, phase, w, sub=None):
    parts, l0 = [], 0
    for c in chroms:
        n = c[0].shape[0]
        parts.append(ol.oracle_r2_ld(c[0], phase[l0:l0 + n], c[1], w, idx=sub))
        l0 += n
    return np.concatenate(parts, axis=0)


@functools.lru_cache(maxsize=None)
def oracle_weights(nind, w, phased, subname):
    """the oracle's weights of a case; computed once, never written to"""
    chroms, phase, subs = panel(nind, w)
    return oracle_r2(chroms, phase, w, subs[subname]) if phased else oracle_ld(chroms, w, subs[subname])


# ------------------------------------------------------------------------------------------- integer references in numpy

def _sel(nind, sub):
    return np.arange(nind) if sub is None else np.asarray(sub, dtype=np.int64)


def locus_counts(chroms):
    """[nloci][2] int64 = {#homozygous, #non-missing} over ALL individuals"""
    g = np.concatenate([c[0] for c in chroms], axis=0)
    present = g != -9
    hom = present & (g != 1)
    return np.stack([hom.sum(axis=1), present.sum(axis=1)], axis=1).astype(np.int64)


def _band(full, w):
    """out[i][d] = full[i][i + d] for d = 1 .. w-1 with i + d inside the matrix, 0 elsewhere and at d = 0"""
    n = full.shape[0]
    out = np.zeros((n, w), dtype=np.int64)
    for d in range(1, min(w, n)):
        out[:n - d, d] = np.diagonal(full, d)
    return out


def _gram(a, b=None):
    """a @ b.T of 0 / 1 matrices: float64 products of integers below 2^53 are exact, and BLAS runs them"""
    a = a.astype(np.float64)
    b = a if b is None else b.astype(np.float64)
    return np.rint(a @ b.T).astype(np.int64)


def pair_counts(chroms, w, sub=None):
    """[nloci][w][2] int64 = {tot, HAB} of the SNPs (l, l + d) over the subsample, d = 1 .. w-1 inside the chromosome; 0
    elsewhere and at d = 0"""
    out = []
    for c in chroms:
        g = c[0][:, _sel(c[0].shape[1], sub)]
        present = g != -9
        hom = present & (g != 1)
        out.append(np.stack([_band(_gram(present), w), _band(_gram(hom), w)], axis=2))
    return np.concatenate(out, axis=0)


def phased_pair_counts(chroms, phase, w, sub=None):
    """[nloci][w][2] int64 = {2 * #(both non-missing), x11}, x11 = 2 #(2,2) + #(1,2) + #(2,1) + #(1,1 and firstCopy equal)"""
    out, l0 = [], 0
    for c in chroms:
        sel = _sel(c[0].shape[1], sub)
        n = c[0].shape[0]
        g = c[0][:, sel]
        fc = phase[l0:l0 + n][:, sel] != 0
        l0 += n
        two, one = g == 2, g == 1
        o1, o0 = one & fc, one & ~fc
        x11 = 2 * _gram(two) + _gram(one, two) + _gram(two, one) + _gram(o1) + _gram(o0)
        out.append(np.stack([_band(2 * _gram(g != -9), w), _band(x11, w)], axis=2))
    return np.concatenate(out, axis=0)


def brute_counts(geno, w, sub=None, phase=None):
    """the same counts by a triple loop over (l, d, individual) on ONE chromosome: the definition, for the small-panel check"""
    n, nind = geno.shape
    sel = _sel(nind, sub)
    loc = np.zeros((n, 2), dtype=np.int64)
    pair = np.zeros((n, w, 2), dtype=np.int64)
    for l in range(n):
        for k in range(nind):
            if geno[l, k] != -9:
                loc[l, 1] += 1
                loc[l, 0] += geno[l, k] != 1
        for d in range(1, w):
            if l + d >= n:
                break
            for k in sel:
                a, b = geno[l, k], geno[l + d, k]
                if a == -9 or b == -9:
                    continue
                if phase is None:
                    pair[l, d, 0] += 1
                    pair[l, d, 1] += a != 1 and b != 1
                else:
                    pair[l, d, 0] += 2
                    if a == 2 and b == 2:
                        pair[l, d, 1] += 2
                    elif a + b == 3:
                        pair[l, d, 1] += 1
                    elif a == 1 and b == 1 and phase[l, k] == phase[l + d, k]:
                        pair[l, d, 1] += 1
    return loc, pair


# ---------------------------------------------------------------------------------------- the floating-point part, restated

def ld_from_counts(n, w, fa, pair):
    """LD [n][w] of ONE chromosome from its per-SNP frequencies fa (homFreq; phased: the allele frequencies) and its pair
    counts [n][w][2]: hr2 / r2 (garlic-data.cpp:558-617) with the counts already taken, then the ordered window sums
    (garlic-data.cpp:521-527) -- term i = s .. s+w-1 in that order from 0.0, 1.0 where i is the column's SNP"""
    c = np.zeros((n, n), dtype=np.float64)                    # c[i][j]: the pair's value as SNP i's term, |i - j| < w
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (fa > 0) & (fa < 1)
        for d in range(1, min(w, n)):
            i = np.arange(n - d)
            j = i + d
            hab = pair[i, d, 1].astype(np.float64) / pair[i, d, 0].astype(np.float64)
            for a, b in ((i, j), (j, i)):                     # not symmetric: the denominator is multiplied in argument order
                h = hab - fa[a] * fa[b]
                v = h * h / (((fa[a] * (1 - fa[a])) * fa[b]) * (1 - fa[b]))
                v = np.where(v > 1, 1.0, v)
                c[a, b] = np.where(ok[a] & ok[b], v, 0.0)
        np.fill_diagonal(c, 1.0)
        ld = np.zeros((n, w), dtype=np.float64)
        ns = n - w + 1
        if ns > 0:
            s = np.arange(ns)[:, None]
            t = s + np.arange(w)[None, :]
            acc = np.zeros((ns, w), dtype=np.float64)
            for j in range(w):
                acc = acc + c[s + j, t]
            ld[:ns] = acc
    return ld


def hom_freq(loc):
    with np.errstate(invalid="ignore", divide="ignore"):
        return loc[:, 0].astype(np.float64) / loc[:, 1].astype(np.float64)
