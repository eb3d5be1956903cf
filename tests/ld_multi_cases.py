"""Cases and restatements for the multi-size LD weights (garlic_panel_compute_ld_multi); importable without a GPU.

  groups_of      the grouping rule of include/garlic_hip.h, restated
  shared_pass    the shared pass in plain numpy: pair values from the formula in the header of ld_kernels.hpp, ONE
                 left-to-right accumulation at the largest size, truncated at the chromosome end, snapshots after W_i terms
"""
import functools

import numpy as np

import oracle_lib as ol

LDM_MAX_SIZES = 4
LDS_MAX = 128 * 1024
MG, ERROR, M, MU = 200000, 0.001, 7, 1e-9

# the size lists, chosen on the limits the code has
SIZE_LISTS = [
    [33, 34],                 # the narrowest sharing sizes
    [33, 64, 65, 100],        # a full group; 64 / 65: a size at and past a whole wave
    [100, 50, 100],           # unordered, with a repeat
    [16, 32, 33, 40],         # 32 and below do not share
    [40, 100, 129, 130],      # 130 leaves the fused MFMA pair form
    [34, 36, 38, 40, 42],     # LDM_MAX_SIZES + 1 sharing sizes: two groups
]
NINDS = [40, 64, 150]


def shares(w):
    """the size takes the SNP-per-thread sum kernel (no sum-form switch set)"""
    return 32 < w <= 512


def lds_bytes(w, n):
    """LDS of a shared pass whose largest size is w and that serves n sizes"""
    t = (w + 16 + 63) // 64 * 64
    ring = 2048 * ((t + 127) // 128) + 130
    return 8 * max(ring + (n - 1) * 9 * t, 17 * t)


def groups_of(sizes, solo=False):
    """(groups, n_shared): the shared groups in ascending order, then the sizes on their own, ascending"""
    uniq = sorted(set(int(w) for w in sizes))
    sharing = [w for w in uniq if shares(w) and not solo]
    if len(sharing) < 2:
        sharing = []
    groups = []
    for w in sharing:
        if groups and len(groups[-1]) < LDM_MAX_SIZES and lds_bytes(w, len(groups[-1]) + 1) <= LDS_MAX:
            groups[-1].append(w)
        else:
            groups.append([w])
    n_shared = len(groups)
    groups += [[w] for w in uniq if w not in sharing]
    return groups, n_shared


def passes_of(sizes, solo=False):
    """(pair stages, sum passes) the rule predicts"""
    groups, n_shared = groups_of(sizes, solo)
    alone = len(groups) - n_shared
    return (1 if n_shared else 0) + alone, n_shared + alone


def group_index(sizes, solo=False):
    """{size: index of its group}"""
    groups, _ = groups_of(sizes, solo)
    return {w: g for g, grp in enumerate(groups) for w in grp}


def chrom_sizes(sizes):
    wmin, wmax = min(sizes), max(sizes)
    return [1, wmin - 1, wmin, wmin + 1, wmax - 1, wmax, wmax + 1, wmax + 31, wmax + 32, wmax + 33, 400]


def make_chroms(sizes, nind, seed, max_gap=10 ** 9, gaps=0):
    """one chromosome per length of chrom_sizes, 5 % missing; in the last (400 SNPs): a monomorphic, an all-heterozygous and
    an all-missing SNP"""
    rng = np.random.default_rng(seed)
    chroms = [list(ol.random_panel(rng, n, nind, max_gap=max_gap, gaps=gaps, miss=0.05)) for n in chrom_sizes(sizes)]
    g = chroms[-1][0]
    g[5, :] = 2
    g[9, :] = 1
    g[13, :] = -9
    return chroms


@functools.lru_cache(maxsize=None)
def case(list_index, nind):
    """(chroms, sub, {W: oracle LD of everyone}, {W: oracle LD of the subsample}); computed once, never written to"""
    sizes = SIZE_LISTS[list_index]
    chroms = make_chroms(sizes, nind, 7000 + 10 * list_index + nind)
    rng = np.random.default_rng(list_index + nind)
    sub = np.sort(rng.choice(nind, size=max(2, nind // 3), replace=False)).astype(np.int32)
    return chroms, sub, oracle_ld(chroms, sizes), oracle_ld(chroms, sizes, sub)


def oracle_ld(chroms, sizes, sub=None):
    return {w: np.concatenate([ol.oracle_hr2_ld(c[0], w, idx=sub) for c in chroms], axis=0) for w in sorted(set(sizes))}


def oracle_r2(chroms, phase, sizes, sub=None):
    out = {}
    for w in sorted(set(sizes)):
        parts, l0 = [], 0
        for c in chroms:
            parts.append(ol.oracle_r2_ld(c[0], phase[l0:l0 + c[0].shape[0]], c[1], w, idx=sub))
            l0 += c[0].shape[0]
        out[w] = np.concatenate(parts, axis=0)
    return out


def rows_without_window(chroms, w):
    """global indices of the window starts that have no full window of w inside their chromosome"""
    rows, l0 = [], 0
    for c in chroms:
        n = c[0].shape[0]
        rows += list(range(l0 + max(0, n - w + 1), l0 + n))
        l0 += n
    return np.asarray(rows, dtype=np.int64)


# ---------------------------------------------------------------------------------------------- the shared pass, restated

def pair_values(geno, idx=None):
    """c[i][j] = hr2(i, j) as SNP i's term (the formula is not symmetric in floating point), 1.0 on the diagonal"""
    geno = np.asarray(geno)
    nloci, nind = geno.shape
    present = geno != -9
    hom = present & ((geno == 0) | (geno == 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        hf = hom.sum(axis=1).astype(np.float64) / present.sum(axis=1).astype(np.float64)      # over every individual
        sel = np.arange(nind) if idx is None else np.asarray(idx, dtype=np.int64)
        m = present[:, sel].astype(np.float64)             # counts as sums of 0 / 1 products: exact in float64
        h = hom[:, sel].astype(np.float64)
        total = m @ m.T
        hab = h @ h.T
        hab = hab / total
        ha, hb = hf[:, None], hf[None, :]
        hh = hab - ha * hb
        v = hh * hh / (((ha * (1 - ha)) * hb) * (1 - hb))
        v = np.where(v > 1, 1.0, v)
        ok = (hf > 0) & (hf < 1)
        c = np.where(ok[:, None] & ok[None, :], v, 0.0)
    np.fill_diagonal(c, 1.0)
    return c


def shared_pass(geno, sizes, idx=None):
    """{W: LD [nloci][W]} of one chromosome from one accumulation at max(sizes)"""
    sizes = sorted(set(int(w) for w in sizes))
    wmax = sizes[-1]
    n = geno.shape[0]
    c = pair_values(geno, idx)
    out = {w: np.zeros((n, w), dtype=np.float64) for w in sizes}
    acc = np.zeros((n, wmax), dtype=np.float64)           # acc[s][k]: the running sum of LD[s][k]
    s = np.arange(n)[:, None]
    k = np.arange(wmax)[None, :]
    t = s + k                                             # the column's SNP
    cpad = np.zeros((n + wmax, n + wmax), dtype=np.float64)
    cpad[:n, :n] = c
    for j in range(min(wmax, n)):                         # term j of every start: SNP i = s + j
        live = (s + j < n) & (t < n)                      # the accumulation stops at the chromosome's last SNP
        acc = np.where(live, acc + cpad[s + j, t], acc)
        for w in sizes:
            if j == w - 1 and n - w + 1 > 0:              # snapshot after w terms, for the starts with a full window
                out[w][:n - w + 1, :] = acc[:n - w + 1, :w]
    return out
