"""Panels with a dense run structure (plain numpy, no GPU) for tests/test_runs_cpu.py and tests/test_gpu_runs.py.

A run is a maximal stretch of SNPs that no max_gap hole or centromere cuts.  oracle_lib.random_panel has a handful of
holes per chromosome; the panels here have hundreds of runs per chromosome, their lengths drawn from a menu around the
window size W and around the 32-window bit words, so that run heads, tails, MISSING fills of exactly W - 1 columns and
bit words shared by several runs occur at arbitrary columns.

Every case function returns (chroms, guarantees): chroms is a list of (geno, freq, pos, cS, cE) tuples of the shape
oracle_lib.random_panel returns, guarantees a dict computed from oracle_mask and the positions alone (never from a GPU
result).  TEST INFRASTRUCTURE ONLY.
"""
import numpy as np

import oracle_lib as ol

MAX_GAP = 5000
# valid windows per run whose heads and tails the kernels' 32- and 64-window tiles treat differently
VALID_COUNTS = (1, 2, 31, 32, 33, 63, 64, 65)


def menu(W):
    """run lengths in SNPs: no window, one window, a few, around one and two 32-window words, a few windows wide"""
    return [1, W - 1, W, W + 1, W + 2, 2 * W - 1, 2 * W, W + 30, W + 31, W + 32, W + 33, W + 62, W + 63, W + 64, W + 65,
            3 * W + 7]


def draw_lens(rng, W, n_runs=400, max_snps=25000, each=5):
    """`each` runs of every menu length, then random draws from the menu up to n_runs runs or max_snps SNPs; shuffled"""
    m = [x for x in menu(W) if x >= 1]
    lens = m * each
    total = sum(lens)
    while len(lens) < n_runs:
        x = int(rng.choice(m))
        if total + x > max_snps:
            break
        lens.append(x)
        total += x
    lens = np.array(lens)
    rng.shuffle(lens)
    return [int(x) for x in lens]


def _genotypes(rng, W, nind, nloci, miss=0.03, mono=0.01, tracts_per_1000=2.0):
    """HWE draws with missing genotypes, a few freq in {0, 1} survivors (as random_panel), and per individual a few
    homozygous tracts of W .. 6W+40 SNPs: without them too few windows clear a cutoff of 0"""
    freq = rng.uniform(0.02, 0.98, size=nloci)
    k = rng.random(nloci)
    freq[k < mono / 2] = 0.0
    freq[(k >= mono / 2) & (k < mono)] = 1.0
    p = freq[:, None]
    u = rng.random((nloci, nind))
    geno = np.where(u < (1 - p) ** 2, 0, np.where(u < (1 - p) ** 2 + 2 * p * (1 - p), 1, 2)).astype(np.int16)
    # tracts_per_1000 of them per 1000 SNPs, but never more than cover about half of a row (0.7 of it, less their overlaps) at wide windows
    n_tracts = max(2, int(min(round(tracts_per_1000 * nloci / 1000.0), round(0.7 * nloci / (3.5 * W + 20)))))
    for i in range(nind):
        for _ in range(n_tracts):
            n = int(rng.integers(W, 6 * W + 41))
            a = int(rng.integers(0, max(1, nloci - n)))
            seg = geno[a:a + n, i]
            het = seg == 1
            seg[het] = np.where(rng.random(int(het.sum())) < freq[a:a + n][het], 2, 0)
    geno[rng.random((nloci, nind)) < miss] = -9
    return geno, freq


def positions_of(rng, lens, max_gap=MAX_GAP, inner=200, start=None):
    """one chromosome as a concatenation of runs of the given SNP counts: the first step of each run is
    max_gap + 1 + small, the steps inside a run 1 .. inner"""
    nloci = int(sum(lens))
    steps = rng.integers(1, inner + 1, size=nloci).astype(np.int64)
    heads = np.cumsum([0] + list(lens[:-1]))
    steps[heads] = max_gap + 1 + rng.integers(0, 50, size=len(lens))
    if start is not None:
        steps[0] = start
    pos = np.cumsum(steps)
    assert pos[-1] < 2 ** 31
    return pos.astype(np.int32)


def dense_panel(rng, W, nind, lens, max_gap=MAX_GAP, *, centro=(0, 0), start=None, tracts_per_1000=2.0):
    """-> (geno, freq, pos, cS, cE), the tuple shape of oracle_lib.random_panel"""
    pos = positions_of(rng, lens, max_gap, start=start)
    geno, freq = _genotypes(rng, W, nind, pos.shape[0], tracts_per_1000=tracts_per_1000)
    return geno, freq, pos, int(centro[0]), int(centro[1])


# ---------------------------------------------------------------------------------------------- what a panel guarantees

def breaks_of(pos, cS, cE, max_gap):
    """bool [nloci]: SNP l starts a run (l = 0, or the pair (l-1, l) is more than max_gap apart or touches the
    centromere: inGap's three clauses, restated in numpy)"""
    p = np.asarray(pos, dtype=np.int64)
    b = np.ones(p.shape[0], dtype=bool)
    if p.shape[0] > 1:
        q0, q1 = p[:-1], p[1:]
        gap = (cS <= q0) & (cE >= q0) | (cS <= q1) & (cE >= q1) | (cS >= q0) & (cE <= q1)
        b[1:] = (q1 - q0 > max_gap) | gap
    return b


def n_boundaries(chroms, max_gap):
    """run starts over all chromosomes (each chromosome's first SNP is one)"""
    return int(sum(np.count_nonzero(breaks_of(c[2], c[3], c[4], max_gap)) for c in chroms))


def guarantees(chroms, W, max_gap=MAX_GAP, scores=None, cutoffs=()):
    """From oracle_mask and the positions: runs, runs by valid-window count, 32-bit words (chromosome-local SNP index
    // 32, the bit rows' words) that hold valid windows of >= 2 and >= 3 runs, words with >= 2 break bits, the share of
    valid windows; with the oracle's scores also the share of valid windows at or above each cutoff."""
    g = {"n_snps": 0, "n_runs": 0, "runs_by_valid": {k: 0 for k in VALID_COUNTS}, "words_2runs": 0, "words_3runs": 0,
         "words_2breaks": 0, "valid_share": 0.0, "share_at_or_above": {}}
    n_valid = 0
    for (geno, freq, pos, cS, cE) in chroms:
        n = pos.shape[0]
        brk = breaks_of(pos, cS, cE, max_gap)
        run_id = np.cumsum(brk) - 1
        valid = ol.oracle_mask(pos, cS, cE, W, max_gap).astype(bool)
        # the mask is the run structure seen through W: a window is valid iff its W SNPs lie in one run
        run_len = np.bincount(run_id)
        off = np.arange(n) - np.flatnonzero(brk)[run_id]
        assert W < 2 or np.array_equal(valid, off + W <= run_len[run_id])
        g["n_snps"] += n
        g["n_runs"] += int(run_len.shape[0])
        per_run = np.bincount(run_id[valid], minlength=run_len.shape[0])
        for k in VALID_COUNTS:
            g["runs_by_valid"][k] += int(np.count_nonzero(per_run == k))
        word = np.arange(n) // 32
        nw = int(word[-1]) + 1
        pairs = np.unique(np.stack([word[valid], run_id[valid]], axis=1), axis=0) if valid.any() else np.zeros((0, 2), int)
        runs_in_word = np.bincount(pairs[:, 0], minlength=nw)
        g["words_2runs"] += int(np.count_nonzero(runs_in_word >= 2))
        g["words_3runs"] += int(np.count_nonzero(runs_in_word >= 3))
        g["words_2breaks"] += int(np.count_nonzero(np.bincount(word[brk], minlength=nw) >= 2))
        n_valid += int(np.count_nonzero(valid))
    g["valid_share"] = n_valid / max(1, g["n_snps"])
    if scores is not None:
        v = np.concatenate([s[s != ol.MISSING].ravel() for s in scores])
        for c in cutoffs:
            g["share_at_or_above"][c] = float(np.count_nonzero(v >= c)) / max(1, v.shape[0])
    return g


def oracle_segments(chroms, scores, W, cutoff, mg, frac):
    """the oracle's scores through the oracle's inWin[] loop and its restatement of the segment walk (pinned against the
    real assembleROHWindows in tests/test_oracle_vs_ref.py) -> [(individual, chromosome, first SNP, last SNP)] in the
    reference's order"""
    out = []
    for c, (g, f, p, cs, ce) in enumerate(chroms):
        cov = ol.oracle_roh_coverage(np.ascontiguousarray(scores[c]), W, cutoff)
        out += [(i, c, a, b) for i, a, b in ol.oracle_roh_segments(cov, p, cs, ce, W, mg, frac)]
    return sorted(out)


# ---------------------------------------------------------------------------------------------- the named cases

def _snp_budget(W):
    return 25000 if W <= 150 else 36000


def dense(W, nind, seed=1, max_gap=MAX_GAP):
    """one chromosome of about 400 runs (fewer at wide windows: at most 25k SNPs, 36k at W > 150)"""
    rng = np.random.default_rng([seed, W, 11])
    lens = draw_lens(rng, W, max_snps=_snp_budget(W))
    chroms = [dense_panel(rng, W, nind, lens, max_gap)]
    return chroms, guarantees(chroms, W, max_gap)


def centromere(W, nind, seed=1, max_gap=MAX_GAP):
    """no holes at all.  Chromosome 0: the centromere holds 120 SNPs, cS == pos[a] and cE == pos[b] exactly (120
    consecutive one-SNP runs, the closed ends of inGap).  Chromosome 1: a centromere that holds no SNP, strictly
    between two neighbours less than max_gap apart (inGap's third clause).  Chromosome 2: (0, 0)."""
    rng = np.random.default_rng([seed, W, 12])
    chroms = []
    n0 = 3000 + 3 * W
    g, f, p, _, _ = dense_panel(rng, W, nind, [n0], max_gap)
    a = 1000 + int(rng.integers(0, 32))
    b = a + 119
    chroms.append((g, f, p, int(p[a]), int(p[b])))
    n1 = 1500 + 2 * W
    g, f, p, _, _ = dense_panel(rng, W, nind, [n1], max_gap)
    k = 700 + int(rng.integers(0, 32))
    p = p.copy()
    p[k + 1:] += 10                                    # room for a centromere strictly between SNPs k and k + 1
    assert 2 < p[k + 1] - p[k] < max_gap
    chroms.append((g, f, p, int(p[k]) + 1, int(p[k + 1]) - 1))
    chroms.append(dense_panel(rng, W, nind, [900 + W], max_gap))
    gu = guarantees(chroms, W, max_gap)
    gu["centromere_snps"] = b - a + 1
    return chroms, gu


BORDER_LOCI = (63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096)   # global loci that start a run
BORDER_STRETCH = (1900, 2200)                                           # 300 consecutive boundaries across locus 2048


def borders(W, nind, seed=1, max_gap=MAX_GAP):
    """boundaries placed by global index: next to the 64-lane wave borders, the 256-thread stride and the 2048-SNP
    workgroup borders of the boundary kernels, and a stretch where every SNP is one.  The first chromosome is 5 SNPs
    long, so chromosome-local and global indices differ."""
    rng = np.random.default_rng([seed, W, 13])
    first = dense_panel(rng, W, nind, [5], max_gap)
    n = 4600
    starts = sorted(set(BORDER_LOCI) | set(range(*BORDER_STRETCH)))
    local = [0] + [s - 5 for s in starts]
    lens = [b - a for a, b in zip(local, local[1:] + [n])]
    second = dense_panel(rng, W, nind, lens, max_gap)
    chroms = [first, second]
    gu = guarantees(chroms, W, max_gap)
    brk = breaks_of(second[2], 0, 0, max_gap)
    assert sorted(int(x) + 5 for x in np.flatnonzero(brk)[1:]) == starts
    return chroms, gu


def all_breaks(W, nind, seed=1, max_gap=MAX_GAP, nloci=4500):
    """every neighbouring pair more than max_gap apart: no valid window for W >= 2"""
    rng = np.random.default_rng([seed, W, 14])
    chroms = [dense_panel(rng, W, nind, [1] * nloci, max_gap), dense_panel(rng, W, nind, [1] * 70, max_gap)]
    gu = guarantees(chroms, W, max_gap)
    assert gu["n_runs"] == nloci + 70 and (W < 2 or gu["valid_share"] == 0.0)
    return chroms, gu


def many_blocks(W=2, nind=8, seed=1, max_gap=MAX_GAP, nloci=140000):
    """140,000 SNPs in about 9,000 runs: 69 workgroups of 2048 SNPs, so the carry loop of the boundary scan runs twice"""
    rng = np.random.default_rng([seed, W, 15])
    m = menu(2) + [1, 2, 3, 4, 5, 6, 7, 8] * 2
    lens, total = [], 0
    while total < nloci:
        x = min(int(rng.choice(m)), nloci - total)
        lens.append(x)
        total += x
    chroms = [dense_panel(rng, W, nind, lens, max_gap, tracts_per_1000=0.2)]
    return chroms, guarantees(chroms, W, max_gap)


def from_zero(W, nind, seed=1, max_gap=MAX_GAP):
    """a dense chromosome shifted to start at position 0, its first break inside word 0, beside one that does not
    start at 0"""
    rng = np.random.default_rng([seed, W, 16])
    lens = draw_lens(rng, W, n_runs=150, max_snps=9000, each=2)
    short = [x for x in lens if x < 32]
    lens.remove(short[0])
    lens.insert(0, short[0])
    g, f, p, cs, ce = dense_panel(rng, W, nind, lens, max_gap)
    p = (p - p[0]).astype(np.int32)
    chroms = [(g, f, p, 0, 0), dense_panel(rng, W, nind, draw_lens(rng, W, n_runs=60, max_snps=5000, each=1), max_gap)]
    gu = guarantees(chroms, W, max_gap)
    assert chroms[0][2][0] == 0 and breaks_of(p, 0, 0, max_gap)[1:32].any() and chroms[1][2][0] > 0
    return chroms, gu


CASES = {"dense": dense, "centromere": centromere, "borders": borders, "all_breaks": all_breaks, "from_zero": from_zero}
