"""Panels, poisons and oracle answers of tests/test_gpu_caller_stream.py; importable without a GPU.

Every delayed-input case of that file puts a POISON into the buffer the library will read and the real data behind a delay on
the caller's stream.  A case tests something only if the poison's answer is another one than the real data's, so every
`*_and_poison` function here computes both with the CPU oracle and asserts that they differ in every chromosome that holds a
window (one shorter than the window is MISSING, and without LD weights, whatever the data say), census rows in every chromosome.
The poisons: all-missing genotypes (-9; .bed code 1), likelihoods of 0.5, LD weights of 0, phase bits of 0, counts of 0, scores
of NaN."""
import functools

import numpy as np

import bed_cases
import oracle_lib as ol

MG, ERROR, M, MU = 200000, 0.001, 7, 1e-9
SIZES = [900, 410, 64, 7]            # the last is shorter than every window below
NINDS = [70, 130]                    # ragged 64-individual blocks: 1 + 6 and 2 + 2
SCORE_WS = [10, 50]
WLOD_WS = [10, 100]                  # stream / strip forms of the weighted kernels
TGLS_WS = [40, 200]                  # both sides of the one-stream ring's 144
FRAC = 0.25
GL_VALUES = np.array([1e-6, 1e-3, 0.01, 0.2])      # bounded: the TGLS ring forms are due
GL_POISON = 0.5


@functools.lru_cache(maxsize=None)
def panel(nind, gaps=True, seed=0):
    """(chroms, gpos): chroms as oracle_lib.random_panel's tuples.  gaps False: no hole wider than max_gap, no centromere"""
    rng = np.random.default_rng(9300 + nind + 1000 * seed + (0 if gaps else 7))
    chroms = [ol.random_panel(rng, n, nind, max_gap=MG, gaps=2 if gaps and n >= 100 else 0, centro=gaps and n >= 100, mono=0.0)
              for n in SIZES]          # (the short chromosomes whole: the one of 64 SNPs holds windows of 10, 40 and 50)
    gpos = [c[2] * 1e-6 for c in chroms]
    return chroms, gpos


def sizes():
    return list(SIZES)


def nloci():
    return sum(SIZES)


def geno_of(chroms):
    return np.ascontiguousarray(np.concatenate([c[0] for c in chroms], axis=0))


def holds_window(W, gaps=True, seed=0):
    """per chromosome: some window of W SNPs is scored (oracle_mask; the map is the same for every individual count)"""
    chroms, _ = panel(NINDS[0], gaps, seed)
    return [bool(ol.oracle_mask(p, cs, ce, W, MG).any()) for g, f, p, cs, ce in chroms]


def _differ(real, poison, W, what):
    """bit patterns differ in every chromosome that holds a window (W None: in every chromosome)"""
    assert len(real) == len(poison) == len(SIZES)
    if W is not None:
        held = holds_window(W)
        assert held == [n >= W for n in SIZES], (what, held)
    for c, n in enumerate(SIZES):
        a, b = np.ascontiguousarray(real[c]), np.ascontiguousarray(poison[c])
        if W is not None and not held[c]:
            continue
        assert a.shape != b.shape or not np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, "poison answers as the data do", c)


# ---- window scores

@functools.lru_cache(maxsize=None)
def lod_scores(nind, W, gaps=True, seed=0):
    chroms, _ = panel(nind, gaps, seed)
    return [ol.oracle_calc_lod(g, f, p, cs, ce, W, ERROR, MG) for g, f, p, cs, ce in chroms]


@functools.lru_cache(maxsize=None)
def lod_scores_and_poison(nind, W):
    """(scores of the panel, scores of the same panel with every genotype missing)"""
    chroms, _ = panel(nind)
    real = lod_scores(nind, W)
    poison = [ol.oracle_calc_lod(np.full_like(g, -9), f, p, cs, ce, W, ERROR, MG) for g, f, p, cs, ce in chroms]
    _differ(real, poison, W, ("genotypes", nind, W))
    return real, poison


@functools.lru_cache(maxsize=None)
def likelihoods(nind):
    """(codes uint8 per chromosome, error probabilities per chromosome)"""
    chroms, _ = panel(nind)
    rng = np.random.default_rng(9350 + nind)
    codes = [rng.integers(0, len(GL_VALUES), size=c[0].shape).astype(np.uint8) for c in chroms]
    return codes, [GL_VALUES[k] for k in codes]


@functools.lru_cache(maxsize=None)
def tgls_scores_and_poison(nind, W):
    chroms, _ = panel(nind)
    _, gl = likelihoods(nind)
    real = [ol.oracle_calc_lod(g, f, p, cs, ce, W, ERROR, MG, gl=gl[c]) for c, (g, f, p, cs, ce) in enumerate(chroms)]
    poison = [ol.oracle_calc_lod(g, f, p, cs, ce, W, ERROR, MG, gl=np.full(g.shape, GL_POISON)) for g, f, p, cs, ce in chroms]
    _differ(real, poison, W, ("likelihoods", nind, W))
    return real, poison


@functools.lru_cache(maxsize=None)
def ld_weights(nind, W):
    rng = np.random.default_rng(9400 + nind + W)
    return [rng.uniform(1.0, max(2.0, W / 4.0), size=(n, W)) for n in SIZES]


@functools.lru_cache(maxsize=None)
def wlod_scores_and_poison(nind, W):
    chroms, gpos = panel(nind)
    lds = ld_weights(nind, W)
    real = [ol.oracle_calc_wlod(g, f, p, gpos[c], lds[c], cs, ce, W, ERROR, MG, MU, M) for c, (g, f, p, cs, ce) in enumerate(chroms)]
    with np.errstate(all="ignore"):
        poison = [ol.oracle_calc_wlod(g, f, p, gpos[c], np.zeros_like(lds[c]), cs, ce, W, ERROR, MG, MU, M)
                  for c, (g, f, p, cs, ce) in enumerate(chroms)]
    _differ(real, poison, W, ("LD weights", nind, W))
    return real, poison


# ---- what reads a score matrix

def flat_feed(scores, step):
    """(the oracle's feed, its per-chromosome counts)"""
    parts = [ol.oracle_flatten(s, step) for s in scores]
    return np.concatenate(parts), [len(x) for x in parts]


@functools.lru_cache(maxsize=None)
def feed_and_poison(nind, W):
    """flatten (step W) of the scores and of a matrix of NaN: the latter is empty"""
    real = [ol.oracle_flatten(s, W) for s in lod_scores(nind, W)]
    poison = [ol.oracle_flatten(np.full_like(s, np.nan), W) for s in lod_scores(nind, W)]
    _differ(real, poison, W, ("flatten", nind, W))
    return np.concatenate(real), [len(x) for x in real]


@functools.lru_cache(maxsize=None)
def cutoff_of(nind, W):
    """a cutoff that leaves windows, covered SNPs and segments to compare: the scored windows' 0.7 quantile"""
    scored = np.concatenate([x[np.isfinite(x) & (x != ol.MISSING)] for x in lod_scores(nind, W)])
    return float(np.quantile(scored, 0.7))


@functools.lru_cache(maxsize=None)
def coverage_and_poison(nind, W):
    """assembleROHWindows' coverage counts of the scores and of a matrix of NaN (no window is >= the cutoff)"""
    cutoff = cutoff_of(nind, W)
    real = [ol.oracle_roh_coverage(s, W, cutoff) for s in lod_scores(nind, W)]
    poison = [ol.oracle_roh_coverage(np.full_like(s, np.nan), W, cutoff) for s in lod_scores(nind, W)]
    _differ(real, poison, W, ("coverage", nind, W))
    return real, poison


def segments(nind, W, frac=FRAC):
    from run_cases import oracle_segments
    chroms, _ = panel(nind)
    return oracle_segments(chroms, lod_scores(nind, W), W, cutoff_of(nind, W), MG, frac)


def score_matrix(scores, base, pitch, total, nind):
    """the oracle's scores in the layout of garlic_lod_out_layout; NaN in the padding"""
    host = np.full(total, np.nan, dtype=np.float64)
    for c, s in enumerate(scores):
        host[base[c]: base[c] + nind * pitch[c]].reshape(nind, pitch[c])[:, :s.shape[1]] = s
    return host


def rows_of(host, base, pitch, nind):
    """per chromosome [nind][nloci_c] of a buffer in that layout"""
    return [np.ascontiguousarray(host[base[c]: base[c] + nind * pitch[c]].reshape(nind, pitch[c])[:, :n]) for c, n in enumerate(SIZES)]


# ---- LD weights

def _per_chr(ld):
    off = np.concatenate([[0], np.cumsum(SIZES)])
    return [ld[off[c]:off[c + 1]] for c in range(len(SIZES))]


@functools.lru_cache(maxsize=None)
def hr2(nind, W):
    chroms, _ = panel(nind)
    return np.concatenate([ol.oracle_hr2_ld(c[0], W) for c in chroms], axis=0)


@functools.lru_cache(maxsize=None)
def hr2_and_poison(nind, W):
    """calcHR2LD's weights, and what zero counts finish to (0/0 everywhere)"""
    real = hr2(nind, W)
    chroms, _ = panel(nind)
    poison = np.concatenate([ol.oracle_hr2_ld(np.full_like(c[0], -9), W) for c in chroms], axis=0)
    _differ(_per_chr(real), _per_chr(poison), W, ("LD counts", nind, W))
    return real


@functools.lru_cache(maxsize=None)
def phase(nind):
    """HapData::firstCopy uint8 [nloci][nind]"""
    return np.random.default_rng(9450 + nind).integers(0, 2, size=(nloci(), nind)).astype(np.uint8)


def phase_rows(first_copy):
    return np.ascontiguousarray(np.packbits(first_copy, axis=1, bitorder="little"))


@functools.lru_cache(maxsize=None)
def r2_and_poison(nind, W):
    """calcR2LD's weights from the phase and from phase bits of 0"""
    chroms, _ = panel(nind)
    off = np.concatenate([[0], np.cumsum(SIZES)])
    def r2(fc):
        return [ol.oracle_r2_ld(g, fc[off[c]:off[c + 1]], f, W) for c, (g, f, *_) in enumerate(chroms)]
    real, poison = r2(phase(nind)), r2(np.zeros_like(phase(nind)))
    _differ(real, poison, W, ("phase bits", nind, W))
    return np.concatenate(real, axis=0)


# ---- PLINK .bed rows

BED_POISON = 0x55                    # four genotypes of code 1: missing


@functools.lru_cache(maxsize=None)
def bed(nind, W):
    """(packed rows, census counts, census counted, oracle scores of the recoded genotypes) on the map and frequencies of
    panel(nind); the poison image recodes to all-missing genotypes and counts nothing"""
    chroms, _ = panel(nind)
    rng = np.random.default_rng(9500 + nind)
    codes = rng.integers(0, 4, size=(nloci(), nind)).astype(np.uint8)
    codes[rng.random(codes.shape) < 0.05] = bed_cases.MISS
    counts, counted = bed_cases.census(codes)
    geno = bed_cases.recode(codes, counted)
    p_counts, p_counted = bed_cases.census(np.full_like(codes, bed_cases.MISS))
    off = np.concatenate([[0], np.cumsum(SIZES)])
    for c in range(len(SIZES)):
        assert not np.array_equal(counts[off[c]:off[c + 1]], p_counts[off[c]:off[c + 1]]), ("census", c)
        assert not np.array_equal(counted[off[c]:off[c + 1]], p_counted[off[c]:off[c + 1]]), ("census", c)
    real = [ol.oracle_calc_lod(np.ascontiguousarray(geno[off[c]:off[c + 1]]), f, p, cs, ce, W, ERROR, MG)
            for c, (g, f, p, cs, ce) in enumerate(chroms)]
    poison = [ol.oracle_calc_lod(np.full_like(g, -9), f, p, cs, ce, W, ERROR, MG) for g, f, p, cs, ce in chroms]
    _differ(real, poison, W, ("bed rows", nind, W))
    rows = bed_cases.pack_rows(codes)
    assert (bed_cases.pack_rows(np.full((1, 4), bed_cases.MISS, dtype=np.uint8), garbage=False) == BED_POISON).all()
    return rows, counts, counted, real


def all_cpu_checks():
    """every poison / data pair of the GPU file, for a run without a GPU"""
    for nind in NINDS:
        for W in SCORE_WS:
            lod_scores_and_poison(nind, W)
            feed_and_poison(nind, W)
            coverage_and_poison(nind, W)
            bed(nind, W)
        for W in TGLS_WS:
            tgls_scores_and_poison(nind, W)
        for W in WLOD_WS:
            wlod_scores_and_poison(nind, W)
        hr2_and_poison(nind, 10)
        r2_and_poison(nind, 10)
        assert len(segments(nind, 10)) > 0
