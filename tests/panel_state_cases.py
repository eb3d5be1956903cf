"""A host model of one garlic_panel's inputs, the setters that change them and the consumers that read them; importable
without a GPU.

  Model        plain numpy state: genotypes, freq, pos, gpos, centromeres, likelihoods (or none), first-copy phase, the LD
               weights per installed window size, the term budget and feed order, and the call arguments (W, error, max_gap,
               M, mu, LD subsample)
  Setter       name + fn(model, rng) -> apply(panel, ctx): fn changes the model and returns what does the same to an
               abi.Panel.  `clears` names the caches of garlic_hip.hip the change has to invalidate.  neutral: no input changes
               (release_scratch, the term budget): the oracle's answers must stay what they were
  oracle()     the oracle's answer of one consumer for the model's state at this moment (tests/oracle_lib.py); gpu() the
               library's; same() the comparison: bit for bit, segments as sorted tuples, counts with array_equal
  SCRIPTS      one named script per cached thing of the panel: build, run the consumers, then per transition apply one setter
               and run the consumers again.  A consumer written "=name" is one the script's transitions leave unchanged
               on purpose (the raw scores after a change of M or mu): it is there for the order of the calls
  random_plan  the 25 steps of one seed, drawn from setters and consumers before anything runs
"""
import numpy as np

import oracle_lib as ol
from feed_sort_cases import sorted_by_key

MISSING = ol.MISSING
ERR_STATE = 3                      # abi.ERR_STATE: the documented code of a call whose precondition fails
DICT, CONT, DICT16 = 1, 2, 3       # abi.TGLS_*
FEED_SORTED = 1                    # abi.FEED_ORDER_SORTED
CUT, FRAC, STEP = 0.0, 0.25, 5
W_OTHER = 33                       # the second size of the multi-size feeds
EXACT_LIMIT = -9990.0              # lod_exact_needed: W * (most negative finite term) <= this -> the by-value chain may run


class Model:
    def __init__(self, seed, W=20, nind=70, sizes=None, max_gap=200000):
        rng = np.random.default_rng(seed)
        self.sizes = [600, 129, W - 1] if sizes is None else list(sizes)
        self.nind, self.nloci = nind, sum(self.sizes)
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        chroms = [ol.random_panel(rng, n, nind, max_gap=max_gap, miss=0.03, gaps=2 if n > 50 else 0) for n in self.sizes]
        self.geno = plant_roh(rng, np.concatenate([c[0] for c in chroms], axis=0))
        self.freq = np.concatenate([c[1] for c in chroms])
        self.pos = np.concatenate([c[2] for c in chroms])
        self.cs = [c[3] for c in chroms]
        self.ce = [c[4] for c in chroms]
        self.gpos = new_gpos(rng, self)
        self.gl, self.gl_mode, self.gl_dict, self.gl_codes = None, 0, set(), None
        self.phase, self.have_phase = np.zeros((self.nloci, nind), dtype=np.uint8), False
        self.ld = {}
        self.budget, self.feed_order = 0, 0
        self.W, self.error, self.max_gap, self.M, self.mu, self.sub = W, 0.001, max_gap, 7, 1e-9, None
        self.planes_made = False       # an LD call has run: the bit planes of (genotypes, subsample) are cached
        self.cache = {}

    def chrom(self, c, a):
        return a[self.off[c]: self.off[c + 1]]

    def touched(self):
        self.cache = {}


def plant_roh(rng, geno):
    """homozygous stretches of 30 to 120 SNPs in every third individual: windows above the cutoff, ROH segments to find"""
    nloci, nind = geno.shape
    for i in range(0, nind, 3):
        for _ in range(3):
            n = int(rng.integers(30, 121))
            a = int(rng.integers(0, max(1, nloci - n)))
            g = geno[a:a + n, i]
            g[g == 1] = 2 * rng.integers(0, 2, size=int(np.count_nonzero(g == 1)))
    return geno


def new_gpos(rng, m):
    out = []
    for c in range(len(m.sizes)):
        p = m.chrom(c, m.pos)
        out.append(np.cumsum(np.diff(p, prepend=0) * 1e-6 * rng.uniform(0.5, 1.5, size=p.shape[0])))
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------------------------ the oracle

def scores(m, kind, W=None):
    """per chromosome [nind][nloci_c]: kind lod, lod_gl, wlod or wlod_gl, for the model's arguments"""
    W = m.W if W is None else W
    key = (kind, W, m.error, m.max_gap, m.M, m.mu)
    if key not in m.cache:
        out = []
        for c in range(len(m.sizes)):
            g, f, p = m.chrom(c, m.geno), m.chrom(c, m.freq), m.chrom(c, m.pos)
            gl = m.chrom(c, m.gl) if kind.endswith("_gl") else None
            if kind.startswith("wlod"):
                out.append(ol.oracle_calc_wlod(g, f, p, m.chrom(c, m.gpos), m.chrom(c, m.ld[W]), m.cs[c], m.ce[c], W, m.error,
                                               m.max_gap, m.mu, m.M, gl=gl))
            else:
                out.append(ol.oracle_calc_lod(g, f, p, m.cs[c], m.ce[c], W, m.error, m.max_gap, gl=gl))
        m.cache[key] = out
    return m.cache[key]


def subset_idx(m):
    return np.array([m.nind - 1, 3, 64 % m.nind, 0, 17], dtype=np.int32)


def _feed(m, kind, W, step, idx=None):
    sc = scores(m, kind, W)
    parts = [ol.oracle_flatten(x, step) if idx is None else ol.oracle_flatten_subset(x, step, idx) for x in sc]
    feed = np.concatenate(parts)
    return (sorted_by_key(feed) if m.feed_order == FEED_SORTED else feed), [len(x) for x in parts]


def _cov(m, kind):
    return [ol.oracle_roh_coverage(np.ascontiguousarray(x), m.W, CUT) for x in scores(m, kind)]


def _seg(m, kind):
    out = []
    for c, cov in enumerate(_cov(m, kind)):
        out += [(i, c, a, b) for i, a, b in ol.oracle_roh_segments(cov, m.chrom(c, m.pos), m.cs[c], m.ce[c], m.W, m.max_gap, FRAC)]
    return sorted(out)


def _ld(m, W, phased):
    if phased:
        return np.concatenate([ol.oracle_r2_ld(m.chrom(c, m.geno), m.chrom(c, m.phase), m.chrom(c, m.freq), W, idx=m.sub)
                               for c in range(len(m.sizes))], axis=0)
    return np.concatenate([ol.oracle_hr2_ld(m.chrom(c, m.geno), W, idx=m.sub) for c in range(len(m.sizes))], axis=0)


def exact_needed(m, W=None):
    """lod_exact_needed for the unweighted --error scores, from the model: the most negative finite term of the per-SNP
    table {lod(0), lod(1), lod(2)} (and +0.0 for a missing genotype and the pad rows) times W against -9990"""
    W = m.W if W is None else W
    tmin = 0.0
    for f in m.freq:
        for g in (0, 1, 2):
            t = ol.oracle().oracle_lod(g, float(f), m.error)
            if np.isfinite(t):
                tmin = min(tmin, t)
    return W * tmin <= EXACT_LIMIT


def chain_kind(m):
    """garlic_panel_chain_kind after the unweighted score call: 0 the tuned chain alone; 1 its scored windows were scanned for the
    value -9999.0 and none held it; 2 one did and the by-value chain ran"""
    if not exact_needed(m):
        return 0
    for c, sc in enumerate(scores(m, "lod")):
        valid = ol.oracle_mask(m.chrom(c, m.pos), m.cs[c], m.ce[c], m.W, m.max_gap).astype(bool)
        if np.any(sc[:, valid] == MISSING):
            return 2
    return 1


# consumer -> (what it needs, kind of comparison).  needs: "ld" weights for W and gpos, "gl" likelihoods, "phase"
CONSUMERS = {
    "lod32": ((), "scores"), "lod1": ((), "scores"), "lod_gl": (("gl",), "scores"),
    "wlod": (("ld",), "scores"), "wlod_gl": (("ld", "gl"), "scores"),
    "feed": ((), "feed"), "feed_w": (("ld",), "feed"), "feed_gl": (("gl",), "feed"), "feed_subset": ((), "feed"),
    "feed_multi": ((), "feeds"), "feed_multi_tgls": (("gl",), "feeds"),
    "cov": ((), "counts"), "cov_w": (("ld",), "counts"), "cov_gl": (("gl",), "counts"),
    "seg": ((), "segments"), "seg_w": (("ld",), "segments"), "seg_gl": (("gl",), "segments"),
    "ld": ((), "ld"), "ld_phased": (("phase",), "ld"),
    "chain_kind": ((), "int"),
}
_KIND = {"": "lod", "_w": "wlod", "_gl": "lod_gl"}


def refused(m, name):
    """the error code the library must answer when the state lacks what the consumer needs, else None"""
    for need in CONSUMERS[name][0]:
        if (need == "ld" and m.W not in m.ld) or (need == "gl" and m.gl is None) or (need == "phase" and not m.have_phase):
            return ERR_STATE
    return None


def oracle(m, name):
    """the oracle's answer for the state at this moment.  ld / ld_phased also install their weights in the model, as
    garlic_panel_compute_ld does in the panel (every other installed size goes)."""
    if name in ("lod32", "lod1"):
        return scores(m, "lod")
    if name in ("lod_gl", "wlod", "wlod_gl"):
        return scores(m, name)
    if name.startswith("feed_multi"):
        kind = "lod_gl" if name.endswith("tgls") else "lod"
        return [_feed(m, kind, W, s) for W, s in ((m.W, max(4, m.W)), (W_OTHER, STEP))]
    if name == "feed_subset":
        return _feed(m, "lod", m.W, STEP, subset_idx(m))
    if name.startswith("feed"):
        return _feed(m, _KIND[name[4:]], m.W, STEP)
    if name.startswith("cov"):
        return _cov(m, _KIND[name[3:]])
    if name.startswith("seg"):
        return _seg(m, _KIND[name[3:]])
    if name in ("ld", "ld_phased"):
        w = _ld(m, m.W, name == "ld_phased")
        m.ld = {m.W: w}
        m.planes_made = True
        m.touched()
        return w
    if name == "chain_kind":
        return chain_kind(m)
    raise KeyError(name)


def gpu(panel, m, name):
    """the library's answer in the oracle's form"""
    a = (m.W, m.error, m.max_gap)
    wk = dict(M=m.M, mu=m.mu)
    if name in ("lod32", "lod1"):
        return [np.ascontiguousarray(x) for x in panel.lod_windows(*a, pitch_align=32 if name == "lod32" else 1)]
    if name == "lod_gl":
        return [np.ascontiguousarray(x) for x in panel.lod_windows(*a, pitch_align=32, use_gl=True)]
    if name in ("wlod", "wlod_gl"):
        return [np.ascontiguousarray(x) for x in panel.wlod_windows(*a, m.M, m.mu, pitch_align=32, use_gl=name == "wlod_gl")]
    if name.startswith("feed_multi"):
        sizes, steps = [m.W, W_OTHER], [max(4, m.W), STEP]
        if name.endswith("tgls"):
            feeds, per = panel.lod_feed_multi_tgls(sizes, m.max_gap, steps=steps)
        else:
            feeds, per = panel.lod_feed_multi(sizes, m.error, m.max_gap, steps=steps)
        return [(np.array(f), [int(v) for v in p]) for f, p in zip(feeds, per)]
    if name.startswith("feed"):
        feed, per = panel.lod_feed(*a, STEP, use_gl=name == "feed_gl", weighted=name == "feed_w",
                                   ind_idx=subset_idx(m) if name == "feed_subset" else None, **wk)
        return feed, [int(v) for v in per]
    if name.startswith("cov"):
        cov = panel.roh_coverage_fused(*a, CUT, pitch_align=8 if name == "cov" else 1, use_gl=name == "cov_gl",
                                       weighted=name == "cov_w", **wk)
        return [np.ascontiguousarray(x[:, :n]) for x, n in zip(cov, m.sizes)]
    if name.startswith("seg"):
        rows = panel.roh_segments(*a, CUT, FRAC, use_gl=name == "seg_gl", weighted=name == "seg_w", **wk)
        return sorted(tuple(int(v) for v in r) for r in rows)
    if name in ("ld", "ld_phased"):
        return panel.compute_ld(m.W, sub_idx=m.sub, phased=name == "ld_phased")
    if name == "chain_kind":
        panel.lod_windows(*a, pitch_align=32)
        return panel.chain_kind()
    raise KeyError(name)


def same(name, got, want):
    kind = CONSUMERS[name][1]
    if kind in ("scores",):
        return len(got) == len(want) and all(ol.bits_equal(g, w) for g, w in zip(got, want))
    if kind == "feed":
        return list(got[1]) == list(want[1]) and ol.bits_equal(got[0], want[0])
    if kind == "feeds":
        return len(got) == len(want) and all(list(g[1]) == list(w[1]) and ol.bits_equal(g[0], w[0]) for g, w in zip(got, want))
    if kind == "counts":
        return len(got) == len(want) and all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))
    if kind == "segments":
        return got == want
    if kind == "ld":
        return ol.bits_equal(got, want)
    return got == want


def _scored_change(old, new):
    """a value that is a score (not MISSING) now and is not what stood there before"""
    old, new = np.ascontiguousarray(old, dtype=np.float64), np.ascontiguousarray(new, dtype=np.float64)
    if old.shape != new.shape:
        return bool(np.any(new != MISSING))
    return bool(np.any((old.view(np.uint64) != new.view(np.uint64)) & (new != MISSING)))


def differs(name, old, new):
    """the setter between old and new has changed something a stale cache would get wrong: a scored value, a count, a segment"""
    kind = CONSUMERS[name][1]
    if kind == "scores":
        return any(_scored_change(o, n) for o, n in zip(old, new))
    if kind == "feed":
        return _scored_change(old[0], new[0])
    if kind == "feeds":
        return any(_scored_change(o[0], n[0]) for o, n in zip(old, new))      # (the second size is not the model's W)
    if kind == "counts":
        return any(not np.array_equal(o, n) for o, n in zip(old, new))
    if kind == "segments":
        return len(set(old) ^ set(new)) > 0      # at least one tuple that one state has and the other has not
    if kind == "ld":
        return not ol.bits_equal(old, new)
    return old != new


# ------------------------------------------------------------------------------------------------------------ the setters

class Setter:
    def __init__(self, name, fn, clears=(), neutral=False):
        self.name, self.fn, self.clears, self.neutral = name, fn, tuple(clears), neutral

    def __call__(self, m, rng):
        """changes the model; returns apply(panel, ctx) that does the same to a panel"""
        apply = self.fn(m, rng)
        m.touched()
        return apply


def _maf_freq(rng, m):
    f = rng.uniform(0.02, 0.98, size=m.nloci)
    f[rng.random(m.nloci) < 0.01] = 1.0
    return f


def s_freq(m, rng):
    m.freq = _maf_freq(rng, m)
    f = m.freq.copy()
    return lambda p, ctx: p.set_freq(f)


def s_freq_mono(m, rng):
    """every frequency 0 or 1: every term +0.0, W * tab_min = 0 (the tuned chain alone)"""
    m.freq = rng.integers(0, 2, size=m.nloci).astype(np.float64)
    f = m.freq.copy()
    return lambda p, ctx: p.set_freq(f)


def _set_map(m):
    pos, cs, ce, gp = m.pos.copy(), list(m.cs), list(m.ce), m.gpos.copy()
    return lambda p, ctx: p.set_map(pos, cs, ce, gpos=gp)


def s_map_gpos(m, rng):
    m.gpos = new_gpos(rng, m)
    return _set_map(m)


def s_map_pos(m, rng):
    """new positions: the holes wider than max_gap move"""
    out = []
    for c, n in enumerate(m.sizes):
        steps = rng.integers(1, 4000, size=n).astype(np.int64)
        for _ in range(3 if n > 50 else 1):
            steps[rng.integers(1, n)] += m.max_gap + int(rng.integers(1, 1000))
        out.append(np.cumsum(steps).astype(np.int32))
    m.pos = np.concatenate(out)
    for c, n in enumerate(m.sizes):      # the centromeres keep their SNP indices' neighbourhood: inside the new positions
        if m.ce[c] > 0:
            a = n // 3
            m.cs[c], m.ce[c] = int(out[c][a]) - 1, int(out[c][min(n - 1, a + 2)]) + 1
    return _set_map(m)


def s_map_centro(m, rng):
    """the centromeres move to another stretch of SNPs"""
    for c, n in enumerate(m.sizes):
        if n > 8:
            p = m.chrom(c, m.pos)
            a = int(rng.integers(n // 2 + 2, 3 * n // 4))
            m.cs[c], m.ce[c] = int(p[a]) - 1, int(p[min(n - 1, a + 2)]) + 1
    return _set_map(m)


def s_arg(field, values):
    def fn(m, rng):
        cur = getattr(m, field)
        other = [v for v in values if v != cur]
        setattr(m, field, other[int(rng.integers(0, len(other)))])
        return lambda p, ctx: None
    return fn


def _new_geno(rng, m, n):
    f = rng.uniform(0.05, 0.95, size=n)[:, None]
    u = rng.random((n, m.nind))
    g = np.where(u < (1 - f) ** 2, 0, np.where(u < (1 - f) ** 2 + 2 * f * (1 - f), 1, 2)).astype(np.int16)
    g[rng.random(g.shape) < 0.03] = -9
    return plant_roh(rng, g)


def s_geno_all(m, rng):
    m.geno = _new_geno(rng, m, m.nloci)
    g = m.geno.copy()
    return lambda p, ctx: p.set_genotypes(g)


def partial_range(m):
    """[b, b + n): neither end on a 16-locus word; inside chromosome 0, more than W loci"""
    return 37, 16 * 9 + 6


def s_geno_range(m, rng):
    b, n = partial_range(m)
    new = _new_geno(rng, m, n)
    new[:, 0] = (m.geno[b:b + n, 0] + 1) % 3      # every replaced locus differs from what stood there
    m.geno = m.geno.copy()
    m.geno[b:b + n] = new
    return lambda p, ctx: p.set_genotypes(new, locus_begin=b)


def pack2bit(geno, lead):
    """SNP-major 2-bit rows of a data set whose first `lead` individuals are someone else's"""
    code = np.where((geno >= 0) & (geno <= 2), geno, 3).astype(np.uint8)
    code = np.concatenate([np.full((geno.shape[0], lead), 1, np.uint8), code], axis=1)
    code = np.concatenate([code, np.full((geno.shape[0], (-code.shape[1]) % 4), 3, np.uint8)], axis=1).reshape(geno.shape[0], -1, 4)
    return (code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6)).astype(np.uint8)


def s_geno_2bit(m, rng):
    m.geno = _new_geno(rng, m, m.nloci)
    rows = pack2bit(m.geno, 5)
    return lambda p, ctx: p.set_genotypes_2bit(rows, ind_offset=5)


def s_geno_bed(m, rng):
    """a .bed image of more rows and more individuals than the panel: a row map that drops rows, ind_offset 3"""
    import bed_cases as bc
    lead, nrows = 3, m.nloci + 9
    codes = rng.integers(0, 4, size=(nrows, lead + m.nind + 2)).astype(np.uint8)
    codes[rng.random(codes.shape) < 0.03] = bc.MISS
    dest = np.full(nrows, -1, dtype=np.int64)
    keep = np.sort(rng.choice(nrows, size=m.nloci, replace=False))
    dest[keep] = np.arange(m.nloci)
    _, counted = bc.census(codes)
    m.geno = np.ascontiguousarray(bc.recode(codes, counted)[keep][:, lead:lead + m.nind])
    rows = bc.pack_rows(codes)

    def apply(p, ctx):
        from garlic_amd import abi
        with abi.Bed(ctx, nrows, codes.shape[1]) as bed:
            bed.set_rows(rows)
            p.set_genotypes_bed(bed, dest, ind_offset=lead)
    return apply


def _note_values(m, values, mode_if_new):
    """the panel's dictionary takes the values in; a full one-byte dictionary goes on with the values themselves"""
    if m.gl_mode == CONT:
        return
    if m.gl_mode == 0 or (mode_if_new == DICT16 and m.gl_mode == DICT):
        m.gl_mode = mode_if_new
    m.gl_dict |= set(np.unique(np.asarray(values, dtype=np.float64)).view(np.uint64).tolist())
    if len(m.gl_dict) > (256 if m.gl_mode == DICT else 65536):
        m.gl_mode, m.gl_dict = CONT, set()


def s_gl_dict(m, rng):
    table = rng.choice([1e-16, 1e-5, 1e-3, 0.01, 0.05, 0.2, 0.5, 1.0], size=5, replace=False)
    m.gl, m.gl_codes = rng.choice(table, size=(m.nloci, m.nind)), None
    _note_values(m, m.gl, DICT)
    gl = m.gl.copy()
    return lambda p, ctx: p.set_gl(gl)


def s_gl_cont(m, rng):
    m.gl, m.gl_codes = 10.0 ** rng.uniform(-9, 0, size=(m.nloci, m.nind)), None
    _note_values(m, m.gl, DICT)
    gl = m.gl.copy()
    return lambda p, ctx: p.set_gl(gl)


def s_gl_codes(m, rng):
    """one-byte codes with their table; the second time on: the same codes with another table"""
    if m.gl_codes is None or m.gl_codes.dtype != np.uint8:
        m.gl_codes = rng.integers(0, 6, size=(m.nloci, m.nind)).astype(np.uint8)
    table = 10.0 ** -rng.integers(1, 12, size=6).astype(np.float64) * rng.choice([1.0, 2.0, 5.0], size=6)
    m.gl = table[m.gl_codes]
    _note_values(m, table, DICT)
    codes = m.gl_codes.copy()
    return lambda p, ctx: p.set_gl_codes(codes, table)


def s_gl_codes16(m, rng):
    table = 10.0 ** rng.uniform(-9, 0, size=1000)
    codes = rng.integers(0, 1000, size=(m.nloci, m.nind)).astype(np.uint16)
    m.gl, m.gl_codes = table[codes], codes
    _note_values(m, table, DICT16)
    return lambda p, ctx: p.set_gl_codes16(codes, table)


def phase_range(m):
    return 21, 300


def s_phase(m, rng):
    b, n = phase_range(m)
    new = rng.integers(0, 2, size=(n, m.nind)).astype(np.uint8)
    new[:, 0] = 1 - m.phase[b:b + n, 0]
    m.phase = m.phase.copy()
    m.phase[b:b + n] = new
    m.have_phase = True
    return lambda p, ctx: p.set_phase(new, locus_begin=b)


def s_phase_bits(m, rng):
    b, n = phase_range(m)
    b, n = b + 50, n + 77
    new = rng.integers(0, 2, size=(n, m.nind)).astype(np.uint8)
    new[:, 0] = 1 - m.phase[b:b + n, 0]
    m.phase = m.phase.copy()
    m.phase[b:b + n] = new
    m.have_phase = True
    rows = np.packbits(new != 0, axis=1, bitorder="little")
    return lambda p, ctx: p.set_phase_bits(rows, locus_begin=b)


def s_ld(m, rng):
    w = rng.uniform(1.0, max(2.0, m.W / 4.0), size=(m.nloci, m.W))
    m.ld = {m.W: w}
    W = m.W
    return lambda p, ctx: p.set_ld(W, w)


def s_sub(m, rng):
    """another --ld-subsample (an argument of compute_ld; the bit planes are cached per subsample)"""
    m.sub = np.sort(rng.choice(m.nind, size=int(rng.integers(m.nind // 3, m.nind - 1)), replace=False)).astype(np.int32)
    return lambda p, ctx: None


LD_MULTI = [10, 20, 40]


def s_ld_multi(m, rng):
    """compute_ld_multi installs the three sizes; the comparison of its outputs with the oracle is part of applying it"""
    want = {W: _ld(m, W, False) for W in LD_MULTI}
    m.ld = dict(want)
    m.planes_made = True
    sub = m.sub

    def apply(p, ctx):
        outs = p.compute_ld_multi(LD_MULTI, sub_idx=sub)
        for W, out in zip(LD_MULTI, outs):
            assert ol.bits_equal(out, want[W]), f"compute_ld_multi: the weights of W = {W} differ from the oracle"
    return apply


def s_budget(m, rng):
    """the term budget switched on (room for one-block slabs: two block buffers) or off; the scores do not depend on it"""
    m.budget = 0 if m.budget else 1
    on, nblk = m.budget, (m.nind + 63) // 64

    def apply(p, ctx):
        p.set_tgls_term_budget(p.tgls_terms_info()["whole_bytes"] // nblk * min(2, nblk) if on else 0)
    return apply


def s_feed_order(m, rng):
    m.feed_order = 1 - m.feed_order
    order = m.feed_order
    return lambda p, ctx: p.set_feed_order(order)


def s_release(m, rng):
    return lambda p, ctx: p.release_scratch()


GENO = ("terms", "planes")
SETTERS = {s.name: s for s in [
    Setter("set_freq", s_freq, ("tab", "tabgl", "terms", "dfreq", "wtab")),
    Setter("set_freq_mono", s_freq_mono, ("tab", "tabgl", "terms", "dfreq", "wtab")),
    Setter("set_map_gpos", s_map_gpos, ("seg", "plan", "decay", "wtab", "terms_scaled")),
    Setter("set_map_pos", s_map_pos, ("seg", "plan", "decay", "wtab", "terms_scaled")),
    Setter("set_map_centro", s_map_centro, ("seg", "plan", "decay", "wtab", "terms_scaled")),
    Setter("arg_error", s_arg("error", [0.001, 0.05, 1e-6]), ("tab", "wtab")),
    Setter("arg_max_gap", s_arg("max_gap", [200000, 3900, 3800]), ("seg", "plan")),
    Setter("arg_M", s_arg("M", [7, 3, 12]), ("decay", "wtab", "terms_scaled")),
    Setter("arg_mu", s_arg("mu", [1e-9, 1e-5, 4e-5]), ("decay", "wtab", "terms_scaled")),
    Setter("arg_W", s_arg("W", [10, 20, 40]), ("plan",)),
    Setter("set_genotypes", s_geno_all, GENO),
    Setter("set_genotypes_range", s_geno_range, GENO),
    Setter("set_genotypes_2bit", s_geno_2bit, GENO),
    Setter("set_genotypes_bed", s_geno_bed, GENO),
    Setter("set_gl_dict", s_gl_dict, ("tabgl", "terms")),
    Setter("set_gl_cont", s_gl_cont, ("tabgl", "terms")),
    Setter("set_gl_codes", s_gl_codes, ("tabgl", "terms")),
    Setter("set_gl_codes16", s_gl_codes16, ("tabgl", "terms", "values16")),
    Setter("set_phase", s_phase, ("phase",)),
    Setter("set_phase_bits", s_phase_bits, ("phase",)),
    Setter("set_ld", s_ld, ("ld",)),
    Setter("arg_sub", s_sub, ("planes",)),
    Setter("compute_ld_multi", s_ld_multi, ("ld",)),
    Setter("set_tgls_term_budget", s_budget, ("terms",), neutral=True),
    Setter("set_feed_order", s_feed_order, ("feed",)),
    Setter("release_scratch", s_release, ("scratch", "planes"), neutral=True),
]}


# ------------------------------------------------------------------------------------------------------------ the scripts

UNW = ["lod32", "lod1", "feed", "feed_subset", "feed_multi", "cov", "seg"]
WTD = ["wlod", "feed_w", "cov_w", "seg_w"]
TGLS = ["lod_gl", "feed_gl", "feed_multi_tgls", "cov_gl", "seg_gl"]


class Script:
    def __init__(self, name, cache, build, consumers, transitions, W=20, nind=70, seed=1, rounds=None):
        self.name, self.cache, self.build, self.consumers, self.transitions = name, cache, build, consumers, transitions
        self.W, self.nind, self.seed = W, nind, seed
        # rounds: the consumers of the build state and of the state after each transition, where they are not the same list
        self.rounds = [list(consumers)] * (len(transitions) + 1) if rounds is None else rounds
        assert len(self.rounds) == len(transitions) + 1


SCRIPTS = [
    # d_tab / h_tab: the unweighted chain, the feed kernels, the fused coverage and the segments after new frequencies / another error
    Script("tab", "d_tab / h_tab", [], UNW, ["set_freq", "arg_error", "set_freq"]),
    # segments: the map in its three forms and max_gap (gpos alone moves the weighted scores only: see decay)
    Script("segments", "segments", [], UNW, ["set_map_pos", "arg_max_gap", "set_map_centro", "arg_max_gap"]),
    # plan: another W, another layout (lod32 / lod1 alternate inside the consumers), the block subset (feed_subset), the slab blocks
    Script("plan", "plan", [], UNW, ["arg_W", "set_map_pos", "arg_W"], W=40),
    # decay and d_wtab: the narrow wLOD kernel (W = 10) and the tile kernels (W = 20)
    Script("decay", "decay", ["set_ld"], WTD, ["set_map_gpos", "arg_M", "arg_mu", "set_map_pos"]),
    Script("wtab_narrow", "d_wtab", ["set_ld"], WTD, ["arg_error", "arg_M", "set_freq", "arg_mu"], W=10),
    Script("wtab", "d_wtab", ["set_ld"], WTD, ["arg_error", "arg_mu", "arg_M"]),
    # d_tabgl: one-byte codes after new frequencies, new values, a new value table over the same codes
    Script("tabgl", "d_tabgl", ["set_gl_codes"], TGLS, ["set_gl_codes", "set_freq", "set_gl_dict", "set_gl_codes"]),
    # d_values16: 16-bit codes after a new table, new frequencies (wide_bound_known), then the overflow-free return of set_gl
    Script("values16", "d_values16", ["set_gl_codes16"], TGLS, ["set_gl_codes16", "set_freq", "set_gl_dict"]),
    # the likelihood mode on one panel: dictionary -> continuous (set_gl overflows) -> codes into a continuous panel
    Script("gl_modes", "d_tabgl, d_values16", ["set_gl_dict", "set_ld"], TGLS + ["wlod_gl"],
           ["set_gl_cont", "set_freq", "set_gl_codes16", "set_gl_dict"], ),
    Script("gl_modes_16", "d_values16", ["set_gl_dict"], TGLS, ["set_gl_codes16", "set_gl_cont"]),
    # the term matrix after every genotype door
    Script("terms_geno", "term matrix / slabs", ["set_gl_dict"], TGLS + ["lod32", "cov", "seg", "feed"],
           ["set_genotypes", "set_genotypes_range", "set_genotypes_2bit", "set_genotypes_bed"]),
    Script("terms_geno_cont", "term matrix / slabs", ["set_gl_cont"], ["lod_gl", "feed_gl", "seg_gl"],
           ["set_genotypes_range", "set_genotypes_bed", "set_freq"]),
    # ... under a term budget (130 individuals: three blocks, one-block slabs), switched on and off
    Script("terms_slabs", "term matrix / slabs", ["set_gl_dict", "set_ld"], ["lod_gl", "feed_gl", "seg_gl", "wlod_gl"],
           ["set_tgls_term_budget", "set_genotypes_range", "set_freq", "set_tgls_term_budget", "set_gl_dict"], nind=130),
    # the scaled term matrix, order one: raw -> weighted -> set_map -> raw.  The weighted call is the last before every set_map:
    # the matrix holds (term * nomut) * norec of the old map when the new one arrives
    Script("terms_scaled_map", "term matrix (scaled)", ["set_gl_dict", "set_ld"], ["lod_gl", "wlod_gl"],
           ["set_map_pos", "set_map_gpos", "set_map_pos"],
           rounds=[["lod_gl", "wlod_gl"], ["lod_gl", "wlod_gl"], ["wlod_gl"], ["lod_gl", "wlod_gl"]]),
    Script("terms_scaled_map_cont", "term matrix (scaled)", ["set_gl_cont", "set_ld"], ["lod_gl", "wlod_gl"],
           ["set_map_pos", "set_map_gpos"], rounds=[["lod_gl", "wlod_gl"], ["lod_gl", "wlod_gl"], ["wlod_gl", "=lod_gl"]]),
    # order two: weighted(M, mu) -> weighted(M', mu) -> weighted(M', mu') -> raw.  No raw call between the weighted ones: the
    # matrix is scaled by the old (M, mu) when the call with the new ones comes, and the raw call finds a scaled matrix
    Script("terms_scaled_args", "term matrix (scaled)", ["set_gl_cont", "set_ld"], ["wlod_gl", "=lod_gl"], ["arg_M", "arg_mu"],
           rounds=[["=lod_gl", "wlod_gl"], ["wlod_gl"], ["wlod_gl", "=lod_gl"]]),
    Script("terms_scaled_args_dict", "term matrix (scaled)", ["set_gl_dict", "set_ld"], ["wlod_gl", "=lod_gl"], ["arg_mu", "arg_M"],
           rounds=[["=lod_gl", "wlod_gl"], ["wlod_gl"], ["wlod_gl", "=lod_gl"]]),
    # d_freq: the continuous mode reads the frequencies on the device
    Script("dfreq", "d_freq, wide_bound_known", ["set_gl_cont"], ["lod_gl", "feed_gl", "cov_gl"], ["set_freq", "set_freq"]),
    # LD planes: subsample A then B, new genotypes through each door, release_scratch in between
    Script("ld_planes", "LD planes", ["arg_sub"], ["ld"],
           ["arg_sub", "set_genotypes_range", "release_scratch", "set_genotypes_2bit", "arg_W", "set_genotypes_bed"], W=40),
    Script("ld_planes_narrow", "LD planes", [], ["ld", "wlod"], ["set_genotypes_range", "arg_sub", "set_genotypes"], W=10),
    # the installed sets: compute_ld_multi, then new genotypes (the weights stay what was installed), each size read
    Script("ld_sets", "LD weights in use and ld_sets", ["compute_ld_multi"], ["wlod", "feed_w", "seg_w"],
           ["set_genotypes_range", "arg_W", "compute_ld_multi", "arg_W", "set_ld", "set_genotypes"]),
    # the phase planes over partial ranges, bytes and bit rows
    Script("phase", "phase planes d_phase", ["set_phase"], ["ld_phased"],
           ["set_phase_bits", "set_phase", "set_genotypes_range", "set_freq", "arg_sub"], W=40),
    # per call: the chain kind across the "exact needed" threshold (W = 40, error 1e-260: see test_panel_state_cpu), the feed
    # form with it, the feed order, the scratch
    Script("chain_kind", "last_chain_kind", ["error_tiny", "set_freq_mono"], ["chain_kind", "lod32", "feed", "feed_multi", "cov", "seg"],
           ["set_freq", "set_freq_mono", "set_freq"], W=40),
    Script("per_call", "feed form, feed_slots, work lists", ["set_gl_dict", "set_ld"],
           ["feed", "feed_w", "feed_gl", "feed_subset", "feed_multi", "feed_multi_tgls"],
           ["set_feed_order", "release_scratch", "set_freq", "set_feed_order", "set_genotypes_range"]),
]


def s_error_tiny(m, rng):
    m.error = 1e-260
    return lambda p, ctx: None


SETTERS["error_tiny"] = Setter("error_tiny", s_error_tiny, ("tab", "wtab"))


def script_rng(sc):
    return np.random.default_rng(1000 + sc.seed)


def start(sc):
    """the model of a script before its build setters"""
    return Model(sc.seed, W=sc.W, nind=sc.nind)


# ------------------------------------------------------------------------------------------------------------ random steps

RANDOM_SEEDS = [626, 790]
RANDOM_BUILD = ["set_gl_dict", "set_ld"]      # the state the 25 steps start from: likelihoods and weights are there to go stale


def random_start(seed):
    m, rng = Model(seed), np.random.default_rng(seed + 500)
    return m, rng, [SETTERS[name](m, rng) for name in RANDOM_BUILD]

N_STEPS, MIN_CONSUMERS = 25, 10
RANDOM_SETTERS = ["set_freq", "set_map_gpos", "set_map_pos", "set_map_centro", "arg_error", "arg_max_gap", "arg_M", "arg_mu", "arg_W",
                  "set_genotypes", "set_genotypes_range", "set_genotypes_2bit", "set_genotypes_bed", "set_gl_dict", "set_gl_cont",
                  "set_gl_codes", "set_gl_codes16", "set_phase", "set_phase_bits", "set_ld", "arg_sub", "compute_ld_multi",
                  "set_feed_order", "release_scratch"]
RANDOM_CONSUMERS = [c for c in CONSUMERS]
CACHES = ("tab", "seg", "decay", "terms", "planes")


def random_plan(seed):
    """[(is_consumer, name)] of one seed: fixed before anything runs, at least MIN_CONSUMERS consumers"""
    rng = np.random.default_rng(seed)
    while True:
        plan = []
        for _ in range(N_STEPS):
            if rng.random() < 0.5:
                plan.append((True, RANDOM_CONSUMERS[int(rng.integers(0, len(RANDOM_CONSUMERS)))]))
            else:
                plan.append((False, RANDOM_SETTERS[int(rng.integers(0, len(RANDOM_SETTERS)))]))
        if sum(1 for c, _ in plan if c) >= MIN_CONSUMERS:
            return plan


_SCORES = set(CONSUMERS) - {"ld", "ld_phased"}
READERS = {"tab": {"lod32", "lod1", "feed", "feed_subset", "feed_multi", "cov", "seg", "chain_kind"},
           "seg": _SCORES,
           "decay": {"wlod", "wlod_gl", "feed_w", "cov_w", "seg_w"},
           "terms": {"lod_gl", "wlod_gl", "feed_gl", "feed_multi_tgls", "cov_gl", "seg_gl"},
           "planes": {"ld", "ld_phased"}}


class Reach:
    """which caches a sequence can catch stale: a reader filled the cache, a setter that changes an input then had to clear it,
    and a reader of the same cache ran after that -- only then would a missed invalidation show"""

    def __init__(self):
        self.filled, self.pending, self.hit = set(), set(), set()

    def consumer(self, name):
        """a consumer that ran (not a refused one)"""
        for cache, readers in READERS.items():
            if name in readers:
                if cache in self.pending:
                    self.hit.add(cache)
                    self.pending.discard(cache)
                self.filled.add(cache)

    def setter(self, s):
        if not s.neutral:
            self.pending |= {c for c in s.clears if c in self.filled}
