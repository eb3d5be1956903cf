"""CPU: the scripts and random sequences of tests/panel_state_cases.py are able to fail -- on the model alone, no device.

(a) every scripted setter changes what every consumer after it reads (else a stale cache would pass the GPU test);
(b) the partial genotype ranges really are partial: new genotypes, and both boundary words hold old and new loci;
(c) the chain-kind script crosses the "exact needed" threshold of lod_exact_needed (garlic_hip.hip: W * tab_min <= -9990, tab_min
    the most negative finite term of the per-SNP table);
(d) the random seeds reach the caches: tab, segments, decay, term matrix, LD planes."""
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import panel_state_cases as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the rows of the table of cached things: every one needs a script whose pairs (setter, consumer) hold
CACHE_ROWS = ["d_tab / h_tab", "segments", "plan", "decay", "d_wtab", "d_tabgl", "d_values16", "term matrix / slabs",
              "term matrix (scaled)", "d_freq, wide_bound_known", "LD planes", "LD weights in use and ld_sets", "phase planes d_phase",
              "last_chain_kind", "feed form, feed_slots, work lists"]


def replay(sc):
    """the script on the model: [(setter or None, {consumer: answer})] -- the build state first, then one entry per transition"""
    m, rng = ps.start(sc), ps.script_rng(sc)
    for name in sc.build:
        ps.SETTERS[name](m, rng)
    out = []
    for name in [None] + list(sc.transitions):
        if name is not None:
            ps.SETTERS[name](m, rng)
        answers = {}
        for cons in sc.rounds[len(out)]:
            base = cons.lstrip("=")
            assert ps.refused(m, base) is None, (sc.name, name, cons)
            answers[cons] = ps.oracle(m, base)
        out.append((name, answers))
    return m, out


@pytest.fixture(scope="module")
def replays():
    return {sc.name: replay(sc) for sc in ps.SCRIPTS}


def test_every_setter_changes_what_the_consumers_read(replays, capsys):
    covered, stale = [], []
    for sc in ps.SCRIPTS:
        _, steps = replays[sc.name]
        last = dict(steps[0][1])          # consumer -> its answer the last time the script ran it
        for setter, after in steps[1:]:
            for cons, new in after.items():
                base = cons.lstrip("=")
                if cons in last:
                    if ps.SETTERS[setter].neutral or cons.startswith("="):
                        assert ps.same(base, last[cons], new), f"{sc.name}: {setter} must leave {base} as it was"
                    else:
                        (covered if ps.differs(base, last[cons], new) else stale).append((sc.cache, sc.name, setter, base))
                last[cons] = new
    assert not stale, "a stale cache would pass (script, setter, consumer): %s" % [s[1:] for s in stale]
    with capsys.disabled():
        print("\ncovered (cache | script | setter -> consumer):")
        for row in sorted(set(covered)):
            print("  %-34s %-18s %-22s -> %s" % row)
    caches = {c[0] for c in covered}
    for row in CACHE_ROWS:
        assert any(row in c for c in caches), f"no script covers the cache '{row}'"
    # every setter and every consumer of the issue's lists is in some covered pair
    assert {c[2] for c in covered} >= set(ps.SETTERS) - {"set_tgls_term_budget", "release_scratch", "error_tiny"}
    assert {c[3] for c in covered} == set(ps.CONSUMERS)
    scripted = {t for sc in ps.SCRIPTS for t in sc.transitions}
    assert {"set_tgls_term_budget", "release_scratch"} <= scripted


def test_constants_are_the_bindings():
    from garlic_amd import abi
    assert ps.ERR_STATE == abi.ERR_STATE and ps.FEED_SORTED == abi.FEED_ORDER_SORTED and ps.MISSING == abi.MISSING
    assert (ps.DICT, ps.CONT, ps.DICT16) == (abi.TGLS_DICTIONARY, abi.TGLS_CONTINUOUS, abi.TGLS_DICTIONARY16)


def test_scaled_term_orders():
    """the two orders of the scaled term matrix as calls: a weighted use_gl call is the last score call before every set_map of
    terms_scaled_map, and no raw call stands between the weighted calls of terms_scaled_args"""
    by = {sc.name: sc for sc in ps.SCRIPTS}
    for name in ("terms_scaled_map", "terms_scaled_map_cont"):
        sc = by[name]
        assert all(t.startswith("set_map") for t in sc.transitions) and sc.rounds[0][0] == "lod_gl"
        assert all(r[-1].lstrip("=") == "wlod_gl" for r in sc.rounds[:-1]) and "lod_gl" in [c.lstrip("=") for c in sc.rounds[-1]]
    for name in ("terms_scaled_args", "terms_scaled_args_dict"):
        sc = by[name]
        assert sorted(sc.transitions) == ["arg_M", "arg_mu"]
        calls = [c.lstrip("=") for r in sc.rounds for c in r]
        assert calls == ["lod_gl", "wlod_gl", "wlod_gl", "wlod_gl", "lod_gl"]


def test_script_shapes():
    """chromosomes of 600, 129 and W - 1 loci; 70 and 130 individuals; W = 10, 20 and 40"""
    assert {sc.W for sc in ps.SCRIPTS} == {10, 20, 40} and {sc.nind for sc in ps.SCRIPTS} == {70, 130}
    for sc in ps.SCRIPTS:
        m = ps.start(sc)
        assert m.sizes == [600, 129, sc.W - 1]
        assert np.count_nonzero(m.geno == -9) > 0.02 * m.geno.size and any(c > 0 for c in m.ce)
        assert any(np.any(np.diff(m.chrom(c, m.pos)) > m.max_gap) for c in range(3))


def test_partial_genotype_ranges_are_real():
    m = ps.Model(5)
    b, n = ps.partial_range(m)
    assert b % 16 != 0 and (b + n) % 16 != 0 and n > 40
    src = open(os.path.join(ROOT, "garlic_amd", "csrc", "lod_kernels.hpp")).read()
    assert int(re.search(r"constexpr int GOFF = (\d+);", src).group(1)) % 16 == 0      # words of the panel = words of the locus index
    old = m.geno.copy()
    ps.SETTERS["set_genotypes_range"](m, np.random.default_rng(6))
    changed = np.any(old != m.geno, axis=1)
    assert changed[b:b + n].all() and not changed[:b].any() and not changed[b + n:].any()
    for word in (b // 16, (b + n - 1) // 16):          # both boundary words keep some of their neighbours' genotypes
        loci = np.arange(16 * word, 16 * word + 16)
        assert changed[loci].any() and not changed[loci].all()
    pb, pn = ps.phase_range(m)
    assert pb % 64 != 0 and (pb + pn) % 64 != 0 and pn < m.nloci


def test_chain_kind_script_crosses_the_threshold(replays):
    src = open(os.path.join(ROOT, "garlic_amd", "csrc", "garlic_hip.hip")).read()
    body = src[src.index("bool lod_exact_needed("):]
    body = body[:body.index("\n}\n")]
    assert "p->tab_min" in body and re.search(r"\(double\)W \* tmin <= -9990\.0", body), "the rule the model restates has changed"
    assert ps.EXACT_LIMIT == -9990.0
    sc = next(s for s in ps.SCRIPTS if s.name == "chain_kind")
    m, rng = ps.start(sc), ps.script_rng(sc)
    for name in sc.build:
        ps.SETTERS[name](m, rng)
    kinds, sides = [], []
    for name in [None] + list(sc.transitions):
        if name is not None:
            ps.SETTERS[name](m, rng)
        tmin = min([0.0] + [t for f in m.freq for g in (0, 1, 2) for t in [ol.oracle().oracle_lod(g, float(f), m.error)] if np.isfinite(t)])
        sides.append(sc.W * tmin <= ps.EXACT_LIMIT)
        kinds.append(ps.chain_kind(m))
    assert sides == [False, True, False, True]
    assert [k > 0 for k in kinds] == sides and all(a != b for a, b in zip(kinds, kinds[1:]))


def replay_random(seed):
    """the seed's sequence on the model alone -> (consumers that ran, refusals, caches a stale table of which would show: Reach)"""
    m, rng, _ = ps.random_start(seed)
    checked, refusals, reach = 0, 0, ps.Reach()
    for is_consumer, name in ps.random_plan(seed):
        if is_consumer:
            if ps.refused(m, name) is None:
                ps.oracle(m, name)
                reach.consumer(name)
                checked += 1
            else:
                refusals += 1
        else:
            reach.setter(ps.SETTERS[name])
            ps.SETTERS[name](m, rng)
    return checked, refusals, reach.hit


@pytest.mark.parametrize("seed", ps.RANDOM_SEEDS)
def test_random_seeds_reach_the_caches(seed):
    plan = ps.random_plan(seed)
    assert len(plan) == ps.N_STEPS and sum(1 for c, _ in plan if c) >= ps.MIN_CONSUMERS
    assert plan == ps.random_plan(seed)
    checked, refusals, hit = replay_random(seed)
    assert checked >= 6, (checked, refusals)
    assert hit >= set(ps.CACHES), f"seed {seed}: no reader after a setter that clears {set(ps.CACHES) - hit} while it holds something"
