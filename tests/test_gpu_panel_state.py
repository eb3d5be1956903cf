"""GPU: one long-lived garlic_panel through changes of its inputs -- every cached table must follow every setter.

A panel keeps about fifteen derived things between calls (term tables, segments, the work plan, decay factors, score rows,
likelihood tables and term matrices, LD bit planes, installed LD sets, phase planes ...).  A missed invalidation does not
crash: it returns plausible scores of the previous inputs.  Here every result is compared bit for bit with the CPU oracle's
answer FOR THE STATE AT THAT MOMENT (tests/panel_state_cases.py holds the model), never with an earlier GPU result.

  scripts   one per cached thing: build, run the consumers that read the cache, apply one setter it depends on, run them again,
            ... ; the end state is then built directly on a fresh panel, whose chain_kind / feed_info / tgls_mode must be the
            long-lived panel's.  tests/test_panel_state_cpu.py shows that every (setter, consumer) pair really changes.
  random    two fixed seeds, 25 steps each drawn from setters and consumers on one panel; a consumer whose precondition fails
            must raise the library's GARLIC_ERR_STATE, and counts as checked only then."""
import contextlib
import os

import numpy as np
import pytest

import panel_state_cases as ps

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def continuous_uploads():
    """GARLIC_TGLS_CONTINUOUS for the likelihood uploads inside: the library reads it in the upload doors only (begin_gl_upload),
    no score or feed call looks at it, and it is back to what it was before any of those runs"""
    old = os.environ.get("GARLIC_TGLS_CONTINUOUS")
    os.environ["GARLIC_TGLS_CONTINUOUS"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["GARLIC_TGLS_CONTINUOUS"]
        else:
            os.environ["GARLIC_TGLS_CONTINUOUS"] = old


def new_panel(ctx, m):
    """a fresh panel built directly in the model's state"""
    from garlic_amd import abi
    panel = abi.Panel(ctx, m.sizes, m.nind)
    try:
        panel.set_map(m.pos, m.cs, m.ce, gpos=m.gpos)
        panel.set_freq(m.freq)
        panel.set_genotypes(m.geno)
        if m.gl is not None:
            if m.gl_mode == ps.DICT16:
                values, codes = np.unique(m.gl, return_inverse=True)
                panel.set_gl_codes16(codes.reshape(m.gl.shape).astype(np.uint16), values)
            elif m.gl_mode == ps.CONT and np.unique(m.gl).shape[0] <= 256:
                with continuous_uploads():       # few values in a panel that keeps the values themselves
                    panel.set_gl(m.gl)
            else:
                panel.set_gl(m.gl)
        if m.have_phase:
            panel.set_phase(m.phase)
        if m.W in m.ld:
            panel.set_ld(m.W, m.ld[m.W])
        if m.budget:
            nblk = (m.nind + 63) // 64
            panel.set_tgls_term_budget(panel.tgls_terms_info()["whole_bytes"] // nblk * min(2, nblk))
        panel.set_feed_order(m.feed_order)
    except Exception:
        panel.close()
        raise
    return panel


def check(panel, m, name, where):
    """one consumer against the oracle for the state of this moment; a refused one must raise the documented code"""
    from garlic_amd import abi
    code = ps.refused(m, name)
    if code is not None:
        with pytest.raises(abi.GarlicError) as e:
            ps.gpu(panel, m, name)
        assert e.value.code == code, f"{where}: {name} refused with {e.value.code}, not {code}"
        return
    got = ps.gpu(panel, m, name)
    want = ps.oracle(m, name)
    assert ps.same(name, got, want), f"{where}: {name} differs from the oracle for the current state"


def probe(panel, m):
    """which forms the panel picks for the state: (chain_kind, feed_info, tgls_mode) after the same calls"""
    out = []
    a = (m.W, m.error, m.max_gap)
    panel.lod_windows(*a, pitch_align=32)
    out.append(("chain_kind", panel.chain_kind()))
    panel.lod_feed(*a, ps.STEP)
    out.append(("feed_info", panel.feed_info()))
    if m.gl is not None:
        panel.lod_windows(*a, pitch_align=32, use_gl=True)
        out.append(("chain_kind gl", panel.chain_kind()))
        out.append(("tgls_mode", panel.tgls_mode()))
        panel.lod_feed(*a, ps.STEP, use_gl=True)
        out.append(("feed_info gl", panel.feed_info()))
    if m.W in m.ld:
        panel.lod_feed(*a, ps.STEP, weighted=True, M=m.M, mu=m.mu)
        out.append(("feed_info weighted", panel.feed_info()))
    return out


def liveness(panel):
    st = panel.stats()
    assert st["n_stall_reruns"] == 0 and st["n_count_timeouts"] == 0, st


@pytest.mark.parametrize("sc", ps.SCRIPTS, ids=[s.name for s in ps.SCRIPTS])
def test_script(gpu_ctx, sc):
    from garlic_amd import abi
    m, rng = ps.start(sc), ps.script_rng(sc)
    with abi.Panel(gpu_ctx, m.sizes, m.nind) as panel:
        panel.set_map(m.pos, m.cs, m.ce, gpos=m.gpos)
        panel.set_freq(m.freq)
        panel.set_genotypes(m.geno)
        for name in sc.build:
            ps.SETTERS[name](m, rng)(panel, gpu_ctx)
        for step, name in enumerate([None] + list(sc.transitions)):
            if name is not None:
                ps.SETTERS[name](m, rng)(panel, gpu_ctx)
            for cons in sc.rounds[step]:
                check(panel, m, cons.lstrip("="), f"{sc.name}, after {step} transitions ({name})")
        assert m.gl is None or panel.tgls_mode()[0] == m.gl_mode
        if sc.name == "chain_kind":
            panel.lod_windows(m.W, m.error, m.max_gap, pitch_align=32)
            assert (panel.chain_kind() > 0) == ps.exact_needed(m)
        liveness(panel)
        with new_panel(gpu_ctx, m) as fresh:
            want = probe(fresh, m)
            assert probe(panel, m) == want, f"{sc.name}: the long-lived panel picks other forms than a fresh one in its state"
            for cons in sc.consumers:
                check(fresh, m, cons.lstrip("="), f"{sc.name}, fresh panel")


@pytest.mark.parametrize("seed", ps.RANDOM_SEEDS)
def test_random_sequence(gpu_ctx, seed):
    from garlic_amd import abi
    m, rng, build = ps.random_start(seed)      # (the build setters leave map, frequencies and genotypes alone)
    n_checked = 0
    with abi.Panel(gpu_ctx, m.sizes, m.nind) as panel:
        panel.set_map(m.pos, m.cs, m.ce, gpos=m.gpos)
        panel.set_freq(m.freq)
        panel.set_genotypes(m.geno)
        for apply in build:
            apply(panel, gpu_ctx)
        for step, (is_consumer, name) in enumerate(ps.random_plan(seed)):
            if is_consumer:
                check(panel, m, name, f"seed {seed}, step {step}")
                n_checked += 1
            else:
                ps.SETTERS[name](m, rng)(panel, gpu_ctx)
        assert n_checked >= ps.MIN_CONSUMERS
        liveness(panel)
        with new_panel(gpu_ctx, m) as fresh:
            want = probe(fresh, m)
            assert probe(panel, m) == want
