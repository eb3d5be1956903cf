"""GPU: the LD weights of several window sizes from shared passes (garlic_panel_compute_ld_multi, garlic_ld_finish_multi,
garlic_panel_ld_info) against the CPU oracle per size, bit for bit; every listed size is installed; the grouping rule is
the one of include/garlic_hip.h (ld_multi_cases.groups_of); GARLIC_LD_MULTI_SOLO=1 gives the same doubles from one pass
per size."""
import numpy as np
import pytest

import ld_multi_cases as cases
import oracle_lib as ol
from garlic_amd import abi

pytestmark = pytest.mark.gpu
MG, ERROR, M, MU = cases.MG, cases.ERROR, cases.M, cases.MU


def make_panel(ctx, chroms, nind):
    panel = abi.Panel(ctx, [c[0].shape[0] for c in chroms], nind)
    panel.set_map(np.concatenate([c[2] for c in chroms]), [c[3] for c in chroms], [c[4] for c in chroms],
                  gpos=np.concatenate([c[2] for c in chroms]) * 1e-6)
    panel.set_freq(np.concatenate([c[1] for c in chroms]))
    panel.set_genotypes(np.concatenate([c[0] for c in chroms], axis=0))
    return panel


def check_outputs(got, sizes, want, chroms, what):
    assert len(got) == len(sizes)
    for ld, w in zip(got, sizes):
        assert ol.bits_equal(ld, want[w]), (what, w, ol.count_mismatch(ld, want[w]))
        assert not ld[cases.rows_without_window(chroms, w)].view(np.uint64).any(), (what, w)      # +0.0


def check_info(panel, sizes, solo=False):
    installed, groups, nbytes, n_pair, n_sum = panel.ld_info()
    index = cases.group_index(sizes, solo)
    assert installed == sorted(index)
    assert groups == [index[w] for w in installed]
    assert nbytes == sum((16 + (panel.nloci + w + 64) * w) * 8 for w in installed)
    assert (n_pair, n_sum) == cases.passes_of(sizes, solo)


@pytest.mark.parametrize("nind", cases.NINDS)
@pytest.mark.parametrize("li", range(len(cases.SIZE_LISTS)))
def test_multi_matches_oracle(gpu_ctx, li, nind):
    """every size of the list, all individuals and a sorted random subsample"""
    sizes = cases.SIZE_LISTS[li]
    chroms, sub, want_all, want_sub = cases.case(li, nind)
    with make_panel(gpu_ctx, chroms, nind) as panel:
        check_outputs(panel.compute_ld_multi(sizes), sizes, want_all, chroms, "all")
        check_info(panel, sizes)
        check_outputs(panel.compute_ld_multi(sizes, sub_idx=sub), sizes, want_sub, chroms, "sub")
        check_info(panel, sizes)
        # outputs wanted for some of the sizes only
        some = [k % 2 == 1 for k in range(len(sizes))]
        got = panel.compute_ld_multi(sizes, want_output=some)
        for ld, w, k in zip(got, sizes, some):
            assert (ld is not None) == k
            assert ld is None or ol.bits_equal(ld, want_all[w]), w


def test_multi_equals_single(gpu_ctx):
    sizes = cases.SIZE_LISTS[1]
    chroms, *_ = cases.case(1, 64)
    with make_panel(gpu_ctx, chroms, 64) as panel:
        got = panel.compute_ld_multi(sizes)
        for ld, w in zip(got, sizes):
            assert ol.bits_equal(ld, panel.compute_ld(w)), w


def test_solo_switch_gives_the_same_doubles(gpu_ctx, monkeypatch):
    """GARLIC_LD_MULTI_SOLO=1: every group is a group of one -- one sum pass per size"""
    li, nind = 1, 150
    sizes = cases.SIZE_LISTS[li]
    chroms, sub, want_all, want_sub = cases.case(li, nind)
    monkeypatch.setenv("GARLIC_LD_MULTI_SOLO", "1")
    with make_panel(gpu_ctx, chroms, nind) as panel:
        check_outputs(panel.compute_ld_multi(sizes, sub_idx=sub), sizes, want_sub, chroms, "solo")
        check_info(panel, sizes, solo=True)
        assert panel.ld_info()[3:] == (len(sizes), len(sizes))
        monkeypatch.setenv("GARLIC_LD_MULTI_SOLO", "0")
        check_outputs(panel.compute_ld_multi(sizes), sizes, want_all, chroms, "shared again")
        check_info(panel, sizes)
        assert panel.ld_info()[3:] == (1, 1)


def test_empty_subsample_through_finish_multi(gpu_ctx):
    """a shard that holds no member of the subsample: zero pair counts, 0/0 = x86's NaN in every weight that has a pair"""
    li, nind = 3, 64
    sizes = cases.SIZE_LISTS[li]
    chroms, *_ = cases.case(li, nind)
    empty = np.zeros(0, dtype=np.int32)
    want = cases.oracle_ld(chroms, sizes, empty)
    assert np.isnan(want[max(sizes)]).any()
    with make_panel(gpu_ctx, chroms, nind) as panel:
        loc, pair = panel.ld_counts(max(sizes), sub_idx=empty)
        assert not pair.any()
        check_outputs(panel.ld_finish_multi(sizes, loc, pair), sizes, want, chroms, "empty")
        check_info(panel, sizes)


def test_phased(gpu_ctx):
    li, nind = 1, 64
    sizes = cases.SIZE_LISTS[li]
    chroms, sub, *_ = cases.case(li, nind)
    nloci = sum(c[0].shape[0] for c in chroms)
    phase = np.random.default_rng(9).integers(0, 2, size=(nloci, nind)).astype(np.uint8)
    with make_panel(gpu_ctx, chroms, nind) as panel:
        with pytest.raises(abi.GarlicError):
            panel.compute_ld_multi(sizes, phased=True)             # no phase yet
        panel.set_phase(phase)
        got = panel.compute_ld_multi(sizes, sub_idx=sub, phased=True)
        check_outputs(got, sizes, cases.oracle_r2(chroms, phase, sizes, sub), chroms, "phased")
        check_info(panel, sizes)


@pytest.mark.parametrize("li", [2, 3])
def test_every_size_is_installed(gpu_ctx, li):
    """no LD matrix asked for; then wLOD scores and one weighted feed per size with no further LD call"""
    sizes = cases.SIZE_LISTS[li]
    nind = 40
    chroms = cases.make_chroms(sizes, nind, 300 + li, max_gap=MG, gaps=2)
    gpos = [c[2] * 1e-6 for c in chroms]
    want_ld = cases.oracle_ld(chroms, sizes)
    with make_panel(gpu_ctx, chroms, nind) as panel:
        assert panel.compute_ld_multi(sizes, want_output=False) == [None] * len(sizes)
        check_info(panel, sizes)
        for w in sizes + sizes[::-1]:                              # back and forth: the sets stay
            out = panel.wlod_windows(w, ERROR, MG, M, MU, pitch_align=32)
            feed, per_chr = panel.lod_feed(w, ERROR, MG, w, weighted=True, M=M, mu=MU)
            off, flat = 0, []
            for c, (g, f, p, cs, ce) in enumerate(chroms):
                ldc = want_ld[w][off:off + g.shape[0]]
                off += g.shape[0]
                want = ol.oracle_calc_wlod(g, f, p, gpos[c], ldc, cs, ce, w, ERROR, MG, MU, M)
                assert ol.bits_equal(out[c], want), (w, c)
                flat.append(ol.oracle_flatten(want, w))
            assert [len(x) for x in flat] == list(per_chr), w
            assert ol.bits_equal(feed, np.concatenate(flat)), w
        panel.release_scratch()                                    # keeps the installed weights
        assert panel.ld_info()[0] == sorted(set(sizes))


def test_two_shards(gpu_ctx):
    """70 + 60 individuals: the counts at the largest size are summed, both shards finish to the whole panel's weights"""
    li, nind, cut = 4, 130, 70
    sizes = cases.SIZE_LISTS[li]
    chroms = cases.make_chroms(sizes, nind, 41)
    sub = np.sort(np.random.default_rng(2).choice(nind, size=60, replace=False)).astype(np.int32)
    want = cases.oracle_ld(chroms, sizes, sub)
    parts = []
    for lo, hi in ((0, cut), (cut, nind)):
        shard = [(c[0][:, lo:hi].copy(), c[1], c[2], c[3], c[4]) for c in chroms]
        parts.append((make_panel(gpu_ctx, shard, hi - lo), (sub[(sub >= lo) & (sub < hi)] - lo).astype(np.int32)))
    counts = [panel.ld_counts(max(sizes), sub_idx=s) for panel, s in parts]
    loc = counts[0][0] + counts[1][0]
    pair = counts[0][1] + counts[1][1]
    for panel, _ in parts:
        check_outputs(panel.ld_finish_multi(sizes, loc, pair), sizes, want, chroms, "shard")
        check_info(panel, sizes)
        panel.close()


def test_a_single_call_leaves_one_set(gpu_ctx):
    sizes = cases.SIZE_LISTS[2]
    chroms, *_ = cases.case(2, 40)
    with make_panel(gpu_ctx, chroms, 40) as panel:
        panel.compute_ld_multi(sizes, want_output=False)
        assert panel.ld_info()[0] == [50, 100]
        panel.compute_ld(50, want_output=False)
        assert panel.ld_info() == ([50], [-1], (16 + (panel.nloci + 50 + 64) * 50) * 8, 0, 0)
        panel.wlod_windows(50, ERROR, 10 ** 9, M, MU, pitch_align=32)
        with pytest.raises(abi.GarlicError) as err:
            panel.wlod_windows(100, ERROR, 10 ** 9, M, MU, pitch_align=32)
        assert err.value.code == abi.ERR_STATE


def test_repeated_calls_are_identical(gpu_ctx):
    li, nind = 1, 150
    sizes = cases.SIZE_LISTS[li]
    chroms, _, want_all, _ = cases.case(li, nind)
    with make_panel(gpu_ctx, chroms, nind) as panel:
        first = panel.compute_ld_multi(sizes)
        check_outputs(first, sizes, want_all, chroms, "first")
        for _ in range(19):
            again = panel.compute_ld_multi(sizes)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
