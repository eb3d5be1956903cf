"""GPU: the unweighted chain pass as one launch -- lod_chain_kernel writes the plan's MISSING stretches itself, a repeated
asynchronous pass is that kernel between one pair of events, and the work list is in the order the host model picks
(garlic_amd/host/chain_order.hpp).  fill_missing_kernel stays for every plan with nothing to score.

Every comparison is bit for bit against the oracle (tests/oracle_lib.py) on the dense-run panels of tests/run_cases.py:
per chromosome hundreds of runs of 1, W-1, W, W+1, .. 2W, 3W+7 SNPs, a centromere inside a run, a chromosome of W-1 SNPs
(test_gpu_runs.Data "all").  Before every call the output buffer is filled with a NaN whose payload is the call's own number, so a
cell nobody wrote -- or one left from an earlier call -- is not the oracle's value."""
import functools
import itertools

import numpy as np
import pytest

import oracle_lib as ol
import run_cases as rc
from garlic_amd import abi
from test_gpu_runs import Data
from test_gpu_window_regimes import assert_scores, open_panel

pytestmark = pytest.mark.gpu
MG, ERR = rc.MAX_GAP, 0.001
WS = [2, 33, 100, 130]
NINDS = [1, 40, 64, 65, 200]          # fewer items than workgroups at the small ones; a ragged last block at 40, 65, 200
_calls = itertools.count(1)


@pytest.fixture(autouse=True)
def torch_first(gpu_ctx):
    """torch finds the device before the library opens it (tests/conftest.py, gpu_ctx); the tests open contexts of their own"""


@functools.lru_cache(maxsize=None)
def data(name, W, nind):
    return Data(name, W, nind)


def poisoned(total):
    """(tensor of `total` doubles, its bit pattern): a quiet NaN that carries the number of this call"""
    import torch
    bits = 0x7FF8000000000000 | next(_calls)
    t = torch.full((int(total),), bits, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return t.view(torch.float64), bits


def rows_of(host, panel, sizes, nrows, pitch_align):
    base, pitch, total = panel.out_layout(pitch_align, nrows)
    return [host[base[c]: base[c] + nrows * pitch[c]].reshape(nrows, pitch[c])[:, :n] for c, n in enumerate(sizes)]


def run_once(panel, d, W, pitch_align, ind_begin=0, ind_count=None, slack=0):
    """one call into a freshly poisoned buffer -> (rows per chromosome, the doubles behind the layout, poison bits)"""
    ind_count = d.nind - ind_begin if ind_count is None else ind_count
    total = panel.out_layout(pitch_align, ind_count)[2]
    out, bits = poisoned(total + slack)
    panel.lod_windows_device(out.data_ptr(), W, ERR, MG, ind_begin=ind_begin, ind_count=ind_count, pitch_align=pitch_align)
    panel.ctx.synchronize()
    host = out.cpu().numpy()
    return rows_of(host, panel, d.sizes, ind_count, pitch_align), host[total:], bits


@pytest.mark.parametrize("pitch_align", [32, 1])
@pytest.mark.parametrize("nind", NINDS)
@pytest.mark.parametrize("W", WS)
def test_dense_panels(W, nind, pitch_align):
    """lod_chain_kernel<true> (pitch_align 32) and <false> (1): scores and MISSING stretches from the one launch"""
    d = data("all", W, nind)
    with abi.Context(0) as ctx, d.open(ctx) as panel:
        got, _, _ = run_once(panel, d, W, pitch_align)
        st = panel.stats()
        assert st["n_chain_items"] > 0 and st["n_missing"] > 0 and panel.chain_kind() == 0
        assert_scores(got, d.scores(), ("dense", W, nind, pitch_align))


@pytest.mark.parametrize("pitch_align", [32, 1])
@pytest.mark.parametrize("begin,count", [(0, 40), (64, 65), (3, 130)])
@pytest.mark.parametrize("W", [33, 100])
def test_sub_ranges(W, begin, count, pitch_align):
    """ind_begin / ind_count: the rows of the range, bit for bit; what lies behind the range's layout keeps the poison"""
    d = data("all", W, 200)
    want = [s[begin: begin + count] for s in d.scores()]
    with abi.Context(0) as ctx, d.open(ctx) as panel:
        got, behind, bits = run_once(panel, d, W, pitch_align, ind_begin=begin, ind_count=count, slack=4096)
        assert_scores(got, want, ("sub-range", W, begin, count, pitch_align))
        assert (behind.view(np.int64) == bits).all(), ("written behind the range", W, begin, count, pitch_align)


def short_chromosomes(W, nind):
    rng = np.random.default_rng([W, nind, 77])
    """every chromosome shorter than the window"""
    return [ol.random_panel(rng, n, nind, max_gap=MG, gaps=0) for n in (W - 1, min(5, W - 1), 1, max(1, W // 2))]


@pytest.mark.parametrize("pitch_align", [32, 1])
@pytest.mark.parametrize("W", [2, 33, 100])
@pytest.mark.parametrize("shape", ["all_breaks", "short"])
def test_no_chain_launch(shape, W, pitch_align):
    """no run to score: the chain kernel is not launched, so fill_missing_kernel still writes every cell"""
    nind = 70
    if shape == "all_breaks":
        d = data("all_breaks", W, nind)
        chroms, want = d.chroms, d.scores()
    else:
        chroms = short_chromosomes(W, nind)
        want = [ol.oracle_calc_lod(g, f, p, cs, ce, W, ERR, MG) for g, f, p, cs, ce in chroms]
    sizes = [c[0].shape[0] for c in chroms]
    with abi.Context(0) as ctx, open_panel(ctx, chroms, nind) as panel:
        total = panel.out_layout(pitch_align, nind)[2]
        out, _ = poisoned(total)
        panel.lod_windows_device(out.data_ptr(), W, ERR, MG, pitch_align=pitch_align)
        ctx.synchronize()
        st = panel.stats()
        assert st["n_chain_items"] == 0 and st["n_missing"] == sum(sizes) > 0
        got = rows_of(out.cpu().numpy(), panel, sizes, nind, pitch_align)
        assert_scores(got, want, (shape, W, pitch_align))
        assert all((np.ascontiguousarray(g) == ol.MISSING).all() for g in got)


@pytest.mark.parametrize("pitch_align", [32, 1])
def test_repeated_passes(pitch_align):
    """set_async: three enqueued passes into one buffer, the buffer poisoned again, two more; another window size and back
    (a new plan each time: queue counters and list uploaded again).  After every group the rows are the oracle's, and
    the call's stats and the recent kernel times come from the one pair of events around the kernel."""
    import torch
    W, W2, nind = 100, 33, 200
    d = data("all", W, nind)
    with abi.Context(0) as ctx, d.open(ctx) as panel:
        ctx.set_async(True)
        total = panel.out_layout(pitch_align, nind)[2]
        out, _ = poisoned(total)

        def group(w, n):
            bits = 0x7FF8000000000000 | next(_calls)
            out.view(torch.int64).fill_(bits)
            torch.cuda.synchronize()
            for _ in range(n):
                panel.lod_windows_device(out.data_ptr(), w, ERR, MG, pitch_align=pitch_align)
            ctx.synchronize()
            assert_scores(rows_of(out.cpu().numpy(), panel, d.sizes, nind, pitch_align), d.scores(W=w), ("repeat", w, n, pitch_align))

        group(W, 1)          # plans and waits
        group(W, 3)
        st = panel.stats()
        assert st["chain_kernel_ms"] > 0 and st["total_ms"] >= st["chain_kernel_ms"] and st["n_stall_reruns"] == 0
        ms = ctx.recent_kernel_ms(3)
        assert len(ms) == 3 and min(ms) > 0
        group(W, 2)
        group(W2, 1)
        group(W2, 2)
        group(W, 1)
        group(W, 3)
        assert panel.stats()["chain_kernel_ms"] > 0


def test_twenty_launches_identical():
    W, nind = 100, 200
    d = data("all", W, nind)
    with abi.Context(0) as ctx, d.open(ctx) as panel:
        first = None
        for k in range(20):
            got, _, _ = run_once(panel, d, W, 32)
            flat = np.concatenate([np.ascontiguousarray(g).ravel() for g in got]).view(np.int64)
            if first is None:
                first = flat
                assert_scores(got, d.scores(), ("launch 0",))
            assert np.array_equal(flat, first), ("launch", k)
