"""GPU: the library on a stream the CALLER owns (garlic_ctx_create with a hip_stream), with no host sync around the calls.

The contract is plain stream order: a device buffer the caller's stream is still writing when a `where = GARLIC_DEVICE` call
starts is read with its final contents, and a device output is complete for whatever the caller enqueues next on that stream.
Two instruments pin it (tests/stream_cases.py holds the panels, the poisons and the oracle's answers):

  input behind a delay     the buffer holds a poison; on the caller's stream go device work that keeps it busy, the copy of
                           the real data into the buffer, and an event.  The event must still be pending when the library is
                           called (asserted: a drained stream would test nothing), and the answer must be the real data's.
  output consumed unsynced the output buffer holds NaN (a sentinel for integers); straight after the call `out.clone()` goes
                           on the same stream, the host waits once at the end of the test, and the clone is what is compared.

Between producer and consumer there is no torch.cuda.synchronize(), no ctx.synchronize() and no .cpu().  Expected values are
the CPU oracle's, bit for bit; the KDE and the GMM fit are held to the bounds of tests/test_gpu_kde.py and
tests/test_gpu_gmm.py (their own check functions).  Every test has its own torch stream and context."""
import threading

import numpy as np
import pytest

import feed_sort_cases as fcases
import gmm_cases as gcases
import kde_cases as kcases
import oracle_lib as ol
import stream_cases as sc
import tgls_slab_cases as scases
from garlic_amd import abi

pytestmark = pytest.mark.gpu
MG, ERROR, M, MU = sc.MG, sc.ERROR, sc.M, sc.MU
NAN = float("nan")
DELAY_TARGET_MS, DELAY_CAP_MS = 100.0, 200.0


class Busy:
    """Device work that keeps a stream busy for about DELAY_TARGET_MS: a chain of 4096 x 4096 float32 matmuls, sized once per
    module from HIP-event times of the chain itself, never more than DELAY_CAP_MS.  Measured on an MI355X: 1.014 ms per
    product, 99 products, 100.4 ms (a delayed-input test takes 0.09 - 0.14 s, most of it this wait)."""

    def __init__(self):
        import torch
        self.a = torch.rand((4096, 4096), dtype=torch.float32, device="cuda") * (1.0 / 4096.0)
        self.b = self.a.clone()
        torch.mm(self.a, self.a, out=self.b)                 # (the BLAS library's first call sets itself up)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(8):
            torch.mm(self.a, self.a, out=self.b)
        t1.record()
        torch.cuda.synchronize()
        self.ms_each = t0.elapsed_time(t1) / 8.0
        self.count = max(1, min(int(DELAY_TARGET_MS / self.ms_each) + 1, int(DELAY_CAP_MS / self.ms_each)))
        print("delay: %.3f ms per product, %d products, %.1f ms" % (self.ms_each, self.count, self.ms_each * self.count))

    def run(self):
        import torch
        for _ in range(self.count):
            torch.mm(self.a, self.a, out=self.b)


@pytest.fixture(scope="module")
def busy():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return Busy()


class Rig:
    """one torch stream and one context on it"""

    def __init__(self, async_device=False):
        import torch
        self.torch = torch
        self.s = torch.cuda.Stream()
        assert self.s.cuda_stream != 0
        self.ctx = abi.Context(0, stream=self.s.cuda_stream)
        if async_device:
            self.ctx.set_async(True)

    def behind_delay(self, busy, pairs):
        """the delay, then dst.copy_(src) for every pair, then the event `produced`, all on the caller's stream"""
        torch = self.torch
        torch.cuda.synchronize()                     # the poison is in place (before the producer: not between it and a consumer)
        with torch.cuda.stream(self.s):
            busy.run()
            for dst, src in pairs:
                dst.copy_(src, non_blocking=True)
            produced = torch.cuda.Event()
            produced.record(self.s)
        return produced

    def clone(self, t):
        with self.torch.cuda.stream(self.s):
            return t.clone()

    def fill(self, t, v):
        with self.torch.cuda.stream(self.s):
            t.fill_(v)

    def full(self, shape, v, dtype):
        return self.torch.full(shape if isinstance(shape, tuple) else (shape,), v, dtype=dtype, device="cuda")

    def dev(self, a):
        return self.torch.from_numpy(np.array(a, order="C")).cuda()           # (a copy: cached cases are read-only)

    def wait(self):
        self.s.synchronize()

    def close(self):
        self.s.synchronize()
        self.ctx.close()


@pytest.fixture
def rig(busy):
    r = Rig()
    yield r
    r.close()


@pytest.fixture
def async_rig(busy):
    r = Rig(async_device=True)
    yield r
    r.close()


def open_panel(ctx, nind, *, geno=True, gaps=True, seed=0):
    chroms, gpos = sc.panel(nind, gaps, seed)
    panel = abi.Panel(ctx, sc.sizes(), nind)
    panel.set_map(np.concatenate([c[2] for c in chroms]), [c[3] for c in chroms], [c[4] for c in chroms], gpos=np.concatenate(gpos))
    panel.set_freq(np.concatenate([c[1] for c in chroms]))
    if geno:
        panel.set_genotypes(sc.geno_of(chroms))
    return panel


def same_scores(snap, layout, nind, want, what):
    base, pitch, _ = layout
    got = sc.rows_of(snap.cpu().numpy(), base, pitch, nind)
    for c in range(len(want)):
        bad = ol.count_mismatch(got[c], np.ascontiguousarray(want[c]))
        assert bad == 0, (what, "chromosome", c, bad, "doubles differ")


def pending(produced):
    """the condition of every delayed-input case: the caller's stream has not reached the event yet"""
    assert produced.query() is False, "the stream drained before the library was called: the case tested nothing"


# =========================================================================== 1. device inputs behind a delay

@pytest.mark.parametrize("nind", sc.NINDS)
def test_delayed_genotypes(rig, busy, nind):
    """set_genotypes_device reads int16 rows the stream is still writing; the scores at W = 10 and 50 are the data's"""
    import torch
    chroms, _ = sc.panel(nind)
    real = rig.dev(sc.geno_of(chroms))
    buf = rig.full((sc.nloci(), nind), -9, torch.int16)
    with open_panel(rig.ctx, nind, geno=False) as panel:
        layout = panel.out_layout(32, nind)
        out = rig.full(layout[2], NAN, torch.float64)
        produced = rig.behind_delay(busy, [(buf, real)])
        pending(produced)
        panel.set_genotypes_device(buf.data_ptr(), nind, 0, sc.nloci())
        snaps = []
        for W in sc.SCORE_WS:
            panel.lod_windows_device(out.data_ptr(), W, ERROR, MG, pitch_align=32)
            snaps.append(rig.clone(out))
            rig.fill(out, NAN)
        rig.wait()
        for W, snap in zip(sc.SCORE_WS, snaps):
            same_scores(snap, layout, nind, sc.lod_scores_and_poison(nind, W)[0], ("genotypes", nind, W))


@pytest.mark.parametrize("nind", sc.NINDS)
def test_delayed_likelihoods(rig, busy, nind):
    """set_gl_device; TGLS scores from both ring forms (W = 40 and 200)"""
    import torch
    _, gl = sc.likelihoods(nind)
    real = rig.dev(np.concatenate(gl, axis=0))
    buf = rig.full((sc.nloci(), nind), sc.GL_POISON, torch.float64)
    with open_panel(rig.ctx, nind) as panel:
        layout = panel.out_layout(32, nind)
        out = rig.full(layout[2], NAN, torch.float64)
        produced = rig.behind_delay(busy, [(buf, real)])
        pending(produced)
        panel.set_gl_device(buf.data_ptr(), nind, 0, sc.nloci())
        snaps = []
        for W in sc.TGLS_WS:
            panel.lod_windows_device(out.data_ptr(), W, ERROR, MG, pitch_align=32, use_gl=True)
            snaps.append(rig.clone(out))
            rig.fill(out, NAN)
        rig.wait()
        for W, snap in zip(sc.TGLS_WS, snaps):
            same_scores(snap, layout, nind, sc.tgls_scores_and_poison(nind, W)[0], ("likelihoods", nind, W))


@pytest.mark.parametrize("W", sc.WLOD_WS)
@pytest.mark.parametrize("nind", sc.NINDS)
def test_delayed_ld_weights(rig, busy, nind, W):
    """set_ld_device; weighted scores from the stream form (W = 10) and the strip form (W = 100)"""
    import torch
    real = rig.dev(np.concatenate(sc.ld_weights(nind, W), axis=0))
    buf = rig.full((sc.nloci(), W), 0.0, torch.float64)
    with open_panel(rig.ctx, nind) as panel:
        layout = panel.out_layout(32, nind)
        out = rig.full(layout[2], NAN, torch.float64)
        produced = rig.behind_delay(busy, [(buf, real)])
        pending(produced)
        panel.set_ld_device(W, buf.data_ptr())
        panel.wlod_windows_device(out.data_ptr(), W, ERROR, MG, M, MU, pitch_align=32)
        snap = rig.clone(out)
        rig.wait()
        same_scores(snap, layout, nind, sc.wlod_scores_and_poison(nind, W)[0], ("LD weights", nind, W))


@pytest.mark.parametrize("nind", sc.NINDS)
def test_delayed_phase_bits(rig, busy, nind):
    """set_phase_bits_device; the phased LD weights (calcR2LD) read the bits"""
    import torch
    W = 10
    rows = sc.phase_rows(sc.phase(nind))
    real = rig.dev(rows)
    buf = rig.full(rows.shape, 0, torch.uint8)
    want = sc.r2_and_poison(nind, W)
    with open_panel(rig.ctx, nind) as panel:
        produced = rig.behind_delay(busy, [(buf, real)])
        pending(produced)
        panel.set_phase_bits_device(buf.data_ptr(), rows.shape[1], 0, sc.nloci())
        got = panel.compute_ld(W, phased=True)
        assert ol.bits_equal(got, want), ("phase bits", nind, ol.count_mismatch(got, want))


@pytest.mark.parametrize("nind", sc.NINDS)
def test_delayed_bed_rows(rig, busy, nind):
    """Bed.set_rows_device, then census_device, then set_genotypes_bed: the census and the scores are the file's"""
    import torch
    W = 10
    rows, counts, counted, want = sc.bed(nind, W)
    real = rig.dev(rows)
    buf = rig.full(rows.shape, sc.BED_POISON, torch.uint8)
    d_counts = rig.full((sc.nloci(), 2), -1, torch.int32)
    d_counted = rig.full(sc.nloci(), 9, torch.uint8)
    with abi.Bed(rig.ctx, sc.nloci(), nind) as bed, open_panel(rig.ctx, nind, geno=False) as panel:
        layout = panel.out_layout(32, nind)
        out = rig.full(layout[2], NAN, torch.float64)
        produced = rig.behind_delay(busy, [(buf, real)])
        pending(produced)
        bed.set_rows_device(buf.data_ptr(), rows.shape[1], 0, sc.nloci())
        bed.census_device(d_counts.data_ptr(), d_counted.data_ptr())
        snap_counts, snap_counted = rig.clone(d_counts), rig.clone(d_counted)
        panel.set_genotypes_bed(bed, np.arange(sc.nloci(), dtype=np.int64), 0)
        panel.lod_windows_device(out.data_ptr(), W, ERROR, MG, pitch_align=32)
        snap = rig.clone(out)
        rig.wait()
        assert np.array_equal(snap_counts.cpu().numpy(), counts) and np.array_equal(snap_counted.cpu().numpy(), counted)
        same_scores(snap, layout, nind, want, ("bed rows", nind))


@pytest.mark.parametrize("nind", sc.NINDS)
def test_delayed_ld_counts(rig, busy, nind):
    """ld_finish_device fed by count tensors the stream is still writing (a sharded panel's all-reduce ends like that)"""
    import torch
    W = 10
    want = sc.hr2_and_poison(nind, W)
    with open_panel(rig.ctx, nind) as panel:
        loc, pair = panel.ld_counts(W)
        real_loc, real_pair = rig.dev(loc), rig.dev(pair)
        d_loc, d_pair = rig.full(loc.shape, 0, torch.int32), rig.full(pair.shape, 0, torch.int32)
        ld = rig.full((sc.nloci(), W), NAN, torch.float64)
        produced = rig.behind_delay(busy, [(d_loc, real_loc), (d_pair, real_pair)])
        pending(produced)
        panel.ld_finish_device(W, d_loc.data_ptr(), d_pair.data_ptr(), ld.data_ptr())
        snap = rig.clone(ld)
        rig.wait()
        got = snap.cpu().numpy()
        assert ol.bits_equal(got, want), ("LD counts", nind, ol.count_mismatch(got, want))


@pytest.mark.parametrize("W", sc.SCORE_WS)
@pytest.mark.parametrize("nind", sc.NINDS)
def test_delayed_scores_flatten(rig, busy, nind, W):
    """flatten_device reads a score tensor the stream is still writing"""
    import torch
    want, _ = sc.feed_and_poison(nind, W)
    with open_panel(rig.ctx, nind) as panel:
        base, pitch, total = panel.out_layout(32, nind)
        real = rig.dev(sc.score_matrix(sc.lod_scores(nind, W), base, pitch, total, nind))
        scores = rig.full(total, NAN, torch.float64)
        feed = rig.full(len(want) + 8, NAN, torch.float64)
        produced = rig.behind_delay(busy, [(scores, real)])
        pending(produced)
        n = panel.flatten_device(scores.data_ptr(), W, feed.data_ptr(), len(want) + 8)
        snap = rig.clone(feed)
        rig.wait()
        assert n == len(want), (nind, W, n, len(want))
        assert ol.bits_equal(snap.cpu().numpy()[:n], want), (nind, W)


@pytest.mark.parametrize("nind", sc.NINDS)
def test_delayed_scores_coverage(rig, busy, nind):
    """roh_coverage_device reads a score tensor the stream is still writing"""
    import torch
    W = 10
    want, _ = sc.coverage_and_poison(nind, W)
    with open_panel(rig.ctx, nind) as panel:
        base, pitch, total = panel.out_layout(32, nind)
        cbase, cpitch, ctotal = panel.out_layout(8, nind)
        real = rig.dev(sc.score_matrix(sc.lod_scores(nind, W), base, pitch, total, nind))
        scores = rig.full(total, NAN, torch.float64)
        cov = rig.full(ctotal, -1, torch.int16)
        produced = rig.behind_delay(busy, [(scores, real)])
        pending(produced)
        panel.roh_coverage_device(scores.data_ptr(), W, sc.cutoff_of(nind, W), cov.data_ptr(), pitch_align=32, inwin_pitch_align=8)
        snap = rig.clone(cov)
        rig.wait()
        got = sc.rows_of(snap.cpu().numpy(), cbase, cpitch, nind)
        for c in range(len(want)):
            assert np.array_equal(got[c], want[c]), (nind, c)


def _delayed_values(rig, busy, x):
    """a device tensor of NaN that gets x behind the delay -> (tensor, produced)"""
    import torch
    real = rig.dev(x)
    buf = rig.full(x.shape[0], NAN, torch.float64)
    return buf, real, rig.behind_delay(busy, [(buf, real)])


def test_delayed_feed_sort(rig, busy):
    x = fcases.content("normal", 3 * fcases.fs_tile() + 17)
    want = fcases.sorted_by_key(x)
    assert not ol.bits_equal(want, np.full_like(x, np.nan))
    buf, real, produced = _delayed_values(rig, busy, x)
    pending(produced)
    rig.ctx.feed_sort(buf.data_ptr(), n=x.shape[0])
    snap = rig.clone(buf)
    rig.wait()
    assert ol.bits_equal(snap.cpu().numpy(), want)


def test_delayed_feed_kde(rig, busy):
    """(a NaN among the values is refused: reading the poison fails the call)"""
    from test_gpu_kde import check_kde
    x = kcases.content("bimodal", 3 * kcases.kde_chunk() + 17)
    buf, real, produced = _delayed_values(rig, busy, x)
    pending(produced)
    got = rig.ctx.feed_kde(buf.data_ptr(), n=x.shape[0])
    rig.wait()
    check_kde(got, np.array(x), "KDE of values behind a delay")


def test_delayed_gmm_fit(rig, busy):
    """(the fit of NaN lengths is NaN in every field: the reference's fields are finite)"""
    from test_gpu_gmm import check_fields
    name, n, k, iters = "three", 3 * gcases.block_points() + 17, 3, 2
    x = gcases.content(name, n)
    a0, m0, v0 = gcases.init(x, k)
    f64, ld = gcases.fixed_reference(name, n, k)[iters]
    assert np.isfinite(gcases.flat(ld).astype(np.float64)).all()
    buf, real, produced = _delayed_values(rig, busy, x)
    pending(produced)
    got = rig.ctx.gmm_fit(buf.data_ptr(), a0, m0, v0, n=n, max_iter=iters, precision=-1.0)
    rig.wait()
    assert got["k"] == k and got["iterations"] == iters
    assert check_fields(got, f64, ld, "GMM fit of lengths behind a delay") <= 1.0


# =========================================================================== 2. device outputs consumed unsynchronised

@pytest.mark.parametrize("nind", sc.NINDS)
def test_output_lod_windows(rig, nind):
    import torch
    with open_panel(rig.ctx, nind) as panel:
        layout = panel.out_layout(32, nind)
        out = rig.full(layout[2], NAN, torch.float64)
        torch.cuda.synchronize()
        snaps = []
        for W in sc.SCORE_WS:
            panel.lod_windows_device(out.data_ptr(), W, ERROR, MG, pitch_align=32)
            snaps.append(rig.clone(out))
            rig.fill(out, NAN)
        rig.wait()
        for W, snap in zip(sc.SCORE_WS, snaps):
            same_scores(snap, layout, nind, sc.lod_scores(nind, W), ("lod_windows_device", nind, W))


@pytest.mark.parametrize("nind", sc.NINDS)
def test_output_wlod_windows(rig, nind):
    import torch
    with open_panel(rig.ctx, nind) as panel:
        layout = panel.out_layout(32, nind)
        out = rig.full(layout[2], NAN, torch.float64)
        torch.cuda.synchronize()
        snaps = []
        for W in sc.WLOD_WS:
            panel.set_ld(W, np.concatenate(sc.ld_weights(nind, W), axis=0))
            panel.wlod_windows_device(out.data_ptr(), W, ERROR, MG, M, MU, pitch_align=32)
            snaps.append(rig.clone(out))
            rig.fill(out, NAN)
        rig.wait()
        for W, snap in zip(sc.WLOD_WS, snaps):
            same_scores(snap, layout, nind, sc.wlod_scores_and_poison(nind, W)[0], ("wlod_windows_device", nind, W))


@pytest.mark.parametrize("nind", sc.NINDS)
def test_output_coverage_fused(rig, nind):
    import torch
    with open_panel(rig.ctx, nind) as panel:
        cbase, cpitch, ctotal = panel.out_layout(8, nind)
        cov = rig.full(ctotal, -1, torch.int16)
        torch.cuda.synchronize()
        snaps = []
        for W in sc.SCORE_WS:
            panel.roh_coverage_fused_device(W, ERROR, MG, sc.cutoff_of(nind, W), cov.data_ptr(), pitch_align=8)
            snaps.append(rig.clone(cov))
            rig.fill(cov, -1)
        rig.wait()
        for W, snap in zip(sc.SCORE_WS, snaps):
            got = sc.rows_of(snap.cpu().numpy(), cbase, cpitch, nind)
            want, _ = sc.coverage_and_poison(nind, W)
            for c in range(len(want)):
                assert np.array_equal(got[c], want[c]), (nind, W, c)


def test_output_census(rig):
    import torch
    nind = 130
    rows, counts, counted, _ = sc.bed(nind, 10)
    d_counts = rig.full((sc.nloci(), 2), -1, torch.int32)
    d_counted = rig.full(sc.nloci(), 9, torch.uint8)
    torch.cuda.synchronize()
    with abi.Bed(rig.ctx, sc.nloci(), nind) as bed:
        bed.set_rows(rows)
        bed.census_device(d_counts.data_ptr(), d_counted.data_ptr())
        snap_counts, snap_counted = rig.clone(d_counts), rig.clone(d_counted)
        rig.wait()
    assert np.array_equal(snap_counts.cpu().numpy(), counts) and np.array_equal(snap_counted.cpu().numpy(), counted)


@pytest.mark.parametrize("nind", sc.NINDS)
def test_output_ld_counts_into_finish(rig, nind):
    """ld_counts_device's tensors go straight into ld_finish_device, its ld_ptr straight into a clone"""
    import torch
    W = 10
    with open_panel(rig.ctx, nind) as panel:
        d_loc = rig.full((sc.nloci(), 2), -1, torch.int32)
        d_pair = rig.full((sc.nloci(), W, 2), -1, torch.int32)
        ld = rig.full((sc.nloci(), W), NAN, torch.float64)
        torch.cuda.synchronize()
        panel.ld_counts_device(W, d_loc.data_ptr(), d_pair.data_ptr())
        snap_loc, snap_pair = rig.clone(d_loc), rig.clone(d_pair)
        panel.ld_finish_device(W, d_loc.data_ptr(), d_pair.data_ptr(), ld.data_ptr())
        snap = rig.clone(ld)
        rig.wait()
        want_loc, want_pair = panel.ld_counts(W)
    assert np.array_equal(snap_loc.cpu().numpy(), want_loc) and np.array_equal(snap_pair.cpu().numpy(), want_pair)
    got = snap.cpu().numpy()
    assert ol.bits_equal(got, sc.hr2(nind, W)), (nind, ol.count_mismatch(got, sc.hr2(nind, W)))


@pytest.mark.parametrize("nind", sc.NINDS)
def test_output_flatten_feed(rig, nind):
    """scores straight into flatten_device, its feed buffer straight into a clone"""
    import torch
    W = 50
    want, _ = sc.feed_and_poison(nind, W)
    with open_panel(rig.ctx, nind) as panel:
        layout = panel.out_layout(32, nind)
        out = rig.full(layout[2], NAN, torch.float64)
        feed = rig.full(len(want) + 8, NAN, torch.float64)
        torch.cuda.synchronize()
        panel.lod_windows_device(out.data_ptr(), W, ERROR, MG, pitch_align=32)
        n = panel.flatten_device(out.data_ptr(), W, feed.data_ptr(), len(want) + 8)
        snap = rig.clone(feed)
        rig.wait()
    assert n == len(want)
    assert ol.bits_equal(snap.cpu().numpy()[:n], want), nind


# =========================================================================== 3. async pipeline on the caller's stream

@pytest.mark.parametrize("gaps", [True, False], ids=["gaps-and-centromere", "no-gaps"])
def test_async_passes_between_the_callers_fills_and_clones(async_rig, busy, gaps):
    """set_async: the first pass plans, three more only enqueue -- behind pending work, each between the caller's out.fill_(nan)
    and out.clone().  Every snapshot is the oracle's: each pass ran after the fill before it and before the clone behind it, and
    wrote its MISSING stretches without a fill launch.  Stats and kernel times answer afterwards as in
    test_async_context_enqueues_repeated_calls"""
    import torch
    rig, nind, W = async_rig, 130, 50
    want = sc.lod_scores(nind, W, gaps)
    with open_panel(rig.ctx, nind, gaps=gaps) as panel:
        layout = panel.out_layout(32, nind)
        out = rig.full(layout[2], NAN, torch.float64)
        torch.cuda.synchronize()
        panel.lod_windows_device(out.data_ptr(), W, ERROR, MG, pitch_align=32)           # plans
        first = rig.clone(out)
        rig.fill(out, NAN)
        produced = rig.behind_delay(busy, [])
        pending(produced)
        snaps = []
        for _ in range(3):
            panel.lod_windows_device(out.data_ptr(), W, ERROR, MG, pitch_align=32)
            snaps.append(rig.clone(out))
            rig.fill(out, NAN)
        done = torch.cuda.Event()
        done.record(rig.s)
        assert done.query() is False, "the three passes did not only enqueue"
        st = panel.stats()                                                               # waits for the last pass
        ms = rig.ctx.recent_kernel_ms()
        rig.wait()
        assert st["chain_kernel_ms"] > 0 and st["n_valid_windows"] + st["n_missing"] == sc.nloci()
        assert len(ms) >= 4 and all(m > 0 for m in ms[-3:]), ms
        for k, snap in enumerate([first] + snaps):
            same_scores(snap, layout, nind, want, ("async pass", k, gaps))
        assert torch.isnan(out).all(), "a pass wrote after the caller's last fill"
        assert st["n_missing"] > 0


# =========================================================================== 4. side streams behind a pending pass

class PendingPass:
    """an asynchronous context whose stream holds the delay and an enqueue-only pass into `out` when the body runs"""

    def __init__(self, rig, busy, nind, codes=False):
        import torch
        self.rig, self.nind, self.W = rig, nind, 50
        self.panel = open_panel(rig.ctx, nind)
        if codes:
            c, _ = sc.likelihoods(nind)
            self.panel.set_gl_codes(np.concatenate(c, axis=0), sc.GL_VALUES)
        self.layout = self.panel.out_layout(32, nind)
        self.out = rig.full(self.layout[2], NAN, torch.float64)
        torch.cuda.synchronize()
        self.panel.lod_windows_device(self.out.data_ptr(), self.W, ERROR, MG, pitch_align=32)       # plans
        rig.fill(self.out, NAN)
        rig.behind_delay(busy, [])
        self.panel.lod_windows_device(self.out.data_ptr(), self.W, ERROR, MG, pitch_align=32)       # enqueues
        self.passed = torch.cuda.Event()
        self.passed.record(rig.s)
        assert self.passed.query() is False, "the pass is not pending: the case tests nothing"

    def check_pass(self):
        snap = self.rig.clone(self.out)
        self.rig.wait()
        same_scores(snap, self.layout, self.nind, sc.lod_scores(self.nind, self.W), ("the pending pass", self.nind))
        self.panel.close()


@pytest.mark.parametrize("nind", sc.NINDS)
def test_feed_multi_behind_a_pending_pass(async_rig, busy, nind):
    """garlic_lod_feed_multi: one stream per window size, each behind the context's stream"""
    pp = PendingPass(async_rig, busy, nind)
    feeds, per_chr = pp.panel.lod_feed_multi(sc.SCORE_WS, ERROR, MG)
    for k, W in enumerate(sc.SCORE_WS):
        want, counts = sc.feed_and_poison(nind, W)
        assert list(per_chr[k]) == counts and ol.bits_equal(feeds[k], want), (nind, W)
    pp.check_pass()


@pytest.mark.parametrize("nind", sc.NINDS)
def test_feed_multi_tgls_slabs_behind_a_pending_pass(async_rig, busy, nind):
    """garlic_lod_feed_multi_tgls under a term budget of two blocks: slabs built on the slab stream, the sizes' own streams
    behind them.  130 individuals (three blocks): three one-block slabs; 70 (two blocks): the budget holds both, one slab"""
    pp = PendingPass(async_rig, busy, nind, codes=True)
    budget = 2 * scases.block_bytes(sc.nloci())
    slab_blocks = scases.slab_blocks_for(budget, sc.nloci(), nind)
    assert slab_blocks == (1 if nind == 130 else 2)
    pp.panel.set_tgls_term_budget(budget)
    feeds, per_chr = pp.panel.lod_feed_multi_tgls(sc.TGLS_WS, MG)
    terms = pp.panel.tgls_terms_info()
    assert terms["slab_blocks"] == slab_blocks and terms["n_slabs"] == -(-((nind + 63) // 64) // slab_blocks), terms
    for k, W in enumerate(sc.TGLS_WS):
        parts = [ol.oracle_flatten(s, W) for s in sc.tgls_scores_and_poison(nind, W)[0]]
        assert list(per_chr[k]) == [len(x) for x in parts], (nind, W)
        assert ol.bits_equal(feeds[k], np.concatenate(parts)), (nind, W)
    pp.check_pass()


def test_lod_kde_behind_a_pending_pass(async_rig, busy):
    """garlic_lod_kde: the feed, the sort and the KDE kernels"""
    from test_gpu_kde import check_kde
    nind, W = 130, 10
    pp = PendingPass(async_rig, busy, nind)
    got, per_chr = pp.panel.lod_kde(W, ERROR, MG, W)
    want, counts = sc.feed_and_poison(nind, W)
    assert list(per_chr) == counts
    check_kde(got, np.sort(want), "lod_kde behind a pending pass")
    pp.check_pass()


@pytest.mark.parametrize("nind", sc.NINDS)
def test_roh_segments_behind_a_pending_pass(async_rig, busy, nind):
    W = 10
    pp = PendingPass(async_rig, busy, nind)
    got = pp.panel.roh_segments(W, ERROR, MG, sc.cutoff_of(nind, W), sc.FRAC)
    want = sc.segments(nind, W)
    assert len(want) > 0 and [tuple(int(v) for v in r) for r in got] == want, (nind, len(got), len(want))
    pp.check_pass()


@pytest.mark.parametrize("nind", sc.NINDS)
def test_compute_ld_behind_a_pending_pass(async_rig, busy, nind):
    W = 10
    pp = PendingPass(async_rig, busy, nind)
    got = pp.panel.compute_ld(W)
    assert ol.bits_equal(got, sc.hr2(nind, W)), (nind, ol.count_mismatch(got, sc.hr2(nind, W)))
    pp.check_pass()


# =========================================================================== 5. two contexts at once

def test_two_contexts_on_two_threads(busy):
    """two host threads, each with its own torch stream, context and panel (different data): eight rounds of alloc_scores ->
    lod_windows_device -> clone -> free through the shared score-buffer pool, then a lod_feed.  Every result is that thread's
    oracle answer; a GARLIC_ERR_INVALID in one thread leaves the other's garlic_hip_last_error() text as it was"""
    import torch
    W, rounds = 50, 8
    ninds = (70, 130)
    for k, nind in enumerate(ninds):
        sc.lod_scores(nind, W, True, k)                      # (the oracle, before the threads start)
    assert not all(ol.bits_equal(a[:70], b[:70]) for a, b in zip(sc.lod_scores(70, W, True, 0), sc.lod_scores(130, W, True, 1)))
    gate = threading.Barrier(2, timeout=120)
    result, errors = [None, None], []

    def work(k):
        try:
            torch.cuda.set_device(0)
            nind = ninds[k]
            r = Rig()
            text = []
            with open_panel(r.ctx, nind, seed=k) as panel:
                layout = panel.out_layout(32, nind)
                gate.wait()
                snaps = []
                for _ in range(rounds):
                    buf = r.ctx.alloc_scores(layout[2])
                    panel.lod_windows_device(buf.ptr, W, ERROR, MG, pitch_align=32)
                    snaps.append(r.clone(buf.tensor()))
                    buf.free()
                feed, per_chr = panel.lod_feed(W, ERROR, MG, W)
                if k == 1:
                    text.append(abi.lib().garlic_hip_last_error())
                gate.wait()
                if k == 0:
                    with pytest.raises(abi.GarlicError) as e:
                        panel.lod_windows(1, ERROR, MG)
                    assert e.value.code == abi.ERR_INVALID
                    text.append(abi.lib().garlic_hip_last_error())
                gate.wait()
                if k == 1:
                    text.append(abi.lib().garlic_hip_last_error())
                r.wait()
                result[k] = (layout, [s.cpu().numpy() for s in snaps], feed, list(per_chr), text)
            r.close()
        except BaseException as e:                           # noqa: B036 (reported by the main thread)
            errors.append((k, e))
            gate.abort()

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0][1]
    for k, nind in enumerate(ninds):
        (base, pitch, _), snaps, feed, per_chr, text = result[k]
        want = sc.lod_scores(nind, W, True, k)
        for i, host in enumerate(snaps):
            got = sc.rows_of(host, base, pitch, nind)
            for c in range(len(want)):
                assert ol.count_mismatch(got[c], want[c]) == 0, ("thread", k, "round", i, "chromosome", c)
        flat, counts = sc.flat_feed(want, W)
        assert per_chr == counts and ol.bits_equal(feed, flat), ("thread", k, "feed")
    assert b"window size must be > 1" in result[0][4][0]
    before, after = result[1][4]
    assert before == after and after != result[0][4][0], (before, after)
