"""GPU: GMM::estimate on the device (csrc/gmm_kernels.hpp, garlic_gmm_fit) against the numpy reference of
tests/gmm_cases.py -- never against a second run of the kernels, except where the claim is that two runs agree.

Tolerance (not from what the kernels give): per case the float64 sequential reference's largest relative deviation from
the long-double reference over the fields a, mean, var, loglik, bic is that case's rounding noise -- what the reference's
own arithmetic leaves undetermined.  The device gets 8 times it on every field: its exp and log are good to 2 ulp where
glibc's are good to under 1, and those errors travel through the same iterations with the same amplification (the
cancellation in var = S2 / S0 - mean^2 above all) as the float64 roundings do.  A field that is NaN in the reference
(n = 1: the variance of one length is 0 * inf) must be NaN on the device.

Measured on an MI355X (profiles/gmm_parity.txt): of 148 comparable cases the device deviates less
than the float64 reference itself in 127 and stays within the bound in all; the largest deviation / bound is 0.74
(three-64-2, 25 updates: device 3.15e-15 on var of the large class, float64 reference 5.33e-16, bound 4.26e-15), the next
0.37.  That case is why the kernels' sums carry their rounding errors in a second double: with plain FP64 sums in the
kernels' tree order the device landed at 1.01e-14 there -- as the sequential float64 arithmetic does with the 64 points
reversed (five random orders: 3.1e-15 to 2.1e-14) -- the order of the adds alone, fed back through 25 updates and the
30-fold cancellation of var = S2 / S0 - mean^2."""
import numpy as np
import pytest

import gmm_cases as cases
import oracle_lib as ol
from garlic_amd import abi

pytestmark = pytest.mark.gpu
LD = np.longdouble
FACTOR = 8.0


def same_fit(a, b):
    return all(a[k] == b[k] for k in ("k", "iterations", "converged")) and \
        all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in ("loglik", "bic")) and \
        all(ol.bits_equal(a[k], b[k]) for k in ("a", "mean", "var"))


def check_fields(got, f64, ld, what):
    """the largest relative deviation of a field from the long-double reference over the bound, FACTOR x the reference's own
    noise (the caller asserts that it is <= 1); a NaN pattern that differs fails here"""
    noise = cases.noise(f64, ld)
    g, q = cases.flat(got).astype(LD), cases.flat(ld).astype(LD)
    if noise is None:                       # the two references disagree on which fields are NaN: nothing is determined
        print("%s: the float64 and long-double references have different NaNs; not compared" % what)
        return 0.0
    assert (np.isnan(g) == np.isnan(q)).all(), (what, "NaN pattern", g, q)
    if np.isnan(q).all():
        return 0.0
    noise = max(noise, 2.0 ** -53)          # the reference never agrees with itself better than half an ulp of a double
    ok = ~np.isnan(q) & (q != 0)
    assert (g[~np.isnan(q) & (q == 0)] == 0).all(), what
    dev = float(np.max(np.abs(g[ok] - q[ok]) / np.abs(q[ok])))
    print("%s: device deviation %.3g, reference noise %.3g, bound %.3g" % (what, dev, noise, FACTOR * noise))
    return dev / (FACTOR * noise)


@pytest.fixture(scope="module")
def fixed_refs():
    cases.warm(cases.fixed_cases(), cases.fixed_reference)
    return cases.fixed_reference


@pytest.mark.parametrize("name,n,k", cases.fixed_cases(), ids=lambda v: str(v))
def test_fixed_iteration_counts(gpu_ctx, fixed_refs, name, n, k):
    """precision -1 never stops: exactly max_iter updates, every field against the long-double reference"""
    x = cases.data_of(name, n)
    a0, m0, v0 = cases.init(x, k)
    missed = []
    for iters in cases.FIXED_ITERS:
        f64, ld = fixed_refs(name, n, k)[iters]
        got = gpu_ctx.gmm_fit(x, a0, m0, v0, max_iter=iters, precision=-1.0)
        what = "%s n=%d K=%d iterations=%d" % (name, n, k, iters)
        assert got["k"] == k and got["iterations"] == iters and got["converged"] == 0, what
        assert gpu_ctx.gmm_fit_info()["blocks"] == cases.blocks(n), what
        ratio = check_fields(got, f64, ld, what)
        if ratio > 1.0:
            missed.append((what, ratio))
    assert not missed, missed


def test_stop_rule(gpu_ctx):
    """precision 1e-5, max_iter 1000: the reference's stop iteration (tests/test_gmm_cpu.py asserts that its float64 and
    long-double forms agree on it), converged, the parameters within the bound"""
    cases.warm(cases.stop_cases(), cases.stop_reference)
    for name, n, k in cases.stop_cases():
        x = cases.data_of(name, n)
        a0, m0, v0 = cases.init(x, k, recurrence=name.startswith("refs"))
        f64, ld = cases.stop_reference(name, n, k)
        assert f64["iterations"] == ld["iterations"]
        got = gpu_ctx.gmm_fit(x, a0, m0, v0, max_iter=cases.MAX_ITER, precision=cases.PRECISION)
        what = "stop %s n=%d K=%d" % (name, n, k)
        assert got["iterations"] == ld["iterations"] and got["converged"] == 1, (what, got["iterations"], ld["iterations"])
        ratio = check_fields(got, f64, ld, what)
        assert ratio <= 1.0, (what, ratio)


def test_degenerate_inputs(gpu_ctx):
    """one or two lengths, three classes: NaN parameters as in the reference, no convergence, no error"""
    for n in (1, 2):
        x = cases.content("three", n)
        a0, m0, v0 = cases.init(x, 3)
        ld = cases.fit(x, a0, m0, v0, 5, cases.PRECISION, LD)
        assert np.isnan(cases.flat(ld)).any() and ld["converged"] == 0, n
        got = gpu_ctx.gmm_fit(x, a0, m0, v0, max_iter=5, precision=cases.PRECISION)
        assert got["converged"] == 0 and got["iterations"] == 5, (n, got)
        assert (np.isnan(cases.flat(got)) == np.isnan(cases.flat(ld).astype(np.float64))).all(), (n, got, ld)


def test_determinism_and_placement(gpu_ctx):
    import torch
    b = cases.block_points()
    for name, n, k in (("three", 3 * b + 17, 3), ("two", 65, 2), ("three", cases.BIG, 8)):
        x = cases.content(name, n)
        a0, m0, v0 = cases.init(x, k)
        first = gpu_ctx.gmm_fit(x, a0, m0, v0, max_iter=7, precision=-1.0)
        assert same_fit(first, gpu_ctx.gmm_fit(x, a0, m0, v0, max_iter=7, precision=-1.0)), (name, n, k)
        t = torch.from_numpy(np.array(x)).cuda()
        on_device = gpu_ctx.gmm_fit(t.data_ptr(), a0, m0, v0, n=n, max_iter=7, precision=-1.0)
        torch.cuda.synchronize()
        assert ol.bits_equal(t.cpu().numpy(), x), "the caller's device buffer was modified"
        assert same_fit(first, on_device), (name, n, k)
        # another context: nothing of the result depends on what a context keeps
        with abi.Context(0) as other:
            assert same_fit(first, other.gmm_fit(x, a0, m0, v0, max_iter=7, precision=-1.0))
        # a batch boundary inside the fit (the host reads the state every 64 updates): 130 updates at once or piecewise
    x = cases.content("two", 65)
    a0, m0, v0 = cases.init(x, 2)
    whole = gpu_ctx.gmm_fit(x, a0, m0, v0, max_iter=130, precision=-1.0)
    part = gpu_ctx.gmm_fit(x, a0, m0, v0, max_iter=64, precision=-1.0)
    rest = gpu_ctx.gmm_fit(x, part["a"], part["mean"], part["var"], max_iter=66, precision=-1.0)
    assert whole["iterations"] == 130 and all(ol.bits_equal(whole[f], rest[f]) for f in ("a", "mean", "var"))
    assert whole["loglik"] == rest["loglik"]


def test_refusals_and_info(gpu_ctx):
    import ctypes as C
    x = cases.content("three", 65)
    a0, m0, v0 = cases.init(x, 3)
    L, h = abi.lib(), gpu_ctx.handle
    g = abi.Gmm()
    p = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    xp = C.c_void_p(x.ctypes.data)
    good = dict(x=xp, n=65, where=abi.HOST, k=3, a=p(a0), m=p(m0), v=p(v0), it=5, out=C.byref(g))
    def call(**kw):
        c = dict(good, **kw)
        return L.garlic_gmm_fit(h, c["x"], c["n"], c["where"], c["k"], c["a"], c["m"], c["v"], c["it"], 1e-5, c["out"])
    assert call() == abi.OK and g.k == 3 and 1 <= g.iterations <= 5
    for bad in (dict(x=None), dict(n=0), dict(n=-3), dict(k=0), dict(k=abi.GMM_MAX_K + 1), dict(it=0), dict(where=2), dict(a=None),
                dict(m=None), dict(v=None), dict(out=None)):
        assert call(**bad) == abi.ERR_INVALID, bad
        assert b"GMM fit" in L.garlic_hip_last_error()
    assert L.garlic_gmm_fit(None, xp, 65, abi.HOST, 3, p(a0), p(m0), p(v0), 5, 1e-5, C.byref(g)) == abi.ERR_INVALID
    gpu_ctx.gmm_fit(x, a0, m0, v0, max_iter=3)
    info = gpu_ctx.gmm_fit_info()
    assert info["blocks"] == cases.blocks(65) == 1 and info["scratch_bytes"] > 0 and info["em_ms"] > 0
    big = cases.content("three", cases.BIG)
    gpu_ctx.gmm_fit(big, *cases.init(big, 3), max_iter=2, precision=-1.0)
    assert gpu_ctx.gmm_fit_info()["blocks"] == cases.blocks(cases.BIG) > 1
