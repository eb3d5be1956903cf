"""GPU: the KDE of several feeds from one set of launches (csrc/kde_multi_kernels.hpp, garlic_feed_kde_multi /
garlic_lod_kde_multi).  The claim is bit identity with the single-feed calls -- a feed's KDE is a pure function of
(values, n) and its partition a function of n alone, so what else is in the batch must not show -- checked at the sizes
where the batching can go wrong; the single-feed calls themselves are checked against the long-double reference in
tests/test_gpu_kde.py, and check_kde runs on the batched results here as well (its tolerances, unchanged)."""
import ctypes as C

import numpy as np
import pytest

import feed_sort_cases as fcases
import kde_cases as cases
import oracle_lib as ol
import wlod_feed_cases as wcases
from garlic_amd import abi
from test_gpu_kde import bad_feeds, check_kde, open_panel, same_struct

MG, ERROR = fcases.MG, fcases.ERROR
gpu = pytest.mark.gpu
MIX = ["bimodal", "wide", "narrow", "two_values"]


def batch_sizes():
    c = cases.kde_chunk()
    return [2, 3, 64, 65, c - 1, c, c + 1, 3 * c + 17, cases.BIG]


def mixed_feeds():
    return [(MIX[k % len(MIX)], n) for k, n in enumerate(batch_sizes())]


_single = {}


def single(ctx, x):
    """ctx.feed_kde of one feed with feed_kde_info after it, computed once per feed and left unchanged"""
    key = (x.shape[0], x.tobytes() if x.shape[0] < 4096 else (x[:64].tobytes(), x[-64:].tobytes(), float(x.sum())))
    if key not in _single:
        got = ctx.feed_kde(np.ascontiguousarray(x))
        _single[key] = (got, ctx.feed_kde_info())
    return _single[key]


def run_multi(ctx, feeds, device, **kw):
    if not device:
        return ctx.feed_kde_multi([np.ascontiguousarray(f) for f in feeds], **kw)
    import torch
    ts = [torch.from_numpy(np.concatenate([f, [0.0]])).cuda() for f in feeds]        # (never empty: a real address for n = 0 too)
    got = ctx.feed_kde_multi([t.data_ptr() for t in ts], ns=[f.shape[0] for f in feeds], **kw)
    torch.cuda.synchronize()
    for t, f in zip(ts, feeds):
        assert ol.bits_equal(t.cpu().numpy()[:-1], f), "the caller's device buffer was modified"
    return got


# ------------------------------------------------------------------------------------------------ 1. bit identity in a batch

@gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_batch_equals_single_calls_at_every_size(gpu_ctx, device):
    todo = mixed_feeds()
    feeds = [cases.content(name, n) for name, n in todo]
    for order, label in ((list(range(len(feeds))), "as listed"), (list(range(len(feeds)))[::-1], "reversed")):
        got, status, _ = run_multi(gpu_ctx, [feeds[i] for i in order], device)
        assert status == [abi.OK] * len(feeds), (label, status)
        for k, i in enumerate(order):
            want, _ = single(gpu_ctx, feeds[i])
            assert same_struct(got[k], want), (todo[i], label, "device" if device else "host")
            if todo[i][0] in ("bimodal", "wide") and label == "as listed":
                check_kde(got[k], feeds[i], (todo[i], "in a batch"))


@gpu
def test_one_feed_and_two_identical_feeds(gpu_ctx):
    c = cases.kde_chunk()
    x = cases.content("bimodal", 3 * c + 17)
    got, status, third = gpu_ctx.feed_kde_multi([np.array(x)])
    assert status == [abi.OK] and third is None and same_struct(got[0], single(gpu_ctx, x)[0])
    got, status, _ = gpu_ctx.feed_kde_multi([np.array(x), np.array(x)])
    assert status == [abi.OK, abi.OK]
    assert same_struct(got[0], got[1]) and same_struct(got[0], single(gpu_ctx, x)[0])


# ------------------------------------------------------------------------------------------------ 2. chunks_per_slice = 2 beside a tiny feed

@gpu
def test_more_chunks_than_slices_next_to_a_tiny_feed(gpu_ctx):
    c = cases.kde_chunk()
    assert (cases.HUGE + c - 1) // c > 2048 and (cases.HUGE + c - 1) // c % 2 == 1
    feeds = [cases.content("uniform", cases.HUGE), cases.content("wide", 65)]
    got, status, _ = run_multi(gpu_ctx, feeds, False)
    info = gpu_ctx.feed_kde_multi_info(2)
    print(info)
    assert status == [abi.OK, abi.OK]
    for k, f in enumerate(feeds):
        want, winfo = single(gpu_ctx, f)
        assert same_struct(got[k], want), k
        assert info["chunks"][k] == winfo["chunks"] and info["pairs_skipped"][k] == winfo["pairs_skipped"]
    assert info["moments_ms"] > 0 and info["sums_ms"] > 0 and info["scratch_bytes"] > 0


# ------------------------------------------------------------------------------------------------ 3. launches and waits

@gpu
@pytest.mark.parametrize("n_feeds", [1, 3, 9])
def test_six_launches_and_two_waits_whatever_the_batch(gpu_ctx, n_feeds):
    todo = mixed_feeds()[-n_feeds:]
    feeds = [cases.content(name, n) for name, n in todo]
    got, status, _ = run_multi(gpu_ctx, feeds, False)
    info = gpu_ctx.feed_kde_multi_info(n_feeds)
    print(n_feeds, info)
    assert status == [abi.OK] * n_feeds
    assert info["kernel_launches"] == 6 and info["host_waits"] == 2
    for k, f in enumerate(feeds):
        _, winfo = single(gpu_ctx, f)
        assert info["chunks"][k] == winfo["chunks"] and info["pairs_skipped"][k] == winfo["pairs_skipped"], (todo[k], info, winfo)
    with pytest.raises(abi.GarlicError):
        gpu_ctx.feed_kde_multi_info(n_feeds + 1)
    assert abi.lib().garlic_feed_kde_multi_info(gpu_ctx.handle, n_feeds, None, None, None, None, None, None, None) == abi.OK


@gpu
def test_single_and_multi_info_records_do_not_mix(gpu_ctx):
    """garlic_feed_kde runs the multi-feed driver with one feed, yet "the last KDE on the context" and "the last multi-feed
    KDE" stay two records: neither call shows in the other's _info (scratch_bytes apart: the scratch is one)"""
    c = cases.kde_chunk()
    three = [cases.content("bimodal", n) for n in (c - 1, c, c + 1)]
    fourth = cases.content("wide", 3 * c + 17)

    def records():
        multi = gpu_ctx.feed_kde_multi_info(3)
        one = dict(gpu_ctx.feed_kde_info(), **gpu_ctx.feed_kde_times())
        multi.pop("scratch_bytes"), one.pop("scratch_bytes")
        return multi, one

    for multi_first in (True, False):
        if multi_first:
            _, status, _ = run_multi(gpu_ctx, three, False)
            multi_before, _ = records()
            gpu_ctx.feed_kde(np.ascontiguousarray(fourth))
            multi, one = records()
            assert multi == multi_before, "the single call shows in the multi-feed record"
        else:
            gpu_ctx.feed_kde(np.ascontiguousarray(fourth))
            _, one_before = records()
            _, status, _ = run_multi(gpu_ctx, three, False)
            multi, one = records()
            assert one == one_before, "the multi-feed call shows in the single record"
        assert status == [abi.OK] * 3
        assert multi["chunks"] == [1, 1, 2] and multi["kernel_launches"] == 6 and multi["host_waits"] == 2, multi
        assert one["chunks"] == 4 and one["pairs_skipped"] > 0 and one["moments_ms"] > 0 and one["sums_ms"] > 0, one
        with pytest.raises(abi.GarlicError):
            gpu_ctx.feed_kde_multi_info(4)


# ------------------------------------------------------------------------------------------------ 4. refusals inside a batch

def filled(n):
    outs = (abi.Kde * n)()
    C.memset(C.byref(outs), 0x5A, C.sizeof(outs))
    return outs


@gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals_inside_a_batch(gpu_ctx, device):
    c = cases.kde_chunk()
    good = [cases.content("bimodal", 65), cases.content("wide", c + 1), cases.content("narrow", 3 * c + 17)]
    bad = bad_feeds()
    feeds, bad_at = [], {}
    for k, (what, x, word) in enumerate(bad):           # good, bad, good, bad, ...
        feeds.append(good[k % len(good)])
        bad_at[len(feeds)] = (what, word)
        feeds.append(np.ascontiguousarray(x))
    feeds.append(good[0])
    outs = filled(len(feeds))
    untouched = bytes(filled(1))
    got, status, _ = run_multi(gpu_ctx, feeds, device, outs=outs)
    text = abi.lib().garlic_hip_last_error().decode()
    info = gpu_ctx.feed_kde_multi_info(len(feeds))
    lowest = min(bad_at)
    assert ("feed %d:" % lowest) in text and bad_at[lowest][1] in text, text
    assert info["kernel_launches"] == 6 and info["host_waits"] == 2
    for i, f in enumerate(feeds):
        if i in bad_at:
            assert status[i] == abi.ERR_INVALID and got[i] is None, (i, bad_at[i])
            assert bytes(outs[i]) == untouched, (i, bad_at[i])
            assert info["chunks"][i] == (0 if f.shape[0] < 2 else (f.shape[0] + c - 1) // c)
        else:
            assert status[i] == abi.OK and same_struct(got[i], single(gpu_ctx, f)[0]), i
    # every kind of refusal on its own beside one good feed: the text names it
    for what, x, word in bad:
        outs2 = filled(2)
        got, status, _ = run_multi(gpu_ctx, [good[0], np.ascontiguousarray(x)], device, outs=outs2)
        text = abi.lib().garlic_hip_last_error().decode()
        assert status == [abi.OK, abi.ERR_INVALID] and "feed 1:" in text and word in text, (what, status, text)
        assert bytes(outs2[1]) == untouched and same_struct(got[0], single(gpu_ctx, good[0])[0]), what
    # strict: the call fails and nothing is written
    outs = filled(len(feeds))
    before = bytes(outs)
    with pytest.raises(abi.GarlicError) as e:
        run_multi(gpu_ctx, feeds, device, outs=outs, strict=True)
    assert e.value.code == abi.ERR_INVALID and ("feed %d:" % lowest) in str(e.value)
    assert bytes(outs) == before
    for what, x, word in bad:                          # (refused before and after the moments alike)
        outs2 = filled(2)
        with pytest.raises(abi.GarlicError) as e:
            run_multi(gpu_ctx, [good[1], np.ascontiguousarray(x)], device, outs=outs2, strict=True)
        assert e.value.code == abi.ERR_INVALID and word in str(e.value), (what, str(e.value))
        assert bytes(outs2) == bytes(filled(2)), what
    got, status, _ = run_multi(gpu_ctx, good, device, strict=True)       # and the context still works
    assert status == [abi.OK] * 3 and all(same_struct(g, single(gpu_ctx, f)[0]) for g, f in zip(got, good))


@gpu
def test_nothing_active_after_the_moments_skips_the_sums(gpu_ctx):
    c = cases.kde_chunk()
    outs = filled(3)
    before = bytes(outs)
    got, status, _ = gpu_ctx.feed_kde_multi([np.full(c + 5, -3.25), np.full(2, 1.0), np.zeros(0)], outs=outs)
    info = gpu_ctx.feed_kde_multi_info(3)
    assert status == [abi.ERR_INVALID] * 3 and got == [None] * 3 and bytes(outs) == before
    assert info["kernel_launches"] == 4 and info["host_waits"] == 1 and info["chunks"] == [2, 1, 0], info
    assert "feed 0:" in abi.lib().garlic_hip_last_error().decode()


@gpu
def test_argument_errors_leave_everything_untouched(gpu_ctx):
    L = abi.lib()
    x = np.array([1.0, 2.0, 4.0])
    ptrs = (C.c_void_p * 33)(*([x.ctypes.data] * 33))
    ns = np.full(33, 3, dtype=np.int64)
    nsp = ns.ctypes.data_as(C.POINTER(C.c_int64))
    outs = filled(33)
    before = bytes(outs)
    status = np.full(33, -7, dtype=np.int32)
    stp = status.ctypes.data_as(C.POINTER(C.c_int32))
    for n_feeds in (0, 33, -1):
        assert L.garlic_feed_kde_multi(gpu_ctx.handle, ptrs, nsp, n_feeds, abi.HOST, outs, stp) == abi.ERR_INVALID, n_feeds
    assert L.garlic_feed_kde_multi(gpu_ctx.handle, ptrs, nsp, 2, 7, outs, stp) == abi.ERR_INVALID
    assert L.garlic_feed_kde_multi(None, ptrs, nsp, 2, abi.HOST, outs, stp) == abi.ERR_INVALID
    assert L.garlic_feed_kde_multi(gpu_ctx.handle, None, nsp, 2, abi.HOST, outs, stp) == abi.ERR_INVALID
    assert L.garlic_feed_kde_multi(gpu_ctx.handle, ptrs, None, 2, abi.HOST, outs, stp) == abi.ERR_INVALID
    assert L.garlic_feed_kde_multi(gpu_ctx.handle, ptrs, nsp, 2, abi.HOST, None, stp) == abi.ERR_INVALID
    holes = (C.c_void_p * 2)(x.ctypes.data, None)
    assert L.garlic_feed_kde_multi(gpu_ctx.handle, holes, nsp, 2, abi.HOST, outs, stp) == abi.ERR_INVALID
    assert bytes(outs) == before and (status == -7).all()
    ns[1] = 0                                           # a NULL feed of no values is that feed's refusal, not the call's
    assert L.garlic_feed_kde_multi(gpu_ctx.handle, holes, nsp, 2, abi.HOST, outs, stp) == abi.OK
    assert list(status[:2]) == [abi.OK, abi.ERR_INVALID] and bytes(outs[1]) == bytes(filled(1))
    assert same_struct(outs[0].as_dict(), gpu_ctx.feed_kde(x))


# ------------------------------------------------------------------------------------------------ 5. garlic_lod_kde_multi

NIND = 200
SIZES = [(10, 10), (25, 25), (100, 100), (100, 4), (10, 2), (5000, 5000)]
CHAINED = [(10, 10), (25, 25), (100, 100), (100, 4), (5000, 5000)]       # every step >= 4: the sizes keep their own kernels and slots
KINDS = {"unweighted": "lod", "tgls": "tgls"}


def test_every_size_but_the_widest_has_a_feed():
    """CPU, the oracle: on the panel of the tests below every size of SIZES but the 5000-wide one has at least 2 feed values,
    with everyone and with the subset; the 5000-wide one has none"""
    for kind in KINDS.values():
        for idx in (None, fcases.SUBSET):
            for W, step in SIZES:
                n = sum(len(f) for f in wcases.flat(fcases.oracle_scores(NIND, kind, W), step, idx))
                assert (n == 0) if W == 5000 else (n >= 2), (kind, W, step, n)


@gpu
@pytest.mark.parametrize("subset", [False, True], ids=["everyone", "subset"])
@pytest.mark.parametrize("sizes", [SIZES, CHAINED], ids=["with a step of 2", "steps from 4"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_lod_kde_multi_is_lod_kde_per_size(gpu_ctx, kind, sizes, subset):
    idx = fcases.SUBSET if subset else None
    ws, steps = [w for w, _ in sizes], [s for _, s in sizes]
    tgls = kind == "tgls"
    panel, _ = open_panel(gpu_ctx, kind, 10)
    with panel:
        want = []
        for W, step in sizes:
            try:
                want.append(panel.lod_kde(W, ERROR, MG, step, use_gl=tgls, ind_idx=idx))
            except abi.GarlicError as e:
                assert W == 5000 and e.code == abi.ERR_INVALID and "at least 2 values" in str(e), (W, step, str(e))
                want.append(None)
        assert [w is None for w in want] == [W == 5000 for W in ws]
        # what the multi feed call reports for the same arguments
        if tgls:
            _, ref_chr = panel.lod_feed_multi_tgls(ws, MG, steps=steps, ind_idx=idx)
            ref_info = (panel.feed_info(), panel.feed_multi_info(len(ws)))
        else:
            _, ref_chr = panel.lod_feed_multi(ws, ERROR, MG, steps=steps, ind_idx=idx)
            ref_info = (panel.feed_info(), None)
        for order in (abi.FEED_ORDER_REFERENCE, abi.FEED_ORDER_SORTED):
            panel.set_feed_order(order)
            before, _ = panel.lod_feed(10, ERROR, MG, 10, use_gl=tgls, ind_idx=idx)
            part, _ = panel.lod_kde_part(10, ERROR, MG, 10, use_gl=tgls, ind_idx=idx)
            with part:
                assert part.count() == len(before)
                outs = filled(len(ws))
                got, status, per_chr = panel.lod_kde_multi(ws, ERROR, MG, steps=steps, use_gl=tgls, ind_idx=idx, outs=outs)
                text = abi.lib().garlic_hip_last_error().decode()
                info = (panel.feed_info(), panel.feed_multi_info(len(ws)) if tgls else None)
                with pytest.raises(abi.GarlicError) as e:       # the part borrowed the panel's scratch before the call
                    part.count()
                assert e.value.code == abi.ERR_STATE and "stale" in str(e.value)
            assert info == ref_info, (kind, order)
            assert np.array_equal(per_chr, ref_chr), (kind, order)
            for i, (W, step) in enumerate(sizes):
                if want[i] is None:
                    assert status[i] == abi.ERR_INVALID and got[i] is None and bytes(outs[i]) == bytes(filled(1)), (W, step)
                    assert ("feed %d:" % i) in text and "at least 2 values (the feed holds 0)" in text, text
                else:
                    assert status[i] == abi.OK and same_struct(got[i], want[i][0]), (kind, W, step, order)
                    assert list(per_chr[i]) == list(want[i][1]), (kind, W, step)
            after, _ = panel.lod_feed(10, ERROR, MG, 10, use_gl=tgls, ind_idx=idx)       # the order setting is as it was
            assert ol.bits_equal(after, before), (kind, order)
            assert ol.bits_equal(before, np.sort(before)) == (order == abi.FEED_ORDER_SORTED)
        panel.set_feed_order(abi.FEED_ORDER_REFERENCE)
        # strict: the refused size fails the call, nothing is written; without that size it succeeds
        outs = filled(len(ws))
        with pytest.raises(abi.GarlicError) as e:
            panel.lod_kde_multi(ws, ERROR, MG, steps=steps, use_gl=tgls, ind_idx=idx, outs=outs, strict=True)
        assert e.value.code == abi.ERR_INVALID and "at least 2 values" in str(e.value) and bytes(outs) == bytes(filled(len(ws)))
        got, status, _ = panel.lod_kde_multi(ws[:-1], ERROR, MG, steps=steps[:-1], use_gl=tgls, ind_idx=idx, strict=True)
        assert all(same_struct(g, w[0]) for g, w in zip(got, want[:-1]))
        check_kde(got[0], np.sort(before), (kind, "size 10"))


@gpu
def test_lod_kde_multi_arguments(gpu_ctx):
    panel, _ = open_panel(gpu_ctx, "unweighted", 10)
    with panel:
        L = abi.lib()
        i32 = C.POINTER(C.c_int32)
        ws = np.full(33, 10, dtype=np.int32)
        st = np.full(33, 10, dtype=np.int32)
        wp, sp = ws.ctypes.data_as(i32), st.ctypes.data_as(i32)
        outs = filled(33)
        before = bytes(outs)
        for n_sizes in (0, 33):
            assert L.garlic_lod_kde_multi(panel.handle, wp, sp, n_sizes, ERROR, MG, 0, None, 0, outs, None, None) == abi.ERR_INVALID
        assert L.garlic_lod_kde_multi(None, wp, sp, 2, ERROR, MG, 0, None, 0, outs, None, None) == abi.ERR_INVALID
        assert L.garlic_lod_kde_multi(panel.handle, None, sp, 2, ERROR, MG, 0, None, 0, outs, None, None) == abi.ERR_INVALID
        assert L.garlic_lod_kde_multi(panel.handle, wp, None, 2, ERROR, MG, 0, None, 0, outs, None, None) == abi.ERR_INVALID
        assert L.garlic_lod_kde_multi(panel.handle, wp, sp, 2, ERROR, MG, 0, None, 0, None, None, None) == abi.ERR_INVALID
        ws[1] = 1                                       # the feed calls' validation
        assert L.garlic_lod_kde_multi(panel.handle, wp, sp, 2, ERROR, MG, 0, None, 0, outs, None, None) == abi.ERR_INVALID
        ws[1], st[1] = 10, 0
        assert L.garlic_lod_kde_multi(panel.handle, wp, sp, 2, ERROR, MG, 0, None, 0, outs, None, None) == abi.ERR_INVALID
        st[1] = 10
        bad_idx = np.array([0, 0], dtype=np.int32)
        assert L.garlic_lod_kde_multi(panel.handle, wp, sp, 2, ERROR, MG, 0, bad_idx.ctypes.data_as(i32), 2, outs, None, None) == abi.ERR_INVALID
        assert bytes(outs) == before
        got, status, _ = panel.lod_kde_multi([10] * 32, ERROR, MG)        # the most sizes a call takes
        want, _ = panel.lod_kde(10, ERROR, MG, 10)
        assert status == [abi.OK] * 32 and all(same_struct(g, want) for g in got)
