"""GPU: the KDE feed sorted on the device (csrc/feed_sort_kernel.hpp), bit for bit against numpy's sort of the transformed
keys -- never against a second run of the sorter.  No tolerance.

  1. the sorter alone (garlic_feed_sort, host and device buffers): every size around the wave and the tile, contents from
     random to all-equal, keys that differ in one byte only (one pass runs, seven are skipped)
  2. through every feed call with GARLIC_FEED_ORDER_SORTED: np.sort of the ORACLE's feed (unique: tests/test_feed_sort_cpu.py),
     count, per-chromosome counts and the reported forms those of the reference-order call
  3. the order set back: the oracle's order again
  4. a capacity one short of the count: nothing written, the count reported, in both orders"""
import ctypes as C

import numpy as np
import pytest

import feed_sort_cases as cases
import oracle_lib as ol
from garlic_amd import abi

pytestmark = pytest.mark.gpu
MG, ERROR, M, MU = cases.MG, cases.ERROR, cases.M, cases.MU


def same_bits(a, b):
    """ol.bits_equal: the uint64 views compared (signed zeros and NaN payloads count)"""
    return ol.bits_equal(a, b)


def check_sort(ctx, x, what, device=False):
    want = cases.sorted_by_key(x)
    if device:
        import torch
        t = torch.from_numpy(x.copy()).cuda()
        ctx.feed_sort(t.data_ptr() if x.shape[0] else 0, n=x.shape[0])
        torch.cuda.synchronize()
        got = t.cpu().numpy()
    else:
        got = x.copy()
        ctx.feed_sort(got)
    info = ctx.feed_sort_info()
    assert same_bits(got, want), (what, int((got.view(np.uint64) != want.view(np.uint64)).sum()))
    if x.shape[0] > 1:
        assert info["passes_run"] + info["passes_skipped"] == 8, (what, info)
    return info


# ------------------------------------------------------------------------------------------------ 1. the sorter alone

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", cases.CONTENTS)
def test_sorter_sizes_and_contents(gpu_ctx, name, device):
    for n in cases.sizes():
        info = check_sort(gpu_ctx, cases.content(name, n), (name, n, device), device)
        if name == "equal" and n > 1:
            assert info["passes_run"] == 0, (n, info)
        if n > 1:
            assert info["scratch_bytes"] >= 8 * n


@pytest.mark.parametrize("byte", range(8))
def test_keys_that_differ_in_one_byte(gpu_ctx, byte):
    for n in (2, cases.fs_tile() + 1, 3 * cases.fs_tile() + 17):
        info = check_sort(gpu_ctx, cases.one_byte_keys(byte, n), ("byte", byte, n))
        assert (info["passes_run"], info["passes_skipped"]) == (1, 7), (byte, n, info)
    info = check_sort(gpu_ctx, cases.one_byte_keys(byte, 3 * cases.fs_tile() + 17, seed=1), ("byte", byte, "device"), device=True)
    assert (info["passes_run"], info["passes_skipped"]) == (1, 7), (byte, info)


def test_sorter_arguments(gpu_ctx):
    L = abi.lib()
    x = np.array([2.0, 1.0])
    assert L.garlic_feed_sort(gpu_ctx.handle, None, 0, abi.HOST) == abi.OK                       # n = 0: nothing happens
    assert L.garlic_feed_sort(gpu_ctx.handle, None, 2, abi.HOST) == abi.ERR_INVALID
    assert L.garlic_feed_sort(gpu_ctx.handle, C.c_void_p(x.ctypes.data), -1, abi.HOST) == abi.ERR_INVALID
    assert L.garlic_feed_sort(gpu_ctx.handle, C.c_void_p(x.ctypes.data), 2, 7) == abi.ERR_INVALID
    assert list(x) == [2.0, 1.0]
    assert L.garlic_feed_sort_info(gpu_ctx.handle, None, None, None) == abi.OK


# ------------------------------------------------------------------------------------------------ 2. - 4. the feed calls

def open_panel(ctx, nind, call):
    chroms, gpos, lds, codes, values, gl = cases.panel(nind)
    panel = abi.Panel(ctx, [c[0].shape[0] for c in chroms], nind)
    panel.set_map(np.concatenate([c[2] for c in chroms]), [c[3] for c in chroms], [c[4] for c in chroms], gpos=np.concatenate(gpos))
    panel.set_freq(np.concatenate([c[1] for c in chroms]))
    panel.set_genotypes(np.concatenate([c[0] for c in chroms], axis=0))
    if cases.KIND[call] in ("tgls", "wlod_gl"):
        panel.set_gl_codes(np.concatenate(codes, axis=0), values)
    if cases.KIND[call] in ("wlod", "wlod_gl"):
        panel.set_ld(cases.W, np.concatenate(lds, axis=0))
    if call == "tgls_slabs":
        panel.set_tgls_term_budget(cases.slab_budget(nind))
    return panel


def run_call(panel, call, idx):
    """-> ([feed per size], [per-chromosome counts per size], what the info calls report)"""
    sizes = cases.call_sizes(call)
    if call == "multi":
        feeds, per_chr = panel.lod_feed_multi([w for w, _ in sizes], ERROR, MG, steps=[s for _, s in sizes], ind_idx=idx)
        return feeds, [list(r) for r in per_chr], panel.feed_info()
    if call == "multi_tgls":
        feeds, per_chr = panel.lod_feed_multi_tgls([w for w, _ in sizes], MG, steps=[s for _, s in sizes], ind_idx=idx)
        return feeds, [list(r) for r in per_chr], (panel.feed_info(), panel.feed_multi_info(len(sizes)))
    (w, step), kind = sizes[0], cases.KIND[call]
    feed, per_chr = panel.lod_feed(w, ERROR, MG, step, use_gl=kind in ("tgls", "wlod_gl"), weighted=kind.startswith("wlod"), M=M, mu=MU,
                                   ind_idx=idx)
    return [feed], [list(per_chr)], panel.feed_info()


FORMS = {"chain": abi.FEED_CHAIN, "scores": abi.FEED_FROM_SCORES, "wlod": abi.FEED_SAMPLED_WLOD, "wlod_gl": abi.FEED_SAMPLED_WLOD,
         "tgls": abi.FEED_TGLS_CHAIN, "tgls_slabs": abi.FEED_TGLS_CHAIN, "multi": abi.FEED_CHAIN}


@pytest.mark.parametrize("call,nind,subset", cases.panel_cases())
def test_feed_calls_sorted_then_reference_again(gpu_ctx, call, nind, subset):
    idx = cases.SUBSET if subset else None
    want = cases.oracle_feeds(call, nind, subset)
    with open_panel(gpu_ctx, nind, call) as panel:
        ref_feeds, ref_chr, ref_info = run_call(panel, call, idx)
        for k, per_chr in enumerate(want):           # the default order is the oracle's
            assert ref_chr[k] == [len(x) for x in per_chr], (call, k)
            assert same_bits(ref_feeds[k], np.concatenate(per_chr)), (call, k, "reference order")
        if call in FORMS:
            assert ref_info[0] == FORMS[call], (call, ref_info)
        else:
            groups = ref_info[1]["groups"]
            assert len(set(groups)) == 2 and ref_info[1]["forms"].count(abi.FEED_TGLS_CHAIN_SHARED) == 4, ref_info
        panel.set_feed_order(abi.FEED_ORDER_SORTED)
        feeds, per, info = run_call(panel, call, idx)
        sort_info = gpu_ctx.feed_sort_info()
        print(call, nind, subset, "values", [len(f) for f in feeds], sort_info)
        for k, per_chr in enumerate(want):
            flat = np.concatenate(per_chr)
            assert len(feeds[k]) == len(flat) and per[k] == ref_chr[k], (call, k)
            assert same_bits(feeds[k], np.sort(flat)), (call, k, "sorted")
        assert info == ref_info, (call, info, ref_info)
        if len(feeds[-1]) > 1:
            assert sort_info["passes_run"] + sort_info["passes_skipped"] == 8
        panel.set_feed_order(abi.FEED_ORDER_REFERENCE)           # nothing is left behind
        again, per, info = run_call(panel, call, idx)
        for k, per_chr in enumerate(want):
            assert per[k] == ref_chr[k] and same_bits(again[k], np.concatenate(per_chr)), (call, k, "reference order again")
        assert info == ref_info


def test_other_orders_are_refused(gpu_ctx):
    with open_panel(gpu_ctx, 1, "chain") as panel:
        for bad in (-1, 2, 100):
            with pytest.raises(abi.GarlicError) as e:
                panel.set_feed_order(bad)
            assert e.value.code == abi.ERR_INVALID


@pytest.mark.parametrize("call", ["chain", "scores", "tgls", "multi", "multi_tgls"])
def test_capacity_one_short_writes_nothing(gpu_ctx, call):
    nind = 65
    want = cases.oracle_feeds(call, nind)
    sizes = cases.call_sizes(call)
    L = abi.lib()
    with open_panel(gpu_ctx, nind, call) as panel:
        for order in (abi.FEED_ORDER_REFERENCE, abi.FEED_ORDER_SORTED):
            panel.set_feed_order(order)
            totals = [sum(len(x) for x in per_chr) for per_chr in want]
            bufs = [np.full(t, 123.25) for t in totals]
            caps = np.array([t - 1 for t in totals], dtype=np.int64)
            counts = np.zeros(len(sizes), dtype=np.int64)
            ws = np.array([w for w, _ in sizes], dtype=np.int32)
            st = np.array([s for _, s in sizes], dtype=np.int32)
            ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
            i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
            if call == "multi":
                rc = L.garlic_lod_feed_multi(panel.handle, ws.ctypes.data_as(i32p), st.ctypes.data_as(i32p), len(sizes), ERROR, MG, None, 0,
                                             ptrs, caps.ctypes.data_as(i64p), counts.ctypes.data_as(i64p), None)
            elif call == "multi_tgls":
                rc = L.garlic_lod_feed_multi_tgls(panel.handle, ws.ctypes.data_as(i32p), st.ctypes.data_as(i32p), len(sizes), MG, None, 0,
                                                  ptrs, caps.ctypes.data_as(i64p), counts.ctypes.data_as(i64p), None)
            else:
                rc = L.garlic_lod_feed(panel.handle, int(ws[0]), ERROR, MG, int(call == "tgls"), 0, M, MU, int(st[0]),
                                       C.c_void_p(bufs[0].ctypes.data), int(caps[0]), counts.ctypes.data_as(i64p), None)
            assert rc == abi.OK
            assert list(counts) == totals, (call, order)
            for b in bufs:
                assert (b == 123.25).all(), (call, order, "written despite the capacity")
