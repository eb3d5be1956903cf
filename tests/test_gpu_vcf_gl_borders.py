"""GPU: tgls_vcf_parse_kernel (csrc/vcf_gl_kernels.hpp) with every line event on the borders of its passes: FORMAT and its key
anywhere behind a long INFO, the key first in FORMAT, column state carried over passes without events, line ends on the last
and first bytes of a pass, offences decided in a later pass than the first.  The lines and what they plant are those of
tests/vcf_gl_border_cases.py (tests/test_vcf_gl_borders_cpu.py checks their geometry and spells out the rule's answers).

Every test builds one slab per alignment and makes one call with it; every row is compared: the statuses with the rule's, the
values of every row the rule leaves clean bit for bit, and a slab that is clean throughout also code for code with
garlic_tgls_set_rows_text on the twin text.  Slabs are 0.2 to 3.7 MB of lines of 4 to 13 KB with 3 samples."""
import numpy as np
import pytest

import tgls_cases as tc
import vcf_gl_border_cases as bc
import vcf_gl_cases as vg
from garlic_amd import abi

pytestmark = pytest.mark.gpu

COLON, TAB = 0x3A, 0x09
TWO = ["dev0", "dev5"]


def clean_runs(status):
    """[(first row, count)] of the rows without a status"""
    runs, r, n = [], 0, len(status)
    while r < n:
        if status[r, 0]:
            r += 1
            continue
        e = r
        while e < n and not status[e, 0]:
            e += 1
        runs.append((r, e - r))
        r = e
    return runs


def compare_rows(obj, want, want_status, note):
    for r0, n in clean_runs(want_status):
        got = obj.get_rows(row_begin=r0, row_count=n)
        same = tc.bits(got) == tc.bits(want[r0:r0 + n])
        assert same.all(), (note, "row", r0 + int(np.argwhere(~same)[0][0]), np.argwhere(~same)[:5].tolist())


def check_slab(gpu_ctx, slab, where, key=bc.KEY, missing_raw=None, col_idx=None, poison=COLON):
    text, lb, marks, nind = slab
    rows = len(lb) - 1
    want, want_status = vg.parse_slab(text, lb, nind, key, missing_raw, col_idx)
    note = (where, key, missing_raw, poison)
    with abi.Tgls(gpu_ctx, rows, nind, col_idx) as obj:
        status, err = vg.feed(obj, text, lb, where, key=key, missing_raw=missing_raw, poison=poison)
        differ = np.flatnonzero((status != want_status).any(axis=1))
        assert differ.size == 0, (note, [(int(r), status[r].tolist(), want_status[r].tolist(), marks[r]) for r in differ[:4]])
        assert (err is None) == (not (want_status[:, 0] >= vg.FEW).any()), (note, err)
        compare_rows(obj, want, want_status, note)
        if want_status.any():
            return want_status
        assert not np.isnan(want).any()
        assert obj.info() == (np.unique(tc.bits(want)).shape[0], rows, 0)
        if col_idx is not None:
            return want_status
        twin_text, twin_lb = tc.slab_of(vg.twin_tgls(text, lb, nind, key, missing_raw))
        with abi.Tgls(gpu_ctx, rows, nind) as twin:
            st, err = twin.set_rows_text(twin_text, twin_lb)
            assert err is None and not st.any()
            assert np.array_equal(tc.bits(obj.values()), tc.bits(twin.values())), note
            assert np.array_equal(tc.bits(twin.get_rows()), tc.bits(obj.get_rows())), note
    return want_status


# ------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("where", TWO)
@pytest.mark.parametrize("key", bc.KEYS)
def test_format_and_its_key_on_every_border_byte(gpu_ctx, key, where):
    """FORMAT's first byte, the key's first and last byte and FORMAT's tab on every offset of BORDER behind a long INFO that
    holds colons and the key's letters; keys of 1, 2 and 16 bytes, first, in the middle and last among decoys that contain
    them or are contained; FORMAT wholly in the third pass; the key named twice.  856 lines, 3.7 MB, clean: the twin too"""
    st = check_slab(gpu_ctx, bc.format_slab(key, int(where[3:])), where, key=key)
    assert not st.any()


@pytest.mark.parametrize("where", TWO)
@pytest.mark.parametrize("key", bc.KEYS)
def test_a_format_of_decoys_only_across_the_border(gpu_ctx, key, where):
    st = check_slab(gpu_ctx, bc.no_key_slab(key, int(where[3:])), where, key=key)
    assert st[1::2].tolist() == [[vg.NO_KEY, 0]] * (len(st) // 2) and not st[0::2].any()


# ------------------------------------------------------------------------------------------------ b
@pytest.mark.parametrize("where", TWO)
@pytest.mark.parametrize("missing_raw", [None, 0.0, 99.0])
def test_the_key_first_in_format(gpu_ctx, missing_raw, where):
    """k == 0: the value stands on the column's own first byte, which stands on every offset of BORDER: values of 1, 17, 32
    and 33 bytes, `.`, an empty column, `.:3`, `:3`, a bare value, `.:./.:4`, `:./.`.  781 lines, 3.3 MB"""
    st = check_slab(gpu_ctx, bc.key_first_slab(int(where[3:])), where, missing_raw=missing_raw)
    per_form = bc.FIRST_STATUS if missing_raw is None else [s if s[0] == vg.DEFERRED else [0, 0] for s in bc.FIRST_STATUS]
    assert st.tolist() == per_form * len(bc.BORDER)


@pytest.mark.parametrize("where", TWO)
def test_the_key_first_and_the_straddling_column_not_kept(gpu_ctx, where):
    """the column on the border holds a list, nothing, 40 digits or a colon and is not kept: clean, the others' values stand"""
    st = check_slab(gpu_ctx, bc.key_first_slab(int(where[3:]), forms=bc.UNKEPT_FORMS), where, col_idx=[2, 0])
    assert not st.any()


# ------------------------------------------------------------------------------------------------ c
@pytest.mark.parametrize("where", TWO)
@pytest.mark.parametrize("missing_raw", [None, 99.0])
@pytest.mark.parametrize("k", bc.CARRY_KS)
def test_column_state_carried_over_passes(gpu_ctx, k, missing_raw, where):
    """a column that begins in one pass and whose k-th colon, closing tab or line end stands in the next, or in the one after
    that behind a pass without events: the colons counted so far and the column's leading `.` are what the passes carry.
    613 lines, 2.7 MB"""
    slab = bc.carried_slab(k, int(where[3:]))
    st = check_slab(gpu_ctx, slab, where, missing_raw=missing_raw)
    for mark, s in zip(slab[2], st.tolist()):
        called_without = mark["case"] not in ("value", "once") and not mark["dot"] and missing_raw is None
        assert s == ([vg.NO_VALUE, 2 if mark["case"] == "short last" else 1] if called_without else [0, 0]), (mark, s)


# ------------------------------------------------------------------------------------------------ d
@pytest.mark.parametrize("poison", [COLON, TAB])
@pytest.mark.parametrize("missing_raw", [None, 99.0])
def test_line_ends_at_pass_borders_followed_by_a_line(gpu_ctx, missing_raw, poison):
    """a value, a short column and a tab in front of the line's end; \\n, \\r\\n and the next line's offset as the end; a row cut
    in front of its newline; line lengths P - 1, P, P + 1, 2P and P + 16k - 1, and the same as offsets in the pass; at all 16
    alignments.  About 240 lines, 1.0 MB per alignment"""
    for align in bc.ALIGNS:
        slab = bc.line_end_slab(align)
        st = check_slab(gpu_ctx, slab, "dev%d" % align, missing_raw=missing_raw, poison=poison)
        for mark, s in zip(slab[2], st.tolist()):
            if "variant" in mark:
                assert s == mark["status" if missing_raw is None else "status_missing"], (align, mark, s)


@pytest.mark.parametrize("poison", [COLON, TAB])
def test_line_ends_at_pass_borders_alone_in_the_slab(gpu_ctx, poison):
    """the same lines, each the only row of a slab that ends with it, behind it nothing but poison (or what a cut leaves):
    one device buffer per alignment holds them 64 bytes and more apart, one call per line"""
    import torch
    for align in bc.ALIGNS:
        rows = bc.end_rows(lambda size: align)
        buf, at = bytearray(), []
        for data, rest, mark in rows:
            buf += bytes([poison]) * (64 + (align - len(buf) - 64) % bc.PIECE)
            at.append(len(buf))
            buf += data + rest
        buf += bytes([poison]) * 64
        dev = torch.empty(len(buf) + bc.PIECE, dtype=torch.uint8, device="cuda")
        skew = (-dev.data_ptr()) % bc.PIECE
        dev[skew:skew + len(buf)] = torch.frombuffer(buf, dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        want = np.full((len(rows), 3), np.nan)
        want_status = np.zeros((len(rows), 2), dtype=np.int32)
        got_status = np.zeros_like(want_status)
        with abi.Tgls(gpu_ctx, len(rows), 3) as obj:
            for r, (data, rest, mark) in enumerate(rows):
                lb = np.array([0, len(data)], dtype=np.int64)
                assert (dev.data_ptr() + skew + at[r]) % bc.PIECE == align == mark["first"]
                # a cut row's slab goes on behind it; every other slab ends with its line
                w, ws = vg.parse_slab(data + rest, lb, 3, bc.KEY)
                want[r], want_status[r] = w[0], ws[0]
                assert ws[0].tolist() == mark["status"]
                try:
                    st, err = obj.set_rows_vcf(dev.data_ptr() + skew + at[r], lb, bc.KEY, row_begin=r, text_bytes=len(data + rest),
                                               where=abi.DEVICE)
                except abi.GarlicError as e:
                    raise AssertionError((align, mark, str(e)))
                got_status[r] = st[0]
            differ = np.flatnonzero((got_status != want_status).any(axis=1))
            assert differ.size == 0, (align, poison, [(got_status[r].tolist(), rows[r][2]) for r in differ[:4]])
            compare_rows(obj, want, want_status, (align, poison))


# ------------------------------------------------------------------------------------------------ e
@pytest.mark.parametrize("where", TWO + ["dev15"])
@pytest.mark.parametrize("missing_raw", [None, 99.0])
def test_offences_decided_in_a_later_pass(gpu_ctx, missing_raw, where):
    """bc.LATE: too many and too few columns found in the third pass, alone and with a deferred value in the first; NO_VALUE
    and DEFERRED two passes apart, in both orders of column (the lower column wins: a NO_VALUE of the third pass at a column
    below a DEFERRED of the first cannot be written, columns stand in byte order).  8 lines of 8 KB"""
    st = check_slab(gpu_ctx, bc.late_slab(int(where[3:])), where, missing_raw=missing_raw)
    assert st.tolist() == ([x[3] for x in bc.LATE] if missing_raw is None else bc.LATE_WITH_MISSING)
