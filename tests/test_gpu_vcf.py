"""GPU: VCF text parsed on the device (garlic_bed_set_rows_vcf), the order plane of an image, its census and the phase fill
(garlic_panel_set_phase_bed), byte for byte against the numpy restatement in tests/vcf_cases.py.

vcf_parse_kernel has no switch point: every line takes the same passes of 256 sixteen-byte pieces.  What changes with the
shape is covered by shape: lines shorter than a piece and lines of several passes (nind 1250 with subfields: about 20 KB),
fields that span pieces, one field longer than a wave's 1024 bytes and longer than a quarter of a pass, rows whose last
byte / plane byte is ragged (every nind % 8), slabs that start at every offset from an aligned address."""
import numpy as np
import pytest

import oracle_lib as ol
import vcf_cases as vc
from garlic_amd import abi

pytestmark = pytest.mark.gpu


class DeviceSlab:
    """the text at `offset` bytes past a 16-byte aligned device address, with 64 bytes of `poison` on each side"""

    def __init__(self, text, offset, poison):
        import torch
        self.buf = torch.full((len(text) + 160,), poison, dtype=torch.uint8, device="cuda")
        base = self.buf.data_ptr()
        self.at = (-base) % 16 + 64 + offset
        self.buf[self.at:self.at + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        self.ptr = base + self.at
        assert self.ptr % 16 == offset


def parse(ctx, nind, text, lb, where="host", offset=0, poison=0x09, nrows=None, row_begin=0, bed=None):
    """-> (bed, status, err)"""
    rows = len(lb) - 1
    bed = abi.Bed(ctx, rows if nrows is None else nrows, nind) if bed is None else bed
    if where == "host":
        status, err = bed.set_rows_vcf(text, lb, row_begin=row_begin)
    else:
        slab = DeviceSlab(text, offset, poison)
        status, err = bed.set_rows_vcf(slab.ptr, lb, row_begin=row_begin, text_bytes=len(text), where=abi.DEVICE)
    return bed, status, err


def check_clean(bed, status, err, text, lb, nind, tag):
    image, plane, want_status, codes, order = vc.parse_slab(text, lb, nind)
    assert err is None and not want_status.any() and not status.any(), (tag, err, status[status[:, 0] != 0][:3])
    assert np.array_equal(bed.get_rows(), image), tag
    assert np.array_equal(bed.get_order_rows(), plane), tag
    return codes, order


def case_text(nind, seed=0, rows=None, **kw):
    rng = np.random.default_rng(100 + nind + seed)
    rows = (40 if nind <= 65 else 12) if rows is None else rows
    codes, order = vc.random_genotypes(rng, rows, nind)
    lines = vc.make_lines(rng, codes, order, **kw)
    return rng, codes, order, lines


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("nind", vc.NINDS)
def test_rows_plane_and_census_match_the_restatement(gpu_ctx, nind, where):
    """a mix of bare, short and piece-spanning fields; the census of the image with its plane; the same census after
    garlic_bed_set_rows + garlic_bed_set_order_rows from the fetched copies (the route to a further device); and an image of
    the same bytes without a plane, which counts as before"""
    _, codes, order, lines = case_text(nind)
    text, lb = vc.slab_of(lines)
    bed, status, err = parse(gpu_ctx, nind, text, lb, where, offset=nind % 16)
    with bed:
        got_codes, got_order = check_clean(bed, status, err, text, lb, nind, (nind, where))
        assert np.array_equal(got_codes, codes) and np.array_equal(got_order, order)
        counts, counted = bed.census()
        want_counts, want_counted = vc.census(codes, order)
        assert np.array_equal(counted, want_counted) and np.array_equal(counts, want_counts)
        if nind > 1:
            assert counted[0] == 1 and counted[1] == 1 and counted[2] == 0      # 1|0 first; ./. then 1|0; 0|1 first
        image, plane = bed.get_rows(), bed.get_order_rows()
        with abi.Bed(gpu_ctx, len(lines), nind) as second:
            second.set_rows(image)
            second.set_order_rows(plane)
            c2, k2 = second.census()
            assert np.array_equal(k2, want_counted) and np.array_equal(c2, want_counts)
            assert np.array_equal(second.get_order_rows(), plane)
        with abi.Bed(gpu_ctx, len(lines), nind) as plain:
            plain.set_rows(image)
            c3, k3 = plain.census()
            bed_counts, bed_counted = vc.census(codes)
            assert np.array_equal(k3, bed_counted) and np.array_equal(c3, bed_counts)
            with pytest.raises(abi.GarlicError) as e:
                plain.get_order_rows()
            assert e.value.code == abi.ERR_STATE
        if nind >= 5:
            assert (vc.census(codes)[1] != want_counted).any()      # the plane decides on some row of the case


@pytest.mark.parametrize("offset", range(16))
def test_every_slab_offset_and_two_poisons(gpu_ctx, offset):
    """the device slab between poisoned neighbours (tabs, then '1's): same bytes out whatever the neighbours hold"""
    nind = 9
    _, codes, order, lines = case_text(nind, seed=offset, rows=6)
    lines[-1] = lines[-1].rstrip(b"\n")          # the slab ends with the line: the poison follows the last genotype directly
    text, lb = vc.slab_of(lines, header=b"")     # and the first line begins with the slab
    out = []
    for poison in (0x09, 0x31):
        bed, status, err = parse(gpu_ctx, nind, text, lb, "device", offset, poison)
        with bed:
            check_clean(bed, status, err, text, lb, nind, (offset, poison))
            out.append((bed.get_rows(), bed.get_order_rows()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("form", ["crlf", "no_last_newline", "left_out", "wave_field", "crlf_no_last_newline"])
def test_line_forms(gpu_ctx, form, where):
    nind = 13
    kw = {}
    if form.startswith("crlf"):
        kw["newline"] = b"\r\n"
    if form == "wave_field":
        kw["wave_at"] = (2, 5)
    _, codes, order, lines = case_text(nind, rows=9, **kw)
    keep = None
    if form.endswith("no_last_newline"):
        lines[-1] = lines[-1].rstrip(b"\r\n")
    if form == "left_out":
        keep = [0, 1, 4, 5, 8]                   # lines 2-3 and 6-7 stay in the text; line_begin passes over them
    text, lb = vc.slab_of(lines, keep)
    bed, status, err = parse(gpu_ctx, nind, text, lb, where, offset=5)
    with bed:
        got_codes, _ = check_clean(bed, status, err, text, lb, nind, (form, where))
        assert np.array_equal(got_codes, codes if keep is None else codes[keep])


@pytest.mark.parametrize("nind", [7, 8, 9, 65])
def test_row_begin_into_a_prefilled_image(gpu_ctx, nind):
    """rows [7, 12) of a 20-row image that holds a pattern: the rows and plane rows outside the call keep it, the rows inside
    are the restatement's (pad bits zero)"""
    _, codes, order, lines = case_text(nind, rows=5)
    text, lb = vc.slab_of(lines)
    rb, pb = (nind + 3) // 4, (nind + 7) // 8
    pat_rows = (np.arange(20 * rb, dtype=np.uint32).reshape(20, rb) * 37 + 0xA5).astype(np.uint8)
    pat_plane = (np.arange(20 * pb, dtype=np.uint32).reshape(20, pb) * 91 + 0x5A).astype(np.uint8)
    with abi.Bed(gpu_ctx, 20, nind) as bed:
        bed.set_rows(pat_rows)
        bed.set_order_rows(pat_plane)
        _, status, err = parse(gpu_ctx, nind, text, lb, "device", offset=3, row_begin=7, bed=bed)
        assert err is None and not status.any()
        image, plane, _, _, _ = vc.parse_slab(text, lb, nind)
        pat_rows[7:12] = image
        pat_plane[7:12] = plane
        assert np.array_equal(bed.get_rows(), pat_rows)
        assert np.array_equal(bed.get_order_rows(), pat_plane)


PH_FILE_NIND, PH_NIND, PH_ROWS, PH_LOCI, PH_W = 80, 67, 60, 56, 5


@pytest.fixture(scope="module")
def phase_case():
    rng = np.random.default_rng(77)
    codes, order = vc.random_genotypes(rng, PH_ROWS, PH_FILE_NIND, miss=0.05)
    lines = vc.make_lines(rng, codes, order, styles=("bare", "short"))
    text, lb = vc.slab_of(lines)
    # dropped rows and gaps: rows 0, 20-24 and the last are dropped; loci 10-12 get no row
    keep = [r for r in range(PH_ROWS) if r not in (0, 20, 21, 22, 23, 24, PH_ROWS - 1)]
    loci = [l for l in range(PH_LOCI) if l not in (10, 11, 12)][:len(keep)]
    keep = keep[:len(loci)]
    dest = np.full(PH_ROWS, -1, dtype=np.int64)
    dest[keep] = loci
    return text, lb, codes, order, dest


@pytest.mark.parametrize("ind_offset", [0, 1, 7, 8, 13])
def test_phase_fill_equals_phase_bits(gpu_ctx, phase_case, ind_offset):
    """two panels with the same genotypes: one gets its phase from the image (set_phase_bed), the other the restatement's
    firstCopy through set_phase_bits; their phased LD weights agree bit for bit"""
    text, lb, codes, order, dest = phase_case
    bed, status, err = parse(gpu_ctx, PH_FILE_NIND, text, lb, "host")
    with bed:
        assert err is None
        counts, counted = bed.census()
        want_counts, want_counted = vc.census(codes, order)
        assert np.array_equal(counted, want_counted) and np.array_equal(counts, want_counts)
        fc = vc.first_copy(codes, order, want_counted)[:, ind_offset:ind_offset + PH_NIND]
        assert fc[3].all()                                    # the all-missing row: all ones
        freq = np.full(PH_LOCI, 0.5)
        with np.errstate(invalid="ignore", divide="ignore"):
            f = np.where(counts[:, 1] > 0, counts[:, 0] / np.maximum(counts[:, 1], 1), 0.0)
        freq[dest[dest >= 0]] = f[dest >= 0]
        bits = np.zeros((PH_LOCI, (PH_NIND + 7) // 8), dtype=np.uint8)
        bits[dest[dest >= 0]] = vc.pack_plane(fc[dest >= 0])
        pos = np.arange(PH_LOCI, dtype=np.int32) * 1000 + 5000
        out = []
        for how in ("bed", "bits"):
            with abi.Panel(gpu_ctx, [PH_LOCI], PH_NIND) as panel:
                panel.set_map(pos, [0], [0], gpos=pos * 1e-6)
                panel.set_freq(freq)
                panel.set_genotypes_bed(bed, dest, ind_offset=ind_offset)
                if how == "bed":
                    panel.set_phase_bed(bed, dest, ind_offset=ind_offset)
                else:
                    panel.set_phase_bits(bits)
                out.append(panel.compute_ld(PH_W, phased=True))
        assert ol.bits_equal(out[0], out[1]), ind_offset
        # the phase matters on this case: without it the weights differ
        with abi.Panel(gpu_ctx, [PH_LOCI], PH_NIND) as panel:
            panel.set_map(pos, [0], [0], gpos=pos * 1e-6)
            panel.set_freq(freq)
            panel.set_genotypes_bed(bed, dest, ind_offset=ind_offset)
            panel.set_phase_bits(np.zeros_like(bits))
            assert not ol.bits_equal(panel.compute_ld(PH_W, phased=True), out[0])


def test_phase_fill_needs_a_plane(gpu_ctx):
    codes = np.zeros((4, 9), dtype=np.uint8)
    with abi.Bed(gpu_ctx, 4, 9) as bed, abi.Panel(gpu_ctx, [4], 9) as panel:
        bed.set_rows(vc.pack_image(codes))
        with pytest.raises(abi.GarlicError) as e:
            panel.set_phase_bed(bed, np.arange(4))
        assert e.value.code == abi.ERR_STATE


def offence_text(nind, rows, hits, seed=1):
    """clean lines, with the column text of hits[(row, column)] put in"""
    _, codes, order, lines = case_text(nind, seed=seed, rows=rows)
    for (r, j), col in hits.items():
        parts = lines[r].rstrip(b"\n").split(b"\t")
        parts[9 + j] = col
        lines[r] = b"\t".join(parts) + b"\n"
    return lines


def check_offence(gpu_ctx, nind, lines, want_row, want, where, row_begin=2):
    text, lb = vc.slab_of(lines)
    image, plane, want_status, _, _ = vc.parse_slab(text, lb, nind)
    assert tuple(want_status[want_row]) == want
    bed, status, err = parse(gpu_ctx, nind, text, lb, where, offset=11, nrows=len(lines) + 4, row_begin=row_begin)
    with bed:
        assert np.array_equal(status, want_status), (status, want_status)
        assert err is not None and err.code == abi.ERR_INVALID
        lowest = int(np.flatnonzero(want_status[:, 0])[0])
        assert "row %d " % (row_begin + lowest) in str(err), str(err)
        clean = np.flatnonzero(want_status[:, 0] == 0)
        got_rows = bed.get_rows(row_begin, len(lines))
        got_plane = bed.get_order_rows(row_begin, len(lines))
        assert np.array_equal(got_rows[clean], image[clean]) and np.array_equal(got_plane[clean], plane[clean])
        with pytest.raises(abi.GarlicError) as e:          # rows outside the call and the offending one are not set
            bed.census()
        assert e.value.code == abi.ERR_STATE


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name,col,code", vc.OFFENCES, ids=[o[0] for o in vc.OFFENCES])
def test_each_offence_alone(gpu_ctx, name, col, code, where):
    nind = 9
    check_offence(gpu_ctx, nind, offence_text(nind, 6, {(3, 5): col}), 3, (code, 5), where)


@pytest.mark.parametrize("nind,col", [(9, 8), (9, 0), (300, 299), (300, 150)])
def test_offence_in_the_first_and_last_column(gpu_ctx, nind, col):
    check_offence(gpu_ctx, nind, offence_text(nind, 4, {(1, col): b"./1"}), 1, (vc.HALF_MISSING, col), "device")


@pytest.mark.parametrize("file_nind,nind,want", [(8, 9, (vc.FEW_COLUMNS, 8)), (10, 9, (vc.MANY_COLUMNS, 9)),
                                                 (299, 300, (vc.FEW_COLUMNS, 299)), (301, 300, (vc.MANY_COLUMNS, 300))])
def test_column_count_offences(gpu_ctx, file_nind, nind, want):
    """one line of the call has a sample column too few / too many"""
    lines = offence_text(nind, 5, {})
    _, _, _, other = case_text(file_nind, seed=9, rows=5)
    lines[2] = other[2]
    check_offence(gpu_ctx, nind, lines, 2, want, "device")


def test_a_line_without_sample_columns(gpu_ctx):
    lines = offence_text(9, 3, {})
    lines[1] = b"1\t5\trs\tA\tG\n"
    check_offence(gpu_ctx, 9, lines, 1, (vc.FEW_COLUMNS, 0), "device")


def test_lowest_offending_row_is_named_and_first_column_wins(gpu_ctx):
    nind = 9
    lines = offence_text(nind, 7, {(4, 6): b"0/2", (2, 7): b"1", (2, 3): b"./0"})
    check_offence(gpu_ctx, nind, lines, 2, (vc.HALF_MISSING, 3), "host")


def test_bad_arguments_and_extract_refusal(gpu_ctx):
    nind = 9
    _, codes, order, lines = case_text(nind, rows=4)
    text, lb = vc.slab_of(lines)
    bed, status, err = parse(gpu_ctx, nind, text, lb)
    with bed:
        assert err is None
        with pytest.raises(abi.GarlicError) as e:
            bed.extract(np.arange(4, dtype=np.int32))
        assert e.value.code == abi.ERR_INVALID and "order plane" in str(e.value)
        for bad_lb in (lb[::-1].copy(), np.append(lb[:-1], len(text) + 1), np.append(-1, lb[1:])):
            with pytest.raises(abi.GarlicError) as e:
                bed.set_rows_vcf(text, bad_lb)
            assert e.value.code == abi.ERR_INVALID
        with pytest.raises(abi.GarlicError) as e:
            bed.set_rows_vcf(text, lb, row_begin=1)
        assert e.value.code == abi.ERR_INVALID
        with pytest.raises(abi.GarlicError) as e:
            bed.set_order_rows(np.zeros((4, 1), dtype=np.uint8))      # 9 individuals need 2 bytes
        assert e.value.code == abi.ERR_INVALID
    with abi.Bed(gpu_ctx, 4, nind) as plain:                          # an image without a plane still extracts
        plain.set_rows(vc.pack_image(codes))
        with plain.extract(np.arange(4, dtype=np.int32)) as sub:
            assert sub.nind_total == 4


@pytest.mark.parametrize("rows", [1, 2, 17])
@pytest.mark.parametrize("nind", [9, 257])
def test_row_counts(gpu_ctx, nind, rows):
    """a call of one line is a grid of one workgroup"""
    _, codes, order, lines = case_text(nind, seed=rows, rows=rows)
    text, lb = vc.slab_of(lines)
    bed, status, err = parse(gpu_ctx, nind, text, lb, "device", offset=rows % 16)
    with bed:
        got_codes, got_order = check_clean(bed, status, err, text, lb, nind, (nind, rows))
        assert np.array_equal(got_codes, codes) and np.array_equal(got_order, order)


def padded_line(gt_at=None, total=None, newline=b"\n"):
    """three samples 0|1:777.., 1|0, ./.:88..; gt_at: the offset of the second sample's GT from the line's first byte (the
    first sample's subfield is padded to put it there); total: the length of the line with its newline (the third sample's
    subfield is padded)"""
    head = vc.FIXED % (7, 7) + b"\t0|1:"
    pad = 0 if gt_at is None else gt_at - len(head) - 1
    assert pad >= 0
    line = head + b"7" * pad + b"\t1|0\t./."
    if total is not None:
        fill = total - len(line) - len(newline) - 1
        assert fill >= 0
        line += b":" + b"8" * fill
    return line + newline


@pytest.mark.parametrize("gt_at", list(range(4090, 4101)) + [8189, 8192, 8193])
def test_gt_across_a_pass_boundary(gpu_ctx, gt_at):
    """the line begins at an aligned address, so a pass ends at its byte 4096: the GT `1|0` and the tab in front of it at every
    position around that end (the tab the last byte of the pass: gt_at 4096), and around the end of the second pass"""
    lines = [padded_line(gt_at), padded_line(gt_at)[:-1]]
    text, lb = vc.slab_of(lines, header=b"")
    bed, status, err = parse(gpu_ctx, 3, text, lb, "device", offset=0)
    with bed:
        codes, order = check_clean(bed, status, err, text, lb, 3, gt_at)
        assert codes.tolist() == [[2, 2, 1]] * 2 and order.tolist() == [[0, 1, 0]] * 2


@pytest.mark.parametrize("total", [4095, 4096, 4097, 8192])
@pytest.mark.parametrize("newline", [b"\n", b"\r\n", b""])
def test_line_end_at_a_pass_boundary(gpu_ctx, total, newline):
    """a line that ends exactly where a pass ends (its newline the pass's last byte, its first byte of the next pass, or no
    newline and the slab ends there), alone in its slab and followed by another line"""
    for lines in ([padded_line(total=total, newline=newline)],
                  [padded_line(total=total, newline=newline or b"\n"), padded_line(total=100)]):
        text, lb = vc.slab_of(lines, header=b"")
        bed, status, err = parse(gpu_ctx, 3, text, lb, "device", offset=0)
        with bed:
            codes, _ = check_clean(bed, status, err, text, lb, 3, (total, newline))
            assert codes.tolist() == [[2, 2, 1]] * len(lines)
