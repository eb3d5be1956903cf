"""GPU: TPED text parsed, coded and counted on the device (garlic_bed_set_rows_tped), the census that travels with such an
image (garlic_bed_census, garlic_bed_set_census) and its doors into a panel, against the Python restatement of the
reference's loop in tests/tped_cases.py.  Every comparison is exact.

tped_parse_kernel has no switch point: every line takes the same passes of 256 sixteen-byte pieces (4096 bytes).  What changes
with the shape is covered by shape: every nind % 8, the last allele around the first pass boundary, a line of three passes,
the first allele at every offset of a piece, a device slab at every misalignment, `one` found in the second pass and in the
line's last piece."""
import numpy as np
import pytest

import oracle_lib as ol
import tped_cases as tc
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


def parse(ctx, nind, text, lb, where="host", offset=0, poison=0x41, missing=b"0", bed=None, nrows=None, row_begin=0):
    """-> (bed, row_allele, row_status, error or None)"""
    bed = abi.Bed(ctx, len(lb) - 1 if nrows is None else nrows, nind) if bed is None else bed
    try:
        if where == "host":
            allele, status = bed.set_rows_tped(text, lb, row_begin=row_begin, missing=missing)
        else:
            slab = DeviceSlab(text, offset, poison)
            allele, status = bed.set_rows_tped(slab.ptr, lb, row_begin=row_begin, missing=missing, text_bytes=len(text), where=abi.DEVICE)
        return bed, allele, status, None
    except abi.GarlicError as e:
        if not hasattr(e, "row_status"):
            bed.destroy()
            raise
        return bed, e.row_allele, e.row_status, e


def check_clean(ctx, nind, lines, where="host", offset=0, missing=b"0", keep=None, tag=None, header=b"", poison=0x41):
    text, lb = tc.slab_of(lines, keep, header)
    want = tc.parse_slab(text, lb, nind, missing[0])
    assert not want["status"].any(), (tag, want["status"])
    bed, allele, status, err = parse(ctx, nind, text, lb, where, offset, poison, missing=missing)
    with bed:
        assert err is None and not status.any(), (tag, err, status[status[:, 0] != 0][:3])
        assert np.array_equal(bed.get_rows(), want["image"]), tag
        assert np.array_equal(bed.get_order_rows(), want["plane"]), tag
        assert np.array_equal(allele, want["allele"]), tag
        counts, counted = bed.census()
        assert np.array_equal(counts, want["counts"]) and np.array_equal(counted, want["counted"]), tag
    return want


def lines_of(alleles, lead_width=None, **kw):
    return [tc.make_line(a, lead=tc.lead_of_width(lead_width, r) if lead_width else (b"1", b"rs%d" % r, b"0", b"%d" % (100 * r)), **kw)
            for r, a in enumerate(alleles)]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("nind", tc.NINDS)
def test_rows_plane_allele_and_census(gpu_ctx, nind, where):
    rng = np.random.default_rng(300 + nind)
    alleles = tc.random_alleles(rng, 24, nind)
    alleles[3] = ord("0")                                   # an all-missing line
    check_clean(gpu_ctx, nind, lines_of(alleles), where, offset=nind % 16, tag=(nind, where))


# the last allele of a line with single blanks sits at byte lead_width + 4 * nind - 2 of the line: with these widths and
# counts at bytes 4090 .. 4101, around the first pass boundary (byte 4096 of a line that starts on a piece)
@pytest.mark.parametrize("lead_width", [16, 17, 18, 19])
@pytest.mark.parametrize("nind", [1019, 1020, 1021])
def test_last_allele_around_the_first_pass_boundary(gpu_ctx, nind, lead_width):
    at = lead_width + 4 * nind - 2
    assert tc.PASS_BYTES - 8 < at < tc.PASS_BYTES + 8
    rng = np.random.default_rng(nind + lead_width)
    alleles = tc.random_alleles(rng, 3, nind, third=0.05)
    lines = lines_of(alleles, lead_width)
    assert lines[0][at] == alleles[0][-1] and lines[0][at + 1:] == b"\n"
    check_clean(gpu_ctx, nind, lines[:1], "host", tag=(nind, lead_width))      # the line starts on a piece: the boundary is exact
    check_clean(gpu_ctx, nind, lines, "device", offset=5, tag=(nind, lead_width))


def test_a_line_of_three_passes_and_late_ones(gpu_ctx):
    nind = 2600                                             # 10.4 KB per line
    rng = np.random.default_rng(9)
    alleles = tc.random_alleles(rng, 5, nind, third=0.02)
    alleles[1, :2 * 1500] = ord("0")                        # `one` is found in the second pass
    alleles[1, 2 * 1500] = ord("T")
    alleles[2, :-1] = ord("0")                              # ... in the last piece of the line, from a half-missing genotype
    alleles[2, -1] = ord("C")
    alleles[3, :-2] = ord("0")
    alleles[3, -2:] = [ord("G"), ord("T")]
    lines = lines_of(alleles)
    assert len(lines[0]) > 2 * tc.PASS_BYTES and 16 + 4 * 1500 > tc.PASS_BYTES
    for where in ("host", "device"):
        want = check_clean(gpu_ctx, nind, lines, where, offset=11, tag=where)
    assert list(want["allele"][1:4]) == [ord("T"), ord("C"), ord("G")] and tuple(want["counts"][2]) == (1, 1)


@pytest.mark.parametrize("lead_width", range(16, 32))
def test_first_allele_on_every_offset_of_a_piece(gpu_ctx, lead_width):
    rng = np.random.default_rng(lead_width)
    alleles = tc.random_alleles(rng, 4, 37)
    lines = lines_of(alleles, lead_width)
    assert lines[0][lead_width] == alleles[0][0]
    check_clean(gpu_ctx, 37, lines[:1], "host", tag=lead_width)


@pytest.mark.parametrize("offset", range(1, 16))
def test_every_slab_misalignment_and_two_poisons(gpu_ctx, offset):
    """the device slab between poisoned neighbours (letters, then blanks): the same bytes out whatever the neighbours hold; the
    slab ends with the last line's last allele"""
    rng = np.random.default_rng(40 + offset)
    alleles = tc.random_alleles(rng, 6, 9)
    lines = lines_of(alleles)
    lines[-1] = lines[-1].rstrip(b"\n")
    for poison in (0x41, 0x20):
        check_clean(gpu_ctx, 9, lines, "device", offset, tag=(offset, poison), poison=poison)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("form", ["left_out", "no_last_newline", "crlf", "crlf_no_last_newline", "double_blanks", "mixed_runs", "tabs",
                                  "trailing_run", "leading_run"])
def test_line_selection_ends_and_blanks(gpu_ctx, form, where):
    nind = 13
    rng = np.random.default_rng(61)
    alleles = tc.random_alleles(rng, 9, nind)
    kw = {"crlf": dict(newline=b"\r\n"), "crlf_no_last_newline": dict(newline=b"\r\n"), "double_blanks": dict(sep=b"  "),
          "mixed_runs": dict(sep=lambda k: [b" ", b"  ", b" \t ", b"\t\t"][k % 4]), "tabs": dict(sep=b"\t"),
          "trailing_run": dict(tail=b" \t "), "leading_run": dict(lead_blank=b"  \t")}.get(form, {})
    lines = lines_of(alleles, **kw)
    keep = None
    if form.endswith("no_last_newline"):
        lines[-1] = lines[-1].rstrip(b"\r\n")
    if form == "left_out":
        keep = [0, 1, 4, 5, 8]
    want = check_clean(gpu_ctx, nind, lines, where, offset=7, keep=keep, tag=(form, where), header=b"# not a line\n" if keep else b"")
    ref = [tc.reference_row(alleles[r])[0] for r in (keep or range(9))]
    assert np.array_equal(want["codes"], np.stack(ref))


@pytest.mark.parametrize("missing", [b"0", b"N", b"-"])
def test_missing_characters(gpu_ctx, missing):
    rng = np.random.default_rng(missing[0])
    alleles = tc.random_alleles(rng, 8, 21, letters=b"ACGT0N-".replace(missing, b""), third=0.2, missing=missing[0])
    want = check_clean(gpu_ctx, 21, lines_of(alleles), missing=missing, tag=missing)
    assert (want["codes"] == tc.MISS).any()


def test_half_missing_third_alleles_all_missing_and_high_bytes(gpu_ctx):
    def al(text):
        return np.array([ord(c) for c in text.split()], dtype=np.uint8)
    rows = [al("0 G A A G A A G 0 0 A 0 G G"),              # one = G from a half-missing genotype, then hom of the other allele
            al("G 0 A A G A A G 0 0 A 0 G G"),
            al("0 0 0 A G G A A G A 0 0 0 G"),
            al("C C C G T A A C G T T T C A"),              # four letters
            al("A A A C C A G G A A C C A A"),              # three
            al("0 0 0 0 0 0 0 0 0 0 0 0 0 0")]
    rows.append(np.array([0x80, 0xFF, 0xFF, 0xFF, 0x30, 0x80, 0x80, 0x80, 0xC3, 0xA9, 0xFE, 0x80, 0x80, 0x7F], dtype=np.uint8))
    for where in ("host", "device"):
        want = check_clean(gpu_ctx, 7, lines_of(rows), where, offset=3, tag=where)
    assert tuple(want["counts"][0]) == (5, 10) and want["allele"][0] == ord("G") and want["counted"][5] == 2
    assert want["allele"][6] == 0x80


def offence_lines(nind, begin):
    """begin: the offset of the line in its slab (the slab starts on a piece)"""
    lead_width = 15 if begin % 2 == 0 else 16
    rng = np.random.default_rng(5)
    alleles = tc.random_alleles(rng, 1, nind)[0]
    clean = tc.make_line(alleles, lead=tc.lead_of_width(lead_width))
    at = lambda a: lead_width + 2 * a                       # byte of allele a
    glue = lambda a: clean[:at(a)] + b"TT" + clean[at(a) + 1:]
    piece_a = next(a for a in range(1, 2 * nind) if (begin + at(a) + 1) % 16 == 0)      # its second byte is a piece's first
    return clean, {
        "two_bytes_first": (glue(0), (tc.LONG_ALLELE, 0)),
        "two_bytes_last": (glue(2 * nind - 1), (tc.LONG_ALLELE, nind - 1)),
        "two_bytes_over_a_piece": (glue(piece_a), (tc.LONG_ALLELE, piece_a // 2)),
        "one_token_few": (clean[:-3] + b"\n", (tc.FEW_COLUMNS, nind - 1)),
        "two_tokens_few": (clean[:-5] + b"\n", (tc.FEW_COLUMNS, nind - 1)),
        "two_tokens_many": (clean[:-1] + b" A C\n", (tc.MANY_COLUMNS, nind)),
        "under_four_tokens": (b"1 rs1 0\n", (tc.FEW_COLUMNS, 0)),
        "vertical_tab": (clean[:at(7)] + b"\v" + clean[at(7) + 1:], (tc.BAD_BYTE, 3)),
    }, piece_a


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", ["two_bytes_first", "two_bytes_last", "two_bytes_over_a_piece", "one_token_few", "two_tokens_few",
                                  "two_tokens_many", "under_four_tokens", "vertical_tab"])
def test_offences(gpu_ctx, name, where):
    """the offending line between clean ones: exact {code, individual}, GARLIC_ERR_INVALID, and the other rows of the call
    written, counted as set and equal to the restatement"""
    nind = 30
    rng = np.random.default_rng(8)
    others = lines_of(tc.random_alleles(rng, 4, nind))
    clean, cases, piece_a = offence_lines(nind, len(others[0]) + len(others[1]))
    line, want_status = cases[name]
    lines = others[:2] + [line] + others[2:]
    text, lb = tc.slab_of(lines)
    want = tc.parse_slab(text, lb, nind)
    assert tuple(want["status"][2]) == want_status and not want["status"][[0, 1, 3, 4]].any()
    bed, allele, status, err = parse(gpu_ctx, nind, text, lb, where, offset=0)
    with bed:
        assert err is not None and err.code == abi.ERR_INVALID and "row 2" in str(err), err
        assert np.array_equal(status, want["status"])
        ok = [0, 1, 3, 4]
        assert np.array_equal(bed.get_rows()[ok], want["image"][ok]) and np.array_equal(bed.get_order_rows()[ok], want["plane"][ok])
        assert np.array_equal(allele[ok], want["allele"][ok])
        with pytest.raises(abi.GarlicError) as e:            # the offending row does not count as set
            bed.census()
        assert e.value.code == abi.ERR_STATE and "4 of 5" in str(e.value)
        # the row set again from the clean line completes the image
        t2, lb2 = tc.slab_of([clean])
        bed.set_rows_tped(t2, lb2, row_begin=2)
        lines[2] = clean
        text, lb = tc.slab_of(lines)
        full = tc.parse_slab(text, lb, nind)
        counts, counted = bed.census()
        assert np.array_equal(counts, full["counts"]) and np.array_equal(counted, full["counted"])
        assert np.array_equal(bed.get_rows(), full["image"])


PN_ROWS, PN_LOCI, PN_W = 40, 36, 5


def panel_outputs(ctx, nind, fill, freq):
    pos = np.arange(PN_LOCI, dtype=np.int32) * 1000 + 5000
    with abi.Panel(ctx, [PN_LOCI], nind) as panel:
        panel.set_map(pos, [0], [0], gpos=pos * 1e-6)
        panel.set_freq(freq)
        fill(panel)
        ld = panel.compute_ld(PN_W, phased=True)
        lod = panel.lod_windows(PN_W, 0.001, 200000)
    return ld, lod


def panel_case(file_nind):
    rng = np.random.default_rng(500 + file_nind)
    alleles = tc.random_alleles(rng, PN_ROWS, file_nind, half=0.08, third=0.03)
    alleles[0, :4] = [ord("0"), ord("G"), ord("A"), ord("A")]       # a leading half-missing genotype decides `one`
    alleles[5, :6] = [ord("0"), ord("0"), ord("T"), ord("0"), ord("C"), ord("C")]
    alleles[7] = ord("0")
    keep = [r for r in range(PN_ROWS) if r not in (3, 20, 21, PN_ROWS - 1)]
    loci = [l for l in range(PN_LOCI) if l not in (10, 11)][:len(keep)]
    keep = keep[:len(loci)]
    dest = np.full(PN_ROWS, -1, dtype=np.int64)
    dest[keep] = loci
    return alleles, dest


@pytest.mark.parametrize("file_nind,nind,ind_offset", [(9, 9, 0), (9, 5, 3), (65, 65, 0), (65, 33, 0), (65, 32, 33), (65, 13, 7)])
def test_panel_from_a_tped_image_equals_the_host_readers_arrays(gpu_ctx, file_nind, nind, ind_offset):
    """set_genotypes_bed + set_phase_bed from the image against set_genotypes + set_phase of the arrays the host reader holds
    (int16 copies of `one`, the reference's own firstCopy): the unweighted scores and the phased LD weights, bit for bit.  Then
    the second-device door: rows + plane + census into a fresh image gives the same; without set_census it does not."""
    alleles, dest = panel_case(file_nind)
    text, lb = tc.slab_of(lines_of(alleles))
    data, fc, f = tc.host_arrays(alleles)
    live = dest >= 0
    geno = np.full((PN_LOCI, nind), -9, dtype=np.int16)
    geno[dest[live]] = data[live, ind_offset:ind_offset + nind]
    first = np.zeros((PN_LOCI, nind), dtype=np.uint8)
    first[dest[live]] = fc[live, ind_offset:ind_offset + nind]
    freq = np.full(PN_LOCI, 0.5)
    freq[dest[live]] = f[live]
    bed, _, _, err = parse(gpu_ctx, file_nind, text, lb)
    with bed:
        assert err is None

        def from_host(panel):
            panel.set_genotypes(geno)
            panel.set_phase(first)

        def from_image(image):
            def fill(panel):
                panel.set_genotypes(np.full((PN_LOCI, nind), -9, dtype=np.int16))      # loci no row maps to
                panel.set_genotypes_bed(image, dest, ind_offset=ind_offset)
                panel.set_phase(np.zeros((PN_LOCI, nind), dtype=np.uint8))
                panel.set_phase_bed(image, dest, ind_offset=ind_offset)
            return fill
        want_ld, want_lod = panel_outputs(gpu_ctx, nind, from_host, freq)
        got_ld, got_lod = panel_outputs(gpu_ctx, nind, from_image(bed), freq)
        assert ol.bits_equal(got_ld, want_ld) and ol.bits_equal(np.ascontiguousarray(got_lod[0]), np.ascontiguousarray(want_lod[0]))
        rows, plane = bed.get_rows(), bed.get_order_rows()
        counts, counted = bed.census()
        with abi.Bed(gpu_ctx, PN_ROWS, file_nind) as second:
            second.set_rows(rows)
            second.set_order_rows(plane)
            second.set_census(counts, counted)
            c2, k2 = second.census()
            assert np.array_equal(c2, counts) and np.array_equal(k2, counted)
            ld2, lod2 = panel_outputs(gpu_ctx, nind, from_image(second), freq)
            assert ol.bits_equal(ld2, want_ld) and ol.bits_equal(np.ascontiguousarray(lod2[0]), np.ascontiguousarray(want_lod[0]))
            # setting rows again discards the supplied census: the image rule counts row 0 differently
            second.set_rows(rows)
            c3, k3 = second.census()
            assert k3[0] == 1 and counted[0] == 0 and not np.array_equal(c3, counts)
        if ind_offset == 0:
            with abi.Bed(gpu_ctx, PN_ROWS, file_nind) as bare:
                bare.set_rows(rows)
                bare.set_order_rows(plane)
                ld3, lod3 = panel_outputs(gpu_ctx, nind, from_image(bare), freq)
                assert not ol.bits_equal(np.ascontiguousarray(lod3[0]), np.ascontiguousarray(want_lod[0]))      # the door is needed


def test_state_errors(gpu_ctx):
    rng = np.random.default_rng(2)
    alleles = tc.random_alleles(rng, 4, 9)
    text, lb = tc.slab_of(lines_of(alleles))
    want = tc.parse_slab(text, lb, 9)

    def code_of(call):
        with pytest.raises(abi.GarlicError) as e:
            call()
        return e.value.code
    with abi.Bed(gpu_ctx, 4, 9) as bed:                      # a TPED image takes no rows of the other kind
        bed.set_rows_tped(text, lb[:3])
        assert code_of(lambda: bed.set_rows(want["image"])) == abi.ERR_STATE
        assert code_of(lambda: bed.set_order_rows(want["plane"])) == abi.ERR_STATE
        assert code_of(lambda: bed.set_rows_vcf(b"1\t2\n", [0, 4])) == abi.ERR_STATE
        assert code_of(bed.census) == abi.ERR_STATE                                  # rows 2 and 3 are not set
        assert code_of(lambda: bed.set_census(want["counts"], want["counted"])) == abi.ERR_STATE
        assert code_of(lambda: bed.extract([0, 1])) in (abi.ERR_INVALID, abi.ERR_STATE)
        for blank in (b" ", b"\t", b"\r", b"\n"):
            assert code_of(lambda: bed.set_rows_tped(text, lb, missing=blank)) == abi.ERR_INVALID
        bed.set_rows_tped(text, lb[2:], row_begin=2)
        counts, counted = bed.census()
        assert np.array_equal(counts, want["counts"]) and np.array_equal(counted, want["counted"])
        assert code_of(lambda: bed.extract([0, 1])) == abi.ERR_INVALID               # as on every image with an order plane
    for first in ("rows", "order", "vcf"):                   # and an image of the other kind takes no TPED rows
        with abi.Bed(gpu_ctx, 4, 9) as bed:
            if first == "rows":
                bed.set_rows(want["image"][:1])
            elif first == "order":
                bed.set_order_rows(want["plane"][:1])
            else:
                vcf_line = b"1\t1\tr\tA\tG\t.\t.\t.\tGT" + b"\t0|1" * 9 + b"\n"
                bed.set_rows_vcf(vcf_line, [0, len(vcf_line)])
            assert code_of(lambda: bed.set_rows_tped(text, lb)) == abi.ERR_STATE
    with abi.Bed(gpu_ctx, 4, 9) as bed:
        bed.set_rows(want["image"])
        bad = want["counts"].copy()
        bad[1] = (5, 4)
        assert code_of(lambda: bed.set_census(bad, want["counted"])) == abi.ERR_INVALID
        bad[1] = (-1, 4)
        assert code_of(lambda: bed.set_census(bad, want["counted"])) == abi.ERR_INVALID
        k = want["counted"].copy()
        k[2] = 3
        assert code_of(lambda: bed.set_census(want["counts"], k)) == abi.ERR_INVALID
        bed.set_census(want["counts"], want["counted"])
        counts, counted = bed.census()
        assert np.array_equal(counts, want["counts"]) and np.array_equal(counted, want["counted"])
