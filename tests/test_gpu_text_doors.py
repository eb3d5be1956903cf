"""GPU: the four text doors (garlic_bed_set_rows_vcf, garlic_bed_set_rows_tped, garlic_tgls_set_rows_text,
garlic_tgls_set_rows_vcf) on the same bad arguments.  Every case is refused with GARLIC_ERR_INVALID before anything is
launched, and garlic_hip_last_error() is the text each door has always answered with: the bed doors and the tgls doors word
the row range differently, everything else is one text.  Objects are 2 rows x 3 samples; a good call closes every case, so a
refusal leaves the object usable."""
import ctypes as C

import numpy as np
import pytest

from garlic_amd import abi

pytestmark = pytest.mark.gpu

ROWS, NIND = 2, 3
TEXTS = {
    "bed_vcf": b"1\t10\ta\tA\tC\t.\t.\t.\tGT\t0/0\t0|1\t1/1\n1\t20\tb\tA\tC\t.\t.\t.\tGT\t./.\t1|0\t0/0\n",
    "bed_tped": b"1 a 0 10 A A A C C C\n1 b 0 20 0 0 C A A A\n",
    "tgls_text": b"1 a 0 10 0.5 1 2\n1 b 0 20 3 4.25 5\n",
    "tgls_vcf": b"1\t10\ta\tA\tC\t.\t.\t.\tGT:GQ\t0/0:1\t0|1:2\t1/1:3\n1\t20\tb\tA\tC\t.\t.\t.\tGT:GQ\t./.:4\t1|0:5\t0/0:6\n",
}
DOORS = sorted(TEXTS)
ROW_RANGE = {"bed": "row range [%d,+%d) outside image of %d rows", "tgls": "row range [%d,+%d) outside the object's %d rows"}
OFFSETS = "line_begin[%d] = %d: the offsets must ascend inside the slab of %d bytes"


def line_offsets(text):
    first = text.index(b"\n") + 1
    return [0, first, len(text)]


def call(door, obj, text, text_bytes, lb, row_begin, row_count, where):
    """the door's C entry itself: (return code, garlic_hip_last_error())"""
    L = abi.lib()
    buf = np.frombuffer(text, dtype=np.uint8)
    lb = np.ascontiguousarray(lb, dtype=np.int64)
    status = np.zeros((max(row_count, 1), 2), dtype=np.int32)
    head = (obj.handle, C.c_void_p(buf.ctypes.data), text_bytes, lb.ctypes.data_as(C.POINTER(C.c_int64)), row_begin, row_count)
    st = C.c_void_p(status.ctypes.data)
    if door == "bed_vcf":
        rc = L.garlic_bed_set_rows_vcf(*head, st, where)
    elif door == "bed_tped":
        rc = L.garlic_bed_set_rows_tped(*head, ord("0"), None, st, where)
    elif door == "tgls_text":
        rc = L.garlic_tgls_set_rows_text(*head, st, where)
    else:
        rc = L.garlic_tgls_set_rows_vcf(*head, b"GQ", None, st, where)
    return rc, L.garlic_hip_last_error().decode()


CASES = ["where", "empty", "rows past the end", "rows in front", "no rows", "descending", "behind the slab", "negative"]


def bad_call(door, text, case):
    """(the arguments behind the object, the text of the refusal)"""
    n, lb = len(text), line_offsets(text)
    rows = ROW_RANGE[door.split("_")[0]]
    return {
        "where": ((text, n, lb, 0, ROWS, 2), "where must be GARLIC_HOST or GARLIC_DEVICE"),
        "empty": ((text, 0, [0, 0, 0], 0, ROWS, abi.HOST), "text_bytes 0: the slab is empty"),
        "rows past the end": ((text, n, lb, 1, ROWS, abi.HOST), rows % (1, ROWS, ROWS)),
        "rows in front": ((text, n, lb, -1, ROWS, abi.HOST), rows % (-1, ROWS, ROWS)),
        "no rows": ((text, n, lb, 0, 0, abi.HOST), rows % (0, 0, ROWS)),
        "descending": ((text, n, [lb[1], 0, n], 0, ROWS, abi.HOST), OFFSETS % (1, 0, n)),
        "behind the slab": ((text, n, [0, lb[1], n + 1], 0, ROWS, abi.HOST), OFFSETS % (2, n + 1, n)),
        "negative": ((text, n, [-1, lb[1], n], 0, ROWS, abi.HOST), OFFSETS % (0, -1, n)),
    }[case]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("door", DOORS)
def test_bad_arguments_are_refused_with_the_doors_own_text(gpu_ctx, door, case):
    text = TEXTS[door]
    with (abi.Bed(gpu_ctx, ROWS, NIND) if door.startswith("bed") else abi.Tgls(gpu_ctx, ROWS, NIND)) as obj:
        args, want = bad_call(door, text, case)
        assert call(door, obj, *args) == (abi.ERR_INVALID, want)
        rc, msg = call(door, obj, text, len(text), line_offsets(text), 0, ROWS, abi.HOST)
        assert rc == abi.OK, msg
