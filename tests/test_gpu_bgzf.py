"""GPU: BGZF blocks inflated on the device (garlic_bgzf_inflate), bytes and statuses against Python's zlib.

bgzf_inflate_kernel takes one wave per block and four blocks per workgroup; the cases of tests/bgzf_cases.py cover every
block type and tree shape, the longest and the oldest match, members at both size limits and every status.  The sanitizer
run of the same decoder body on the host (tests/test_bgzf_cpu.py) is what shows that it stays inside its ranges."""
import zlib

import numpy as np
import pytest

import bgzf_cases as bc
from garlic_amd import abi

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5


def inflate(ctx, members, where):
    """-> (status, err, the bytes of every output range, the guard bytes in front and behind)"""
    import torch
    comp = b"".join(members)
    bb = np.cumsum([0] + [len(m) for m in members])
    ob = np.cumsum([0] + [bc.isize_of(m) for m in members])
    out = torch.full((int(ob[-1]) + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if where == "host":
        status, err = abi.bgzf_inflate(ctx, comp, bb, out.data_ptr() + GUARD, ob)
    else:
        dev = torch.frombuffer(bytearray(comp), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        status, err = abi.bgzf_inflate(ctx, dev.data_ptr(), bb, out.data_ptr() + GUARD, ob, comp_bytes=len(comp), where=abi.DEVICE)
    host = out.cpu().numpy()
    ranges = [host[GUARD + ob[k]:GUARD + ob[k + 1]].tobytes() for k in range(len(members))]
    return status, err, ranges, (host[:GUARD], host[GUARD + ob[-1]:])


def guards_intact(guards):
    return all((g == FILL).all() for g in guards)


@pytest.mark.parametrize("where", ["host", "device"])
def test_every_clean_case(gpu_ctx, where):
    cases = bc.clean_cases()
    status, err, ranges, guards = inflate(gpu_ctx, [m for _, m in cases], where)
    assert err is None and not status.any(), (err, [(cases[k][0], int(status[k])) for k in np.flatnonzero(status)])
    for (name, m), got in zip(cases, ranges):
        assert got == zlib.decompress(m, 31), name
    assert guards_intact(guards)


@pytest.mark.parametrize("where", ["host", "device"])
def test_every_corrupt_case_between_clean_neighbours(gpu_ctx, where):
    text_member = bc.member(bc.text(), 6)
    members, want = [text_member], [bc.OK]
    for _, m, status in bc.corrupt_cases():
        members += [m, text_member]
        want += [status, bc.OK]
    status, err, ranges, guards = inflate(gpu_ctx, members, where)
    assert status.tolist() == want
    assert err is not None and err.code == abi.ERR_INVALID and "block 1 " in str(err), err
    assert all(r == bc.text() for r in ranges[::2]) and guards_intact(guards)


def test_300_mixed_members_in_one_call(gpu_ctx):
    clean, corrupt = [m for _, m in bc.clean_cases()], bc.corrupt_cases()
    members, want = [], []
    for k in range(300):
        if k % 7 == 3:
            _, m, status = corrupt[(k // 7) % len(corrupt)]
        else:
            m, status = clean[k % len(clean)], bc.OK
        members.append(m)
        want.append(status)
    status, err, ranges, guards = inflate(gpu_ctx, members, "host")
    assert status.tolist() == want and err is not None
    for k, m in enumerate(members):          # what stands in front of and behind every bad block's range is its neighbours' bytes
        if want[k] == bc.OK:
            assert ranges[k] == zlib.decompress(m, 31), k
    assert guards_intact(guards)


def test_2000_random_members_in_one_call(gpu_ctx):
    pairs = bc.random_members()
    status, err, ranges, guards = inflate(gpu_ctx, [m for m, _ in pairs], "host")
    assert err is None and not status.any(), (err, np.flatnonzero(status)[:5])
    bad = [k for k, (_, data) in enumerate(pairs) if ranges[k] != data]
    assert not bad and guards_intact(guards), bad[:5]


def test_lists_are_checked_before_the_launch(gpu_ctx):
    import torch
    m = bc.member(b"ACGT\n", 6)
    out = torch.zeros(1 << 17, dtype=torch.uint8, device="cuda")
    for bb, ob in [([0, len(m) + 1], [0, 5]), ([0, 20], [0, 5]), ([0, len(m)], [0, 70000]), ([0, len(m)], [5, 0])]:
        with pytest.raises(abi.GarlicError) as e:
            abi.bgzf_inflate(gpu_ctx, m, bb, out.data_ptr(), ob)
        assert e.value.code == abi.ERR_INVALID
    status, err = abi.bgzf_inflate(gpu_ctx, m, [0], out.data_ptr(), [0])
    assert err is None and status.shape == (0,)


def test_device_download_is_the_twin_of_upload(gpu_ctx):
    import torch
    data = np.arange(1000, dtype=np.uint8)
    buf = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    abi.device_upload(gpu_ctx, buf.data_ptr(), data)
    assert np.array_equal(abi.device_download(gpu_ctx, buf.data_ptr() + 3, 900), data[3:903])
    assert np.array_equal(buf.cpu().numpy(), data)
