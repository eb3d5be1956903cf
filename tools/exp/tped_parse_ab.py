#!/usr/bin/env python3
"""TPED parse on the device, two figures on one GPU (profiles/tped_parse_ab.txt):

 (a) garlic_bed_set_rows_tped on text that is resident on the device (where = GARLIC_DEVICE), timed with events on the
     context's stream: the line_begin upload, tped_parse_kernel and the status / allele read-back, as GB/s of text and as a
     fraction of the 8 TB/s HBM peak;
 (b) the load phase of garlic-lod --tped (wall time from the start of the process to its "Loaded N loci x M individuals" line)
     through the device reader (GARLIC_TPED_DEVICE_READER=1) against GARLIC_TPED_HOST_READER=1 in the same build.

Shape: --lines x --nind (default 20,000 x 10,000: about 800 MB of uncompressed text), two letters per line at a random
frequency, 2 % missing genotypes, single blanks.

    python tools/exp/tped_parse_ab.py [--lines N] [--nind M] [--reps K] [--dir D] [--skip-tool]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
LEAD = 16


def device_text(lines, nind, seed=1):
    """uint8 tensor [lines][LEAD + 4 * nind] on the device: `1 rsNNNNNNN 0 P ` and the alleles, a blank behind each but the
    last, which a newline follows"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    width = LEAD + 4 * nind
    text = torch.full((lines, width), 0x20, dtype=torch.uint8, device="cuda")
    lead = np.full((lines, LEAD), 0x20, dtype=np.uint8)
    for r in range(lines):
        s = b"1 rs%07d 0 %d" % (r, r % 10)
        lead[r, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    text[:, :LEAD] = torch.from_numpy(lead).cuda()
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    a = letters[torch.randint(0, 4, (lines, 1), generator=g, device="cuda")]
    b = letters[(torch.randint(1, 4, (lines, 1), generator=g, device="cuda") + torch.searchsorted(letters, a.contiguous())) % 4]
    p = torch.rand((lines, 1), generator=g, device="cuda") * 0.8 + 0.1
    al = torch.where(torch.rand((lines, 2 * nind), generator=g, device="cuda") < p, a, b)
    miss = (torch.rand((lines, nind), generator=g, device="cuda") < 0.02).repeat_interleave(2, dim=1)
    al = torch.where(miss, torch.full_like(al, 0x30), al)
    text[:, LEAD::2] = al
    text[:, -1] = 0x0A
    return text


def kernel_figure(args, out):
    import torch
    from garlic_amd import abi
    text = device_text(args.lines, args.nind)
    width = text.shape[1]
    nbytes = text.numel()
    lb = np.arange(args.lines + 1, dtype=np.int64) * width
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ms = []
    with abi.Context(0, stream=stream.cuda_stream) as ctx, abi.Bed(ctx, args.lines, args.nind) as bed:
        for rep in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            allele, status = bed.set_rows_tped(text.data_ptr(), lb, text_bytes=nbytes, where=abi.DEVICE)
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
            assert not status.any()
        counts, counted = bed.census()
    assert (counted == 0).all() and (counts[:, 1] <= 2 * args.nind).all() and (counts[:, 1] > 1.9 * args.nind).all()
    best = min(ms[1:])
    out.append("(a) garlic_bed_set_rows_tped, text resident on the device: %d lines x %d individuals, %.1f MB" % (args.lines, args.nind, nbytes / 1e6))
    out.append("    events on the context's stream around the call (line_begin upload, tped_parse_kernel, status and allele read-back):")
    out.append("    first %.2f ms (allocates the plane and the scratch), then %s ms; best %.3f ms" % (ms[0], ", ".join("%.2f" % m for m in ms[1:]), best))
    out.append("    = %.0f GB/s of text = %.1f %% of the 8 TB/s HBM peak" % (nbytes / best / 1e6, 100 * nbytes / (best * 1e-3) / HBM_PEAK))
    return text


def load_seconds(cmd, env):
    t0 = time.perf_counter()
    p = subprocess.Popen(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, env=env)
    took, note = None, False
    for line in p.stderr:
        note = note or line.startswith("TPED device reader")
        if line.startswith("Loaded ") and " loci x " in line:
            took = time.perf_counter() - t0
            break
    p.kill()
    p.wait()
    return took, note


def tool_figure(args, text, out):
    os.makedirs(args.dir, exist_ok=True)
    path = os.path.join(args.dir, "ab.tped")
    text.cpu().numpy().tofile(path)
    with open(os.path.join(args.dir, "ab.tfam"), "w") as f:
        f.write("".join("POP ind%d 0 0 0 -9\n" % i for i in range(args.nind)))
    e2e = os.path.join(ROOT, "tests", "golden", "e2e")
    cmd = [os.path.join(ROOT, "garlic_amd", "host", "garlic-lod"), "--tped", path, "--tfam", os.path.join(args.dir, "ab.tfam"), "--out",
           os.path.join(args.dir, "ab"), "--centromere", os.path.join(e2e, "tiny.centromeres.txt"), "--winsize", "30", "--raw-lod", "--error", "0.001"]
    out.append("(b) load phase of garlic-lod --tped (process start to the \"Loaded ... loci x ... individuals\" line), %.1f MB file, page cache warm:"
               % (os.path.getsize(path) / 1e6))
    for name, var in (("device reader", None), ("GARLIC_TPED_HOST_READER=1", "1")) * args.tool_reps:
        env = dict(os.environ)
        env.pop("GARLIC_TPED_HOST_READER", None)
        env["GARLIC_TPED_DEVICE_READER"] = "1"
        if var:
            env["GARLIC_TPED_HOST_READER"] = var
        took, note = load_seconds(cmd, env)
        out.append("    %-26s %s%s" % (name, "%.2f s" % took if took is not None else "did not load", "  (fell back to the host reader)" if note else ""))
    os.remove(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=20000)
    ap.add_argument("--nind", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tool-reps", type=int, default=2)
    ap.add_argument("--dir", default="/tmp/tped_parse_ab")
    ap.add_argument("--skip-tool", action="store_true")
    args = ap.parse_args()
    out = ["TPED parse on the device (garlic_bed_set_rows_tped, tped_parse_kernel), one MI355X", ""]
    text = kernel_figure(args, out)
    if not args.skip_tool:
        out.append("")
        tool_figure(args, text, out)
    print("\n".join(out))


if __name__ == "__main__":
    main()
