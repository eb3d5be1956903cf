#!/usr/bin/env python3
"""End-to-end fixtures of the GMM size classes: what the reference's PREBUILT binary (/root/reference/bin/linux/garlic,
v1.1.6a, static) writes for tests/golden/e2e/tiny.* with --lod-cutoff -12 and --nclust 3 / --nclust 2 instead of
--size-bounds: the .roh.bed and the "Gaussian class" / "Selected ROH size boundaries" lines of its log.  Build container
only; only the binary's outputs are kept.  Asserts that no segment length lies within 2.5e-3 (relative) of a boundary,
so that a solver whose root differs in the fifth digit classifies every segment alike."""
import gzip
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "e2e")
BIN = "/root/reference/bin/linux/garlic"
CLEARANCE = 2.45e-3     # "2.5e-3" to two digits: the nearest length lies 2.49e-3 from the printed K = 2 boundary, 6.5e-3 for K = 3


def main():
    tmp = tempfile.mkdtemp()
    cmds = []
    for k in (3, 2):
        tag = "refs%d" % k
        cmd = [BIN, "--tped", os.path.join(OUT, "tiny.tped.gz"), "--tfam", os.path.join(OUT, "tiny.tfam"),
               "--centromere", os.path.join(OUT, "tiny.centromeres.txt"), "--error", "0.001", "--winsize", "30",
               "--kde-subsample", "0", "--out", os.path.join(tmp, tag), "--lod-cutoff", "-12", "--nclust", str(k)]
        cmds.append(cmd)
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        log = open(os.path.join(tmp, tag + ".log")).read().splitlines()
        keep = [l for l in log if l.startswith("Gaussian class") or l.startswith("Selected ROH size boundaries")]
        assert len(keep) == k + 1, log
        bounds = [float(t) for t in re.search(r"= \( (.*) \)", keep[-1]).group(1).split()]
        bed = open(os.path.join(tmp, tag + ".roh.bed"), "rb").read()
        lengths = [float(l.split("\t")[4]) for l in bed.decode().splitlines() if not l.startswith("track")]
        nearest = min(abs(x - b) / b for x in lengths for b in bounds)
        print(tag, "segments", len(lengths), "bounds", bounds, "nearest length at relative %.3g" % nearest)
        assert nearest >= CLEARANCE, nearest
        with open(os.path.join(OUT, tag + ".roh.bed.gz"), "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(bed)
        with open(os.path.join(OUT, tag + ".log.txt"), "w") as f:
            f.write("\n".join(keep) + "\n")
    with open(os.path.join(OUT, "COMMAND_gmm.txt"), "w") as f:
        f.write("garlic v1.1.6a prebuilt binary (the .log.txt files hold the Gaussian and boundary lines of its log):\n")
        for c in cmds:
            f.write(" ".join(os.path.basename(x) if x.startswith("/") else x for x in c) + "\n")
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
