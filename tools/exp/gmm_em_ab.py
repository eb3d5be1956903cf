#!/usr/bin/env python3
"""The EM loop of garlic_gmm_fit against a single-thread host restatement (tools/exp/gmm_host_time.cpp, built here with
g++ -O3): N = 4,000,000 lengths of tests/gmm_cases.py's three-class generator, K = 3, 100 fixed iterations.  Device:
garlic_gmm_fit_info's em_ms (HIP events around the loop), five repeats after a warm-up.  Writes the figures to stdout in
the form profiles/gmm_em_ab.txt keeps.  usage: python tools/exp/gmm_em_ab.py [N] [K] [iterations]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gmm_cases as cases  # noqa: E402
from garlic_amd import abi  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4000000
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 100
    x = np.array(cases.content("three", n))
    tmp = tempfile.mkdtemp()
    x.tofile(os.path.join(tmp, "lengths.f64"))
    exe = os.path.join(tmp, "gmm_host_time")
    subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "exp", "gmm_host_time.cpp")])
    # the host's initial guess is size_classes.hpp's; hand the device the same recurrences' result through the fsum form
    a0, m0, v0 = cases.init(x, k)
    with abi.Context(0) as ctx:
        ctx.gmm_fit(x, a0, m0, v0, max_iter=iters, precision=-1.0)
        times = []
        for _ in range(5):
            got = ctx.gmm_fit(x, a0, m0, v0, max_iter=iters, precision=-1.0)
            times.append(ctx.gmm_fit_info()["em_ms"])
        info = ctx.gmm_fit_info()
    print("device n=%d K=%d iterations=%d blocks=%d em_ms median=%.3f min=%.3f max=%.3f ms_per_iteration=%.4f loglik=%.17g" % (
        n, k, got["iterations"], info["blocks"], float(np.median(times)), min(times), max(times), float(np.median(times)) / iters, got["loglik"]))
    sys.stdout.flush()
    host = subprocess.run([exe, os.path.join(tmp, "lengths.f64"), str(k), str(iters)], capture_output=True, text=True, check=True).stdout.strip()
    print(host)
    host_ms = float(host.split("ms=")[1].split()[0])
    print("ratio host / device = %.1f" % (host_ms / float(np.median(times))))


if __name__ == "__main__":
    main()
