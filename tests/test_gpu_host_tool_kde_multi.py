"""GPU: garlic-lod --kde over several window sizes -- the sweeps now ask the library for the KDEs of a batch of sizes in one
call (LodEngine::lodKdeMulti, garlic_lod_kde_multi) -- against the per-size loop it replaces, which GARLIC_KDE_MULTI_OFF=1
keeps: every file byte for byte, the selection lines on stderr word for word, with --error and with --tgls, on the
synthetic panel of tests/test_gpu_host_tool_kde.py.  Sizes computed ahead of need that the library refuses (a window wider
than the chromosome) fail the run only when the loop reaches them, and then in the per-size call's words."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_host_tool_kde import BOUNDS, NIND, NSNP, SEED, TOOL, data  # noqa: F401  (data: the module's fixture)

pytestmark = pytest.mark.gpu
TOO_WIDE = NSNP + 1000
START = 20


@pytest.fixture(scope="module")
def tgls(data):  # noqa: F811
    """genotype qualities for the panel: 10 to 40, a handful of distinct values"""
    rng = np.random.default_rng(9971)
    path = str(data / "syn.tgls")
    with open(path, "w") as f:
        for l in range(NSNP):
            f.write("1 rs%d 0 %d %s\n" % (l, 10000 + 1000 * l, " ".join(str(int(v)) for v in rng.choice([10, 20, 30, 40], size=NIND))))
    return ["--tgls", path, "--gl-type", "GQ"]


def run_tool(data, d, extra, multi):  # noqa: F811
    os.makedirs(d, exist_ok=True)
    out = os.path.join(str(d), "mine")
    cmd = [TOOL, "--tped", str(data / "syn.tped"), "--tfam", str(data / "syn.tfam"), "--centromere", str(data / "syn.centromeres.txt"),
           "--out", out, "--error", "0.001", "--kde-seed", SEED, "--kde"]
    env = dict(os.environ)
    env.pop("GARLIC_KDE_MULTI_OFF", None)
    if not multi:
        env["GARLIC_KDE_MULTI_OFF"] = "1"
    r = subprocess.run(cmd + list(extra), capture_output=True, text=True, env=env)
    files = {n: open(os.path.join(str(d), n), "rb").read() for n in sorted(os.listdir(d))}
    files = {n: gzip.decompress(b) if n.endswith(".gz") else b for n, b in files.items()}       # (a gzip header may carry a time)
    return r.returncode, files, r.stderr.replace(str(d), "OUT")       # (the messages name the files written)


def told(stderr):
    """what the run says of its choices and results: everything but the lines that name the library calls made"""
    keep = [l for l in stderr.splitlines() if not l.startswith("Calculating LOD scores with winsize")]
    assert len(keep) < len(stderr.splitlines()), "the run computed something"
    return keep


def both(data, tmp_path, name, extra, ok=True):  # noqa: F811
    """the run as built and with the per-size loop: the same exit code, files and words; -> (files, stderr of the built run)"""
    rc1, files1, err1 = run_tool(data, tmp_path / (name + "_multi"), extra, True)
    rc0, files0, err0 = run_tool(data, tmp_path / (name + "_loop"), extra, False)
    print(name, "\n".join(told(err1)))
    assert (rc1 == 0) == ok and (rc0 == 0) == ok, (name, err1[-1500:], err0[-1500:])
    assert sorted(files1) == sorted(files0), (name, sorted(files1), sorted(files0))
    for n in files1:
        assert files1[n] == files0[n], (name, n)
    assert told(err1) == told(err0), name
    # the built run asked for several sizes at once, the other one never
    assert ("KDE of all sizes on the device in one call" in err1) and ("in one call" not in err0), name
    return files1, err1


def rows_of(err):
    return [(int(a), float(b)) for a, b in re.findall(r"^(\d+)\t(\S+)$", err, re.M)]


@pytest.mark.parametrize("kind", ["error", "tgls"])
def test_winsize_multi_list(data, tgls, tmp_path, kind):  # noqa: F811
    extra = tgls if kind == "tgls" else []
    files, err = both(data, tmp_path, "list", ["--winsize-multi", "30", "60", "90", *BOUNDS, *extra])
    assert [n for n in files if n.endswith(".kde")] == ["mine.30SNPs.kde", "mine.60SNPs.kde", "mine.90SNPs.kde"]
    assert len(re.findall(r"^Selected LOD score cutoff: ", err, re.M)) == 3
    assert any(n.endswith(".roh.bed") for n in files)
    # a size wider than the chromosome at the end of the list: the sizes before it are finished, then the per-size refusal
    files, err = both(data, tmp_path, "list_wide", ["--winsize-multi", "60", str(TOO_WIDE), *extra], ok=False)
    assert "mine.60SNPs.kde" in files and not any(str(TOO_WIDE) in n for n in files)
    assert "ERROR: garlic_lod_kde: feed KDE: needs at least 2 values (the feed holds 0)" in err


@pytest.mark.parametrize("kind", ["error", "tgls"])
def test_auto_winsize_stepping_and_from_a_list(data, tgls, tmp_path, kind):  # noqa: F811
    extra = tgls if kind == "tgls" else []
    # selectWinsize: batches of four sizes ahead of the loop
    files, err = both(data, tmp_path, "step", ["--winsize", str(START), "--auto-winsize", "--auto-winsize-step", "8", *extra])
    rows = rows_of(err)
    assert [w for w, _ in rows] == [START + 8 * i for i in range(len(rows))] and len(rows) > 1, rows
    chosen = rows[-1][0]
    assert rows[-1][1] <= 0.50 and all(m > 0.50 for _, m in rows[:-1])
    assert [n for n in files if n.endswith(".kde")] == ["mine.%dSNPs.kde" % chosen]
    assert "Selected window size: %d" % chosen in err
    # selectWinsizeFromList: the whole list in one call; the size past the chosen one is never reached, so its refusal is
    # not the run's
    files, err = both(data, tmp_path, "list", ["--winsize-multi", str(START), str(chosen), str(TOO_WIDE), "--auto-winsize", *extra])
    assert [w for w, _ in rows_of(err)] == [START, chosen] and "Selected window size: %d" % chosen in err
    assert [n for n in files if n.endswith(".kde")] == ["mine.%dSNPs.kde" % chosen]
    assert "at least 2 values" not in err
    # ... and is when the loop gets there
    files, err = both(data, tmp_path, "list_wide", ["--winsize-multi", str(START), str(TOO_WIDE), "--auto-winsize", *extra], ok=False)
    assert [w for w, _ in rows_of(err)] == [START] and not any(n.endswith(".kde") for n in files)
    assert "ERROR: garlic_lod_kde: feed KDE: needs at least 2 values (the feed holds 0)" in err
