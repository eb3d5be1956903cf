"""GPU: garlic-lod --kde --kde-sharded over several window sizes -- two shards on the one device (--devices 0,0) leave the
sorted feeds of all sizes on the device as one garlic_kde_part_set each, and garlic_kde_parts_multi reduces them
(LodEngine::lodKdeMulti) -- against the per-size loop of garlic_lod_kde_part + garlic_kde_parts, which
GARLIC_KDE_MULTI_OFF=1 keeps: every file byte for byte, the selection lines word for word, one "KDE on 2 shards" per
size used, on the synthetic panel of tests/test_gpu_host_tool_kde.py."""
import re

import pytest

from test_gpu_host_tool_kde import BOUNDS, data  # noqa: F401  (data: the module's fixture)
from test_gpu_host_tool_kde_multi import rows_of, run_tool

pytestmark = pytest.mark.gpu
SHARDED = ["--kde-sharded", "--devices", "0,0"]
ONE_CALL = "KDE of all sizes on the shards in one call"


def told(stderr):
    """what the run says of its choices and results: everything but the lines that name the library calls made"""
    return [l for l in stderr.splitlines() if not l.startswith("Calculating LOD scores with winsize")]


def both(data, tmp_path, name, extra):  # noqa: F811
    rc1, files1, err1 = run_tool(data, tmp_path / (name + "_sets"), SHARDED + extra, True)
    rc0, files0, err0 = run_tool(data, tmp_path / (name + "_loop"), SHARDED + extra, False)
    print(name, "\n".join(told(err1)))
    assert rc1 == 0 and rc0 == 0, (name, err1[-1500:], err0[-1500:])
    assert sorted(files1) == sorted(files0) and files1, (name, sorted(files1), sorted(files0))
    for n in files1:
        assert files1[n] == files0[n], (name, n)
    assert told(err1) == told(err0), name
    assert ONE_CALL in err1 and "in one call" not in err0, name
    return files1, err1


def test_winsize_multi_list_on_two_shards(data, tmp_path):  # noqa: F811
    files, err = both(data, tmp_path, "list", ["--winsize-multi", "30", "60", "90", *BOUNDS])
    assert [n for n in files if n.endswith(".kde")] == ["mine.30SNPs.kde", "mine.60SNPs.kde", "mine.90SNPs.kde"]
    assert len(re.findall(r"^Selected LOD score cutoff: ", err, re.M)) == 3
    assert len(re.findall(r"^KDE on 2 shards$", err, re.M)) == 3
    assert err.count(ONE_CALL) == 1
    assert any(n.endswith(".roh.bed") for n in files)


def test_auto_winsize_from_the_list_on_two_shards(data, tmp_path):  # noqa: F811
    files, err = both(data, tmp_path, "auto", ["--winsize-multi", "30", "60", "90", "--auto-winsize"])
    rows = rows_of(err)
    assert [w for w, _ in rows] == [30, 60, 90][:len(rows)] and rows
    chosen = rows[-1][0]
    assert "Selected window size: %d" % chosen in err
    assert [n for n in files if n.endswith(".kde")] == ["mine.%dSNPs.kde" % chosen]
    assert len(re.findall(r"^KDE on 2 shards$", err, re.M)) == len(rows)       # once per size the search looked at
