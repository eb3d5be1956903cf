"""Batches of split feeds for garlic_kde_parts_multi: F feeds, each split into the same number P of sorted parts (part p of
every feed makes set p).  The feeds are those of tests/kde_cases.py, the splits those of tests/kde_parts_cases.py.
tests/test_kde_parts_multi_cpu.py runs the host descent over them, tests/test_gpu_kde_parts_multi.py the device."""
import numpy as np

import kde_cases as cases
import kde_parts_cases as pcases

EMPTY = np.zeros(0, dtype=np.float64)


def pad(parts, P):
    """the parts of one feed as exactly P parts: empty ones appended"""
    assert len(parts) <= P
    return [np.ascontiguousarray(p) for p in parts] + [EMPTY] * (P - len(parts))


def split(x, P, kind):
    """x into P parts: interleaved, ranges, or lopsided (one of kde_parts_cases.lopsided that fits P, padded with empty parts)"""
    if P == 1:
        return [np.ascontiguousarray(x)]
    if kind == "interleaved":
        return pcases.interleaved(x, P)
    if kind == "ranges":
        return pcases.ranges(x, P)
    assert kind == "lopsided"
    fits = [parts for _, parts in pcases.lopsided(x) if len(parts) <= P]
    return pad(fits[-1], P)


KINDS = ["interleaved", "ranges", "lopsided"]


def batch(F, P, shift=0):
    """[(label, [part of set 0, ..., part of set P - 1])] * F: the contents, the totals of kde_parts_cases.totals() and the
    split kinds go round with the feed index, so one batch mixes lengths from 2 values to several slices"""
    totals = pcases.totals()
    out = []
    for i in range(F):
        name = cases.CONTENTS[(i + shift) % len(cases.CONTENTS)]
        n = totals[(i + 2 * shift) % len(totals)]
        kind = KINDS[(i + shift) % len(KINDS)]
        out.append(("%s %d %s" % (name, n, kind), split(cases.content(name, n), P, kind)))
    return out


def sets_of(feeds, P):
    """[(label, parts)] -> per set p the list of its F parts"""
    return [[parts[p] for _, parts in feeds] for p in range(P)]


def small_mixed():
    """unions of 0, 1, 2, 3 and 65 values in one batch of two sets (the first two cannot have a KDE: they ride along off)"""
    x65 = cases.content("bimodal", 65)
    return [("empty", [EMPTY, EMPTY]), ("one value", [EMPTY, np.array([1.5])]), ("two", [np.array([2.0]), np.array([-1.0])]),
            ("three", [np.array([0.5, 4.0]), np.array([0.5])]), ("65", pcases.interleaved(x65, 2))]


def tied():
    """tied values crossing the parts, and both zeros in both parts"""
    x, zero_parts = pcases.zero_feed()
    two = cases.content("two_values", 65)
    return [("zeros", zero_parts), ("two_values interleaved", pcases.interleaved(two, 2)), ("two_values ranges", pcases.ranges(two, 2))]
