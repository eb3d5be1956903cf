"""The nesting claim behind the multi-size LD weights, pinned without a GPU: ONE left-to-right accumulation at the largest
window size, truncated at the chromosome's end and snapshot after W_i terms, gives calcHR2LD's LD matrix of every size
W_i bit for bit (NaN sign included) -- tail starts and chromosomes shorter than the largest size included.  Also the
grouping rule's restatement on hand-written cases."""
import numpy as np
import pytest

import ld_multi_cases as cases
import oracle_lib as ol


@pytest.mark.parametrize("li", range(len(cases.SIZE_LISTS)))
def test_shared_pass_equals_the_oracle(li):
    sizes = cases.SIZE_LISTS[li]
    nind = 40
    chroms = cases.make_chroms(sizes, nind, 100 + li)
    rng = np.random.default_rng(li)
    sub = np.sort(rng.choice(nind, size=13, replace=False)).astype(np.int32)
    saw_nan = False
    # (the empty subsample -- 0/0 in every pair -- once: it does not depend on the sizes' limits)
    for idx in (None, sub, np.zeros(0, dtype=np.int32)) if li == 0 else (None, sub):
        for c in chroms:
            got = cases.shared_pass(c[0], sizes, idx)
            for w in sorted(set(sizes)):
                want = ol.oracle_hr2_ld(c[0], w, idx=idx)
                assert ol.bits_equal(got[w], want), (sizes, w, c[0].shape[0], ol.count_mismatch(got[w], want))
                saw_nan = saw_nan or bool(np.isnan(want).any())
                n = c[0].shape[0]
                assert not got[w][max(0, n - w + 1):].view(np.uint64).any()        # no full window: +0.0
    assert saw_nan or li != 0


@pytest.mark.skipif(not ol.have_ref(), reason="the reference build is not here")
def test_shared_pass_equals_the_reference():
    sizes = [33, 64, 65, 100]
    chroms = cases.make_chroms(sizes, 40, 5)
    for c in chroms:
        got = cases.shared_pass(c[0], sizes)
        for w in sizes:
            _, want = ol.ref_hr2_ld(c[0], w)
            assert ol.bits_equal(got[w], want), (w, c[0].shape[0])


def test_groups_of():
    g = cases.groups_of
    assert g([33, 34]) == ([[33, 34]], 1)
    assert g([33, 64, 65, 100]) == ([[33, 64, 65, 100]], 1)
    assert g([100, 50, 100]) == ([[50, 100]], 1)
    assert g([16, 32, 33, 40]) == ([[33, 40], [16], [32]], 1)
    assert g([40, 100, 129, 130]) == ([[40, 100, 129, 130]], 1)
    assert g([34, 36, 38, 40, 42]) == ([[34, 36, 38, 40], [42]], 2)
    assert g([10, 20, 100]) == ([[10], [20], [100]], 0)                 # one sharing size: nothing to share with
    assert g([100, 600, 700]) == ([[100], [600], [700]], 0)
    assert g([50, 100], solo=True) == ([[50], [100]], 0)
    # LDS: at 512 (576 threads) the ring is 82960 B and a tile 41472 B -- two sizes fit 128 KB, three do not
    assert cases.lds_bytes(512, 2) == 8 * (2048 * 5 + 130 + 9 * 576) == 124432
    assert cases.lds_bytes(512, 3) > cases.LDS_MAX
    assert g([300, 400, 500, 512]) == ([[300, 400], [500, 512]], 2)
    assert g([40, 50, 60, 512]) == ([[40, 50, 60], [512]], 2)
    assert cases.passes_of([16, 32, 33, 40]) == (3, 3)
    assert cases.passes_of([34, 36, 38, 40, 42]) == (1, 2)
    assert cases.passes_of([34, 36, 38, 40, 42], solo=True) == (5, 5)
    assert cases.group_index([16, 32, 33, 40]) == {33: 0, 40: 0, 16: 1, 32: 2}
