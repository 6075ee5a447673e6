"""Kernel selection on the GPU: the allowance for dynamic LDS above 64 KB belongs to the kernel function for the whole process
(nk_allow_lds, nk_kind.h), so engines that live side by side with different needs must not disturb each other."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util import case_tables, random_population, make_engine

pytestmark = pytest.mark.gpu

LDS_LINE = 36                                   # bytes of one cell's bins in LDS (nk_field.hip)


def _field_engine(ct, pop4, n, seed):
    from nanokappa_amd import field as FD
    eng = make_engine(ct, *pop4, seed=seed)
    lo, h, n = FD.grid_from_bounds(ct['mesh']['bounds'], n)
    eng.set_field(lo, h, n, 10)
    info = eng.field_info()
    assert info['lds_path'] == 1 and LDS_LINE * info['ncells'] > 64 * 1024, info      # bins in LDS, above the default limit of a launch
    return eng


def _maps(eng):
    f = eng.field()
    return f['samples'], [f[k].tobytes() for k in ('N', 'E', 'F')]


def test_two_engines_with_different_lds_needs_above_64k():
    """A (16^3 cells, 144 KB of bins) steps through a field sample, B (13^3 cells, 77 KB; the same kernel function) does, then A
    again: A's maps are those of A alone, bit for bit (the field is bit-reproducible, test_gpu_field).
    The maps are the step-mode sums of the two samples.  A state-mode tally after the last step is NOT compared: it relaxes against
    the temperatures the last step left, and those were seen to differ by one rounding of an FP64 sum between the first run of a
    process and later ones, whichever of them had B beside it (profiles/dispatch_notes.txt: T_sv of the last step 1.1e-13 apart in one subvolume, hence 3 of 32768 integers by one
    unit, while N, E and F of both samples were equal)."""
    ct = case_tables('ttp')
    pop_a, pop_b = random_population(ct, 20000, seed=31), random_population(ct, 20000, seed=32)
    a = _field_engine(ct, pop_a, (16, 16, 16), seed=7)
    b = _field_engine(ct, pop_b, (13, 13, 13), seed=8)
    assert a.field_info()['ncells'] != b.field_info()['ncells']
    a.step(10)
    b.step(10)
    a.step(10)
    together, other = _maps(a), _maps(b)
    a.close()
    b.close()
    solo = _field_engine(ct, pop_a, (16, 16, 16), seed=7)
    solo.step(10)
    solo.step(10)
    alone = _maps(solo)
    solo.close()
    assert together[0] == alone[0] == 2 and other[0] == 1
    assert together[1] == alone[1]
