"""CPU tier: the boundary-shape matrix of the GPU tier (tests/shape_matrix.py) covers both sides of every compile-time switch
of the specialised kernels, every shape of it is prebuilt, and every switch still reads in the kernel source as restated."""
import os
import re

import pytest

import shape_matrix as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metran_amd", "csrc")
ALL_SHAPES = [(N, K) for N in range(1, 64) for K in range(1, 64) if N + K <= 64]


def _sides(name, shapes, sub):
    domain, pred = sm.SWITCHES[name][:2]
    return {pred(N, K) for (N, K) in shapes if sm.in_domain(domain, N, K) and sm.in_domain(sub, N, K)}


@pytest.mark.parametrize("name", sorted(sm.SWITCHES))
def test_matrix_holds_both_sides_of_every_switch(name):
    """Both values of the switch among MATRIX's wide shapes and among its narrow ones -- wherever the switch takes both values
    over all the shapes of that kind."""
    for sub in ("narrow", "wide"):
        if len(_sides(name, ALL_SHAPES, sub)) == 2:
            assert _sides(name, sm.MATRIX, sub) == {False, True}, (name, sub)


@pytest.mark.parametrize("case", sorted(sm.CASES))
def test_matrix_holds_every_boundary_case(case):
    assert any(sm.CASES[case](N, K) for (N, K) in sm.MATRIX), case


def test_removing_a_lone_shape_is_noticed():
    """The guard is sharp: every shape that is the only one on one side of a switch (or of a case) fails it when removed."""
    def covered(shapes):
        ok = all(len(_sides(nm, ALL_SHAPES, sub)) < 2 or _sides(nm, shapes, sub) == {False, True}
                 for nm in sm.SWITCHES for sub in ("narrow", "wide"))
        return ok and all(any(c(N, K) for (N, K) in shapes) for c in sm.CASES.values())

    assert covered(sm.MATRIX)
    lone = [s for s in sm.MATRIX if not covered([t for t in sm.MATRIX if t != s])]
    # the new shapes each close a gap of their own
    assert {(12, 4), (13, 4), (20, 6), (23, 5), (33, 4), (40, 4), (59, 4), (60, 4)} <= set(lone), lone


def _aot_shapes():
    text = open(os.path.join(CSRC, "mk_internal.h")).read()
    block = re.search(r"#define MK_SHAPES\(X\)(.*?)#endif", text, re.S).group(1)
    return {(int(a), int(b)) for a, b in re.findall(r"X\((\d+),\s*(\d+)\)", block)}


def test_every_matrix_shape_is_prebuilt():
    from metran_amd import jit

    assert len(set(sm.MATRIX)) == len(sm.MATRIX)
    assert all(N >= 1 and K >= 1 and N + K <= 64 for (N, K) in sm.MATRIX)
    missing = [s for s in sm.MATRIX if s not in _aot_shapes() and s not in jit.TEST_SHAPES]
    assert not missing, "not compiled into the library and not in metran_amd/jit.py TEST_SHAPES: %s" % missing


def test_wave_smoother_bound_reads_in_the_source_as_restated():
    lines = [ln.split("//")[0].strip() for ln in open(os.path.join(CSRC, "mk_internal.h"))]
    assert "constexpr int wave_smoother_max_n = %d;" % sm.WAVE_SMOOTHER_MAX_N in lines


@pytest.mark.parametrize("name", sorted(sm.SWITCHES))
def test_switch_reads_in_the_source_as_restated(name):
    domain, pred, fname, text, expr = sm.SWITCHES[name]
    lines = [ln.split("//")[0].strip() for ln in open(os.path.join(CSRC, fname))]
    assert text in lines, "%s: %r is no longer a line of %s -- update tests/shape_matrix.py (and MATRIX)" % (name, text, fname)
    if expr is None:
        return
    assert expr in text, (name, expr, text)
    for (N, K) in ALL_SHAPES:
        if sm.in_domain(domain, N, K):
            assert sm.c_expression(expr, N, K) == pred(N, K), (name, N, K)
