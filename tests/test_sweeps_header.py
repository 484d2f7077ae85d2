"""The GENERATED csrc/mk_sweeps.h (scripts/gen_sweeps.py): every asm statement of every sweep is parsed from the header text
and emulated on random data -- forward / backward substitution, the smoothed mean, V = J D and Ps += V J^T -- for every
state dimension it covers (2 .. 16; 11 .. 16 are TILED into several <= 30-operand statements, round 3).  Catches an
ordering or operand-index mistake of the generator without a GPU; the GPU parity tests then check the kernels.
tests/test_abi.py::test_generated_sweeps_header_is_current checks that the header is what the generator writes."""
import re

import numpy as np
import pytest

import sweeps_header as sh
from sweeps_header import emulate, lanes, matrix, stream


def _check_sweeps(n, rng, text=sh.HEADER):
    """Lane r holds row r of the right-hand sides, of J and of P, and row r of L and D in A[.] and D[.]. -> statements of `forward`"""
    L = np.tril(rng.standard_normal((n, n)), -1)      # lane c holds L(c, k) in A[k]
    z = rng.standard_normal((n, n))
    ref = z.copy()
    for k in range(n - 1):
        for c in range(k + 1, n):
            ref[:, c] -= L[c, k] * ref[:, k]
    got = emulate(stream(n, "forward", text=text), {**lanes("z", z), **lanes("A", L)})
    np.testing.assert_allclose(matrix(got, "z", n), ref, atol=1e-12)
    ref = z.copy()
    for k in range(n - 1, 0, -1):
        for c in range(k):
            ref[:, c] -= L[k, c] * ref[:, k]
    got = emulate(stream(n, "backward", text=text), {**lanes("z", z), **lanes("A", L)})
    np.testing.assert_allclose(matrix(got, "z", n), ref, atol=1e-12)
    D, J = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    V = matrix(emulate(stream(n, "jd", text=text), {**lanes("z", J), **lanes("D", D)}), "V", n)
    np.testing.assert_allclose(V, J @ D, atol=1e-12)
    P = rng.standard_normal((n, n))
    got = emulate(stream(n, "vjt", text=text), {**lanes("P", P), **lanes("z", J), **lanes("V", V)})
    np.testing.assert_allclose(matrix(got, "P", n), P + V @ J.T, atol=1e-12)
    delta = rng.standard_normal(n)
    got = emulate(stream(n, "mean", text=text), {**lanes("z", J), "delta": delta, "acc0": np.zeros(n), "acc1": np.zeros(n)})
    np.testing.assert_allclose(got["acc0"] + got["acc1"], J @ delta, atol=1e-12)
    return len(sh.statements(n, "forward", text=text))


def test_every_generated_sweep_computes_what_it_says():
    rng = np.random.default_rng(0)
    statements = {n: _check_sweeps(n, rng) for n in range(2, 17)}
    assert all(statements[n] == 1 for n in range(2, 11)) and all(2 <= statements[n] <= 6 for n in range(11, 17))


def _edit(text, n, fn, K, old, new, count=1):
    """`text` with the regular expression `old` replaced by `new` in the body of Sweeps<n>::fn, exactly `count` times."""
    a, b = sh.span(n, fn, K, text)
    body, hits = re.subn(old, new, text[a:b], count=count)
    assert hits == count
    return text[:a] + body + text[b:]


def test_the_reader_still_catches_a_broken_header():
    """Four mutations of the header text, in memory, and the check each of them must fail (as they did when every test file
    had a reader of its own: this test, test_every_register_is_final_and_old_enough_when_read[6], test_static_walk[8-2], and
    the operand-limit assertion of the parser)."""
    import test_factor_forward_header as ff
    import test_lowrank_header as lr

    bcast = _edit(sh.HEADER, 11, "forward", None, r"row_newbcast:1 ", "row_newbcast:2 ")              # another valid lane
    assert len(re.findall(r'"s_nop \d+', sh.HEADER[slice(*sh.span(6, "factor_forward"))])) == 3
    nop = _edit(sh.HEADER, 6, "factor_forward", None, r' *"s_nop \d+\\n\\t"\n', "")                     # one s_nop less
    unzeroed = _edit(sh.HEADER, 8, "lowrank", 2, r' *"v_mov_b64 %0, 0\\n\\t"\n', "")                    # u[0] (operand 0) not zeroed
    assert [sh.Ins("v_mov_b64", "u[0]", ("0",), None) in stream(8, "lowrank", 2, t) for t in (sh.HEADER, unzeroed)] == [True, False]
    operand = _edit(sh.HEADER, 10, "vjt", None, r'"\+v"\(P\[9\]\)\n', '"+v"(P[9]), "+v"(extra)\n')     # 32 operands
    for check, args in ((_check_sweeps, (11, np.random.default_rng(0), bcast)), (ff.test_every_register_is_final_and_old_enough_when_read, (6, nop)),
                        (lr.test_static_walk, (8, 2, unzeroed)), (sh.statements, (10, "vjt", None, operand))):
        check(*args[:-1], sh.HEADER)
        with pytest.raises(AssertionError):
            check(*args)
