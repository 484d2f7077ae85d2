"""The GENERATED ``Sweeps<n>::lowrank`` and ``Sweeps<n>::lowrank_apply`` of csrc/mk_sweeps.h (scripts/gen_sweeps.py), n = 2 .. 10 and
every factor count K they exist for: the rank-K covariance step of the record smoother.  As
tests/test_factor_forward_header.py does for ``factor_forward``, every asm statement is parsed from the header text and emulated in
numpy, one array element per lane of a 16-lane group (lanes >= n replicate lane n - 1, as in the kernel), and checked against

* u = J (J_f D)^T and P + u B^T, B = [-Gamma ; I_K], formed with numpy;
* the general products where the premise holds (J = B J_f): P + J D J^T;
* a static walk: one statement each, within the operand limit, a DPP source written inside the statement two wait states old,
  every accumulator zeroed before its first multiply-add, 2 n K + N K broadcast multiply-adds in all."""
import numpy as np
import pytest

import sweeps_header as sh
from sweeps_header import emulate, lanes, matrix

G = 16
CASES = [(n, K) for n in range(2, 11) for K in range(1, sh.lowrank_max_k(n) + 1)]


def _statement(n, K, fn, text=sh.HEADER):
    stmts = sh.statements(n, fn, K, text)
    assert len(stmts) == 1, (n, K, fn)         # the ONE asm statement of an overload
    return stmts[0]


def _inputs(n, K, premise):
    rng = np.random.default_rng(100 * n + K)
    N = n - K
    Gam = rng.uniform(-1.0, 1.0, (N, K))
    B = np.vstack([-Gam, np.eye(K)])
    J = B @ rng.standard_normal((K, n)) if premise else rng.standard_normal((n, n))
    D = rng.standard_normal((n, n))
    D = D + D.T
    P = rng.standard_normal((n, n))
    return Gam, B, J, D, P


@pytest.mark.parametrize("n,K", CASES)
def test_statements_compute_u_and_the_update(n, K):
    N = n - K
    assert "lowrank_max_k = %d;" % sh.lowrank_max_k(n) in sh.struct(n)
    for premise in (True, False):
        Gam, B, J, D, P = _inputs(n, K, premise)
        u = matrix(emulate(_statement(n, K, "lowrank"), {**lanes("z", J, G), **lanes("D", D, G)}), "u", K)     # [lane, k]
        want = J @ (D @ J[N:].T)
        scale = max(1.0, float(np.abs(J).max()) ** 2 * float(np.abs(D).max()))
        np.testing.assert_allclose(u[:n], want, rtol=0, atol=4e-15 * n * n * scale)
        np.testing.assert_array_equal(u[n:], np.broadcast_to(u[n - 1], (G - n, K)))   # the replica lanes stay replicas

        # the loadings as the kernel holds them: lane j < N has series j's, lanes >= N those of series N - 1
        regs = emulate(_statement(n, K, "lowrank_apply"), {**lanes("P", P, G), **lanes("u", u), **lanes("gam", Gam, G)})
        Pn = matrix(regs, "P", n)[:n]
        np.testing.assert_allclose(Pn, P + u[:n] @ B.T, rtol=0, atol=4e-15 * n * scale)
        if premise:   # J = B J_f: the two statements ARE the general products
            np.testing.assert_allclose(Pn, P + J @ D @ J.T, rtol=0, atol=1e-14 * n * n * scale)
        else:
            assert float(np.abs(Pn - (P + J @ D @ J.T)).max()) > 1e-3


@pytest.mark.parametrize("n,K", CASES)
def test_static_walk(n, K, text=sh.HEADER):
    N = n - K
    fmacs = 0
    for fn in ("lowrank", "lowrank_apply"):
        zeroed = set()
        for op, _, _ in sh.walk(_statement(n, K, fn, text), ctx=(n, K, fn)):   # a DPP source is two wait states old
            if op.op == "v_fmac_f64_dpp":
                d, s0, lane, sign = op.dst, op.src[0], op.lane, -1.0 if op.src[1].startswith("-") else 1.0
                fmacs += 1
                assert lane < n and s0 != d, (n, K, fn, op)
                if fn == "lowrank":
                    assert d in zeroed and sign == 1.0, (n, K, fn, op)      # accumulators start from zero
                else:
                    assert s0.startswith("gam[") and lane < N and sign == -1.0 and d == "P[%d]" % lane, (n, K, fn, op)
            elif op.op == "v_mov_b64":
                zeroed.add(op.dst)
    assert fmacs == 2 * n * K + N * K
