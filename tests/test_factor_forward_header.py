"""The GENERATED ``Sweeps<n>::factor_forward`` of csrc/mk_sweeps.h (scripts/gen_sweeps.py), n = 2 .. 10: stages 1 .. n-1 of the
right-looking LDL^T with the forward substitution of the right-hand sides and the D^-1 scaling folded into the pivot chains.
Every asm statement is parsed from the header text and emulated in numpy, one array element per lane, and checked against

* an LDL^T of the same matrix (the factor, ``dinv`` and the smallest pivot),
* the SEPARATE order -- factorise, then the header's own ``forward`` statement, then z[c] *= dinv[c] -- bit for bit (the
  stream must apply the same operations to the same values, only in another order),
* a static walk of the stream: every register is final when it is read (the write count it needs), a DPP source is two
  wait states old, a v_rcp_f64 result one, and no statement exceeds the operand limit."""
import numpy as np
import pytest

import sweeps_header as sh
from sweeps_header import emulate, lanes, stream


def _rcp_nr(x):  # rcp_nr of mk_prims.h with the emulation's estimate
    r0 = (1.0 / x) * (1.0 + 2.0 ** -27)
    e = -x * r0 + 1.0
    p = e * e + e
    return r0 * p + r0


def _separate(n, P, W):
    """ldlt_factor<n, 16, false> lane by lane (element r of A[c] is lane r's A[c]), then the header's `forward`, then D^-1."""
    A = [P[:, c].copy() for c in range(n)]       # lane r holds row r: A[c][r] = P[r, c]
    dinv, pivmin = [None] * n, np.full(n, 1.0)
    for j in range(n):
        piv = np.full(n, A[j][j])
        pivmin = np.minimum(pivmin, piv)
        dinv[j] = _rcp_nr(piv)
        lr = A[j] * dinv[j]
        for c in range(j + 1, n):
            A[c] = A[c] + A[c][j] * (-lr)
        A[j] = lr
    (fwd,) = sh.statements(n, "forward")
    regs = emulate(fwd, {**{"A[%d]" % c: A[c] for c in range(n)}, **lanes("z", W)})
    z = [regs["z[%d]" % c] * dinv[c] for c in range(n)]
    return A, dinv, pivmin, z


@pytest.mark.parametrize("n", range(2, 11))
def test_fused_stream_equals_factor_then_forward(n):
    assert "fused_factor = true" in sh.struct(n)
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, n))
    P = M @ M.T + n * np.eye(n)
    P = 0.5 * (P + P.T)
    W = rng.standard_normal((n, n))
    A_ref, dinv_ref, pivmin_ref, z_ref = _separate(n, P, W)

    # entry state of the fused member: stage 0 done by the caller (ldlt_stage0 of mk_prims.h)
    regs = {**lanes("A", P), **lanes("z", W)}
    piv0 = np.full(n, regs["A[0]"][0])
    regs["pivmin"] = np.minimum(np.full(n, 1.0), piv0)
    regs["dinv[0]"] = _rcp_nr(piv0)
    regs["A[0]"] = regs["A[0]"] * regs["dinv[0]"]
    emulate(stream(n, "factor_forward"), regs)

    for c in range(n):
        np.testing.assert_array_equal(regs["dinv[%d]" % c], dinv_ref[c])
        np.testing.assert_array_equal(regs["z[%d]" % c], z_ref[c])
        if c < n - 1:   # column c of L, rows below the diagonal (what the substitutions read)
            np.testing.assert_array_equal(regs["A[%d]" % c][c + 1:], A_ref[c][c + 1:])
    np.testing.assert_array_equal(regs["pivmin"], pivmin_ref)

    # ... and it IS an LDL^T: L D L^T = P, D^-1 L^-1 W^T = z
    L = np.eye(n)
    for c in range(n - 1):
        L[c + 1:, c] = regs["A[%d]" % c][c + 1:]
    d = np.array([1.0 / regs["dinv[%d]" % c][0] for c in range(n)])
    np.testing.assert_allclose(L @ np.diag(d) @ L.T, P, rtol=0, atol=1e-12 * n)
    np.testing.assert_allclose(sh.matrix(regs, "z", n), np.linalg.solve(L @ np.diag(d), W.T).T, rtol=0, atol=1e-12 * n)
    assert float(regs["pivmin"][0]) == min(1.0, d.min())


@pytest.mark.parametrize("n", range(2, 11))
def test_every_register_is_final_and_old_enough_when_read(n, text=sh.HEADER):
    ops = stream(n, "factor_forward", text=text)

    def final_A(k):                  # writes inside the stream that make column k of L: k trailing updates and the division (A[0]: the caller's)
        return k + 1 if k >= 1 else 0

    dpp_fmacs = 0
    # sh.walk: a DPP source is two wait states old (the caller's stage 0 writes A[0] last), a transcendental result one
    for op, _, writes in sh.walk(ops, fresh=["A[0]"], ctx=n):
        d, src = op.dst, [s.lstrip("-") for s in op.src]
        if op.op == "v_fmac_f64_dpp":
            s0, s1, lane = src[0], src[1], op.lane
            dpp_fmacs += 1
            assert op.src[1] == "-" + s1, (n, op)
            if d.startswith("A["):   # trailing update of stage `lane`: column `lane` of L is final, A[c] has had stages 0 .. lane-1
                c = int(d[2:-1])
                assert s0 == d and s1 == "A[%d]" % lane and c > lane
                assert writes.get(s1, 0) == final_A(lane), (n, op)
                assert writes.get(d, 0) == lane, (n, op)
            else:                    # substitution stage k: z[c] -= L(c, k) y_k; y_k has had its k updates and no scaling yet
                c, k = int(d[2:-1]), int(s1[2:-1])
                assert s0 == "A[%d]" % k and lane == c and c > k
                assert writes.get(s0, 0) == final_A(k), (n, op)
                assert writes.get(s1, 0) == k, (n, op)
                assert writes.get(d, 0) == k, (n, op)
        elif op.op == "v_mov_b64_dpp":
            j = op.lane
            assert src[0] == "A[%d]" % j, (n, op)
            assert writes.get(src[0], 0) == j, (n, op)            # every trailing update of column j is in
        elif op.op == "v_mul_f64" and d.startswith("z["):        # D^-1: y_c final, 1/d_c refined, and no substitution reads y_c later
            c = int(d[2:-1])
            assert writes.get(d, 0) == c and (c == 0 or writes.get("dinv[%d]" % c, 0) == 2), (n, op)
            assert not any(o.op == "v_fmac_f64_dpp" and o.src[1] == "-" + d for o in ops[ops.index(op) + 1:]), (n, op)
        elif op.op == "v_mul_f64" and d.startswith("A["):        # L(., j) = A[j] / d_j
            j = int(d[2:-1])
            assert writes.get(d, 0) == j and writes.get("dinv[%d]" % j, 0) == 2, (n, op)
    # no more broadcast multiply-adds than the trailing updates and the forward substitution had: n(n-1)/2 each
    assert dpp_fmacs == n * (n - 1)
    assert all(writes.get("z[%d]" % c, 0) == c + 1 for c in range(n))
