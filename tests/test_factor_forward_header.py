"""The GENERATED ``Sweeps<n>::factor_forward`` of csrc/mk_sweeps.h (scripts/gen_sweeps.py), n = 2 .. 10: stages 1 .. n-1 of the
right-looking LDL^T with the forward substitution of the right-hand sides and the D^-1 scaling folded into the pivot chains.
Every asm statement is parsed from the header text and emulated in numpy, one array element per lane, and checked against

* an LDL^T of the same matrix (the factor, ``dinv`` and the smallest pivot),
* the SEPARATE order -- factorise, then the header's own ``forward`` statement, then z[c] *= dinv[c] -- bit for bit (the
  stream must apply the same operations to the same values, only in another order),
* a static walk of the stream: every register is final when it is read (the write count it needs), a DPP source is two
  wait states old, a v_rcp_f64 result one, and no statement exceeds the operand limit."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SRC = open(os.path.join(ROOT, "metran_amd", "csrc", "mk_sweeps.h")).read()
DPP = r" row_newbcast:(\d+) row_mask:0xf bank_mask:0xf"


def _body(n):
    a = SRC.index("struct Sweeps<%d>" % n)
    return SRC[a:SRC.index("};", a)]


def _statements(n, fn):
    body = _body(n)
    f = body.index("void %s(" % fn)
    out = []
    for st in body[f:body.index("\n    }\n", f)].split("asm volatile(")[1:]:
        lines = re.findall(r'"([vs]_\w+ [^"]*?)\\n\\t"', st)
        tail = st[st.index(":"):]
        operands = re.findall(r'"[=+&]*v"\(([\w\[\]]+)\)', tail)
        assert len(operands) + len(re.findall(r'"\+v"', tail)) <= 30, (n, fn)   # the inline-asm operand limit
        out.append([re.sub(r"%(\d+)", lambda m: operands[int(m.group(1))], ln) for ln in lines])
    return out


def _stream(n):
    """-> list of (op, dst, sources..., lane) over register NAMES."""
    ops = []
    for st in _statements(n, "factor_forward"):
        for ln in st:
            m = re.match(r"v_fmac_f64_dpp ([\w\[\]]+), ([\w\[\]]+), -([\w\[\]]+)" + DPP + "$", ln)
            if m:
                ops.append(("fmac", m.group(1), m.group(2), m.group(3), int(m.group(4))))
                continue
            m = re.match(r"v_mov_b64_dpp (\w+), ([\w\[\]]+)" + DPP + "$", ln)
            if m:
                ops.append(("bcast", m.group(1), m.group(2), int(m.group(3))))
                continue
            m = re.match(r"s_nop (\d+)$", ln)
            if m:
                ops.append(("nop", int(m.group(1)) + 1))
                continue
            m = re.match(r"(v_rcp_f64|v_min_f64|v_fma_f64|v_mul_f64) (.*)$", ln)
            assert m, ln
            ops.append((m.group(1),) + tuple(a.strip() for a in m.group(2).split(",")))
    return ops


def _val(regs, name):
    if name.startswith("-"):
        return -regs[name[1:]]
    return regs[name] if name in regs else float(name)


def _emulate(ops, regs):
    for op in ops:
        if op[0] == "fmac":                      # dst -= bcast_lane(src0) * src1
            _, d, s0, s1, lane = op
            regs[d] = regs[d] + regs[s0][lane] * (-regs[s1])
        elif op[0] == "bcast":
            regs[op[1]] = np.full_like(regs[op[2]], regs[op[2]][op[3]])
        elif op[0] == "v_rcp_f64":
            # the hardware's estimate is good to 2^-25; the emulation perturbs the exact quotient so that the refinement has work
            regs[op[1]] = (1.0 / _val(regs, op[2])) * (1.0 + 2.0 ** -27)
        elif op[0] == "v_min_f64":
            regs[op[1]] = np.minimum(_val(regs, op[2]), _val(regs, op[3]))
        elif op[0] == "v_fma_f64":
            regs[op[1]] = _val(regs, op[2]) * _val(regs, op[3]) + _val(regs, op[4])
        elif op[0] == "v_mul_f64":
            regs[op[1]] = _val(regs, op[2]) * _val(regs, op[3])
    return regs


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
    regs = {"A[%d]" % c: A[c] for c in range(n)}
    regs.update({"z[%d]" % c: W[:, c].copy() for c in range(n)})
    (fwd,) = _statements(n, "forward") or ([],)
    for ln in fwd:
        d, s0, s1, lane = re.match(r"v_fmac_f64_dpp ([\w\[\]]+), ([\w\[\]]+), -([\w\[\]]+)" + DPP, ln).groups()
        regs[d] = regs[d] + regs[s0][int(lane)] * (-regs[s1])
    z = [regs["z[%d]" % c] * dinv[c] for c in range(n)]
    return A, dinv, pivmin, z


@pytest.mark.parametrize("n", range(2, 11))
def test_fused_stream_equals_factor_then_forward(n):
    assert "fused_factor = true" in _body(n)
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, n))
    P = M @ M.T + n * np.eye(n)
    P = 0.5 * (P + P.T)
    W = rng.standard_normal((n, n))
    A_ref, dinv_ref, pivmin_ref, z_ref = _separate(n, P, W)

    # entry state of the fused member: stage 0 done by the caller (ldlt_stage0 of mk_prims.h)
    regs = {"A[%d]" % c: P[:, c].copy() for c in range(n)}
    regs.update({"z[%d]" % c: W[:, c].copy() for c in range(n)})
    piv0 = np.full(n, regs["A[0]"][0])
    regs["pivmin"] = np.minimum(np.full(n, 1.0), piv0)
    regs["dinv[0]"] = _rcp_nr(piv0)
    regs["A[0]"] = regs["A[0]"] * regs["dinv[0]"]
    _emulate(_stream(n), regs)

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
    Z = np.stack([regs["z[%d]" % c] for c in range(n)], axis=1)      # Z[r, c]: lane r's z[c]
    np.testing.assert_allclose(Z, np.linalg.solve(L @ np.diag(d), W.T).T, rtol=0, atol=1e-12 * n)
    assert float(regs["pivmin"][0]) == min(1.0, d.min())


@pytest.mark.parametrize("n", range(2, 11))
def test_every_register_is_final_and_old_enough_when_read(n):
    ops = _stream(n)
    writes = {}                      # register -> number of writes so far
    age = {"A[0]": 0}                # wait states since the last write (the caller's stage 0 writes A[0] last)
    trans = None

    def tick(k):
        for r in age:
            age[r] += k

    def final_A(k):                  # writes inside the stream that make column k of L: k trailing updates and the division (A[0]: the caller's)
        return k + 1 if k >= 1 else 0

    dpp_fmacs = 0
    for op in ops:
        if op[0] == "nop":
            tick(op[1])
            trans = None
            continue
        if op[0] == "fmac":
            _, d, s0, s1, lane = op
            dpp_fmacs += 1
            assert age.get(s0, 99) >= 2, (n, op)
            assert trans not in (d, s0, s1), (n, op)
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
            dst = d
        elif op[0] == "bcast":
            j = op[3]
            assert op[2] == "A[%d]" % j and age.get(op[2], 99) >= 2, (n, op)
            assert writes.get(op[2], 0) == j, (n, op)            # every trailing update of column j is in
            dst = op[1]
        else:
            srcs = [s.lstrip("-") for s in op[2:]]
            if op[0] != "v_rcp_f64":
                assert trans not in srcs, (n, op)                # a transcendental result is one wait state old
            if op[0] == "v_mul_f64" and op[1].startswith("z["):  # D^-1: y_c final, 1/d_c refined, and no substitution reads y_c later
                c = int(op[1][2:-1])
                assert writes.get(op[1], 0) == c and (c == 0 or writes.get("dinv[%d]" % c, 0) == 2), (n, op)
                assert not any(o[0] == "fmac" and o[3] == op[1] for o in ops[ops.index(op) + 1:]), (n, op)
            if op[0] == "v_mul_f64" and op[1].startswith("A["):  # L(., j) = A[j] / d_j
                j = int(op[1][2:-1])
                assert writes.get(op[1], 0) == j and writes.get("dinv[%d]" % j, 0) == 2, (n, op)
            dst = op[1]
        tick(1)
        age[dst] = 0
        writes[dst] = writes.get(dst, 0) + 1
        trans = dst if op[0] == "v_rcp_f64" else None
    # no more broadcast multiply-adds than the trailing updates and the forward substitution had: n(n-1)/2 each
    assert dpp_fmacs == n * (n - 1)
    assert all(writes.get("z[%d]" % c, 0) == c + 1 for c in range(n))
