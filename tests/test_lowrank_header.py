"""The GENERATED ``Sweeps<n>::lowrank`` and ``Sweeps<n>::lowrank_apply`` of csrc/mk_sweeps.h (scripts/gen_sweeps.py), n = 2 .. 10 and
every factor count K they exist for: the rank-K covariance step of the record smoother.  As
tests/test_factor_forward_header.py does for ``factor_forward``, every asm statement is parsed from the header text and emulated in
numpy, one array element per lane of a 16-lane group (lanes >= n replicate lane n - 1, as in the kernel), and checked against

* u = J (J_f D)^T and P + u B^T, B = [-Gamma ; I_K], formed with numpy;
* the general products where the premise holds (J = B J_f): P + J D J^T;
* a static walk: one statement each, within the operand limit, a DPP source written inside the statement two wait states old,
  every accumulator zeroed before its first multiply-add, 2 n K + N K broadcast multiply-adds in all."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SRC = open(os.path.join(ROOT, "metran_amd", "csrc", "mk_sweeps.h")).read()
DPP = r" row_newbcast:(\d+) row_mask:0xf bank_mask:0xf$"
G = 16


def _max_k(n):
    return max(0, min(n - 1, 5, (30 - 2 * n) // 2))


CASES = [(n, K) for n in range(2, 11) for K in range(1, _max_k(n) + 1)]


def _body(n):
    a = SRC.index("struct Sweeps<%d>" % n)
    return SRC[a:SRC.index("\n};", a) + 1]


def _statement(n, K, fn):
    """The ONE asm statement of an overload -> list of instruction lines over register NAMES."""
    body = _body(n)
    sig = {"lowrank": "void lowrank(double (&u)[%d]," % K, "lowrank_apply": "void lowrank_apply(double (&P)[%d], const double (&u)[%d]," % (n, K)}[fn]
    f = body.index(sig)
    stmts = body[f:body.index("\n    }\n", f)].split("asm volatile(")[1:]
    assert len(stmts) == 1, (n, K, fn)
    st = stmts[0]
    lines = re.findall(r'"([vs]_\w+ [^"]*?)\\n\\t"', st)
    tail = st[st.index(":"):]
    operands = re.findall(r'"[=+&]*v"\(([\w\[\]]+)\)', tail)
    assert len(operands) + len(re.findall(r'"\+v"', tail)) <= 30, (n, K, fn)   # the inline-asm operand limit
    return [re.sub(r"%(\d+)", lambda m: operands[int(m.group(1))], ln) for ln in lines]


def _ops(lines):
    out = []
    for ln in lines:
        m = re.match(r"v_fmac_f64_dpp ([\w\[\]]+), ([\w\[\]]+), (-?)([\w\[\]]+)" + DPP, ln)
        if m:
            out.append(("fmac", m.group(1), m.group(2), m.group(4), -1.0 if m.group(3) else 1.0, int(m.group(5))))
            continue
        m = re.match(r"v_mov_b64 ([\w\[\]]+), 0$", ln)
        if m:
            out.append(("zero", m.group(1)))
            continue
        m = re.match(r"v_add_f64 ([\w\[\]]+), ([\w\[\]]+), ([\w\[\]]+)$", ln)
        if m:
            out.append(("add",) + m.groups())
            continue
        m = re.match(r"s_nop (\d+)$", ln)
        assert m, ln
        out.append(("nop", int(m.group(1)) + 1))
    return out


def _emulate(ops, regs):
    for op in ops:
        if op[0] == "fmac":      # dst += bcast_lane(src0) * (+-src1)
            _, d, s0, s1, sign, lane = op
            regs[d] = regs[d] + regs[s0][lane] * (sign * regs[s1])
        elif op[0] == "zero":
            regs[op[1]] = np.zeros(G)
        elif op[0] == "add":
            regs[op[1]] = regs[op[2]] + regs[op[3]]
    return regs


def _lanes(M):
    """Row r of M in lane r, lanes >= n replicating lane n - 1: {name[c]: per-lane array}."""
    idx = np.minimum(np.arange(G), M.shape[0] - 1)
    return M[idx]


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
    assert "lowrank_max_k = %d;" % _max_k(n) in _body(n)
    for premise in (True, False):
        Gam, B, J, D, P = _inputs(n, K, premise)
        Jl, Dl = _lanes(J), _lanes(D)
        regs = {"z[%d]" % c: Jl[:, c].copy() for c in range(n)}
        regs.update({"D[%d]" % c: Dl[:, c].copy() for c in range(n)})
        _emulate(_ops(_statement(n, K, "lowrank")), regs)
        u = np.stack([regs["u[%d]" % k] for k in range(K)], axis=1)          # [lane, k]
        want = J @ (D @ J[N:].T)
        scale = max(1.0, float(np.abs(J).max()) ** 2 * float(np.abs(D).max()))
        np.testing.assert_allclose(u[:n], want, rtol=0, atol=4e-15 * n * n * scale)
        np.testing.assert_array_equal(u[n:], np.broadcast_to(u[n - 1], (G - n, K)))   # the replica lanes stay replicas

        # the loadings as the kernel holds them: lane j < N has series j's, lanes >= N those of series N - 1
        gl = Gam[np.minimum(np.arange(G), N - 1)]
        regs2 = {"P[%d]" % c: _lanes(P)[:, c].copy() for c in range(n)}
        regs2.update({"u[%d]" % k: u[:, k].copy() for k in range(K)})
        regs2.update({"gam[%d]" % k: gl[:, k].copy() for k in range(K)})
        _emulate(_ops(_statement(n, K, "lowrank_apply")), regs2)
        Pn = np.stack([regs2["P[%d]" % c] for c in range(n)], axis=1)[:n]
        np.testing.assert_allclose(Pn, P + u[:n] @ B.T, rtol=0, atol=4e-15 * n * scale)
        if premise:   # J = B J_f: the two statements ARE the general products
            np.testing.assert_allclose(Pn, P + J @ D @ J.T, rtol=0, atol=1e-14 * n * n * scale)
        else:
            assert float(np.abs(Pn - (P + J @ D @ J.T)).max()) > 1e-3


@pytest.mark.parametrize("n,K", CASES)
def test_static_walk(n, K):
    N = n - K
    fmacs = 0
    for fn in ("lowrank", "lowrank_apply"):
        age, zeroed = {}, set()
        for op in _ops(_statement(n, K, fn)):
            if op[0] == "nop":
                age = {r: a + op[1] for r, a in age.items()}
                continue
            if op[0] == "fmac":
                _, d, s0, s1, sign, lane = op
                fmacs += 1
                assert age.get(s0, 99) >= 2, (n, K, fn, op)                  # a DPP source is two wait states old
                assert lane < n and s0 != d, (n, K, fn, op)
                if fn == "lowrank":
                    assert d in zeroed and sign == 1.0, (n, K, fn, op)      # accumulators start from zero
                else:
                    assert s0.startswith("gam[") and lane < N and sign == -1.0 and d == "P[%d]" % lane, (n, K, fn, op)
                dst = d
            elif op[0] == "zero":
                zeroed.add(op[1])
                dst = op[1]
            else:
                dst = op[1]
            age = {r: a + 1 for r, a in age.items()}
            age[dst] = 0
    assert fmacs == 2 * n * K + N * K


def test_header_is_what_the_generator_writes():
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_sweeps", os.path.join(ROOT, "scripts", "gen_sweeps.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.render() == SRC
    assert [gen.lowrank_max_k(n) for n in range(2, 11)] == [_max_k(n) for n in range(2, 11)]
