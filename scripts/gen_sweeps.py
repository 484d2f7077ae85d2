#!/usr/bin/env python3
"""Writes metran_amd/csrc/mk_sweeps.h: the DPP broadcast-FMA sweeps of the 16-lane smoother as ONE asm statement each.

Why: hipcc's hazard recogniser counts an inline-asm statement as zero wait states and assumes every asm result needs
one before another asm statement may touch it, so a sweep written as one statement per v_fmac_f64_dpp gets an
`s_nop 0` at every sweep boundary (the next sweep's first FMA accumulates into a register the previous sweep's
statements wrote): 31 per step of smoother_record_kernel<8,2>, each a full issue slot.  A statement may have at
most 30 operands ("+v" counts twice): for n <= 10 every sweep is ONE statement; for 11 <= n <= 16 (round 3) a sweep is
TILED into statements of <= 30 operands -- blocks of 7 broadcast sources x 7 or 8 accumulators, ordered so that every
value is final before it is read -- 3 to 6 statements (= padding nops) per sweep instead of one per FMA.

How: a sweep is a list of `Ins` over SYMBOLIC registers (z[3], A[0], Vf[1], acc0, ...).  `stmt` turns such a list into an
asm statement (operand list, constraints, %k numbers, the operand limit), `cut` splits a stream into statements, and
`WaitStates` is the hazard rule inside a statement, where the compiler does not look.  A new sweep is a new list."""
import os

DPP = " row_mask:0xf bank_mask:0xf"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "metran_amd", "csrc", "mk_sweeps.h")
LIMIT = 30  # operands of one asm statement


class Ins:
    """One instruction over symbolic registers: `fmt` takes the registers `regs` in order; it writes `writes` and reads `reads`;
    `dpp` is the register read through DPP (src0), `trans` marks a transcendental, `wait` is the wait states it takes."""

    def __init__(self, fmt, regs, writes=None, reads=(), dpp=None, trans=False, wait=1):
        self.fmt, self.regs, self.writes, self.reads, self.dpp, self.trans, self.wait = fmt, regs, writes, set(reads), dpp, trans, wait


def R(name, idx):
    return ["%s[%d]" % (name, i) for i in idx]


def fmac(acc, src, mul, lane, neg=False):  # acc += bcast_lane(src) * (+-mul)
    return Ins("v_fmac_f64_dpp {0}, {1}, %s{2} row_newbcast:%d%s" % ("-" if neg else "", lane, DPP), [acc, src, mul], acc, [acc, src, mul], dpp=src)


def alu(name, dst, *src, trans=False):  # name dst, src...
    return Ins(name + " " + ", ".join("{%d}" % k for k in range(len(src) + 1)), [dst] + list(src), dst, src, trans=trans)


def zero(r):
    return Ins("v_mov_b64 {0}, 0", [r], r)


def operands(code, order=None):
    """(register, constraint) of one statement, outputs before inputs as the assembler wants them: written first -> "=&v", read
    first -> "+v", never written -> "v".  Within each group the registers stand in the order of their first appearance, or in
    the order the sweep passes as order = (outputs, inputs): the operand order of the committed header is part of a sweep's
    description.  There a register listed as an output that the statement only reads (z[0] of `forward`) is "+v"."""
    seen, first_read, written = [], set(), set()
    for i in code:
        for r in i.regs:
            if r not in seen:
                seen.append(r)
        first_read |= i.reads - written
        if i.writes:
            written.add(i.writes)
    outs, ins = order or ([r for r in seen if r in written], [r for r in seen if r not in written])
    assert sorted(outs + ins) == sorted(seen) and not written & set(ins), (outs, ins, seen)
    return [(r, "=&v" if r in written - first_read else "+v") for r in outs] + [(r, "v") for r in ins]


def op_count(ops):
    return sum(2 if c == "+v" else 1 for _, c in ops)


def stmt(code, order=None, indent="        "):
    """THE renderer: one instruction list -> one asm volatile statement."""
    ops = operands(code, order)
    assert 0 < op_count(ops) <= LIMIT, ops
    idx = {r: "%%%d" % k for k, (r, _) in enumerate(ops)}
    body = "\n".join('%s    "%s\\n\\t"' % (indent, i.fmt.format(*[idx[r] for r in i.regs])) for i in code)
    outs = ", ".join('"%s"(%s)' % (c, r) for r, c in ops if c != "v")
    ins = ", ".join('"v"(%s)' % r for r, c in ops if c == "v")
    return "%sasm volatile(\n%s\n%s    : %s\n%s    : %s);\n" % (indent, body, indent, outs, indent, ins)


def cut(stream):
    """A stream as as few statements of <= 30 operands as its order allows."""
    stmts = [[]]
    for i in stream:
        if stmts[-1] and op_count(operands(stmts[-1] + [i])) > LIMIT:
            stmts.append([])
        stmts[-1].append(i)
    return stmts


class WaitStates:
    """THE hazard rule inside a statement: a register read through DPP and written earlier in the stream must be two wait states
    old, a v_rcp_f64 result one before a non-transcendental reads it.  Every instruction is one wait state, `s_nop k` k + 1.
    `fresh`: registers that count as written by the instruction before the stream."""

    def __init__(self, fresh=()):
        self.age = {r: 0 for r in fresh}    # register -> wait states since its last VALU write (absent: old)
        self.trans = None                   # the transcendental result the last instruction wrote

    def need(self, i):                      # wait states `i` still has to wait
        k = 2 - self.age.get(i.dpp, 2)
        return max(k, 1) if self.trans in i.reads and not i.trans else k

    def issue(self, i):
        """-> `i` behind the s_nop it needs, if any."""
        k = self.need(i)
        out = ([Ins("s_nop %d" % (k - 1), [], wait=k)] if k > 0 else []) + [i]
        self.age = {r: a + sum(j.wait for j in out) for r, a in self.age.items()}
        self.age[i.writes] = 0
        self.trans = i.writes if i.trans else None
        return out


def scale(c):
    return alu("v_mul_f64", "z[%d]" % c, "z[%d]" % c, "dinv[%d]" % c)


FILL_WANT = 8  # independent instructions a stage wants: two ahead of the pivot broadcast, one in every later gap of the chain


def fused_stream(n):
    """Stages 1..n-1 of the right-looking LDL^T with the forward substitution of the right-hand sides folded in (the
    elimination of [Pp | W]) and the D^-1 scaling behind it, as ONE instruction stream.  Entry: stage 0 is done (A[0] holds
    L(., 0), dinv[0] = 1/d_0, both fresh: A[0] counts as written by the instruction before the stream).
    Stage j: the column-j multiply-add of stage j-1's trailing update first, then the pivot broadcast (two wait states behind
    it), v_rcp_f64, the three refinement multiply-adds and L(., j) = A[j] / d_j -- every one of them with an INDEPENDENT
    instruction in front: the rest of stage j-1's trailing update, substitution stage j-1 (column j-1 of L is final), and in
    the late stages, which have few of either, z[c] *= dinv[c] of the columns the substitution has passed.  Every value is
    produced by the operation that produces it in ldlt_factor / Sweeps::forward / the caller's scaling loop."""
    ws, out = WaitStates(fresh=["A[0]"]), []

    def must(i):
        out.extend(ws.issue(i))

    pool = []           # columns whose y_c the substitution has passed: z[c] may take its D^-1
    for j in range(1, n):
        lr, y, a, d = "A[%d]" % (j - 1), "z[%d]" % (j - 1), "A[%d]" % j, "dinv[%d]" % j
        if j >= 2:
            pool.append(j - 2)
        fills = [fmac("A[%d]" % c, "A[%d]" % c, lr, j - 1, True) for c in range(j + 1, n)]
        fills += [fmac("z[%d]" % c, lr, y, c, True) for c in range(j, n)]
        chain = [Ins("v_mov_b64_dpp {0}, {1} row_newbcast:%d%s" % (j, DPP), ["piv", a], "piv", [a], dpp=a),
                 alu("v_rcp_f64", d, "piv", trans=True),
                 Ins("v_fma_f64 {0}, -{1}, {2}, 1.0", ["e", "piv", d], "e", ["piv", d]),
                 alu("v_fma_f64", "e", "e", "e", "e"),
                 alu("v_fma_f64", d, d, "e", d)]
        if j < n - 1:
            chain.append(alu("v_mul_f64", a, a, d))
        take = min(len(pool), max(0, FILL_WANT - len(fills)))
        fills += [scale(pool.pop(0)) for _ in range(take)]
        # the gaps in front of the chain instructions, and the one behind the last (ahead of the next stage's first
        # multiply-add); scarce fills go to the latency gaps of the refinement first, then ahead of the broadcast.
        # v_min_f64 (off the chain) always follows v_rcp_f64: the wait state a transcendental result needs.
        gaps = [2, 1, 1, 1, 1, 1][:len(chain)] + [1]
        have, want = len(fills), [0] * len(gaps)
        for g in [3, 4, 5, 2, 6, 1, 0, 0]:
            if g < len(gaps) and have > 0 and want[g] < gaps[g]:
                want[g] += 1
                have -= 1
        want[-1] += have    # what is left runs behind the stage's last chain instruction
        must(fmac(a, a, lr, j - 1, True))
        for g in range(len(want)):
            for _ in range(want[g]):
                pick = next((f for f in fills if ws.need(f) <= 0), fills[0])
                fills.remove(pick)
                must(pick)
            if g < len(chain):
                must(chain[g])
                if chain[g].trans:
                    must(alu("v_min_f64", "pivmin", "pivmin", "piv"))
        assert not fills
    for c in pool + [n - 2, n - 1]:     # y_{n-2} and y_{n-1} are final only now
        must(scale(c))
    return out


LOWRANK_MAX_K = 5  # factors the rank-K covariance step is generated for (and 2n + 2K <= 30 operands)


def lowrank_max_k(n):
    return max(0, min(n - 1, LOWRANK_MAX_K, (LIMIT - 2 * n) // 2))


def lowrank(n, K):
    """u = J (J_f D)^T (N = n - K, J_f = rows N.. of J): Vf[k] of lane c = sum_j D[c][j] J[N+k][j], then u[k] = sum_c J[r][c] Vf[k] of
    lane c.  K chains run interleaved; K = 1 splits its one chain of n into two (even / odd terms: Vf[0] / Vb, u[0] / ub) and adds
    them.  The zeroing of u stands BETWEEN the two products: with the other chains' last multiply-adds it gives Vf[k] its two wait
    states before the second product reads it through DPP (WaitStates pads where it does not: nowhere today)."""
    N, z, D = n - K, R("z", range(n)), R("D", range(n))
    if K == 1:
        V, u = ["Vf[0]", "Vb"], ["u[0]", "ub"]
        code = [zero(r) for r in V] + [fmac(V[j % 2], z[j], D[j], N) for j in range(n)] + [alu("v_add_f64", V[0], V[0], V[1])]
        code += [zero(r) for r in u] + [fmac(u[c % 2], V[0], z[c], c) for c in range(n)] + [alu("v_add_f64", u[0], u[0], u[1])]
    else:
        V, u = R("Vf", range(K)), R("u", range(K))
        code = [zero(r) for r in V] + [fmac(V[k], z[j], D[j], N + k) for j in range(n) for k in range(K)]
        code += [zero(r) for r in u] + [fmac(u[k], V[k], z[c], c) for c in range(n) for k in range(K)]
    ws = WaitStates()
    return [([j for i in code for j in ws.issue(i)], (u[:K] + V + u[K:], D + z))]


def lowrank_apply(n, K):
    """Ps = Pf + u B^T, B = [-Gamma ; I_K]: P[c] -= u[k] Gamma[c][k] (Gamma[c][k] = gam[k] of lane c < N), P[N+k] += u[k]."""
    N, u, gam = n - K, R("u", range(K)), R("gam", range(K))
    code = [fmac("P[%d]" % c, gam[k], u[k], c, True) for k in range(K) for c in range(N)]
    code += [alu("v_add_f64", "P[%d]" % (N + k), "P[%d]" % (N + k), u[k]) for k in range(K)]
    return [(code, (R("P", range(n)), u + gam))]


def blocks(n, size):
    return [list(range(i, min(n, i + size))) for i in range(0, n, size)]


def tri(n, src, fwd):
    """Forward (z[c] -= bcast_c(A[k]) z[k], k ascending, c > k) or backward (z[c] -= bcast_k(A[c]) z[k], k descending, c < k)
    substitution over blocks of `src` sources: a block's diagonal tile, which makes its sources final, then its sources into the
    accumulators of the blocks still to come, 8 at a time."""
    def ins(k, c):
        return fmac("z[%d]" % c, "A[%d]" % (k if fwd else c), "z[%d]" % k, c if fwd else k, True)

    tiles = []
    for kb in blocks(n, src)[::1 if fwd else -1]:
        ks = kb[::1 if fwd else -1]
        if len(kb) > 1:
            tiles.append(([ins(k, c) for k in ks for c in kb if (c > k if fwd else c < k)], (R("z", kb), R("A", kb[:-1]))))
        rest = list(range(kb[-1] + 1, n)) if fwd else list(range(kb[0]))
        for cs in (rest[i:i + 8] for i in range(0, len(rest), 8)):
            tiles.append(([ins(k, c) for k in ks for c in cs], (R("z", cs), R("z", kb) + R("A", kb if fwd else cs))))
    return tiles


def mean(n):
    """Smoothed mean: acc0 / acc1 += bcast_c(delta) z[c], two chains."""
    return [([fmac("acc%d" % (c % 2), "delta", "z[%d]" % c, c) for c in range(n)], (["acc0", "acc1"], ["delta"] + R("z", range(n))))]


def jd(n, acc, src):
    """V = J D: V[c] = sum_k bcast_k(D[c]) z[k]; the first tile of a block of accumulators zeroes them (early clobber)."""
    return [([zero("V[%d]" % c) for c in cs if ks[0] == 0] + [fmac("V[%d]" % c, "D[%d]" % c, "z[%d]" % k, k) for k in ks for c in cs],
             (R("V", cs), R("D", cs) + R("z", ks))) for cs in blocks(n, acc) for ks in blocks(n, src)]


def vjt(n, acc, src):
    """Ps += V J^T: P[c] += bcast_c(z[k]) V[k], in chunks of k; the inputs stand as (z[k], V[k]) pairs."""
    return [([fmac("P[%d]" % c, "z[%d]" % k, "V[%d]" % k, c) for k in ks for c in cs], (R("P", cs), [r % k for k in ks for r in ("z[%d]", "V[%d]")]))
            for cs in blocks(n, acc) for ks in blocks(n, src)]


def member(doc, sig, tiles, decl=""):
    """A member of Sweeps<n>: its doc comment, signature, local registers and one statement per (instructions, operand order)."""
    body = "".join(stmt(code, order) for code, order in tiles)
    return "    // %s\n    static __device__ __forceinline__ void %s\n    {\n%s%s    }\n" % (doc.replace("\n", "\n    // "), sig, decl, body)


def gen(n):
    """struct Sweeps<n>.  n <= 10: every sweep ONE statement (vjt: 15 - n sources a statement, 2 n + 2 (15 - n) = 30 operands), then
    factor_forward and the rank-K pair.  11 <= n <= 16: the five sweeps tiled, 7 sources x 8 accumulators a statement; jd, whose
    accumulators are "+v" from its second tile on, 6 x 8."""
    tiled = n > 10
    src, acc = (7, 8) if tiled else (n, n)
    ref, cref = "double (&%%s)[%d]" % n, "const double (&%%s)[%d]" % n
    s = "template <>\nstruct Sweeps<%d> {\n    static constexpr bool fused = true;\n" % n
    if tiled:
        s += "    static constexpr bool fused_factor = false; // tiled shapes: ldlt_factor, then forward\n    static constexpr int lowrank_max_k = 0;\n"
    s += member("L y = b: z[c] -= L(c,k) y_k, L(c,k) = A[k] of lane c", "forward(%s, %s)" % (ref % "z", cref % "A"), tri(n, src, True))
    s += member("L^T x = y: z[c] -= L(k,c) z_k, L(k,c) = A[c] of lane k", "backward(%s, %s)" % (ref % "z", cref % "A"), tri(n, src, False))
    s += member("acc0 + acc1 += sum_c bcast_c(delta) z[c] (two chains)", "mean(double &acc0, double &acc1, double delta, %s)" % (cref % "z"), mean(n))
    s += member("V = J D (row r): V[c] = sum_k J[r][k] D[k][c], D[k][:] broadcast from lane k",
                "jd(%s, %s, %s)" % (ref % "V", cref % "D", cref % "z"), jd(n, acc, 6 if tiled else n))
    s += member("Ps[r][c] += sum_k V[r][k] J[c][k], J[c][k] broadcast from lane c",
                "vjt(%s, %s, %s)" % (ref % "P", cref % "z", cref % "V"), vjt(n, acc, LIMIT // 2 - acc))
    if tiled:
        return s + "};\n\n"
    # factor_forward: the stream cut into as few statements of <= 30 operands as its order allows, operands in the order of their first appearance
    s += "    static constexpr bool fused_factor = true;\n"
    s += member("stages 1..%d of A = L D L^T with L y = b folded into the pivot chain and z = D^-1 y behind it; stage 0 is the caller's" % (n - 1),
                "factor_forward(%s, %s, %s, double &pivmin)" % (ref % "A", ref % "z", ref % "dinv"), [(st, None) for st in cut(fused_stream(n))],
                "        double piv, e;\n")
    # lowrank / lowrank_apply, one overload per factor count K (N = n - K): the covariance step of a time step at which every
    # series is observed and R = 0, where Pf = B C B^T with B = [-Gamma ; I_K] and so J D J^T = u B^T
    s += "    static constexpr int lowrank_max_k = %d; // rank-K covariance step: overloads for K = 1 .. this\n" % lowrank_max_k(n)
    for K in range(1, lowrank_max_k(n) + 1):
        N, uK = n - K, "double (&u)[%d]" % K
        s += member("N = %d, K = %d: u = J (J_f D)^T (row r), J_f = rows %d.. of J.  Vf[k] of lane c = sum_j D[c][j] J[%d+k][j], then\n"
                    "u[k] = sum_c J[r][c] Vf[k] of lane c" % (N, K, N, N), "lowrank(%s, %s, %s)" % (uK, cref % "D", cref % "z"), lowrank(n, K),
                    "        double Vf[%d]%s;\n" % (K, ", Vb, ub" if K == 1 else ""))
        s += member("Ps[r][:] = Pf[r][:] + (u B^T)[r][:]: P[c] -= u[k] Gamma[c][k], Gamma[c][k] = gam[k] broadcast from lane c < %d; P[%d+k] += u[k]" % (N, N),
                    "lowrank_apply(%s, const %s, const double (&gam)[%d])" % (ref % "P", uK, K), lowrank_apply(n, K))
    return s + "};\n\n"


def render():
    h = ("// mk_sweeps.h -- GENERATED by scripts/gen_sweeps.py (do not edit): the broadcast-FMA sweeps of the 16-lane smoother,\n"
         "// one asm statement per sweep (see the generator for why).  Included by mk_prims.h inside namespace mk.\n"
         "// The DPP source operands of every statement (A, D, delta, z of the LAST sweep) are old values: the callers keep\n"
         "// the two wait states between their producers and the statement (dpp_guard), scripts/check_dpp_hazards.py checks.\n"
         "#pragma once\n\n"
         "template <int n>\nstruct Sweeps {\n    static constexpr bool fused = false; // wider groups: the per-FMA primitives of Group<16>\n"
         "    static constexpr bool fused_factor = false;\n    static constexpr int lowrank_max_k = 0; // no rank-K covariance step\n};\n\n")
    for n in range(2, 11):
        h += gen(n)
    h += ("// 11 <= n <= 16: a statement takes at most 30 operands -- every sweep is tiled into a few statements (blocks of 7\n"
          "// broadcast sources x 7 or 8 accumulators; a block's sources are final before any later tile reads them)\n"
          "#ifndef MK_NO_TILED_SWEEPS\n")
    for n in range(11, 17):
        h += gen(n)
    h += "#endif\n"
    return h


def main():
    open(OUT, "w").write(render())
    print("wrote", os.path.normpath(OUT))


if __name__ == "__main__":
    main()
