#!/usr/bin/env python3
"""Writes metran_amd/csrc/mk_sweeps.h: the DPP broadcast-FMA sweeps of the 16-lane smoother as ONE asm statement each.

Why: hipcc's hazard recogniser counts an inline-asm statement as zero wait states and assumes every asm result needs
one before another asm statement may touch it, so a sweep written as one statement per v_fmac_f64_dpp gets an
`s_nop 0` at every sweep boundary (the next sweep's first FMA accumulates into a register the previous sweep's
statements wrote): 31 per step of smoother_record_kernel<8,2>, each a full issue slot.  A statement may have at
most 30 operands ("+v" counts twice): for n <= 10 every sweep is ONE statement; for 11 <= n <= 16 (round 3) a sweep is
TILED into statements of <= 30 operands -- blocks of 7 broadcast sources x 7 or 8 accumulators, ordered so that every
value is final before it is read -- 3 to 6 statements (= padding nops) per sweep instead of one per FMA."""
import os

DPP = " row_mask:0xf bank_mask:0xf"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "metran_amd", "csrc", "mk_sweeps.h")


def stmt(lines, outs, ins, indent="        "):
    body = "\n".join('%s    "%s\\n\\t"' % (indent, l) for l in lines)
    return "%sasm volatile(\n%s\n%s    : %s\n%s    : %s);\n" % (indent, body, indent, ", ".join(outs), indent, ", ".join(ins) if ins else "")


class Ins:
    """One instruction of the fused factor-and-forward stream over SYMBOLIC registers (A[c], z[c], dinv[c], pivmin, piv, e):
    `fmt` takes the registers `regs` in order; `dpp` is the register read through DPP (src0), `trans` a transcendental."""

    def __init__(self, fmt, regs, writes, reads, dpp=None, trans=False):
        self.fmt, self.regs, self.writes, self.reads, self.dpp, self.trans = fmt, regs, writes, reads, dpp, trans


def _fmac(acc, src, mul, lane):
    return Ins("v_fmac_f64_dpp {0}, {1}, -{2} row_newbcast:%d%s" % (lane, DPP), [acc, src, mul], acc, {acc, src, mul}, dpp=src)


def _scale(c):
    return Ins("v_mul_f64 {0}, {0}, {1}", ["z[%d]" % c, "dinv[%d]" % c], "z[%d]" % c, {"z[%d]" % c, "dinv[%d]" % c})


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
    age = {}            # register -> wait states since its last VALU write (absent: old)
    last_trans = [None]
    out = []

    def emit(i):
        out.append(i)
        for r in list(age):
            age[r] += 1
        age[i.writes] = 0
        last_trans[0] = i.writes if i.trans else None

    def nop(k):
        out.append(Ins("s_nop %d" % (k - 1), [], None, set()))
        for r in list(age):
            age[r] += k
        last_trans[0] = None

    def ready(i):
        return (i.dpp is None or age.get(i.dpp, 99) >= 2) and not (last_trans[0] in i.reads and not i.trans)

    def must(i):
        need = 0
        if i.dpp is not None:
            need = max(need, 2 - age.get(i.dpp, 99))
        if last_trans[0] in i.reads and not i.trans:
            need = max(need, 1)
        if need > 0:
            nop(need)
        emit(i)

    age["A[0]"] = 0
    pool = []           # columns whose y_c the substitution has passed: z[c] may take its D^-1
    for j in range(1, n):
        lr, y, a, d = "A[%d]" % (j - 1), "z[%d]" % (j - 1), "A[%d]" % j, "dinv[%d]" % j
        if j >= 2:
            pool.append(j - 2)
        fills = [_fmac("A[%d]" % c, "A[%d]" % c, lr, j - 1) for c in range(j + 1, n)]
        fills += [_fmac("z[%d]" % c, lr, y, c) for c in range(j, n)]
        chain = [Ins("v_mov_b64_dpp {0}, {1} row_newbcast:%d%s" % (j, DPP), ["piv", a], "piv", {a}, dpp=a),
                 Ins("v_rcp_f64 {0}, {1}", [d, "piv"], d, {"piv"}, trans=True),
                 Ins("v_fma_f64 {0}, -{1}, {2}, 1.0", ["e", "piv", d], "e", {"piv", d}),
                 Ins("v_fma_f64 {0}, {0}, {0}, {0}", ["e"], "e", {"e"}),
                 Ins("v_fma_f64 {0}, {0}, {1}, {0}", [d, "e"], d, {d, "e"})]
        if j < n - 1:
            chain.append(Ins("v_mul_f64 {0}, {0}, {1}", [a, d], a, {a, d}))
        vmin = Ins("v_min_f64 {0}, {0}, {1}", ["pivmin", "piv"], "pivmin", {"pivmin", "piv"})
        take = min(len(pool), max(0, FILL_WANT - len(fills)))
        fills += [_scale(pool.pop(0)) for _ in range(take)]
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
        must(_fmac(a, a, lr, j - 1))
        for g in range(len(want)):
            for _ in range(want[g]):
                pick = next((f for f in fills if ready(f)), fills[0])
                fills.remove(pick)
                must(pick)
            if g < len(chain):
                must(chain[g])
                if chain[g].trans:
                    emit(vmin)
        assert not fills
    for c in pool + [n - 2, n - 1]:     # y_{n-2} and y_{n-1} are final only now
        must(_scale(c))
    return out


def operands(ins_list):
    """(register, constraint) of one statement: read before written -> "v" / "+v", written first -> "=&v"."""
    order, first_read, written = [], set(), set()
    for i in ins_list:
        for r in i.regs:
            if r not in order:
                order.append(r)
        for r in i.reads:
            if r not in written:
                first_read.add(r)
        if i.writes:
            written.add(i.writes)
    ops = [(r, "+v" if r in first_read else "=&v") for r in order if r in written]
    ops += [(r, "v") for r in order if r not in written]
    return ops


def op_count(ops):
    return sum(2 if c == "+v" else 1 for _, c in ops)


def gen_fused(n):
    """Sweeps<n>::factor_forward: the stream cut into as few statements of <= 30 operands as its order allows."""
    stream, stmts, cur = fused_stream(n), [], []
    for i in stream:
        if cur and op_count(operands(cur + [i])) > 30:
            stmts.append(cur)
            cur = []
        cur.append(i)
    stmts.append(cur)
    s = "    static constexpr bool fused_factor = true;\n"
    s += "    // stages 1..%d of A = L D L^T with L y = b folded into the pivot chain and z = D^-1 y behind it; stage 0 is the caller's\n" % (n - 1)
    s += "    static __device__ __forceinline__ void factor_forward(double (&A)[%d], double (&z)[%d], double (&dinv)[%d], double &pivmin)\n    {\n" % (n, n, n)
    s += "        double piv, e;\n"
    for st in stmts:
        ops = operands(st)
        idx = {r: "%%%d" % k for k, (r, _) in enumerate(ops)}
        lines = [i.fmt.format(*[idx[r] for r in i.regs]) for i in st]
        outs = ['"%s"(%s)' % (c, r) for r, c in ops if c != "v"]
        ins = ['"v"(%s)' % r for r, c in ops if c == "v"]
        s += stmt(lines, outs, ins)
    s += "    }\n"
    return s


LOWRANK_MAX_K = 5  # factors the rank-K covariance step is generated for (and 2n + 2K <= 30 operands)


def lowrank_max_k(n):
    return max(0, min(n - 1, LOWRANK_MAX_K, (30 - 2 * n) // 2))


def lowrank_lines(n, K):
    """u = J (J_f D)^T over SYMBOLIC registers (u[k], Vf[k] / the split chains of K = 1, D[j], z[j]): (text, written, DPP source).
    K chains run interleaved; K = 1 splits its one chain of n into two (even / odd terms) and adds them.  The zeroing of u stands
    BETWEEN the two products: with the other chains' last multiply-adds it gives Vf[k] its two wait states before the second
    product reads it through DPP."""
    N, out = n - K, []
    if K == 1:
        va, vb, ua, ub = "Vf[0]", "Vb", "u[0]", "ub"
        out += [("v_mov_b64 {%s}, 0" % r, r, None) for r in (va, vb)]
        out += [("v_fmac_f64_dpp {%s}, {z[%d]}, {D[%d]} row_newbcast:%d%s" % ((va, vb)[j % 2], j, j, N, DPP), (va, vb)[j % 2], "z[%d]" % j)
                for j in range(n)]
        out += [("v_add_f64 {%s}, {%s}, {%s}" % (va, va, vb), va, None)]
        out += [("v_mov_b64 {%s}, 0" % r, r, None) for r in (ua, ub)]
        out += [("v_fmac_f64_dpp {%s}, {%s}, {z[%d]} row_newbcast:%d%s" % ((ua, ub)[c % 2], va, c, c, DPP), (ua, ub)[c % 2], va) for c in range(n)]
        out += [("v_add_f64 {%s}, {%s}, {%s}" % (ua, ua, ub), ua, None)]
        return out
    out += [("v_mov_b64 {Vf[%d]}, 0" % k, "Vf[%d]" % k, None) for k in range(K)]
    out += [("v_fmac_f64_dpp {Vf[%d]}, {z[%d]}, {D[%d]} row_newbcast:%d%s" % (k, j, j, N + k, DPP), "Vf[%d]" % k, "z[%d]" % j)
            for j in range(n) for k in range(K)]
    out += [("v_mov_b64 {u[%d]}, 0" % k, "u[%d]" % k, None) for k in range(K)]
    out += [("v_fmac_f64_dpp {u[%d]}, {Vf[%d]}, {z[%d]} row_newbcast:%d%s" % (k, k, c, c, DPP), "u[%d]" % k, "Vf[%d]" % k)
            for c in range(n) for k in range(K)]
    return out


def gen_lowrank(n):
    """Sweeps<n>::lowrank / lowrank_apply, one overload per factor count K (N = n - K): the covariance step of a time step at
    which every series is observed and R = 0, where Pf = B C B^T with B = [-Gamma ; I_K] and so J D J^T = u B^T."""
    s = "    static constexpr int lowrank_max_k = %d; // rank-K covariance step: overloads for K = 1 .. this\n" % lowrank_max_k(n)
    for K in range(1, lowrank_max_k(n) + 1):
        N = n - K
        lines, age = [], {}
        for ln in lowrank_lines(n, K):  # a DPP source written inside the statement is two wait states old: pad where it is not
            need = 2 - age.get(ln[2], 99) if ln[2] else 0
            if need > 0:
                lines.append(("s_nop %d" % (need - 1), None, None))
            age = {r: a_ + max(need, 0) + 1 for r, a_ in age.items()}
            age[ln[1]] = 0
            lines.append(ln)
        tmps = ["Vf[0]", "Vb", "ub"] if K == 1 else ["Vf[%d]" % k for k in range(K)]
        regs = ["u[%d]" % k for k in range(K)] + tmps + ["D[%d]" % c for c in range(n)] + ["z[%d]" % c for c in range(n)]
        idx = {r: "%%%d" % i for i, r in enumerate(regs)}
        text = [ln[0] for ln in lines]
        for r in sorted(idx, key=len, reverse=True):
            text = [t.replace("{%s}" % r, idx[r]) for t in text]
        s += "    // N = %d, K = %d: u = J (J_f D)^T (row r), J_f = rows %d.. of J.  Vf[k] of lane c = sum_j D[c][j] J[%d+k][j], then\n" % (N, K, N, N)
        s += "    // u[k] = sum_c J[r][c] Vf[k] of lane c\n"
        s += "    static __device__ __forceinline__ void lowrank(double (&u)[%d], const double (&D)[%d], const double (&z)[%d])\n    {\n" % (K, n, n)
        s += "        double Vf[%d]%s;\n" % (K, ", Vb, ub" if K == 1 else "")
        s += stmt(text, ['"=&v"(%s)' % r for r in regs[:K + len(tmps)]], ['"v"(%s)' % r for r in regs[K + len(tmps):]])
        s += "    }\n"
        # P[c] -= u[k] Gamma[c][k] (Gamma[c][k] = gam[k] of lane c < N), P[N+k] += u[k]     (operands: P 0..n-1, u, gam)
        text = ["v_fmac_f64_dpp %%%d, %%%d, -%%%d row_newbcast:%d%s" % (c, n + K + k, n + k, c, DPP) for k in range(K) for c in range(N)]
        text += ["v_add_f64 %%%d, %%%d, %%%d" % (N + k, N + k, n + k) for k in range(K)]
        s += "    // Ps[r][:] = Pf[r][:] + (u B^T)[r][:]: P[c] -= u[k] Gamma[c][k], Gamma[c][k] = gam[k] broadcast from lane c < %d; P[%d+k] += u[k]\n" % (N, N)
        s += "    static __device__ __forceinline__ void lowrank_apply(double (&P)[%d], const double (&u)[%d], const double (&gam)[%d])\n    {\n" % (n, K, K)
        s += stmt(text, ['"+v"(P[%d])' % c for c in range(n)], ['"v"(u[%d])' % k for k in range(K)] + ['"v"(gam[%d])' % k for k in range(K)])
        s += "    }\n"
    return s


def gen(n):
    s = "template <>\nstruct Sweeps<%d> {\n    static constexpr bool fused = true;\n" % n
    # forward substitution: z[c] -= bcast_c(A[k]) z[k], k = 0..n-2, c = k+1..n-1     (operands: z 0..n-1, A n..2n-2)
    lines = ["v_fmac_f64_dpp %%%d, %%%d, -%%%d row_newbcast:%d%s" % (c, n + k, k, c, DPP) for k in range(n - 1) for c in range(k + 1, n)]
    s += "    // L y = b: z[c] -= L(c,k) y_k, L(c,k) = A[k] of lane c\n"
    s += "    static __device__ __forceinline__ void forward(double (&z)[%d], const double (&A)[%d])\n    {\n" % (n, n)
    s += stmt(lines, ['"+v"(z[%d])' % c for c in range(n)], ['"v"(A[%d])' % k for k in range(n - 1)]) if lines else ""
    s += "    }\n"
    # backward substitution: z[c] -= bcast_k(A[c]) z[k], k = n-1..1, c = 0..k-1
    lines = ["v_fmac_f64_dpp %%%d, %%%d, -%%%d row_newbcast:%d%s" % (c, n + c, k, k, DPP) for k in range(n - 1, 0, -1) for c in range(k)]
    s += "    // L^T x = y: z[c] -= L(k,c) z_k, L(k,c) = A[c] of lane k\n"
    s += "    static __device__ __forceinline__ void backward(double (&z)[%d], const double (&A)[%d])\n    {\n" % (n, n)
    s += stmt(lines, ['"+v"(z[%d])' % c for c in range(n)], ['"v"(A[%d])' % c for c in range(n - 1)]) if lines else ""
    s += "    }\n"
    # smoothed mean: acc0 / acc1 += bcast_c(delta) z[c]           (operands: acc0 0, acc1 1, delta 2, z 3..)
    lines = ["v_fmac_f64_dpp %%%d, %%2, %%%d row_newbcast:%d%s" % (c % 2, 3 + c, c, DPP) for c in range(n)]
    s += "    // acc0 + acc1 += sum_c bcast_c(delta) z[c] (two chains)\n"
    s += "    static __device__ __forceinline__ void mean(double &acc0, double &acc1, double delta, const double (&z)[%d])\n    {\n" % n
    s += stmt(lines, ['"+v"(acc0)', '"+v"(acc1)'], ['"v"(delta)'] + ['"v"(z[%d])' % c for c in range(n)])
    s += "    }\n"
    # V = J D: V[c] = sum_k bcast_k(D[c]) z[k]                    (operands: V 0..n-1 (early clobber), D n.., z 2n..)
    lines = ["v_mov_b64 %%%d, 0" % c for c in range(n)]
    lines += ["v_fmac_f64_dpp %%%d, %%%d, %%%d row_newbcast:%d%s" % (c, n + c, 2 * n + k, k, DPP) for k in range(n) for c in range(n)]
    s += "    // V = J D (row r): V[c] = sum_k J[r][k] D[k][c], D[k][:] broadcast from lane k\n"
    s += "    static __device__ __forceinline__ void jd(double (&V)[%d], const double (&D)[%d], const double (&z)[%d])\n    {\n" % (n, n, n)
    s += stmt(lines, ['"=&v"(V[%d])' % c for c in range(n)], ['"v"(D[%d])' % c for c in range(n)] + ['"v"(z[%d])' % k for k in range(n)])
    s += "    }\n"
    # Ps += V J^T: P[c] += bcast_c(z[k]) V[k], in chunks of k      (operands: P 0..n-1, then (z[k], V[k]) pairs)
    m = max(1, (30 - 2 * n) // 2)
    s += "    // Ps[r][c] += sum_k V[r][k] J[c][k], J[c][k] broadcast from lane c\n"
    s += "    static __device__ __forceinline__ void vjt(double (&P)[%d], const double (&z)[%d], const double (&V)[%d])\n    {\n" % (n, n, n)
    for k0 in range(0, n, m):
        ks = list(range(k0, min(n, k0 + m)))
        lines = ["v_fmac_f64_dpp %%%d, %%%d, %%%d row_newbcast:%d%s" % (c, n + 2 * i, n + 2 * i + 1, c, DPP) for i, k in enumerate(ks) for c in range(n)]
        ins = []
        for k in ks:
            ins += ['"v"(z[%d])' % k, '"v"(V[%d])' % k]
        s += stmt(lines, ['"+v"(P[%d])' % c for c in range(n)], ins)
    s += "    }\n" + gen_fused(n) + gen_lowrank(n) + "};\n\n"
    return s


def blocks(n, size):
    return [list(range(i, min(n, i + size))) for i in range(0, n, size)]


def gen_tiled(n):
    """11 <= n <= 16: the same five sweeps, each as a short sequence of <= 30-operand statements."""
    s = "template <>\nstruct Sweeps<%d> {\n    static constexpr bool fused = true;\n    static constexpr bool fused_factor = false; // tiled shapes: ldlt_factor, then forward\n    static constexpr int lowrank_max_k = 0;\n" % n
    KB = blocks(n, 7)

    def tri(forward):
        out = ""
        order = KB if forward else KB[::-1]
        for kb in order:
            # diagonal tile: sources and accumulators inside the block
            if forward:
                pairs = [(k, c) for k in kb for c in kb if c > k]            # z[c] -= bcast_c(A[k]) z[k]
            else:
                pairs = [(k, c) for k in kb[::-1] for c in kb if c < k]      # z[c] -= bcast_k(A[c]) z[k]
            if pairs:
                zs = sorted({c for _, c in pairs} | {k for k, _ in pairs})
                As = sorted({(k if forward else c) for k, c in pairs})
                zi = {c: i for i, c in enumerate(zs)}
                ai = {k: len(zs) + i for i, k in enumerate(As)}
                lines = ["v_fmac_f64_dpp %%%d, %%%d, -%%%d row_newbcast:%d%s" % (zi[c], ai[k if forward else c], zi[k], c if forward else k, DPP)
                         for k, c in pairs]
                assert 2 * len(zs) + len(As) <= 30
                out += stmt(lines, ['"+v"(z[%d])' % c for c in zs], ['"v"(A[%d])' % k for k in As])
            # off-diagonal tiles: this block's (final) sources into the accumulators of the blocks still to come
            rest = [c for c in range(n) if (c > kb[-1] if forward else c < kb[0])]
            for cb in blocks(len(rest), 8):
                cs = [rest[i] for i in cb]
                pairs = [(k, c) for k in (kb if forward else kb[::-1]) for c in cs]
                zi = {c: i for i, c in enumerate(cs)}
                ki = {k: len(cs) + i for i, k in enumerate(kb)}
                As = sorted({(k if forward else c) for k, c in pairs})
                ai = {a_: len(cs) + len(kb) + i for i, a_ in enumerate(As)}
                lines = ["v_fmac_f64_dpp %%%d, %%%d, -%%%d row_newbcast:%d%s" % (zi[c], ai[k if forward else c], ki[k], c if forward else k, DPP)
                         for k, c in pairs]
                assert 2 * len(cs) + len(kb) + len(As) <= 30, (n, len(cs), len(kb), len(As))
                out += stmt(lines, ['"+v"(z[%d])' % c for c in cs], ['"v"(z[%d])' % k for k in kb] + ['"v"(A[%d])' % a_ for a_ in As])
        return out

    s += "    // L y = b: z[c] -= L(c,k) y_k, L(c,k) = A[k] of lane c\n"
    s += "    static __device__ __forceinline__ void forward(double (&z)[%d], const double (&A)[%d])\n    {\n" % (n, n)
    s += tri(True) + "    }\n"
    s += "    // L^T x = y: z[c] -= L(k,c) z_k, L(k,c) = A[c] of lane k\n"
    s += "    static __device__ __forceinline__ void backward(double (&z)[%d], const double (&A)[%d])\n    {\n" % (n, n)
    s += tri(False) + "    }\n"
    lines = ["v_fmac_f64_dpp %%%d, %%2, %%%d row_newbcast:%d%s" % (c % 2, 3 + c, c, DPP) for c in range(n)]
    s += "    // acc0 + acc1 += sum_c bcast_c(delta) z[c] (two chains)\n"
    s += "    static __device__ __forceinline__ void mean(double &acc0, double &acc1, double delta, const double (&z)[%d])\n    {\n" % n
    s += stmt(lines, ['"+v"(acc0)', '"+v"(acc1)'], ['"v"(delta)'] + ['"v"(z[%d])' % c for c in range(n)])
    s += "    }\n"
    # V = J D: tiles of 8 accumulators x 6 sources (first tile of a column block zeroes its accumulators)
    s += "    // V = J D (row r): V[c] = sum_k J[r][k] D[k][c], D[k][:] broadcast from lane k\n"
    s += "    static __device__ __forceinline__ void jd(double (&V)[%d], const double (&D)[%d], const double (&z)[%d])\n    {\n" % (n, n, n)
    for cs in blocks(n, 8):
        for bi, ks in enumerate(blocks(n, 6)):
            vi = {c: i for i, c in enumerate(cs)}
            di = {c: len(cs) + i for i, c in enumerate(cs)}
            zi = {k: 2 * len(cs) + i for i, k in enumerate(ks)}
            lines = (["v_mov_b64 %%%d, 0" % vi[c] for c in cs] if bi == 0 else [])
            lines += ["v_fmac_f64_dpp %%%d, %%%d, %%%d row_newbcast:%d%s" % (vi[c], di[c], zi[k], k, DPP) for k in ks for c in cs]
            outs = ['"%s"(V[%d])' % ("=&v" if bi == 0 else "+v", c) for c in cs]
            assert (1 if bi == 0 else 2) * len(cs) + len(cs) + len(ks) <= 30
            s += stmt(lines, outs, ['"v"(D[%d])' % c for c in cs] + ['"v"(z[%d])' % k for k in ks])
    s += "    }\n"
    s += "    // Ps[r][c] += sum_k V[r][k] J[c][k], J[c][k] broadcast from lane c\n"
    s += "    static __device__ __forceinline__ void vjt(double (&P)[%d], const double (&z)[%d], const double (&V)[%d])\n    {\n" % (n, n, n)
    for cs in blocks(n, 8):
        for ks in blocks(n, 7):
            pi = {c: i for i, c in enumerate(cs)}
            lines = ["v_fmac_f64_dpp %%%d, %%%d, %%%d row_newbcast:%d%s" % (pi[c], len(cs) + 2 * i, len(cs) + 2 * i + 1, c, DPP)
                     for i, k in enumerate(ks) for c in cs]
            ins = []
            for k in ks:
                ins += ['"v"(z[%d])' % k, '"v"(V[%d])' % k]
            assert 2 * len(cs) + 2 * len(ks) <= 30
            s += stmt(lines, ['"+v"(P[%d])' % c for c in cs], ins)
    s += "    }\n};\n\n"
    return s


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
        h += gen_tiled(n)
    h += "#endif\n"
    return h


def main():
    open(OUT, "w").write(render())
    print("wrote", os.path.normpath(OUT))


if __name__ == "__main__":
    main()
