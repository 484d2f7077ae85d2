"""Reader of the GENERATED csrc/mk_sweeps.h (scripts/gen_sweeps.py) for the host tests of its sweeps: the asm statements of a
member of ``Sweeps<n>`` parsed from header TEXT into instructions over register names, a numpy emulator of those instructions
(one array element per lane) and the walk of the wait states inside a statement.  A test of a sweep holds its inputs, its
reference and its own assertions; the text is an argument so that the same checks can be run on a mutated copy."""
import importlib.util
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "metran_amd", "csrc", "mk_sweeps.h")).read()
DPP = " row_mask:0xf bank_mask:0xf"
OPS = {"v_fmac_f64_dpp": (2, True), "v_mov_b64_dpp": (1, True), "v_mov_b64": (1, False), "v_rcp_f64": (1, False), "v_add_f64": (2, False),
       "v_mul_f64": (2, False), "v_min_f64": (2, False), "v_fma_f64": (3, False)}    # mnemonic -> (sources, reads src[0] through DPP)


class Ins(namedtuple("Ins", "op dst src lane")):
    """op: the mnemonic; dst: the register written (None: s_nop); src: the sources as written -- a register name, "-name", a
    literal, for s_nop its count; lane: the row_newbcast lane of a DPP instruction, which reads src[0] through DPP, else None.
    v_fmac_f64_dpp d, a, b is d += bcast_lane(a) * b, v_mov_b64_dpp d, a is d = bcast_lane(a)."""

    wait = property(lambda i: i.src[0] + 1 if i.op == "s_nop" else 1)    # wait states it takes
    dpp = property(lambda i: i.src[0] if i.lane is not None else None)
    reads = property(lambda i: {s.lstrip("-") for s in i.src if i.op != "s_nop"} | ({i.dst} if i.op == "v_fmac_f64_dpp" else set()))


def generator():
    spec = importlib.util.spec_from_file_location("gen_sweeps", os.path.join(ROOT, "scripts", "gen_sweeps.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def lowrank_max_k(n):
    return max(0, min(n - 1, 5, (30 - 2 * n) // 2))


def struct(n, text=HEADER):
    a = text.index("struct Sweeps<%d>" % n)
    return text[a:text.index("\n};", a) + 1]


def span(n, fn, K=None, text=HEADER):
    """(start, end) in `text` of Sweeps<n>::fn, from its name to the end of its body; K: the factor count of a `lowrank` or
    `lowrank_apply` overload."""
    sig = {"lowrank": "void lowrank(double (&u)[%s]," % K, "lowrank_apply": "void lowrank_apply(double (&P)[%d], const double (&u)[%s]," % (n, K)}
    a = text.index("struct Sweeps<%d>" % n)
    f = text.index(sig.get(fn, "void %s(" % fn), a, text.index("\n};", a))
    return f, text.index("\n    }\n", f) + 1


def _decode(line):
    m = re.match(r"(\w+) (.*?)( row_newbcast:(\d+)%s)?$" % DPP, line)
    op, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
    if op == "s_nop":
        return Ins(op, None, (int(args[0]),), None)
    assert OPS.get(op) == (len(args) - 1, m.group(3) is not None) and (op != "v_mov_b64" or args[1] == "0"), line
    return Ins(op, args[0], tuple(args[1:]), int(m.group(4)) if m.group(3) else None)


def statements(n=None, fn=None, K=None, text=HEADER):
    """The asm statements of Sweeps<n>::fn (n = None: of the whole text), each a list of `Ins` over register NAMES; every
    statement within the inline-asm operand limit ("+v" counts twice)."""
    a, b = span(n, fn, K, text) if n else (0, len(text))
    out = []
    for st in text[a:b].split("asm volatile(")[1:]:
        st = st[:st.index(");\n")]
        lines = re.findall(r'"([vs]_\w+ [^"]*?)\\n\\t"', st)
        ops = re.findall(r'"([=+&]*v)"\(([\w\[\]]+)\)', st)
        assert len(lines) == st.count("\n") - 2 and 0 < sum(2 if c == "+v" else 1 for c, _ in ops) <= 30, (n, fn, K, st[:120])
        out.append([_decode(re.sub(r"%(\d+)", lambda m: ops[int(m.group(1))][1], ln)) for ln in lines])
    return out


def stream(n, fn, K=None, text=HEADER):
    return [i for st in statements(n, fn, K, text) for i in st]


def lanes(name, M, G=None):
    """{name[c]: column c of M, row r in lane r}; of G lanes, those past the last row replicate it (as in the kernel)."""
    idx = np.minimum(np.arange(G or M.shape[0]), M.shape[0] - 1)
    return {"%s[%d]" % (name, c): M[idx, c].copy() for c in range(M.shape[1])}


def matrix(regs, name, n):
    return np.stack([regs["%s[%d]" % (name, c)] for c in range(n)], axis=1)   # [lane, c]


def _val(regs, s):
    if s.startswith("-"):
        return -regs[s[1:]]
    return float(s) if re.match(r"[\d.]+$", s) else regs[s]


def emulate(code, regs):
    """Runs `code` on regs = {register name: per-lane array}; a register read before anything wrote it is a KeyError."""
    for i in code:
        if i.op == "v_fmac_f64_dpp":
            regs[i.dst] = regs[i.dst] + regs[i.src[0]][i.lane] * _val(regs, i.src[1])
        elif i.op == "v_mov_b64_dpp":
            regs[i.dst] = np.full_like(regs[i.src[0]], regs[i.src[0]][i.lane])
        elif i.op == "v_mov_b64":
            regs[i.dst] = np.zeros_like(next(iter(regs.values())))
        elif i.op == "v_rcp_f64":
            # the hardware's estimate is good to 2^-25; the emulation perturbs the exact quotient so that the refinement has work
            regs[i.dst] = (1.0 / _val(regs, i.src[0])) * (1.0 + 2.0 ** -27)
        elif i.op == "v_min_f64":
            regs[i.dst] = np.minimum(_val(regs, i.src[0]), _val(regs, i.src[1]))
        elif i.op == "v_fma_f64":
            regs[i.dst] = _val(regs, i.src[0]) * _val(regs, i.src[1]) + _val(regs, i.src[2])
        elif i.op in ("v_mul_f64", "v_add_f64"):
            a, b = _val(regs, i.src[0]), _val(regs, i.src[1])
            regs[i.dst] = a * b if i.op == "v_mul_f64" else a + b
    return regs


def walk(code, fresh=(), ctx=()):
    """The wait states inside a stream: yields (instruction, age, writes) for every instruction but s_nop BEFORE it issues --
    age: register -> wait states since its last write (`fresh`: written by the instruction before the stream; absent: old),
    writes: register -> writes so far -- after asserting what holds for every sweep: a DPP source written in the stream is two
    wait states old, a v_rcp_f64 result one before a non-transcendental reads it.  The caller asserts what is its sweep's."""
    age, writes, trans = {r: 0 for r in fresh}, {}, None
    for i in code:
        if i.op != "s_nop":
            assert age.get(i.dpp, 99) >= 2, (ctx, i)
            assert i.op == "v_rcp_f64" or trans not in i.reads, (ctx, i)
            yield i, age, writes
        for r in age:
            age[r] += i.wait
        trans = i.dst if i.op == "v_rcp_f64" else None
        if i.dst:
            age[i.dst] = 0
            writes[i.dst] = writes.get(i.dst, 0) + 1
