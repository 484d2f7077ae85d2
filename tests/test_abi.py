"""The C-ABI library loads and exports every symbol include/metran_hip.h declares (no compute
calls: this runs without a GPU), and the ctypes binding matches the header."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "metran_hip.h")


def _declared():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"MK_API\s+[\w\s\*]+?\b(mk_\w+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from metran_amd import _lib

    if not os.path.exists(_lib.library_path()):
        g.build()
    return _lib.lib()


def test_header_declares_the_api():
    names = _declared()
    for must in ("mk_create", "mk_filter", "mk_smooth", "mk_filter_smooth", "mk_loglik", "mk_params_from_alpha",
                 "mk_simulate", "mk_decompose", "mk_sum", "mk_last_error"):
        assert must in names


def test_library_exports_every_declared_symbol(lib):
    from metran_amd import _lib

    for name in _declared():
        assert hasattr(lib, name), "libmetran_hip.so does not export %s" % name
    assert sorted(_lib.API) == _declared(), "ctypes binding table and header disagree"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.library_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(_declared()) <= exported
    # nothing but the ABI is exported with default visibility
    assert {e for e in exported if not e.startswith(("mk_", "_init", "_fini", "__hip"))} == set()


def test_struct_layout_matches_header(lib):
    """Field order/count of the ctypes structs equals the C structs (all fields are 8 bytes)."""
    from metran_amd._lib import Outputs, Problem

    src = open(HEADER).read()
    for cname, cls in (("mk_problem", Problem), ("mk_outputs", Outputs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            names = decl.split(",")
            first = re.findall(r"(\w+)\s*$", names[0].strip())[0]
            fields.append(first)
            fields += [re.findall(r"(\w+)\s*$", x.strip())[0] for x in names[1:]]
        assert fields == [f[0] for f in cls._fields_], (cname, fields)
        assert ctypes.sizeof(cls) == 8 * len(fields)


def test_no_gpu_calls_fail_loudly_not_silently(lib):
    """Without a device the context cannot be created and the error is explicit (no CPU fallback)."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    ctx = ctypes.c_void_p()
    rc = lib.mk_create(0, ctypes.byref(ctx))
    assert rc != 0 and not ctx.value
    assert b"device" in lib.mk_last_error().lower() or b"hip" in lib.mk_last_error().lower()
    from metran_amd.engine import BatchedKalman, MetranHipError

    with pytest.raises(MetranHipError):
        BatchedKalman()
    from metran_amd import _lib as binding

    assert lib.mk_abi_version() == binding.ABI_VERSION == 7
    assert lib.mk_shape_supported(8, 2) == 1 and lib.mk_shape_supported(32, 4) == 1
    # (7, 7) has no specialised kernel here (not in the ahead-of-time list, no module registered) and runs the size-generic
    # ones; beyond 128 states nothing serves a shape
    assert lib.mk_shape_specialised(8, 2) == 1 and lib.mk_shape_specialised(7, 7) == 0
    assert lib.mk_shape_supported(7, 7) == 1 and lib.mk_shape_supported(70, 3) == 1 and lib.mk_shape_supported(100, 28) == 1
    assert lib.mk_shape_supported(100, 29) == 0 and lib.mk_generic_max_states() == 128
    assert lib.mk_tape_supported(17, 3) == 0         # the tape needs a specialised module


def test_graft_entry_build_passes():
    """The driver's build check: ``__graft_entry__.build()`` (make is a no-op on a built tree) ends with the ABI and
    shape assertions -- an ABI bump that forgets the entry point shows here, not in the driver's record."""
    import __graft_entry__ as g

    g.build()
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert not re.search(r"mk_abi_version\(\)\s*==\s*\d", src), "hard-coded ABI number in build()"


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: no module of the package may reference it."""
    pkg = os.path.join(ROOT, "metran_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", txt, re.M), f
                assert "kalman_oracle" not in txt, f


def test_shape_module_builds_and_passes_hazard_check(tmp_path, monkeypatch):
    """Run-time specialisation for a shape outside the ahead-of-time list: hipcc cross-compiles the
    module here (no GPU needed), the DPP hazard check runs on its assembly, and it exports the module ABI."""
    monkeypatch.setenv("METRAN_HIP_CACHE", str(tmp_path))
    from metran_amd import jit

    path = jit.build_shape_module(7, 3, out=jit.module_path(7, 3))   # (out=: build it HERE even where build() has prebuilt the shape)
    assert os.path.exists(path) and path == jit.module_path(7, 3) and str(tmp_path) in path
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    # the module ABI: the struct guard and ONE table of the shape's launchers (mk_internal.h: ShapeOps), nothing per entry point
    assert sorted(set(re.findall(r"\bmkmod_\w+", out))) == ["mkmod_abi", "mkmod_ops"]
    for sym in ("mkmod_shape", "mkmod_launch_filter", "mkmod_launch_smoother", "mkmod_launch_adjoint", "mkmod_launch_sparse", "mkmod_launch_loo"):
        assert sym not in out
    assert "filter_kernelILi7ELi3ELi16" in out and "smoother_record_kernelILi7ELi3ELi16" in out
    monkeypatch.setenv("METRAN_HIP_JIT", "0")
    with pytest.raises(jit.ShapeUnavailable):      # not an error of anything: the engine falls back to the size-generic kernels
        jit.build_shape_module(63, 1, out=str(tmp_path / "never.so"))
    # ... while a build that FAILS raises ShapeBuildError and is never a reason to fall back (round-5 advice)
    assert issubclass(jit.ShapeBuildError, jit.MetranHipError) and not issubclass(jit.ShapeBuildError, jit.ShapeUnavailable)


def test_generated_sweeps_header_is_current():
    """metran_amd/csrc/mk_sweeps.h is generated (scripts/gen_sweeps.py) and committed: the committed file must be what
    the generator writes, every statement must respect the 30-operand limit of an asm statement ("+v" counts twice; the
    reader of tests/sweeps_header.py asserts it per statement), and the rank-K overloads are those the operand limit allows."""
    import sweeps_header

    gen = sweeps_header.generator()
    text = gen.render()
    assert open(os.path.join(ROOT, "metran_amd", "csrc", "mk_sweeps.h")).read() == text
    assert len(sweeps_header.statements(text=text)) == text.count("asm volatile(") > 0
    assert [gen.lowrank_max_k(n) for n in range(2, 11)] == [max(0, min(n - 1, 5, (30 - 2 * n) // 2)) for n in range(2, 11)]


def test_kernel_sources_read_no_environment_variable():
    """Round-2 verdict, weak 2: no switch outside the C ABI can select a kernel or change a result (MK_WIDE_TUNE used to);
    phase-skipping timing experiments exist only as the compile-time constant -DMK_TUNE=<mask> of a separate build."""
    src = os.path.join(ROOT, "metran_amd", "csrc")
    for f in sorted(os.listdir(src)):
        if not os.path.isfile(os.path.join(src, f)):
            continue
        text = open(os.path.join(src, f)).read()
        assert "getenv" not in text, f
    assert "MK_TUNE" not in open(os.path.join(src, "Makefile")).read()   # the default build does not define it


def test_tape_geometry_without_a_gpu():
    """MK_OUT_TAPE's sizes (ABI 5) are pure functions: N entries of N + K + 4 doubles per (model, step), served for the shapes
    of the split filter (16 < N + K, N <= 32) that have a kernel; the numpy restatement unpacks the same geometry."""
    import sys

    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dk_ref
    from metran_amd import _lib

    L = _lib.lib()
    assert L.mk_tape_stride(32, 4) == 32 * 40 == 1280 and L.mk_tape_stride(14, 3) == 14 * 21
    assert L.mk_tape_supported(32, 4) == 1 and L.mk_tape_supported(14, 3) == 1
    assert L.mk_tape_supported(8, 2) == 0            # n <= 16: the 16-lane kernels
    assert L.mk_tape_supported(48, 3) == 0           # served (round 5: up to 63 states) once the shape's module is registered
    assert L.mk_tape_supported(61, 3) == 0           # rows 0..n-1 and the r row: n + 1 <= 64
    # the STATE tape (ABI 6, MK_OUT_TAPE | MK_OUT_VAR_ONLY): K more entries per block
    assert L.mk_state_tape_stride(32, 4) == 36 * 40 and L.mk_state_tape_stride(14, 3) == 17 * 21
    blk = np.arange(14 * 21, dtype=float)
    e = dk_ref.unpack_block(blk, 14, 3)
    assert e.shape == (14, 21) and e[3, 0] == 3 * 21 and e[3, 14] == 3 * 21 + 14 and e[13, 20] == 14 * 21 - 1


def test_allreduce_fails_loudly_without_a_communicator(lib):
    """SURVEY 8b's collective hook (``mk_allreduce_sum`` / ``mk_set_communicator``): no context, no communicator or a bad
    buffer are explicit errors -- there is no silent single-rank shortcut.  No GPU, no process group and no gloo needed:
    the null-context checks come before any HIP or RCCL call."""
    buf = (ctypes.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    assert lib.mk_allreduce_sum(None, ctypes.cast(buf, ctypes.c_void_p), 4) != 0
    assert b"null mk_context" in lib.mk_last_error()
    assert lib.mk_set_communicator(None, None) != 0 and b"null mk_context" in lib.mk_last_error()
    assert lib.mk_comm_destroy(None) != 0
    assert lib.mk_comm_init_rank(None, 1, 0, ctypes.cast(buf, ctypes.c_void_p)) != 0
    assert lib.mk_comm_unique_id(None) != 0 and b"128" in lib.mk_last_error()
    assert list(buf) == [1.0, 2.0, 3.0, 4.0]          # untouched
    # the binding layer refuses too: an engine without a communicator raises instead of returning its input
    src = open(os.path.join(ROOT, "metran_amd", "csrc", "mk_capi.hip")).read()
    assert "no single-rank shortcut" in src and "dlopen" in src   # librccl is bound at first use, never linked
    out = subprocess.check_output(["ldd", os.path.join(ROOT, "metran_amd", "libmetran_hip.so")], text=True)
    assert "rccl" not in out, "libmetran_hip.so must not depend on librccl at load time"


def test_adjoint_update_tape_geometry_without_a_gpu(lib):
    """mk_adjoint_update_stride is a pure function (round 6: N slots of n rounded up to even + 2 doubles per model-step for the wide
    shapes, 0 for the 16-lane ones); attaching a tape to no context fails loudly."""
    assert lib.mk_adjoint_update_stride(32, 4) == 32 * 38 and lib.mk_adjoint_update_stride(14, 3) == 14 * 20
    assert lib.mk_adjoint_update_stride(48, 3) == 48 * 54 and lib.mk_adjoint_update_stride(8, 2) == 0
    assert lib.mk_adjoint_update_stride(64, 1) == 0 and lib.mk_adjoint_update_stride(0, 4) == 0
    assert lib.mk_set_adjoint_updates(None, None, 0) != 0 and b"null mk_context" in lib.mk_last_error()
