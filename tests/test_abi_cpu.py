"""CPU-side checks of the C-ABI boundary: the shared library loads without a GPU and exports every symbol that
include/mrblip_hip.h declares (no compute calls here)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mr-blip_amd", "csrc", "libmrblip_hip.so")
HDR = os.path.join(ROOT, "include", "mrblip_hip.h")


def _declared():
    txt = open(HDR).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mrblip_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    if not os.path.exists(LIB):
        import sys
        sys.path.insert(0, os.path.join(ROOT, "mr-blip_amd", "csrc"))
        import build
        build.build()
    lib = ctypes.CDLL(LIB)
    names = _declared()
    assert len(names) >= 24
    for n in names:
        assert hasattr(lib, n), n
    lib.mrblip_abi_version.restype = ctypes.c_int
    assert lib.mrblip_abi_version() == 1


def test_python_bindings_cover_the_header():
    from mrblip import ops
    assert sorted(ops.EXPORTS) == _declared()


def test_argument_validation_needs_no_gpu():
    from mrblip import ops
    lib = ops._lib
    # K % 64 != 0 must be rejected before any launch
    rc = ops._gemm(None, 8, None, 8, None, 0, None, 0, 4, 8, 10, None, 8, 0, None, 0, None, None, 0, 0, 0, None, 0, 0.0, 0, None)
    assert rc == -1 and b"K%64" in lib.mrblip_last_error()
    # the batched LoRA entry points check their shapes before any launch (null device pointers never reach a kernel)
    def rows_b(M, R, K, ldx):
        return ops._lora_rows_b(None, ldx, 0, None, K, R * K, M, R, K, None, 64, 64, 2, None, 0, 0, 0.0, None)
    for M, R, K, ldx, what in ((16, 16, 48, 48, b"bad shape"), (16, 40, 64, 64, b"bad shape"), (16, 12, 64, 64, b"bad shape"),
                               (1 << 20, 16, 1024, 1024, b"2 GiB")):
        assert rows_b(M, R, K, ldx) == -1, (M, R, K, ldx)
        assert what in lib.mrblip_last_error(), lib.mrblip_last_error()
    for n in (0, 9):
        jobs = (ops.LoraGradsJob * max(n, 1))()
        assert ops._lora_grads_b(jobs, n, None, None) == -1, n
        assert b"1..8 jobs" in lib.mrblip_last_error(), lib.mrblip_last_error()
    rc = ops._lora_dx_add_b(None, 64, None, 64, 64, None, 12 * 64, 12, 16, 64, 2, None, 0, 0, 0.0, None)
    assert rc == -1 and b"lora_dx_add_batched: bad shape" in lib.mrblip_last_error()


# ---- the header as a C interface: it must compile on its own, and its structs must have the layout of the ctypes mirrors in mrblip.ops
def _c_compilers():
    """(C compiler, C++ compiler) found on this machine; either may be None"""
    import shutil
    clang = "/opt/rocm/lib/llvm/bin/clang"
    clang = clang if os.access(clang, os.X_OK) else shutil.which("clang")
    cc = shutil.which("cc") or shutil.which("gcc") or clang
    cxx = shutil.which("g++") or shutil.which("c++") or (clang + "++" if clang and os.access(clang + "++", os.X_OK) else None)
    return cc, cxx


def test_public_header_compiles_as_c_and_cxx():
    import subprocess
    import pytest
    cc, cxx = _c_compilers()
    if cc is None and cxx is None:
        pytest.skip("no C or C++ compiler on this machine")
    if cc is not None:
        r = subprocess.run([cc, "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", HDR], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    if cxx is not None:
        r = subprocess.run([cxx, "-x", "c++", "-Wall", "-Werror", "-fsyntax-only", HDR], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_header_structs_match_the_ctypes_mirrors(tmp_path):
    """sizeof and every field's offsetof of MrblipLoraGradsJob and mrblip_qformer_layer, compiled from the header, against ctypes.sizeof
    and .offset of ops.LoraGradsJob / ops.QformerLayer: a field added to one copy only would silently corrupt the launch arguments."""
    import subprocess
    import pytest
    from mrblip import ops
    cc, cxx = _c_compilers()
    if cc is None and cxx is None:
        pytest.skip("no C or C++ compiler on this machine")
    mirrors = {"MrblipLoraGradsJob": ops.LoraGradsJob, "mrblip_qformer_layer": ops.QformerLayer}
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "mrblip_hip.h"', "int main(void) {"]
    for cname, mirror in mirrors.items():
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in mirror._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    comp = [cc, "-x", "c", "-std=c99"] if cc is not None else [cxx, "-x", "c++"]
    r = subprocess.run(comp + ["-I", os.path.dirname(HDR), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out if l.strip()}
    for cname, mirror in mirrors.items():
        assert got[(cname, "sizeof")] == ctypes.sizeof(mirror), cname
        for f, _ in mirror._fields_:
            assert got[(cname, f)] == getattr(mirror, f).offset, (cname, f)
