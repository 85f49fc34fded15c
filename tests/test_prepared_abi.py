"""The prepared-query entry points at the drop-in boundary (CPU): added to ABI 13 without changing it -- the header
still says 13, the built library exports them, and the ctypes mirror of struct pgpu_prepared_counts has the layout a
C compiler gives the header's."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from pinot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pinot_gpu.h")
PREPARED = ("pgpu_query_prepare", "pgpu_prepared_submit", "pgpu_prepared_counts", "pgpu_prepared_release")


def test_abi_version_is_unchanged():
    text = open(HEADER).read()
    assert re.search(r"^#define PGPU_ABI_VERSION 13$", text, flags=re.M)
    assert _lib.ABI_VERSION == 13 and _lib.load().pgpu_abi_version() == 13


def test_library_exports_the_prepared_entry_points():
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = [n for n, _, _ in _lib.SIGNATURES]
    for name in PREPARED:
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert hasattr(lib, name) and name in names, name


def test_null_arguments_are_refused_without_a_gpu():
    lib = _lib.load()
    out = C.c_void_p(0xBAD0)
    assert lib.pgpu_query_prepare(None, None, None, 0, None, C.byref(out)) == _lib.PGPU_E_INVALID
    assert _lib.last_error() == "null argument" and out.value == 0xBAD0
    assert lib.pgpu_prepared_submit(None, 0, None, 0, C.byref(out)) == _lib.PGPU_E_INVALID
    assert lib.pgpu_prepared_counts(None, C.byref(_lib.PreparedCounts())) == _lib.PGPU_E_INVALID
    assert lib.pgpu_prepared_release(None) == _lib.PGPU_OK


def test_counts_struct_matches_the_c_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    ct = _lib.PreparedCounts
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(struct pgpu_prepared_counts));']
    for fname, _ in ct._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(struct pgpu_prepared_counts, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", str(src), "-o", str(exe)], check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                        text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(ct) == 24
    for fname, _ in ct._fields_:
        assert int(out[fname]) == getattr(ct, fname).offset, fname
