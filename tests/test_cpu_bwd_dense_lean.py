"""xt_bwd_dense_lean_set, the process-wide switch of the table-free Dense backward: the header, the ctypes table of
xingtian_amd/lib.py and the built library agree on it; it returns the previous value, starts at 1 in a fresh process and
refuses anything but 0 or 1 with its name in the message.  (Host words only: nothing is launched.)"""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_ctypes_table_and_library_agree_on_the_entry():
    from xingtian_amd import lib
    header = open(os.path.join(ROOT, "include", "xt_mi355x.h")).read()
    assert re.search(r"\bint\s+xt_bwd_dense_lean_set\s*\(\s*int32_t\s+on\s*\)\s*;", header)
    assert lib.SIGNATURES["xt_bwd_dense_lean_set"] == (ctypes.c_int32, [ctypes.c_int32])
    assert hasattr(lib.load(), "xt_bwd_dense_lean_set") and callable(lib.set_bwd_dense_lean)
    # appended: neither a tuning field nor a new ABI version
    assert "bwd_dense_lean" not in [n for n, _ in lib.Tuning._fields_] and lib.Tuning._fields_[-1][0] == "bwd_fuse21"
    assert int(re.search(r"#define\s+XT_ABI_VERSION\s+(\d+)", header).group(1)) == lib.ABI_VERSION


def test_it_returns_the_previous_value():
    from xingtian_amd import lib
    handle = lib.load()
    first = handle.xt_bwd_dense_lean_set(0)
    try:
        assert first in (0, 1)
        assert handle.xt_bwd_dense_lean_set(1) == 0
        assert handle.xt_bwd_dense_lean_set(1) == 1
        assert handle.xt_bwd_dense_lean_set(0) == 1
        assert lib.set_bwd_dense_lean(True) is False and lib.set_bwd_dense_lean(False) is True
    finally:
        handle.xt_bwd_dense_lean_set(first)


def test_it_refuses_anything_but_0_or_1():
    from xingtian_amd import lib
    handle = lib.load()
    before = handle.xt_bwd_dense_lean_set(1)
    try:
        for bad in (2, -1):
            assert handle.xt_bwd_dense_lean_set(bad) not in (0, 1)
            assert b"xt_bwd_dense_lean_set" in handle.xt_last_error()
            assert handle.xt_bwd_dense_lean_set(1) == 1          # (nothing changed)
            try:
                lib.set_bwd_dense_lean(bad)
            except RuntimeError as e:
                assert "xt_bwd_dense_lean_set" in str(e)
            else:
                raise AssertionError("set_bwd_dense_lean({}) was accepted".format(bad))
    finally:
        handle.xt_bwd_dense_lean_set(before)


def test_the_default_is_1_in_a_fresh_process():
    code = ("import sys; sys.path.insert(0, {!r}); from xingtian_amd import lib; "
            "print('previous', lib.load().xt_bwd_dense_lean_set(1))").format(ROOT)
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True, cwd=ROOT).stdout
    assert "previous 1" in out, out
