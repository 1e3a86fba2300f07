"""The binding's table (tools/host_kernel.py _API) against what tools/libhostkernel.so really exports: every hk_* export is in the table and every
table entry is exported, so an entry added to the host build without its types -- or left in the table after it went -- fails here.  No GPU."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


@pytest.fixture(scope="module")
def exported(hk):
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm is not installed")
    out = subprocess.run([nm, "-D", "--defined-only", hk.build()], check=True, capture_output=True, text=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("hk_"))


def test_every_export_is_in_the_table(hk, exported):
    assert exported, "the library exports no hk_* name"
    assert [n for n in exported if n not in hk.API_SYMBOLS] == []


def test_every_table_entry_is_exported(hk, exported):
    assert [n for n in hk.API_SYMBOLS if n not in exported] == []
    assert len(set(hk.API_SYMBOLS)) == len(hk.API_SYMBOLS)


def test_every_entry_states_its_types(hk):
    """no entry is left to ctypes' defaults, and lib() is the table applied"""
    L = hk.lib()
    for name, res, args in hk._API:
        assert isinstance(args, list), name
        f = getattr(L, name)
        assert f.restype is res and list(f.argtypes) == args, name
