"""CPU: the device-resident decoder entry points (bce_hip_decompress_to_device, bce_hip_verify_device, bce_hip_verify_host) are
exported, declared and bound, refuse null arguments before they touch a device, and `bce` documents `-t` (no GPU touched)."""
import ctypes as C
import os
import re
import subprocess

import bce_amd
from bce_amd import api
from conftest import ROOT

NEW = ("bce_hip_decompress_to_device", "bce_hip_verify_device", "bce_hip_verify_host")
E_ARG = -1


def test_the_three_symbols_are_exported_declared_and_bound():
    lib = C.CDLL(bce_amd.library_path())
    src = open(os.path.join(ROOT, "include", "bce_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    bound = {n: (r, a) for n, r, a in api.SYMBOLS}
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == 6, name
    for name in ("decompress_to_device", "verify_device", "verify"):
        assert callable(getattr(bce_amd, name)), name


def test_null_context_and_null_archive_are_argument_errors():
    lib = bce_amd.load_library()
    arch = (C.c_uint8 * 16)()
    orig = (C.c_uint8 * 16)()
    n = C.c_size_t(0)
    fd = C.c_uint64(7)
    a = C.addressof(arch)
    for archive in (a, None):           # a null context, with and without a null archive beside it
        assert lib.bce_hip_decompress_to_device(None, archive, 16, None, 0, C.byref(n)) == E_ARG
        assert lib.bce_hip_verify_device(None, archive, 16, None, 0, C.byref(fd)) == E_ARG
        assert lib.bce_hip_verify_host(None, archive, 16, C.addressof(orig), 16, C.byref(fd)) == E_ARG
    assert fd.value == 7                 # nothing reported
    # (a null archive in a live context: tests/test_gpu_device_decode.py -- a context needs a device)


def test_usage_has_the_test_paragraph_after_the_scan_one():
    exe = os.path.join(ROOT, "bce_amd", "bin", "bce")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0
    out = r.stdout
    assert "  bce -t file archive.bce\n   Tests archive \"archive.bce\" against \"file\"" in out
    assert "exit status 0 = equal, 1 = differs" in out
    assert out.index("  bce -s config.bcc file\n") < out.index("  bce -t file archive.bce\n")
    # what was there stays as it was
    for line in ("  bce -c archive.bce file [config.bcc]\n", "  bce -d file archive.bce\n", "  bce -s config.bcc file\n", "  bce -cN archive.bcem file [config.bcc]"):
        assert line in out
