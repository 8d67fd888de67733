"""CPU: what `bce -gs`, `-gsd` and `-gsc` judge before they need a device, in the order of the other index commands
(tests/test_cli_index_cpu.py): the file or archive, then -gsc's array, then the device.  The first line behind the banner and the
exit status of each; no file left behind; the usage text lists the three."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")

NO_FILE = ("Error loading file", 255)
NO_ARCHIVE = ("Archive not found.", 255)
BAD_ARCHIVE = ("Could not read Archive.", 254)


@pytest.fixture(scope="module")
def box(tmp_path_factory):
    d = tmp_path_factory.mktemp("sa_cli")
    files = {
        "text": b"banana",
        "empty": b"",
        "ok.sa": np.array([5, 3, 1, 0, 4, 2], dtype=np.uint32).tobytes(),
        "short.sa": np.array([5, 3, 1, 0, 4], dtype=np.uint32).tobytes(),
        "odd.sa": b"\x05\x00\x00",
        # a container's first twelve bytes and one table entry: enough to be told from a plain archive
        "container": b"BCEM" + (1).to_bytes(4, "little") + (1).to_bytes(4, "little") + (6).to_bytes(8, "little") + (8).to_bytes(8, "little") + bytes(8),
    }
    for name, data in files.items():
        (d / name).write_bytes(data)
    work = d / "work"
    work.mkdir()

    def run(*args):
        argv = [str(d / a) if a in files or a == "missing" else str(a) for a in args]
        r = subprocess.run([EXE] + argv, capture_output=True, text=True, cwd=str(work))
        assert os.listdir(str(work)) == [], (args, os.listdir(str(work)))
        lines = r.stdout.split("\n")
        return lines[lines.index("") + 1], r.returncode

    return run


def test_the_text_or_archive_is_judged_first(box):
    for indexed in ("missing", "empty"):
        assert box("-gs", indexed, "out.sa") == NO_FILE, indexed
        assert box("-gsc", indexed, "ok.sa") == NO_FILE and box("-gsc", indexed, "missing") == NO_FILE, indexed
    assert box("-gsd", "missing", "out.sa") == NO_ARCHIVE
    assert box("-gsd", "empty", "out.sa") == BAD_ARCHIVE


def test_a_container_is_refused_before_the_device(box):
    line, code = box("-gsd", "container", "out.sa")
    assert line.startswith("A container holds separate texts") and code == 254


def test_the_array_is_judged_second(box):
    assert box("-gsc", "text", "missing") == NO_FILE
    for name, size in (("short.sa", 20), ("odd.sa", 3), ("empty", 0), ("text", 6)):
        line, code = box("-gsc", "text", name)
        assert code == 254 and (" %d bytes" % size) in line and " 6 bytes" in line and line.rstrip().endswith(" 24"), (name, line)


def test_sound_inputs_miss_the_device_last(box):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present: the commands run (tests/test_gpu_cli_sa.py)")
    for args in (("-gs", "text", "out.sa"), ("-gsd", "text", "out.sa"), ("-gsc", "text", "ok.sa")):
        line, code = box(*args)
        assert line.startswith("No usable HIP device: ") and code == 253, (args, line, code)


def test_other_argument_counts_end_in_the_usage_text(box):
    for args in (("-gs", "text"), ("-gsc", "text"), ("-gsd", "text"), ("-gs", "text", "out.sa", "more"), ("-gsx", "text", "out.sa")):
        assert box(*args) == ("Usage:", 0), args


def test_the_usage_text_lists_the_three_commands():
    out = subprocess.run([EXE], capture_output=True, text=True).stdout
    for line in ("  bce -gs file out.sa\n", "  bce -gsd archive.bce out.sa\n", "  bce -gsc file in.sa\n"):
        assert line in out, line
