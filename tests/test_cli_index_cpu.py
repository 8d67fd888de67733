"""CPU: what the twelve index commands of `bce` (-g -gl -gm -gk -gr -ga and their archive forms) judge before they need a device:
the indexed file or archive, then the second file or the delta, then the device; and the arguments that end in the usage text.
The first line behind the banner and the exit status of each, and no file left in the working directory."""
import os
import struct
import subprocess

import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "bce_amd", "bin", "bce")

NO_FILE = ("Error loading file", 255)
NO_ARCHIVE = ("Archive not found.", 255)
BAD_ARCHIVE = ("Could not read Archive.", 254)
USAGE = ("Usage:", 0)


@pytest.fixture(scope="module")
def box(tmp_path_factory):
    d = tmp_path_factory.mktemp("index_cli")
    files = {
        "text": b"abracadabra" * 100,
        "query": b"cadabraabrac",
        "empty": b"",
        "bad.bcd": b"BCED" + b"\xff" * 70,
        # a well-formed delta without ops against a base of 1100 bytes
        "ok.bcd": b"BCED" + struct.pack("<IQIQIIIQQ", 1, 1100, 0, 0, 0, 16, 256, 0, 0),
    }
    for name, data in files.items():
        (d / name).write_bytes(data)
    work = d / "work"
    work.mkdir()

    def run(*args):
        """(first line behind the banner and its blank line, exit status) of `bce args`, run in an empty directory; a name of
        `files`, or "missing", stands for its path"""
        argv = [str(d / a) if a in files or a == "missing" else str(a) for a in args]
        r = subprocess.run([EXE] + argv, capture_output=True, text=True, cwd=str(work))
        assert os.listdir(str(work)) == [], (args, os.listdir(str(work)))
        lines = r.stdout.split("\n")
        return lines[lines.index("") + 1], r.returncode

    return run


# the arguments of each command in front of and behind the indexed file; "out" is a name in the working directory
PLAIN = {"-g": (("abra",), ()), "-gl": (("abra",), ()), "-gm": ((4,), ("query",)), "-gk": ((2,), ()), "-gr": ((4,), ("query", "out"))}


def _cmd(flag, indexed, in_archive=False):
    front, back = PLAIN[flag]
    return (flag + ("d" if in_archive else ""),) + front + (indexed,) + back


@pytest.mark.parametrize("flag", sorted(PLAIN))
def test_the_indexed_file_or_archive_is_judged_first(box, flag):
    for indexed in ("missing", "empty"):
        assert box(*_cmd(flag, indexed)) == NO_FILE, indexed
    assert box(*_cmd(flag, "missing", True)) == NO_ARCHIVE
    assert box(*_cmd(flag, "empty", True)) == BAD_ARCHIVE


def test_the_indexed_file_is_judged_before_a_second_file_that_is_missing_too(box):
    assert box("-gm", 4, "missing", "missing") == NO_FILE and box("-gmd", 4, "missing", "missing") == NO_ARCHIVE
    assert box("-ga", "missing", "missing", "out") == NO_FILE and box("-ga", "missing", "ok.bcd", "out") == NO_FILE
    assert box("-gad", "missing", "ok.bcd", "out") == NO_ARCHIVE and box("-gad", "empty", "ok.bcd", "out") == BAD_ARCHIVE


@pytest.mark.parametrize("flag,tail", [("-gm", ()), ("-gr", ("out",))])
def test_the_query_is_judged_second(box, flag, tail):
    for query in ("missing", "empty"):
        assert box(flag, 4, "text", query, *tail) == NO_FILE, query
    assert box(flag + "d", 4, "text", "missing", *tail) == NO_FILE


@pytest.mark.parametrize("flag", ["-ga", "-gad"])
def test_the_delta_is_judged_second(box, flag):
    assert box(flag, "text", "missing", "out") == NO_ARCHIVE
    for delta in ("bad.bcd", "query", "empty"):
        assert box(flag, "text", delta, "out") == BAD_ARCHIVE, delta


def test_bounds_outside_their_range_end_in_the_usage_text(box):
    for args in (("-gm", 0, "text", "query"), ("-gm", 4097, "text", "query"), ("-gk", 33, "text"), ("-gr", 0, "text", "query", "out")):
        assert box(*args) == USAGE, args


def _no_device():
    import torch
    return not torch.cuda.is_available()


def test_sound_inputs_miss_the_device_last(box):
    if not _no_device():
        pytest.skip("a device is present: the commands run (tests/test_gpu_cli_*.py)")
    for flag in PLAIN:
        for in_archive in (False, True):                                  # (what an archive holds is read with the device)
            line, code = box(*_cmd(flag, "text", in_archive))
            assert line.startswith("No usable HIP device: ") and code == 253, (flag, in_archive, line, code)
    for flag in ("-ga", "-gad"):
        line, code = box(flag, "text", "ok.bcd", "out")
        assert line.startswith("No usable HIP device: ") and code == 253, (flag, line, code)
