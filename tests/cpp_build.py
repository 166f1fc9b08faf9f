"""Builds one stand-alone program of tests/cpp with g++, for the drivers of this directory.  A plain module: no fixtures, no
plugins.  The programs have a main of their own and run as they are; nothing here touches the environment.

The flag sets, by what a program is:
  HOST_ASAN   the host side of the library over tests/cpp/hip_stub, under AddressSanitizer and UBSan
  HOST_TSAN   the same under ThreadSanitizer
  EXACT       kernel arithmetic bit for bit over the stub: no contraction, every warning an error
  BARE        integer arithmetic checked exhaustively: optimised, nothing else
  CLIENT      a program against the public headers, linked with the built libmtr.so
What only some programs of a kind need goes in `extra`."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIB_DIR = os.path.join(ROOT, "mt_renderer_amd")
STD = "-std=c++17"
_STUB = ["-I", os.path.join(CPP, "hip_stub")]
_HOST = _STUB + ["-I", os.path.join(ROOT, "include")]

# (flags in front of the source, libraries behind it)
HOST_ASAN = ([STD, "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + _HOST, ["-lz"])
HOST_TSAN = ([STD, "-O1", "-g", "-fsanitize=thread", "-w"] + _HOST, ["-lz", "-pthread"])
EXACT = ([STD, "-O2", "-ffp-contract=off", "-Wall", "-Werror"] + _STUB, [])
BARE = ([STD, "-O2"], [])
CLIENT = ([STD, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")], ["-L", LIB_DIR, "-lmtr", "-Wl,-rpath," + LIB_DIR])


def build(program, out_dir, flags, extra=(), exe=None):
    """tests/cpp/<program>.cpp compiled into out_dir; returns the executable's path (named `exe`, or after the program).
    Skips the calling test where there is no g++."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    front, libs = flags
    out = os.path.join(str(out_dir), exe or program)
    subprocess.check_call(["g++", *front, *extra, os.path.join(CPP, program + ".cpp"), "-o", out, *libs])
    return out
