"""CPU: tests/cpp/host_all.h, the host side of libmtr.so as the one translation unit every host-side program of tests/cpp
includes (through harness.h), names every csrc/host_*.cpp -- the files csrc/Makefile builds into the library by wildcard.
The launchers of the animation kernels are weak, so a file missing from the list links all the same and is simply never
run by a harness.  Nothing is compiled here."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_all_lists_every_host_file():
    text = open(os.path.join(ROOT, "tests", "cpp", "host_all.h")).read()
    listed = re.findall(r'^#include "\.\./\.\./mt_renderer_amd/csrc/(host_\w+\.cpp)"$', text, flags=re.M)
    built = [os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "mt_renderer_amd", "csrc", "host_*.cpp"))]
    assert len(listed) == len(set(listed)), listed
    assert set(listed) == set(built), (sorted(set(built) - set(listed)), sorted(set(listed) - set(built)))
