"""CPU: the HOST side of motion matching (mtr_anim_match_create / _destroy, mtr_anim_match_search_device, _search_host and
_scores_host: csrc/host_match.cpp) compiled by g++ with AddressSanitizer and UBSan over the stand-in HIP runtime
(tests/cpp/hip_stub), as a stand-alone program with its own main whose k_match launcher runs csrc/match_math.h on exactly the
words it is handed: every rejected creation and call of SPEC.md section 25 launches nothing and leaves commands and results as
they were (the error names the clip, row or dimension), the valid calls equal a second run of the rule on copies -- through the
device call on two streams and through the host hooks on unaligned memory --, and sets are created and destroyed with searches
queued."""
import re
import subprocess

from tests import cpp_build


def test_match_host_side_under_asan_ubsan(tmp_path):
    exe = cpp_build.build("match_host_asan", tmp_path, cpp_build.HOST_ASAN)
    r = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"searched=(\d+) rejected=(\d+) launches=(\d+) failed=(\d+)", r.stdout)
    assert m, r.stdout
    searched, rejected, launches, failed = map(int, m.groups())
    # per iteration: 21 + 2 + 7 + 2 rejected creations (more with a pose bit to misplace and a row to disorder), 17 rejected
    # calls (2 more with a query to withhold); 4 valid calls and 3 on sets that are destroyed right after
    assert failed == 0 and rejected >= 40 * 49 and launches == searched == 40 * 7, r.stdout
