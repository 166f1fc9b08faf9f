"""CPU: the HOST side of players (mtr_anim_player_create / _destroy, mtr_anim_player_advance_device(_cmds) and
mtr_anim_player_advance_host: csrc/host_player.cpp) compiled by g++ with AddressSanitizer and UBSan over the stand-in HIP
runtime (tests/cpp/hip_stub), as a stand-alone program with its own main whose k_play launcher runs csrc/play_math.h on
exactly the words it is handed: every rejected call of SPEC.md section 20 launches nothing and leaves the states as they
were (the error names the clip), host commands are staged in the player's own buffer before the call returns, device
commands are read where they are, a second stream waits for the player's event, the scratch array is clean after every
call, and players are created and destroyed with advances queued while their command buffer grows."""
import re
import subprocess

from tests import cpp_build


def test_player_host_side_under_asan_ubsan(tmp_path):
    exe = cpp_build.build("player_host_asan", tmp_path, cpp_build.HOST_ASAN)
    r = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"advanced=(\d+) rejected=(\d+) launches=(\d+) cmd_launches=(\d+) failed=(\d+)", r.stdout)
    assert m, r.stdout
    advanced, rejected, launches, cmd_launches, failed = map(int, m.groups())
    assert failed == 0 and rejected == 40 * 42 and launches == advanced and advanced >= 40 * 7 and 0 < cmd_launches < launches, r.stdout
