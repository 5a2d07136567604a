"""The candidate entries of fast_nms_kernel (csrc/fast_entry.h) on the host: tests/native/fast_entry_host.cpp includes the
header the kernel includes and, as a stand-alone program under the address and undefined-behaviour sanitizers, walks every
lane (tid < 252) and every flag bit a lane can set (5 passes x 4 pixels) with every side-flag combination: the lane form
decodes to the phase-1 mapping written out independently (r0 = tid / 18, c = tid % 18, row r0 + 14 it, column 4 c + px),
all entries and the pixels they name are distinct, the side flags survive, the compact form round-trips, and the
multiply-and-shift division is exact for every byte offset of the tile."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "fast_entry_host.cpp")
INC = os.path.join(os.path.dirname(HERE), "relative_pose_estimation_amd", "csrc")


def test_fast_entry_forms_under_the_sanitizers(tmp_path):
    prog = str(tmp_path / "fast_entry_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", INC, "-o", prog, SRC])
    r = subprocess.run([prog], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == f"{252 * 20 * 3} entries, 0 bad", r.stdout
