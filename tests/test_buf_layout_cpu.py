"""The layout of a buffer set (csrc/buf_layout.h: the one device block of a first-use feature, carved into its pieces) on
the host: tests/native/buf_layout_host.cpp includes the header rpe_bufset_fit includes and, as a stand-alone program under
the address and undefined-behaviour sanitizers, lays out piece lists of 1 to 20 entries with sizes from {0, 1, 255, 256,
257, 80 n, 2^33 + 1}: every offset is a multiple of 256, the pieces lie in order and do not overlap, a piece of 0 bytes is
flagged null and takes no room, the total is the sum of the aligned sizes and at least 256, and the 2^33 pieces do not wrap
(the expected sums are kept in 128 bits)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "buf_layout_host.cpp")
INC = os.path.join(os.path.dirname(HERE), "relative_pose_estimation_amd", "csrc")


def test_buffer_set_layout_under_the_sanitizers(tmp_path):
    prog = str(tmp_path / "buf_layout_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", INC, "-o", prog, SRC])
    r = subprocess.run([prog], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == f"{20 * (7 + 500)} lists, 0 bad", r.stdout
