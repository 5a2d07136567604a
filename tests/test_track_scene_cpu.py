"""The argument check of the track scene (csrc/track_scene.h: what rpe_triangulate_tracks and rpe_bundle_windows share) on
the host: tests/native/track_scene_host.cpp includes the header the entry points include and, as a stand-alone program
under the address and undefined-behaviour sanitizers, runs its two phases over arrays of exactly their lengths.  Accepted,
with K and with cameras: no track, no track and no track_start, one track without observations (with and without
observation arrays), 3 tracks / 7 observations / 3 frames.  Refused with exactly its text: each single fault of the
scalars, of the CSR shape, of a pointer that is read and of the obs_frame range -- and no array is read in front of the
check of its pointer and length (a decreasing track_start whose entries pass the observations)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "track_scene_host.cpp")
INC = os.path.join(os.path.dirname(HERE), "relative_pose_estimation_amd", "csrc")


def test_track_scene_check_under_the_sanitizers(tmp_path):
    prog = str(tmp_path / "track_scene_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", INC, "-o", prog, SRC])
    r = subprocess.run([prog], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == f"{2 * 5} accepted, {14} refused, 0 bad", r.stdout
