"""Builds and runs tests/cpp/stage_frame_check.cpp: the frame record of the roll and zoom/crop stages
(video-stab_amd/csrc/planar_layout.h) on its own (plain g++, no HIP, no device)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "stage_frame_check.cpp")
HEADERS = [os.path.join(ROOT, "video-stab_amd", "csrc", n) for n in ("planar_layout.h", "pixfmt.h")]


def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "stage_frame_check")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [SRC] + HEADERS):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", out, SRC])
    return out


def run():
    """(return code, output): 0 and "N checks, 0 failed", or a line per failed check."""
    r = subprocess.run([exe()], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout + r.stderr
