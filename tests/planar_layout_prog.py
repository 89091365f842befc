"""Builds and runs tests/cpp/planar_layout_check.cpp: the layout rules of the roll and zoom/crop stages' three-plane surfaces
(video-stab_amd/csrc/planar_layout.h) on their own (plain g++, no HIP, no device)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "planar_layout_check.cpp")
HEADERS = [os.path.join(ROOT, "video-stab_amd", "csrc", n) for n in ("planar_layout.h", "pixfmt.h")]


def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "planar_layout_check")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [SRC] + HEADERS):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", out, SRC])
    return out


def check(cases):
    """cases: [(fmt, ptr, w, h, pitch, c_pitch, u_off, v_off, need_w, need_h)] -> [(rc, text)]; rc 0: text = "pitch cpitch u v"."""
    text = "".join(" ".join(str(int(v)) for v in c) + "\n" for c in cases)
    r = subprocess.run([exe()], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [ln.split("|", 1) for ln in r.stdout.splitlines()]
    assert len(out) == len(cases), r.stdout
    return [(int(rc), msg) for rc, msg in out]
