"""Builds and runs tests/cpp/pixfmt_check.cpp: the format table and the refusal rules of video-stab_amd/csrc/pixfmt.h on their own
(plain g++, no HIP, no device)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "pixfmt_check.cpp")
HEADER = os.path.join(ROOT, "video-stab_amd", "csrc", "pixfmt.h")


def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "pixfmt_check")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(SRC), os.path.getmtime(HEADER)):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", out, SRC])
    return out


def run(mode, stdin=""):
    r = subprocess.run([exe(), mode], input=stdin, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout
