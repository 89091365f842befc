"""Builds and runs tests/cpp/planes_check.cpp: the plane list of a YUV surface (video-stab_amd/csrc/planar_layout.h, planes()) on
its own (plain g++, no HIP, no device)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "planes_check.cpp")
HEADERS = [os.path.join(ROOT, "video-stab_amd", "csrc", n) for n in ("planar_layout.h", "pixfmt.h")]


def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "planes_check")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in [SRC] + HEADERS):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", out, SRC])
    return out


def planes(cases):
    """cases: [(fmt, w, h, pitch, uv_off, u_off, v_off, c_pitch)] -> per case (n, sample_bytes, [plane dicts], from_list, from_i420_layout);
    the last two: (pitch, cpitch, u, v) of a three-plane format as the list gives it and as i420_layout does, else None."""
    text = "".join(" ".join(str(int(v)) for v in c) + "\n" for c in cases)
    r = subprocess.run([exe()], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases), r.stdout
    out = []
    for ln in lines:
        parts = [[int(v) for v in p.split()] for p in ln.split("|")]
        n, sb = parts[0]
        assert n > 0, ln
        keys = ("off", "pitch", "w", "h", "cn", "sx", "sy", "row_bytes")
        pl = [dict(zip(keys, p)) for p in parts[1:1 + n]]
        rest = parts[1 + n:]
        out.append((n, sb, pl, tuple(rest[0]) if rest else None, tuple(rest[1]) if rest else None))
    return out
