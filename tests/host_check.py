"""Builds a stand-alone CPU restatement dvd_amd/csrc/<name>_host_check.cpp under AddressSanitizer and UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build_host_check(name, tmp_dir):
    """Compile <name>_host_check.cpp into tmp_dir; returns the program's path."""
    exe = tmp_dir / f"{name}_host_check"
    src = os.path.join(ROOT, "dvd_amd", "csrc", f"{name}_host_check.cpp")
    subprocess.run(["g++", *FLAGS, src, "-o", str(exe)], check=True)
    return exe
