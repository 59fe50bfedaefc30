"""The resync's row rules (distributed_amd/csrc/dgp_rows.h) are host-only C++: the header
compiles on its own without HIP, and a stand-alone driver (rows_driver.cpp) feeds the three
normalisers one good row set and every malformed input of the resync. CPU-only."""
import os
import shutil
import subprocess

from conftest import REPO

HEADER = os.path.join(REPO, "distributed_amd", "csrc", "dgp_rows.h")
GXX = shutil.which("g++") or "c++"  # the compiler build.py's ingestion pass and the oracle need too
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]


def test_header_compiles_alone_without_hip():
    src = open(HEADER).read()
    assert "hip/" not in src and "__global__" not in src
    subprocess.run([GXX, *FLAGS, "-fsyntax-only", "-x", "c++", HEADER], check=True, capture_output=True, text=True)


def test_normalisers_accept_the_good_rows_and_refuse_the_malformed(tmp_path):
    exe = str(tmp_path / "rows_driver")
    subprocess.run([GXX, *FLAGS, "-O1", "-o", exe, os.path.join(REPO, "tests", "rows_driver.cpp")], check=True,
                   capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "rows ok", r.stdout + r.stderr
