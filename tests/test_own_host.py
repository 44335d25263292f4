"""The two owners of the library's device memory (pigeon.jl_amd/csrc/pg_own.hpp: CallBufs, HandleBufs) on the host, under AddressSanitizer and UBSan: a stand-alone
program (tests/own_host_main.cpp, its own main, malloc / free behind pg_dev_alloc / pg_dev_free) that runs one scripted life of a handle once without a failure and once
for every allocation of it failing.  Nothing is preloaded and nothing is loaded into Python: the program runs as a child process."""
import os
import subprocess

from conftest import ROOT


def test_owners_free_once_and_null_the_members_on_every_failure_path(tmp_path):
    exe = str(tmp_path / "own_host")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pigeon.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "own_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "10 allocations, 11 runs: ok" in r.stdout, r.stdout
