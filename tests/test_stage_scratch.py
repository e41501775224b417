"""The owner of a coder stage's device blocks (csrc/stage_scratch.hpp) without a device: tests/stage_scratch_check.cpp is a
program of its own with an allocator that fails on the k-th call; built here with the host sanitizers and run as a
child process.  All blocks or none, nothing left behind by a failed call, the device check, the frees of destruction."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_all_blocks_or_none_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "stage_scratch_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "stage_scratch_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 findings")
