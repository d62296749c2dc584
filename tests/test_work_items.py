"""The work-item contract of tinyrenderder_amd/csrc/work_items.h, checked on the host by a stand-alone C++ program
(tests/host/work_items_check.cpp): every item of a list is taken by exactly one workgroup of the raster launch, for list lengths around
the multiples of eight and launch grids sized for longer lists, and the item word survives encode / decode."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_every_item_once_and_item_word_round_trip(tmp_path):
    exe = tmp_path / "work_items_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tinyrenderder_amd", "csrc"),
                        "-o", str(exe), os.path.join(HERE, "host", "work_items_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "36 launches checked, 0 failures" in r.stdout, r.stdout
