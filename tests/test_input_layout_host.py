"""csrc/mlp_input.h on the host: the channel order of both encoders and both embedded-row readers of the view model's input stage
against the reference's embedding and the channel maps of csrc/mlp_index.h, in a stand-alone program built with the host compiler
and -fsanitize=address,undefined (tests/input_layout_check.cpp).  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_encoders_and_row_readers_place_every_channel_where_the_maps_say(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "input_layout_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "input_layout_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "2304 elements, 0 bad" in out.stdout
