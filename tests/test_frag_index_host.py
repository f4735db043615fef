"""csrc/mlp_index.h on the host: the inverse fragment maps of the factored weight-gradient post step against the packing's forward
map, in a stand-alone program built with the host compiler and -fsanitize=address,undefined (tests/frag_index_check.cpp).  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_inverse_fragment_maps_name_the_elements_the_packing_fills(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "frag_index_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "frag_index_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "98304 elements, 0 bad" in out.stdout
