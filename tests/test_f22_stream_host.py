"""csrc/mlp22.h on the host: the source map of the folded split-fp16 forward stream (feature layer folded into dir0), walked by a
stand-alone program built with the host compiler and -fsanitize=address,undefined (tests/f22_stream_check.cpp).  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_folded_stream_names_every_parameter_once_and_the_fold_where_the_kernel_reads_it(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "f22_stream_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "f22_stream_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "1044 pairs, 66 chunks, 495104 parameters, 32768 folded elements, 0 bad" in out.stdout
