"""csrc/mlp_index.h on the host: the source maps of the folded split-bf16 training image (feature layer folded into dir0 in the
training forward and the dZ chain; `nerf_set_option("train_fold", 1)`), walked by a stand-alone program built with the host compiler
and -fsanitize=address,undefined (tests/train_fold_stream_check.cpp).  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_folded_training_streams_name_every_source_once_and_the_copies_lie_behind_them(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "train_fold_stream_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "train_fold_stream_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert ("1056 + 972 pairs, 66 + 61 chunks, 495104 + 459392 parameters, 32768 + 32768 folded elements, 0 bad"
            in out.stdout), out.stdout
