"""csrc/mlp_index.h, csrc/mlp_arch2.h and csrc/mlp_input2.h on the host: the packing maps of the view, image and 2 x 64 models
(every weight reaches its packed image once, every bias its slot), the fused row stage's channel map and the tile map of the
2 x 64 forward kernels, in a stand-alone program built with the host compiler and -fsanitize=address,undefined
(tests/pack_index_check.cpp).  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_parameter_reaches_its_packed_image_and_every_sample_one_lane(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pack_index_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "pack_index_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    # the counts of the maps this header replaced
    for line in ("image out_ch 1 forward: 479488 named once, 2049 never, 12032 padding",
                 "image out_ch 4 forward: 480256 named once, 2052 never, 11264 padding",
                 "image out_ch 3 backward: 459520 named once, 22531 never",
                 "2x64 out_ch 0 forward: 12960 named once, 228 never, 3424 padding",
                 "2x64 out_ch 0 backward: 12448 named once, 740 never",
                 "pack_index_check: 48 channel elements, 0 bad"):
        assert line in out.stdout, out.stdout
