"""csrc/lattice.h on the host: the spacing, the index decomposition, the cell centres and the workgroup count that every volume
kernel takes from it, and its three argument checks, in a stand-alone program built with the host compiler and
-fsanitize=address,undefined (tests/lattice_check.cpp).  The floats are compared as bit patterns with tests/_mesh_ref.py, the
reference marching cubes and the TSDF reference are built on.  R = 512 is where n3 = 2^27 and the int index arithmetic is closest
to its limit.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _mesh_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = (-1.5, -0.7, 0.1), (1.5, 2.3, 0.35)
SIZES = (2, 3, 65, 512)
NERF_OK, NERF_E_NULL, NERF_E_SHAPE = 0, -1, -2


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("lattice") / "lattice_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "lattice_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    per_r, checks, R = {}, {}, None
    for ln in out.stdout.splitlines():
        w = ln.split()
        if w[0] == "R":
            R = int(w[1])
            per_r[R] = {"rc": int(w[3]), "n3": int(w[5]), "blocks": int(w[7]), "p": []}
        elif w[0] == "h":
            per_r[R]["h"] = [int(x, 16) for x in w[1:]]
        elif w[0] == "p":
            per_r[R]["p"].append([int(x) for x in w[1:5]] + [int(x, 16) for x in w[5:]])
        elif w[0] == "check":
            checks[w[1]] = [int(x) for x in w[2:]]
    return per_r, checks


@pytest.mark.parametrize("R", SIZES)
def test_spacing_coordinates_centres_and_blocks_match_the_reference(printed, R):
    got = printed[0][R]
    assert got["rc"] == NERF_OK and got["n3"] == R ** 3
    assert got["blocks"] == -(-R ** 3 // 256)
    assert got["h"] == MR.spacing(R, LO, HI).view(np.uint32).tolist()
    p = np.array(got["p"], np.int64)
    assert len(p) == 1002 and p[0, 0] == 0 and p[1, 0] == R ** 3 - 1
    l, c = p[:, 0], p[:, 1:4]
    assert ((c >= 0) & (c < R)).all()
    assert np.array_equal(c[:, 0] + R * (c[:, 1] + R * c[:, 2]), l)
    want = MR.axis_coords(R, LO, HI).view(np.uint32)                       # [3, R]
    for a in range(3):
        assert np.array_equal(p[:, 4 + a], want[a][c[:, a]].astype(np.int64)), a
    if R > 3:
        assert len(np.unique(l)) > 900                                     # the seeded indices do spread over the lattice


def test_argument_checks(printed):
    checks = printed[1]
    assert checks.pop("res_ok") == [NERF_OK] * 4
    assert checks.pop("res_1") == [NERF_E_SHAPE, NERF_E_SHAPE, 0]
    assert checks.pop("res_513") == [NERF_E_SHAPE, NERF_E_SHAPE, 0]
    assert checks.pop("box_null") == [NERF_E_NULL]
    assert len(checks) == 2 + 4 * 3
    for name, rcs in checks.items():
        assert rcs and all(rc == NERF_E_SHAPE for rc in rcs), (name, rcs)
