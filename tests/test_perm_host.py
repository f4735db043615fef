"""csrc/perm.h on the host: the key schedule and the cycle-walked Feistel permutation that nerf_pixel_permutation and both
nerf_sample_batch entries take from it, in a stand-alone program built with the host compiler and -fsanitize=address,undefined
(tests/perm_check.cpp), against ops.index.pixel_permutation_host.  Domain 1 walks a cycle of the four-value block, 2^33 + 5 has
17-bit halves and values past 2^32.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from nerf_meets_mlx_amd.ops import index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOMAINS = (1, 2, 35, 4096, 640000, (1 << 33) + 5)
SEEDS = (0, 0xFEDCBA9876543210)


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("perm") / "perm_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "perm_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    keys, runs, head = {}, {}, None
    for ln in out.stdout.splitlines():
        w = ln.split()
        if w[0] == "key":
            keys[(int(w[1]), int(w[2]))] = [int(x) for x in w[3:]]
        elif w[0] == "run":
            head = tuple(int(x) for x in w[1:])                            # domain, seed, offset, n
        elif w[0] == "v":
            runs[head] = np.array([int(x) for x in w[1:]], np.uint64)
    return keys, runs


@pytest.mark.parametrize("domain", DOMAINS)
def test_keys_and_values_match_the_host_mirror(printed, domain):
    keys, runs = printed
    n = min(domain, 1000)
    bits = max(2, (domain - 1).bit_length())
    for seed in SEEDS:
        assert keys[(domain, seed)] == [(bits + 1) // 2] + [index._splitmix64((seed + r) & index._M64) & 0xFFFFFFFF for r in range(4)]
        for offset, count in ((0, domain if domain <= 4096 else n), (domain - n, n)):
            got = runs[(domain, seed, offset, count)]
            assert len(got) == count
            assert np.array_equal(got.astype(np.int64), index.pixel_permutation_host(count, domain, seed, offset))


@pytest.mark.parametrize("domain", [d for d in DOMAINS if d <= 4096])
def test_the_whole_domain_is_permuted(printed, domain):
    for seed in SEEDS:
        assert np.array_equal(np.sort(printed[1][(domain, seed, 0, domain)]), np.arange(domain, dtype=np.uint64))
