"""csrc/keep_count.h, the host helper both masked-LM loss launchers share, compiled on its own and checked against Python."""
import os
import shutil
import subprocess

import pytest


def test_drop_worst_keep_count_matches_python(tmp_path):
    """csrc/keep_count.h (the helper both masked-LM loss launchers share) against Python's int(B * (1 - r)) for every B the launcher accepts:
    the ratio travels through the ABI as a float, the count must be the one of the caller's double."""
    import ctypes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rocm_clang = "/opt/rocm/llvm/bin/clang++"                  # the host compiler hipcc itself drives: present wherever the library builds
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    if cxx is None:
        pytest.skip("needs a host C++ compiler")
    src = os.path.join(str(tmp_path), "kc.cpp")
    with open(src, "w") as f:
        f.write('#include <cstdio>\n#include <cstdlib>\n#include "keep_count.h"\n'
                'int main(int argc, char** argv) { for (int i = 1; i < argc; ++i) { const float r = strtof(argv[i], nullptr);\n'
                '  for (int B = 1; B <= 4096; ++B) printf("%d\\n", vlp_drop_worst_keep_count(B, r)); } return 0; }\n')
    exe = os.path.join(str(tmp_path), "kc")
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(root, "vlp_amd", "csrc"), src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ratios = [0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.6, 0.25, 0.5, 1 / 3, 0.123, 0.0, 0.7, 0.8, 0.9, 0.55, 0.99, 2 / 3, 1 / 7, 5 / 6, 0.1234, 0.123456]
    out = subprocess.run([exe] + [repr(ctypes.c_float(x).value) for x in ratios], capture_output=True, text=True, timeout=120).stdout.split()
    got = [int(v) for v in out]
    assert len(got) == 4096 * len(ratios)
    old_wrong = 0
    for i, x in enumerate(ratios):
        want = [int(B * (1 - x)) for B in range(1, 4097)]
        assert got[i * 4096:(i + 1) * 4096] == want, "ratio %r: first mismatch at B = %d" % (
            x, 1 + next(j for j, (a, b) in enumerate(zip(got[i * 4096:], want)) if a != b))
        xf = ctypes.c_float(x).value
        old_wrong += sum(int(B * (1.0 - xf)) != w for B, w in zip(range(1, 4097), want))
    assert old_wrong > 1000          # the widened float (what the launchers computed before) misses Python's count on thousands of these pairs
