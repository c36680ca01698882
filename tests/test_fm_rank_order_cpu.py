"""The order gorse_fm_rank_users ranks a list in, checked without a device: the Python restatement the GPU test compares with
(fm_rank_ref.rank_order) against `sorted` with an explicit key on hand-written lists, and the host fallback's comparator with the
device's sort key in a stand-alone C++ program built with AddressSanitizer and UBSan."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import fm_rank_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
NEG_NAN = np.array([0xffc00123], np.uint32).view(np.float32)[0]

LISTS = [
    [],
    [1.0],
    [NAN],
    [1.0, 2.0],
    [2.0, 2.0, 2.0],
    [0.0, -0.0, 0.0, -0.0],
    [-0.0, 1.0, 0.0, -1.0],
    [NAN, 1.0, NAN, 3.0, 1.0, NEG_NAN],
    [1.0, NEG_NAN, 3.0, -0.0, 3.0, 0.0, NAN, -2.0],
    [-INF, INF, NAN, -INF, INF, 0.0],
    [1e-45, -1e-45, 0.0, -0.0, 1e-45],
]


def _by_sorted(scores):
    def key(i):
        s = float(scores[i])
        if math.isnan(s):
            return (1, 0.0, i)
        return (0, -s, i)  # -(+0.0) == -0.0 == 0.0: equal as floats
    return sorted(range(len(scores)), key=key)


@pytest.mark.parametrize("scores", LISTS, ids=[str(i) for i in range(len(LISTS))])
def test_order_restatement_on_handwritten_lists(scores):
    got = K.rank_order(np.array(scores, np.float32))
    assert got.tolist() == _by_sorted(scores)


def test_order_restatement_written_out():
    # descending; the tie at 3.0 and the zeros of both signs by position; the NaNs last by position, whatever their sign
    assert K.rank_order([1.0, NEG_NAN, 3.0, -0.0, 3.0, 0.0, NAN, -2.0]).tolist() == [2, 4, 0, 3, 5, 7, 1, 6]
    assert K.rank_order([0.0, -0.0, 0.0, -0.0]).tolist() == [0, 1, 2, 3]


def test_order_restatement_random():
    rng = np.random.default_rng(5)
    pool = np.array([NAN, NEG_NAN, 0.0, -0.0, 1.0, -1.0, 0.5, INF, -INF], np.float32)
    for n in (2, 63, 64, 65, 300):
        s = pool[rng.integers(0, pool.size, n)]
        assert K.rank_order(s).tolist() == _by_sorted(s)
    ptr = np.array([0, 3, 3, 8], np.int64)
    s = pool[rng.integers(0, pool.size, 8)]
    want = _by_sorted(s[0:3]) + _by_sorted(s[3:8])
    assert K.rank_orders(s, ptr).tolist() == want


@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("clang++") is None, reason="no host C++ compiler")
def test_host_comparator_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    exe = str(tmp_path / "fm_rank_order")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "fm_rank_order_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fm_rank_order ok" in out.stdout
