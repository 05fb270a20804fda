"""csrc/fastdiv.h on the host: tests/fastdiv_check.cpp (own main, the system C++ compiler, fastdiv.h and nothing else of the
library) is built and run.  It compares quotient and remainder of the multiply-and-shift division with `/` and `%`:
  1. every dividend below 2^22 against every divisor 1 .. 4096 (2^34 pairs, on up to 16 threads);
  2. the divisors the 255 and 271 frame plans produce (961, 625, 31, 25, 29, 27, 3, 124, 248, 632; 1089, 729, 33, ...): every
     dividend below 2^24, the top 2^20 of the range, around multiples of the divisor up to the bound;
  3. six million random pairs up to the documented bound, divisors of every bit length;
  4. the bound itself: dividend 2^31 - 1, divisors next to 1, next to 2^31 - 1 and around every power of two.
No GPU, no Python extension; skipped where no C++ compiler is installed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)

pytestmark = pytest.mark.skipif(CXX is None, reason='no C++ compiler')


def test_fastdiv_agrees_with_the_division_operators(tmp_path):
    exe = str(tmp_path / 'fastdiv_check')
    subprocess.check_call([CXX, '-O2', '-std=c++17', '-pthread', '-I' + os.path.join(ROOT, 'usot_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'fastdiv_check.cpp'), '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0, out
    assert out.count(': ok') == 4 and 'fastdiv: all parts ok' in out, out
