"""CPU: every fixture file under tests/golden/ fits the size limit of a committed file (1 MiB); a larger fixture is stored as
parts (golden_parts.py)."""
import os

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_fixture_files_fit_the_size_limit():
    for name in os.listdir(GOLD):
        path = os.path.join(GOLD, name)
        if os.path.isfile(path):
            assert os.path.getsize(path) < 1 << 20, name
