"""The dense path's bit-level forms (csrc/dense_forms.inc: lev2_window, row_lev2 with sig_codes and row_codes8,
lev2_masks, lev2_window16, lev2_screen, the mismatch counts, fold10x4, transpose4x4) compiled for the CPU from the
source as it stands and run against the textbook edit distance by tools/dense_forms_check.cpp: every pair of reads
over {A, C, N} up to 6 cycles, the scripted shifts of tests/lev2_scripts.py with their first and last mismatch on
every pair of boundary cycles, random pairs at 19 lengths, each pair in both orders; the signature, screen and row
words built from symbols by the stated format, and from raw bytes through the fold and pack arithmetic.  Built with
the address and undefined-behaviour sanitizers.  No GPU."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _build(tmp, name, extra=()):
    exe = str(tmp / name)
    subprocess.check_call(["g++"] + FLAGS + list(extra) + [os.path.join(REPO, "tools", "dense_forms_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("dense_forms")


def test_dense_forms_equal_textbook_distance(tmp):
    out = subprocess.run([_build(tmp, "dense_forms_check"), "1", "0.4"], capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0 and " 0 disagreements" in out.stdout, (out.stdout, out.stderr[-2000:])
    m = re.match(r"(\d+) pairs \((\d+) at distance exactly 2\)", out.stdout)
    assert m and int(m.group(1)) > 1000000 and int(m.group(2)) > 100000


def test_a_last_mismatch_one_field_off_is_caught(tmp):
    """Broken on purpose, must fail: the program's own __clz shim (not the library's source) answers one
    signature field too many, so t lands one field low in lev2_window and lev2_window16."""
    out = subprocess.run([_build(tmp, "dense_forms_check_bad", ["-DDENSE_FORMS_BAD_CLZ"]), "1", "0.05"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 1, (out.stdout, out.stderr[-2000:])
    assert "MISMATCH lev2_window:" in out.stderr and "MISMATCH lev2_window16:" in out.stderr, out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert not re.search(r" 0 disagreements", out.stdout)
