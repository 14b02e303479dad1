"""The tuning table (hysortk_amd/csrc/hsk_tuning.h) on the CPU, under the address and undefined-behaviour sanitizers: tests/tuning_test.cpp
holds the 42 names and their defaults against a list of its own, and Tuning::parse to its grammar -- every name set alone is read back and
leaves the others at their defaults, the first setting of a name wins inside one string and from one parse() to the next, items without '='
or without a name are skipped, only leading spaces are dropped from a name, the value is atoll of what follows '=', unknown names (4 KB of
them, upper-case spellings, a name with a trailing space) are ignored, NULL and "" do nothing."""
import os
import subprocess

from tests import util


def test_tuning_table_and_parse_grammar_under_sanitizers(tmp_path):
    exe = str(tmp_path / "tuning_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "tuning_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out
