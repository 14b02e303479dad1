"""The slice planner of hsk_result_pairs_sliced (hysortk_amd/csrc/hsk_pairplan.h: pair_plan_next, pair_plan_all) on the CPU, under the
address and undefined-behaviour sanitizers: tests/pairplan_test.cpp cuts offset arrays -- all entries without records, long runs of equal
offsets on both sides of a cut, one entry above the budget at the start, in the middle and at the end, budget 1, budgets at and above the
total, offsets near 2^40 and above 2^63 -- into blocks of exactly the sizes the planner states, and holds the cuts to a plain loop over the
entries and to the definition: strictly increasing up to the number of entries, every slice within the budget or a single entry, no slice
able to take one more entry."""
import os
import subprocess

from tests import util


def test_slices_follow_the_plain_loop_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pairplan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "pairplan_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out
