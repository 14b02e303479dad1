"""The radix sort's digit plans (hysortk_amd/csrc/hsk_passplan.h: make_pass_plan, make_hybrid_plan, make_split_prefix_plan) on the CPU, under
the address and undefined-behaviour sanitizers: tests/passplan_test.cpp builds the plan of every K in 3..95 (K % 32 != 0) and of full words
(hsk_stage_sort) at radix_bits 4..8 into blocks of exactly the capacity it hands over, and holds every plan to the definition -- the digits
tile each word's used bits, none wider than radix_bits or across a word, the count is sum(ceil(bits / radix_bits)) <= MAX_PASSES -- and every
split 16-bit prefix to its 16 bits across the two words."""
import os
import subprocess

from tests import util


def test_digit_plans_are_bounded_and_tile_the_key_under_sanitizers(tmp_path):
    exe = str(tmp_path / "passplan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "passplan_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out
