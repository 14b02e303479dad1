"""The parse stage's plan (hysortk_amd/csrc/hsk_parseplan.h: parse_tiling, slab_bytes, parse_rec_cap, place_group) on the CPU, under the
address and undefined-behaviour sanitizers: tests/parseplan_test.cpp takes packed buffers from one byte to 20 GB -- around every tile, block
and slab boundary -- with 1 to 5000 workgroups allowed and 1 to 17 slabs wanted, and holds every plan to the definition the kernels use: the
workgroups' tile ranges, slab by slab, cover every tile exactly once with at most 1024 workgroups, the slabs' byte ranges tile the buffer with
heads of at most SLAB_HEAD bytes, the record capacity of every window is a power of two with 40 % head room, and a placement step's tiles
never hold more records than the kernel stages."""
import os
import subprocess

from tests import util


def test_parse_plans_cover_every_tile_once_under_sanitizers(tmp_path):
    exe = str(tmp_path / "parseplan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "parseplan_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out
