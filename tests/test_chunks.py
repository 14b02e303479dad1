"""The chunk store's address arithmetic (hysortk_amd/csrc/hsk_chunks.h: chunk_deltas, chunk_slot) on the CPU, under the address and
undefined-behaviour sanitizers: tests/chunks_test.cpp holds every slot of every reservation of a 16-record chunk -- every start inside the
chunk, every length up to two chunks, physical chunks in no order whose offsets wrap 32 bits -- and seeded draws for the kernels' chunks of
4096 and 2048 records to the definition: slot i of a reservation is record (ph[v] - 1) * CHUNK + (off0 + i - st) % CHUNK of the store."""
import os
import subprocess

from tests import util


def test_every_slot_of_a_reservation_lands_in_its_chunk_under_sanitizers(tmp_path):
    exe = str(tmp_path / "chunks_test")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17",
                           os.path.join(util.ROOT, "tests", "chunks_test.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.startswith("OK"), out
