"""CPU-side checks of the options of the lane form of SpiralPack batch calls (include/spiral_gpu.h): "pack_batch_lanes", the smallest number of
clients from which answer_batch and answer_batch_instances run as one lane-aware launch sequence (0 .. 8, 0 = never), and the read-only counter
"pack_lane_batches" of the calls that did."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


def test_pack_batch_lanes_round_trip(sa):
    before = sa.get_option("pack_batch_lanes")
    try:
        for v in (0, 2, 8):
            sa.set_option("pack_batch_lanes", v)
            assert sa.get_option("pack_batch_lanes") == v
    finally:
        sa.set_option("pack_batch_lanes", before)


def test_pack_batch_lanes_range(sa):
    before = sa.get_option("pack_batch_lanes")
    try:
        for v in (9, -1):
            with pytest.raises(sa.SpiralGpuError, match="pack_batch_lanes"):
                sa.set_option("pack_batch_lanes", v)
            assert sa.get_option("pack_batch_lanes") == before, "a refused value changed the option"
    finally:
        sa.set_option("pack_batch_lanes", before)


def test_pack_lane_batches_is_zero_in_a_fresh_process(sa):
    code = "import spiral_amd as sa; print('default', sa.get_option('pack_batch_lanes'), 'count', sa.get_option('pack_lane_batches'))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.split() == ["default", "0", "count", "0"], r.stdout


def test_pack_lane_batches_is_read_only(sa):
    count = sa.get_option("pack_lane_batches")
    for v in (0, 1):
        with pytest.raises(sa.SpiralGpuError, match="pack_lane_batches"):
            sa.set_option("pack_lane_batches", v)
    assert sa.get_option("pack_lane_batches") == count
