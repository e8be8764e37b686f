"""The quad tail mode is compiled into one product instance only: the 4-wave instance of the sphere / box BVH
preset with Marble textures (kernel.hip kQuadTail: trace_samples<0, 4, 33>, the product's kernel_mc.hip unit).
Every other trace_samples instance of the built librtamd.so keeps the register, spill and scratch numbers of the
committed table exactly (tests/golden/kernel_resources.json, the table from before the mode): a change of the
shared traversal code that reaches them shows up here (CPU suite). The target instance itself spills no more
than its row of that table (tests/test_kernel_resources.py)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "kernel_resources.json")
TARGETS = ("trace_samples<0, 4, 33>",)
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")


@pytest.fixture(scope="module")
def built():
    assert os.path.exists(kr.DEFAULT_LIB), "librtamd.so is not built (run __graft_entry__.build())"
    return {kr.readable(k): v for k, v in kr.kernel_resources(kr.DEFAULT_LIB).items() if "trace_samples" in k}


@pytest.mark.parametrize("inst", sorted(k for k in json.load(open(TABLE)) if k not in TARGETS))
def test_other_instances_keep_their_numbers(built, inst):
    want = json.load(open(TABLE))[inst]
    got = built[inst]
    assert {k: got[k] for k in FIELDS} == {k: want[k] for k in FIELDS}, inst


@pytest.mark.parametrize("inst", TARGETS)
def test_target_instance_holds_the_lane_maps_and_four_waves(built, inst):
    # the mode's two 16-entry lane maps are the instance's only static LDS; 4 waves per SIMD need <= 128 VGPRs
    assert built[inst]["group_segment_fixed_size"] == 128
    assert built[inst]["vgpr_count"] <= 128
