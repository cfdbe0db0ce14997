"""Static checks of the gfx950 machine code of the two-block final stage (kernels/final_strip.hpp final_strip2_x3_kernel, KIT-ML's width), no GPU:
tools/isa_report.py disassembles libmldhip.so as tests/test_isa_properties.py does for its sibling."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_report  # noqa: E402


@pytest.fixture(scope="module")
def rep():
    if not os.path.exists(isa_report.DEFAULT_LIB) or not os.path.exists(os.path.join(isa_report.LLVM, "llvm-objdump")):
        pytest.skip("libmldhip.so / the LLVM binary tools are not here")
    return isa_report.report()


def test_two_block_final_stage_code(rep):
    hits = [v for k, v in rep.items() if "final_strip2_x3_kernel" in k]
    assert len(hits) == 1, [k for k in rep if "final_strip" in k]
    k = hits[0]
    assert k["scratch"] == 0 and k["flat"] == 0, k
    assert k["mfma"] == 8 * 2 * 3 * 3, k                     # chunks x column blocks x row tiles x split products
    assert k["vgpr"] <= 128, k                               # __launch_bounds__(512, 4): two workgroups per CU, like its sibling
    # the lookup by substring of the three-block kernel still finds exactly one
    assert len([n for n in rep if "final_strip_x3_kernel" in n]) == 1
