"""ISA check of the nearest-neighbour kernels (csrc/prdc.h: k_nn_nearest, k_nn_merge) in the listing `make` leaves in csrc/build/ (-save-temps=obj): the
per-thread list of k_nn_nearest is twice k_prdc_knn's (a column beside every distance), and it must still fit the registers of two blocks per CU --
no spills, no scratch memory."""
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc"


@pytest.fixture(scope="module")
def kernels():
    """{kernel name: metadata block} of the unit's listing"""
    subprocess.check_call(["make", "-C", str(CSRC), "-j4"], stdout=subprocess.DEVNULL)       # no-op when up to date
    text = (CSRC / "build" / "prdc-hip-amdgcn-amd-amdhsa-gfx950.s").read_text()
    md = text[text.index("amdhsa.kernels:"):]
    return {re.search(r"\.name:\s*(\S+)", blk).group(1): blk for blk in re.split(r"\n  - \.", md)[1:]}


@pytest.mark.parametrize("kernel", ["k_nn_nearest", "k_nn_merge"])
def test_no_spills_no_scratch(kernels, kernel):
    found = [(name, blk) for name, blk in kernels.items() if kernel in name]
    assert len(found) == 1, [name for name, _ in found]
    name, blk = found[0]
    get = lambda key: int(re.search(r"\." + key + r":\s*(\S+)", blk).group(1))
    assert get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0, name
    assert get("vgpr_count") <= 256, (name, get("vgpr_count"))                               # two blocks of four waves per CU
