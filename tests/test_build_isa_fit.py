"""ISA check of the Gram kernel of the coefficient fitter (csrc/fit.hip) in the listing `make` leaves in csrc/build/ (-save-temps=obj): no spills, no
scratch memory, and a register count within the occupancy the kernel's __launch_bounds__ claims -- eight waves a workgroup, two a SIMD: 256 VGPRs a wave."""
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc"

# kernel instance (one 16-row block: M <= 16; two: M <= 32) -> the VGPRs a wave may hold
KERNELS = {"k_fit_gramILi1E": 256, "k_fit_gramILi2E": 256}


@pytest.fixture(scope="module")
def kernels():
    """{kernel name: metadata block} of the unit's listing"""
    subprocess.check_call(["make", "-C", str(CSRC), "-j4"], stdout=subprocess.DEVNULL)       # no-op when up to date
    text = (CSRC / "build" / "fit-hip-amdgcn-amd-amdhsa-gfx950.s").read_text()
    md = text[text.index("amdhsa.kernels:"):]
    return {re.search(r"\.name:\s*(\S+)", blk).group(1): blk for blk in re.split(r"\n  - \.", md)[1:]}


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_spills_no_scratch(kernels, kernel):
    found = [(name, blk) for name, blk in kernels.items() if kernel in name]
    assert len(found) == 1, [name for name, _ in found]
    name, blk = found[0]
    get = lambda key: int(re.search(r"\." + key + r":\s*(\S+)", blk).group(1))
    assert get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0, name
    assert get("vgpr_count") <= KERNELS[kernel], (name, get("vgpr_count"))
