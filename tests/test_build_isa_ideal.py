"""ISA check of the ideal denoiser's kernels (csrc/ideal.h) in the listing `make` leaves in csrc/build/ (-save-temps=obj): no spills, no scratch memory, and a
register count within the occupancy each kernel's __launch_bounds__ claims -- k_ideal_part is the sweep's tile at two blocks of four waves per CU."""
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc"

# kernel -> the VGPRs a wave may hold: 512 per SIMD lane over (blocks per CU x waves per block / 4 SIMDs) waves, 256 at the most
KERNELS = {"k_ideal_tplanes": 256, "k_ideal_rows": 256, "k_ideal_part": 256, "k_ideal_merge": 256, "k_ideal_wdebug": 256}


@pytest.fixture(scope="module")
def kernels():
    """{kernel name: metadata block} of the unit's listing"""
    subprocess.check_call(["make", "-C", str(CSRC), "-j4"], stdout=subprocess.DEVNULL)       # no-op when up to date
    text = (CSRC / "build" / "prdc-hip-amdgcn-amd-amdhsa-gfx950.s").read_text()
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
