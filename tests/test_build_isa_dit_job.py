"""ISA check of the Validate-form step with in-kernel noise (csrc/ni_step.hip, k_step_noise_f32prod): one instance, and it fits
its registers -- no VGPR or SGPR spills, no scratch memory -- in the listing `make` leaves in csrc/build/ (-save-temps=obj)."""
import re
import subprocess
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc"
LISTING = CSRC / "build" / "ni_step-hip-amdgcn-amd-amdhsa-gfx950.s"


def test_noise_step_exists_once_without_spills_or_scratch():
    subprocess.check_call(["make", "-C", str(CSRC), "-j4"], stdout=subprocess.DEVNULL)       # no-op when up to date
    md = LISTING.read_text()
    md = md[md.index("amdhsa.kernels:"):]
    found = {}
    for blk in re.split(r"\n  - \.", md)[1:]:
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        if "k_step_noise_f32prod" in name:
            get = lambda key: int(re.search(r"\." + key + r":\s*(\S+)", blk).group(1))
            found[name] = (get("vgpr_spill_count"), get("sgpr_spill_count"), get("private_segment_fixed_size"))
    assert len(found) == 1, found
    for name, (vs, ss, scratch) in found.items():
        assert vs == 0 and ss == 0 and scratch == 0, (name, vs, ss, scratch)
