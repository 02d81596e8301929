"""ISA check of the DiT streaming attention kernel (csrc/dit_flash.h): every instantiation fits its registers -- no spills, no scratch
memory -- in the listing `make` leaves in csrc/build/ (-save-temps=obj)."""
import re
import subprocess
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc"
LISTING = CSRC / "build" / "ncsnpp-hip-amdgcn-amd-amdhsa-gfx950.s"


def test_streaming_attention_has_no_spills_and_no_scratch():
    subprocess.check_call(["make", "-C", str(CSRC), "-j4"], stdout=subprocess.DEVNULL)       # no-op when up to date
    md = LISTING.read_text()
    md = md[md.index("amdhsa.kernels:"):]
    found = {}
    for blk in re.split(r"\n  - \.", md)[1:]:
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        if "k_dit_flash" in name:
            get = lambda key: int(re.search(r"\." + key + r":\s*(\S+)", blk).group(1))
            found[name] = (get("vgpr_spill_count"), get("sgpr_spill_count"), get("private_segment_fixed_size"))
    assert len(found) == 3, found                                     # padded widths (64, 64), (96, 80), (96, 96)
    for name, (vs, ss, scratch) in found.items():
        assert vs == 0 and ss == 0 and scratch == 0, (name, vs, ss, scratch)
