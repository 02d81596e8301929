"""ISA check of the colorization step of the CIFAR10 form (csrc/ni_step.hip, k_step_colorize_f64) in the listing `make` leaves in csrc/build/
(-save-temps=obj): the three-plane body fits its registers -- no VGPR or SGPR spills, no scratch memory -- and every store is a 16-byte one:
hist[k] as two per plane, x_next as one per plane, after the blend.  The blend on its own (k_color_blend) is held to the same."""
import re
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "naturaldiffusion_amd" / "csrc"
LISTING = CSRC / "build" / "ni_step-hip-amdgcn-amd-amdhsa-gfx950.s"


def _kernel(text, kernel):
    """(mangled name, vgpr spills, sgpr spills, scratch bytes, memory mnemonics in program order) of the one kernel whose name contains `kernel`"""
    md = text[text.index("amdhsa.kernels:"):]
    found = []
    for blk in re.split(r"\n  - \.", md)[1:]:
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        if kernel in name:
            get = lambda key: int(re.search(r"\." + key + r":\s*(\S+)", blk).group(1))
            found.append((name, get("vgpr_spill_count"), get("sgpr_spill_count"), get("private_segment_fixed_size")))
    assert len(found) == 1, found
    name, vs, ss, scratch = found[0]
    code = text[:text.index("amdhsa.kernels:")]
    body = code[code.index("\n" + name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    return name, vs, ss, scratch, re.findall(r"^\s+((?:global|flat|scratch|buffer)_\w+)", body, flags=re.M)


@pytest.fixture(scope="module")
def listing():
    subprocess.check_call(["make", "-C", str(CSRC), "-j4"], stdout=subprocess.DEVNULL)       # no-op when up to date
    return LISTING.read_text()


def test_colorize_step_without_spills_or_scratch_nine_16_byte_stores(listing):
    name, vs, ss, scratch, ops = _kernel(listing, "k_step_colorize_f64")
    assert vs == 0 and ss == 0 and scratch == 0, (name, vs, ss, scratch)
    assert not [o for o in ops if o.startswith(("scratch_", "flat_", "buffer_"))], (name, sorted(set(ops)))
    # per plane hist[k] (two fp64 pairs) and x_next, which is stored once per plane -- the blend happens in registers in front of it
    assert [o for o in ops if "_store_" in o] == ["global_store_dwordx4"] * 9, (name, ops)


def test_blend_alone_without_spills_or_scratch_three_16_byte_stores(listing):
    name, vs, ss, scratch, ops = _kernel(listing, "k_color_blend")
    assert vs == 0 and ss == 0 and scratch == 0, (name, vs, ss, scratch)
    assert not [o for o in ops if o.startswith(("scratch_", "flat_", "buffer_"))], (name, sorted(set(ops)))
    assert [o for o in ops if "_store_" in o] == ["global_store_dwordx4"] * 3, (name, ops)
