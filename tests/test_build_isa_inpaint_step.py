"""ISA check of the inpainting step of the CIFAR10 form (csrc/ni_step.hip, k_step_inpaint_f64) in the listing `make` leaves in csrc/build/
(-save-temps=obj): it fits its registers -- no VGPR or SGPR spills, no scratch memory; x_next leaves in one 16-byte store, after the blend; and the
mask costs one 32-bit load per element quad, the only single-dword load of the kernel.  The blend on its own (k_known_blend) is held to the same."""
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


def test_inpaint_step_without_spills_or_scratch_one_16_byte_store_of_x_next_one_mask_word(listing):
    name, vs, ss, scratch, ops = _kernel(listing, "k_step_inpaint_f64")
    assert vs == 0 and ss == 0 and scratch == 0, (name, vs, ss, scratch)
    assert not [o for o in ops if o.startswith(("scratch_", "flat_", "buffer_"))], (name, sorted(set(ops)))
    stores = [o for o in ops if "_store_" in o]
    # hist[k] (two fp64 pairs) and x_next: 16 bytes each, and x_next is stored once -- the blend happens in registers in front of it
    assert stores == ["global_store_dwordx4"] * 3, (name, stores)
    loads = [o for o in ops if "_load_" in o]
    assert loads.count("global_load_dword") == 1, (name, loads)                              # the mask word of the quad
    # x_k, model_out, known, eps_0 and the history rows (two per term): every stream a 16-byte load; the int64 global index the one 8-byte load
    rest = sorted(set(loads) - {"global_load_dword", "global_load_dwordx4"})
    assert rest in ([], ["global_load_dwordx2"]), (name, rest)
    assert loads.count("global_load_dwordx4") >= 6, (name, loads)


def test_blend_alone_without_spills_or_scratch(listing):
    name, vs, ss, scratch, ops = _kernel(listing, "k_known_blend")
    assert vs == 0 and ss == 0 and scratch == 0, (name, vs, ss, scratch)
    assert [o for o in ops if "_store_" in o] == ["global_store_dwordx4"], (name, ops)
    assert [o for o in ops if "_load_" in o].count("global_load_dword") == 1, (name, ops)
